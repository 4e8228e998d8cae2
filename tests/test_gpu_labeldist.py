"""The label-map distance term on the GPU (csrc/labeldist.hip through ilps_amd/labeldist.py) against
tests/_labeldist_oracle.py: indices and status exactly, floats under the bar |got - want| <= 2^-24 |want| + 2^-28 T.  Small
shapes (every combination of B in {1, 3}, V in {1, 65, 257, 600}, W in {1, 7, 48}, C in {2, 32}, with and without sigma,
slack 0 and 0.5, from the generator of tests/_labeldist_cases.py that holds every case the term has to survive), W = 160,
the full size, the prep launch, bit-equality between launches and between a row alone and inside a batch, hostile rows, the
chain through `SMPLLayer`, and `LabelDistanceFitter` (a `ParamFitter`) with all three side terms."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _labeldist_cases as cases  # noqa: E402
import _labeldist_oracle as orc  # noqa: E402
from ilps_amd.labeldist import LabelDistanceSpec, LabelTargets, label_distance, label_distance_torch  # noqa: E402

pytestmark = pytest.mark.gpu

FLOATS = ("e_m2i", "e_i2m", "d2_v", "d2_p", "proj")


def dev():
    return torch.device("cuda:0")


def t(a, dtype=torch.float32):
    return torch.as_tensor(np.asarray(a), dtype=dtype).to(dev())


def bits(a):
    return a.detach().contiguous().view(torch.int32)


def cotangents(p, seed=5):
    B, V, W = p["verts"].shape[0], p["verts"].shape[1], p["W"]
    rng = np.random.default_rng(seed)
    return rng.normal(size=(B, V)).astype(np.float32), rng.normal(size=(B, W, W)).astype(np.float32)


def run(p, sigma, slack, g=None, rows=None, flip_rows=True):
    """The op on the device for problem p (rows: a list of row indices, None = all) -> dict of every output and, with the
    cotangents g = (g_v, g_p), of dverts and dcam, all device tensors."""
    sel = (lambda a: a) if rows is None else (lambda a: None if a is None else a[rows])
    verts, cam = t(sel(p["verts"])), t(sel(p["cam"]))
    if g is not None:
        verts.requires_grad_(True)
        cam.requires_grad_(True)
    spec = LabelDistanceSpec(p["vclass"], p["C"])
    targets = LabelTargets(t(sel(p["labels"]), torch.int32), p["C"], flip_rows=flip_rows)
    vw = None if p["vweight"] is None else t(sel(p["vweight"]))
    (e_v, e_p), det = label_distance(verts, cam, spec, targets, vw, sigma, slack, return_details=True)
    out = dict(det, e_m2i=e_v.detach(), e_i2m=e_p.detach())
    if g is not None:
        torch.autograd.backward([e_v, e_p], [t(sel(g[0])), t(sel(g[1]))])
        out.update(dverts=verts.grad, dcam=cam.grad)
    torch.cuda.synchronize()
    return out


def host(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def same_bits(a, b, rows_a=None, rows_b=None):
    for k in a:
        x = a[k] if rows_a is None else a[k][rows_a]
        y = b[k] if rows_b is None else b[k][rows_b]
        assert torch.equal(bits(x) if x.is_floating_point() else x, bits(y) if y.is_floating_point() else y), k


def check(p, out, sigma, slack, g=None, flip_rows=True):
    fw, gr = cases.reference(p, sigma, slack, flip_rows, *(g if g is not None else (None, None)))
    h = host(out)
    return cases.compare(h, fw, gr, (h["dverts"], h["dcam"]) if g is not None else None), fw


# ---- values and gradients --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("C", [2, 32])
@pytest.mark.parametrize("W", [1, 7, 48])
@pytest.mark.parametrize("V", [1, 65, 257, 600])
@pytest.mark.parametrize("B", [1, 3])
def test_small_shapes_against_the_oracle(B, V, W, C):
    """Every combination, each with and without sigma and at slack 0 and 0.5; the problem holds the zero and NaN weights,
    the vertices outside the image, the don't-care labels, the absent classes and - B = 3 - the all-background image.  The
    same runs: two launches give the same bits, and a row alone gives the bits it has in the batch."""
    p = cases.problem(B, V, W, C, seed=2)
    g = cotangents(p)
    worst = 0.0
    for sigma in (None, 3.0):
        for slack in (0.0, 0.5):
            out = run(p, sigma, slack, g)
            worst = max(worst, check(p, out, sigma, slack, g)[0])
            assert (out["dverts"][:, :, 2] == 0).all()
    print("worst error / bar: %.3g" % worst)
    again = run(p, 3.0, 0.5, g)
    same_bits(out, again)
    if B > 1:
        for b in range(B):
            same_bits(run(p, 3.0, 0.5, g, rows=[b]), out, None, slice(b, b + 1))


def test_the_named_cases_are_in_the_runs():
    """What `test_small_shapes_against_the_oracle` relies on its generator for, asserted: a class of exactly 256 and one of
    257 vertices, a class of vertices absent from the image, a class of pixels without a counted vertex, weights 0 and NaN,
    vertices outside the image, labels -1, C and 255, an all-background image; and exact ties in both directions, which go to
    the lower index on the device as in the oracle."""
    p = cases.problem(3, 600, 48, 32, seed=2)
    counts = np.bincount(p["vclass"][(p["vclass"] >= 1) & (p["vclass"] < 32)], minlength=32)
    assert counts[1] == 256 and counts[2] == 257
    lab, w = p["labels"], p["vweight"]
    assert counts[31] > 0 and not (lab == 31).any()
    assert (lab[0] == 1).any() and not (w[0, p["vclass"] == 1] > 0).any()
    assert (w == 0).any() and np.isnan(w).any()
    for val in (-1, 32, 255):
        assert (lab == val).any()
    assert not ((lab[2] >= 1) & (lab[2] < 32)).any() and (lab[2] == 0).any()
    proj = p["cam"][:, None, 2:] + p["cam"][:, None, :2] * p["verts"][:, :, :2]
    assert (proj < -1).any() and (proj > 48).any()
    out = run(p, None, 0.5)
    _, fw = check(p, out, None, 0.5)
    assert sum(f["ties"][0] for f in fw) > 0 and sum(f["ties"][1] for f in fw) > 0
    h = host(out)
    # (equal to the oracle's np.argmin, and by the definition itself: no lower candidate of the class is as close)
    pts = orc.points(48)
    for b in range(2):
        f, lb = fw[b], lab[b].reshape(-1)
        for i in np.nonzero(f["near_pix"] >= 0)[0][::7]:
            q = int(h["near_pix"][b, i])
            lower = np.nonzero(lb[:q] == p["vclass"][i])[0]
            assert (((f["proj"][i] - pts[lower]) ** 2).sum(1) > f["d2_v"][i]).all()
        nv = h["near_vert"][b].reshape(-1)
        for q in np.nonzero(nv >= 0)[0][::5]:
            lower = np.nonzero((p["vclass"][:nv[q]] == lb[q]) & f["counted"][:nv[q]])[0]
            assert (((f["proj"][lower] - pts[q]) ** 2).sum(1) > f["d2_p"][q]).all()
    assert (h["near_vert"][2] == -1).all() and (h["e_i2m"][2] == 0).all() and (h["near_pix"][2] == -1).all()


def test_single_directions_and_unflipped_rows():
    p = cases.problem(3, 257, 7, 32, seed=3)
    both = run(p, 3.0, 0.5)
    verts, cam = t(p["verts"]).requires_grad_(True), t(p["cam"]).requires_grad_(True)
    spec, targets, vw = LabelDistanceSpec(p["vclass"], 32), LabelTargets(t(p["labels"], torch.int32), 32), t(p["vweight"])
    g = cotangents(p)
    for d, e_key, keys, gi in (("m2i", "e_m2i", ("near_pix", "d2_v"), 0), ("i2m", "e_i2m", ("near_vert", "d2_p"), 1)):
        e, det = label_distance(verts, cam, spec, targets, vw, 3.0, 0.5, directions=d, return_details=True)
        assert torch.equal(bits(e), bits(both[e_key])) and torch.equal(det[keys[0]], both[keys[0]])
        assert torch.equal(bits(det[keys[1]]), bits(both[keys[1]])) and torch.equal(bits(det["proj"]), bits(both["proj"]))
        verts.grad = cam.grad = None
        e.backward(t(g[gi]))
        fw, gr = cases.reference(p, 3.0, 0.5, True, *(g[0] if gi == 0 else None, g[1] if gi == 1 else None))
        cases.compare({"status": det["status"].cpu().numpy()}, fw, gr, (verts.grad.cpu().numpy(), cam.grad.cpu().numpy()))
    out = run(p, None, 0.0, g, flip_rows=False)
    check(p, out, None, 0.0, g, flip_rows=False)


def test_width_160():
    p = cases.problem(1, 600, 160, 2, seed=4)
    g = cotangents(p)
    out = run(p, 8.0, 0.5, g)
    worst, fw = check(p, out, 8.0, 0.5, g)
    assert (fw[0]["near_pix"] >= 0).sum() > 100 and (fw[0]["near_vert"] >= 0).sum() > 5000
    print("W = 160: worst error / bar %.3g" % worst)
    same_bits(out, run(p, 8.0, 0.5, g))


@pytest.fixture(scope="module")
def full_case(smpl_model):
    """V = 6 890, W = 48, B = 4: labels = the arg-max of the decoder's scores at x*, vertices of x* perturbed; the decoder's
    mask == 1 as vweight."""
    from _inputs import make_x
    from ilps_amd.decoder import SMPLDecoder
    from ilps_amd.smpl_model import load_part_tables
    from ilps_amd.render import vertex_parts
    dec = SMPLDecoder(smpl_model, img_wh=48)
    xs = make_x(4, 48, seed=3)
    x0 = xs.copy()
    rng = np.random.default_rng(9)
    x0[:, 2:4] += rng.choice([-5.0, 5.0], (4, 2)).astype(np.float32)
    x0[:, 4:76] += rng.normal(0, 0.1, (4, 72)).astype(np.float32)
    with torch.no_grad():
        labels = dec(t(xs))["seg"].argmax(-1).to(torch.int32)
        o = dec(t(x0))
    vclass = (vertex_parts(load_part_tables(1), 6890) + 1).astype(np.int32)
    return dict(verts=o["verts"].cpu().numpy(), cam=x0[:, :4].copy(), vweight=(o["mask"] == 1).float().cpu().numpy(),
                labels=labels.cpu().numpy(), vclass=vclass, C=32, W=48)


def test_full_size_against_the_oracle(full_case):
    p = full_case
    g = cotangents(p)
    out = run(p, 8.0, 0.5, g)
    worst, fw = check(p, out, 8.0, 0.5, g)
    assert all(f["status"] == 0 for f in fw) and min((f["near_pix"] >= 0).sum() for f in fw) > 100
    print("full size: worst error / bar %.3g" % worst)
    same_bits(out, run(p, 8.0, 0.5, g))
    same_bits(run(p, 8.0, 0.5, g, rows=[2]), out, None, slice(2, 3))


def test_prep_launch_is_the_stable_sort():
    p = cases.problem(3, 65, 48, 32, seed=4)
    for W, C in ((48, 32), (7, 2), (1, 2)):
        lab = p["labels"][:, :W, :W].copy()
        tg = LabelTargets(t(lab, torch.int32), C)
        tg2 = LabelTargets(t(lab, torch.int32), C)
        assert torch.equal(tg.off, tg2.off) and torch.equal(tg.pix, tg2.pix)
        for b in range(3):
            off, pix = orc.prep(lab[b], C)
            assert np.array_equal(tg.off[b].cpu().numpy(), off) and np.array_equal(tg.pix[b].cpu().numpy(), pix)
    big = np.random.default_rng(0).integers(-2, 34, (2, 160, 160))
    tg = LabelTargets(t(big, torch.int64), 32)
    for b in range(2):
        off, pix = orc.prep(big[b], 32)
        assert np.array_equal(tg.off[b].cpu().numpy(), off) and np.array_equal(tg.pix[b].cpu().numpy(), pix)


# ---- hostile rows ----------------------------------------------------------------------------------------------------------

def test_hostile_rows_leave_their_neighbours_alone():
    p = cases.problem(3, 257, 7, 32, seed=6)
    g = cotangents(p)
    clean = run(p, 3.0, 0.5, g)
    counted = (p["vclass"] >= 1) & (p["vclass"] < 32) & (p["vweight"][1] > 0)
    i_c, i_u = int(np.nonzero(counted)[0][0]), int(np.nonzero(~counted)[0][0])

    def variant(edit):
        q = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in p.items()}
        edit(q)
        return q, run(q, 3.0, 0.5, g)
    for edit in (lambda q: q["verts"].__setitem__((1, i_c, 0), np.nan), lambda q: q["verts"].__setitem__((1, i_c, 1), np.inf),
                 lambda q: q["cam"].__setitem__((1, 3), np.inf)):
        q, out = variant(edit)
        assert out["status"].tolist() == [0, 1, 0]
        assert (out["near_pix"][1] == -1).all() and (out["near_vert"][1] == -1).all()
        for k in FLOATS + ("dverts", "dcam"):
            assert torch.isnan(out[k][1]).all(), k
        same_bits(out, clean, [0, 2], [0, 2])
        check(q, out, 3.0, 0.5, g)
    # a NaN in a vertex that is not counted, and in Z of one that is, does nothing (but to that vertex's own proj)
    q, out = variant(lambda q: (q["verts"].__setitem__((1, i_u, 0), np.nan), q["verts"].__setitem__((1, i_c, 2), np.nan)))
    assert out["status"].tolist() == [0, 0, 0] and torch.isnan(out["proj"][1, i_u, 0])
    out["proj"][1, i_u, 0] = clean["proj"][1, i_u, 0]
    same_bits(out, clean)
    # a row whose vweight is all 0: zero outputs, zero gradients
    q, out = variant(lambda q: q["vweight"].__setitem__(1, 0.0))
    assert out["status"].tolist() == [0, 0, 0]
    for k in ("e_m2i", "e_i2m", "dverts", "dcam"):
        assert (out[k][1] == 0).all(), k
    assert (out["near_pix"][1] == -1).all() and (out["near_vert"][1] == -1).all()
    same_bits(out, clean, [0, 2], [0, 2])


# ---- the chain through SMPLLayer -------------------------------------------------------------------------------------------

def test_chain_through_the_smpl_layer(smpl_model, full_case):
    """d (sum g_v e_m2i + sum g_p e_i2m) / dx through SMPLLayer -> label_distance (cam = x[:, :4]) against the float64 SMPL
    oracle chained with float64 autograd of `label_distance_torch`, under test_gpu_parity's `grad_close` bars per column
    block."""
    from _inputs import make_x
    from oracle.torch_oracle import TorchSMPL
    from test_gpu_parity import grad_close
    from ilps_amd.keras_smpl.batch_smpl import SMPLLayer
    layer = SMPLLayer(smpl_model)
    B = 3
    x = make_x(4, 48, seed=3)[:B]
    x[:, 2:4] += 3.0
    rng = np.random.default_rng(6)
    g_v, g_p = rng.uniform(0.5, 1.5, (B, 6890)).astype(np.float32), rng.uniform(0.5, 1.5, (B, 48, 48)).astype(np.float32)
    spec = LabelDistanceSpec(full_case["vclass"], 32)
    lab = full_case["labels"][:B]
    xo = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    o = label_distance_torch(TorchSMPL(smpl_model)(xo), xo[:, :4], spec, LabelTargets(torch.tensor(lab), 32), None, 8.0, 0.5)
    (o["e_m2i"] * torch.tensor(g_v, dtype=torch.float64)).sum().add((o["e_i2m"] * torch.tensor(g_p, dtype=torch.float64)).sum()).backward()
    xg = t(x).requires_grad_(True)
    (e_v, e_p), det = label_distance(layer(xg), xg[:, :4], spec, LabelTargets(t(lab, torch.int32), 32), None, 8.0, 0.5,
                                     return_details=True)
    torch.autograd.backward([e_v, e_p], [t(g_v), t(g_p)])
    assert det["status"].cpu().tolist() == [0] * B
    agree = (det["near_pix"].cpu() == o["near_pix"]).float().mean()
    print("winners shared with the float64 chain: %.5f" % float(agree))
    got, want = xg.grad.cpu().numpy(), xo.grad.numpy()
    np.testing.assert_allclose(e_v.detach().cpu().numpy().sum(1), o["e_m2i"].detach().numpy().sum(1), rtol=2e-3)
    grad_close(got[:, :4], want[:, :4], name="dcam")
    grad_close(got[:, 4:76], want[:, 4:76], name="dtheta")
    grad_close(got[:, 76:], want[:, 76:], name="dbeta")


# ---- ParamFitter -----------------------------------------------------------------------------------------------------------

def load_fit_time():
    import importlib.util
    s = importlib.util.spec_from_file_location("fit_time", os.path.join(ROOT, "tools", "fit_time.py"))
    fit_time = importlib.util.module_from_spec(s)
    s.loader.exec_module(fit_time)
    return fit_time


@pytest.fixture(scope="module")
def fit_case(smpl_model):
    """A LabelDistanceFitter with all three side terms - penetration over test_gpu_scan's soup, test_gpu_keypoints' mixed keypoint
    spec, label distance with sigma = 8 px - and a plain one, on fit_time's problem (B = 3)."""
    from test_gpu_keypoints import mixed_spec
    from test_gpu_scan import body_topology
    from ilps_amd.fitting import LabelDistanceFitter, ParamFitter
    from ilps_amd.keypoints import keypoint_energy
    kspec = mixed_spec(smpl_model)
    fitter = LabelDistanceFitter(smpl_model, img_wh=48, deterministic=True, penetration=body_topology()[0], keypoints=kspec,
                                 kp_sigma=3.0, label_distance=True, ld_sigma=8.0)
    plain = ParamFitter(smpl_model, img_wh=48, deterministic=True)
    labels, x0, xs = load_fit_time().problem(plain, 3, 48, seed=0, pose_sigma=0.05, cam_shift=1.5)
    with torch.no_grad():
        out = fitter.decoder(xs)
        K = kspec.K
        _, det = keypoint_energy(out["verts"], xs[:, :4].contiguous(), kspec, torch.zeros((3, K, 2), device=dev()),
                                 torch.ones((3, K), device=dev()), None, out["J_transformed"], return_details=True)
    conf = torch.linspace(0.3, 1.0, 3 * K, device=dev()).reshape(3, K).clone()
    return fitter, plain, labels, x0, (det["proj"].clone(), conf)


def test_param_fitter_one_iteration_is_the_hand_written_composition(fit_case):
    """All three side terms, in their order: penetration, keypoints, label distance - in the list `autograd.grad`
    accumulates over and in the sum of the loss's columns."""
    from ilps_amd.fitting import FitState, fit_step
    from ilps_amd.keypoints import keypoint_energy
    from ilps_amd.penetration import self_penetration
    fitter, _, labels, x0, kp = fit_case
    wp, wk, wl, B, N, V, K = 30.0, 0.5, 0.25, 3, 48 * 48, 6890, fitter.kp_spec.K
    kw = dict(pen_weight=wp, keypoints=kp, kp_weight=wk, ld_weight=wl)
    r = fitter.fit(labels, init=x0, steps=1, lr=1e-2, history=True, **kw)
    state = FitState.new(x0)
    x = state.x.detach().requires_grad_(True)
    lab = labels.to(torch.int32).reshape(B, 48, 48)
    out = fitter.decoder(x, lab)
    e_pen = self_penetration(out["verts"], fitter.pen_topo, fitter.pen_collide)
    e_kp = keypoint_energy(out["verts"], x[:, :4], fitter.kp_spec, kp[0], kp[1], 3.0, out["J_transformed"])
    e_v, e_p = label_distance(out["verts"], x[:, :4], fitter.ld_spec, LabelTargets(lab, 32), None, 8.0, 0.5)
    e_ld = torch.cat([e_v, e_p.reshape(B, N)], 1)
    assert float(e_pen.detach().sum()) > 0 and float(e_kp.detach().sum()) > 0 and float(e_v.detach().sum()) > 0 \
        and float(e_p.detach().sum()) > 0
    f32 = lambda n, val: torch.full((B, n), val, device=dev())
    (g,) = torch.autograd.grad([out["seg_loss"], e_pen, e_kp, e_ld], [x],
                               grad_outputs=[f32(N, 1.0 / N), f32(V, wp / V), f32(K, wk / K), f32(V + N, wl / (V + N))])
    loss = out["seg_loss"].detach()
    for w, e in ((wp, e_pen), (wk, e_kp), (wl, e_ld)):
        loss = loss + (torch.full((1,), w, device=dev()) * e.detach().mean(1))[:, None]
    hist = torch.empty((1, B), device=dev())
    fit_step(state, g.contiguous(), loss, None, 1.0, None, hist, lr=1e-2)
    assert torch.equal(bits(r.final_x), bits(state.x)) and torch.equal(bits(r.history), bits(hist))
    assert torch.equal(bits(r.loss), bits(state.best_loss)) and torch.equal(bits(r.state.m), bits(state.m))
    assert not torch.equal(r.final_x, x0)
    assert torch.equal(bits(fitter.losses(x0, labels, **kw)), bits(hist[0]))


def test_param_fitter_replay_stage_weights_and_weight_zero(fit_case, smpl_model):
    from ilps_amd.fitting import LabelDistanceFitter, column_scale
    fitter, plain, labels, x0, kp = fit_case
    cs = column_scale(cam=10.0, pose=1.0, shape=0.0)
    kw = dict(init=x0, stages=[(3, cs), (4, cs)], lr=1e-2, history=True, pen_weight=[0.0, 30.0], keypoints=kp, kp_weight=[0.5, 0.0])
    a = fitter.fit(labels, ld_weight=[0.0, 0.5], **kw)
    b = fitter.fit(labels, ld_weight=[0.0, 0.5], graph=True, graph_steps=2, **kw)
    assert a.steps == b.steps == 7
    for k in ("final_x", "history", "x", "loss"):
        assert torch.equal(bits(getattr(a, k)), bits(getattr(b, k))), k
    assert torch.equal(a.step, b.step) and torch.equal(bits(a.state.m), bits(b.state.m))
    # the weights take effect under replay: another second-stage weight changes the second stage's losses only
    c = fitter.fit(labels, ld_weight=[0.0, 0.125], graph=True, graph_steps=2, **kw)
    assert torch.equal(bits(c.history[:3]), bits(b.history[:3])) and (c.history[3] < b.history[3]).all()
    # weight 0: the loss a fitter built without the term records, plus zero - the same bits at the same x
    only = LabelDistanceFitter(smpl_model, img_wh=48, deterministic=True, label_distance=True, ld_sigma=8.0)
    z = only.fit(labels, init=x0, steps=2, lr=1e-2, history=True, ld_weight=0.0)
    q = plain.fit(labels, init=x0, steps=2, lr=1e-2, history=True)
    assert torch.equal(bits(z.history[0]), bits(q.history[0]))
    assert torch.equal(bits(only.losses(x0, labels, ld_weight=0.0)), bits(q.history[0]))
    one = only.fit(labels, init=x0, steps=2, lr=1e-2, history=True, ld_weight=1.0)
    assert torch.equal(bits(only.losses(x0, labels)), bits(one.history[0])) and (one.history[0] > q.history[0]).all()
    with pytest.raises(ValueError, match="ld_weight lists"):
        fitter.fit(labels, ld_weight=[1.0], **kw)
    with pytest.raises(TypeError):                                  # (`ParamFitter.fit` keeps its signature)
        plain.fit(labels, init=x0, steps=1, ld_weight=1.0)
    with pytest.raises(ValueError, match="ld_weight goes with"):
        LabelDistanceFitter(smpl_model, img_wh=48, label_distance=None).fit(labels, init=x0, steps=1, ld_weight=1.0)
    with pytest.raises(TypeError):
        only.fit(labels, init=x0, stepz=1)


def test_param_fitter_visible_weights_follow_the_mask(smpl_model, fit_case):
    from ilps_amd.fitting import LabelDistanceFitter
    _, _, labels, x0, _ = fit_case
    vis = LabelDistanceFitter(smpl_model, img_wh=48, deterministic=True, label_distance="visible", ld_directions="m2i")
    r = vis.fit(labels, init=x0, steps=1, lr=1e-2, history=True, ld_weight=0.5)
    with torch.no_grad():
        lab = labels.to(torch.int32).reshape(3, 48, 48)
        out = vis.decoder(x0, lab)
        e = label_distance(out["verts"], x0[:, :4].contiguous(), vis.ld_spec, LabelTargets(lab, 32),
                           (out["mask"] == 1).float(), None, 0.5, "m2i")
        assert 0 < int((out["mask"] == 1).sum()) < out["mask"].numel()
        loss = out["seg_loss"] + (torch.full((1,), 0.5, device=dev()) * e.mean(1))[:, None]
    np.testing.assert_allclose(r.history[0].cpu().numpy(), loss.mean(1).cpu().numpy(), rtol=1e-5)


def test_the_term_brings_a_shifted_camera_home(smpl_model):
    """fit_time's problem with the camera 12 px off in both axes and no pose noise, only the two translation columns free.
    With the term every row's translation error ends below where it started; the plain fit's end error is printed beside it
    (no claim is made about it)."""
    from ilps_amd.fitting import LabelDistanceFitter, ParamFitter
    with_ld = LabelDistanceFitter(smpl_model, img_wh=48, deterministic=True, label_distance=True)
    plain = ParamFitter(smpl_model, img_wh=48, deterministic=True)
    labels, x0, xs = load_fit_time().problem(plain, 3, 48, seed=0, pose_sigma=0.0, cam_shift=12.0)
    cs = torch.zeros(86)
    cs[2:4] = 1.0
    kw = dict(init=x0, stages=[(150, cs)], lr=0.2)
    err = lambda x: (x[:, 2:4] - xs[:, 2:4]).norm(dim=1)
    a = with_ld.fit(labels, ld_weight=1.0, **kw)
    b = plain.fit(labels, **kw)
    start, end_ld, end_plain = err(x0), err(a.final_x), err(b.final_x)
    print("translation error in px: start %s, with the term %s, without %s"
          % tuple([round(v, 3) for v in e.tolist()] for e in (start, end_ld, end_plain)))
    assert (end_ld < start).all()
