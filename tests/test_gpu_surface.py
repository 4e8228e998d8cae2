"""The dense surface-correspondence term on the GPU (csrc/surface.hip through ilps_amd/surface.py) against
tests/_surface_oracle.py under its rounding bar |got - want| <= 2^-24 |want| + 2^-28 T: small shapes (D in {2, 3}, B in {1, 3},
N in {1, 63, 64, 65, 257}, three topologies, four layouts of the correspondences, with and without the robust function), one
full-size case, bit-equality between launches and between a row alone and inside a batch, permuted rows, hostile rows, the
device restatement, the chain through `SMPLLayer`, and the fitters.  Every comparison prints the worst error-to-bar ratio."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _surface_oracle as orc  # noqa: E402
from test_surface_cpu import CASES, TOPOLOGIES, check_bar, oracle_row, problem, take, tens  # noqa: E402
from ilps_amd.render import MeshTopology  # noqa: E402
from ilps_amd.surface import SurfaceTargets, correspondences_from_render, surface_energy, surface_energy_torch  # noqa: E402

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda:0")


def t(a, dtype=torch.float32):
    return torch.as_tensor(np.asarray(a), dtype=dtype).to(dev())


def bits(a):
    return a.detach().contiguous().view(torch.int32)


def run(p, sigma, g=None, rows=None):
    """The op on the device for problem p (rows: a list of row indices, None = all) -> (e, details, dverts, dcam), the
    gradients for the cotangent g (B, N) numpy (None: no backward)."""
    q = p if rows is None else take(p, rows)
    verts, cam, targets = tens(q, dev(), grad=g is not None)
    e, det = surface_energy(verts, cam, targets, sigma, return_details=True)
    if g is None:
        return e, det, None, None
    e.backward(t(g if rows is None else g[rows]))
    torch.cuda.synchronize()
    return e.detach(), det, verts.grad, None if cam is None else cam.grad


def check_against_oracle(p, sigma, e, det, dverts, dcam, g, refs=None):
    """Every output of every row against the oracle under the bar -> the worst ratio.  refs: the rows' (forward, grads)
    dicts when the caller has them already."""
    B, worst = p["verts"].shape[0], 0.0
    assert det["status"].cpu().tolist() == [0] * B
    for b in range(B):
        fw, gr = oracle_row(p, b, sigma, g) if refs is None else refs[b]
        worst = max(worst, check_bar(e[b].cpu().numpy(), fw["e"], fw["T_e"], "e"),
                    check_bar(det["d2"][b].cpu().numpy(), fw["d2"], fw["T_d2"], "d2"),
                    check_bar(det["point"][b].cpu().numpy(), fw["point"], fw["T_point"], "point"),
                    check_bar(dverts[b].cpu().numpy(), gr["dverts"], gr["T_dverts"], "dverts"))
        if dcam is not None:
            worst = max(worst, check_bar(dcam[b].cpu().numpy(), gr["dcam"], gr["T_dcam"], "dcam"))
            assert (dverts[b, :, 2] == 0).all()
        assert (bits(e[b])[torch.as_tensor(~fw["counted"]).to(dev())] == 0).all()       # exactly 0 where nothing counts
        untouched = ~(fw["A"] != 0).any(0)
        assert (bits(dverts[b])[torch.as_tensor(untouched).to(dev())] == 0).all()       # exact zeros where nothing lands
    return worst


# ---- values and gradients --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("D", [2, 3])
def test_small_shapes_against_the_oracle(D, B, N):
    worst = 0.0
    for kind in TOPOLOGIES:
        for case in CASES:
            p = problem(B, kind, N, D, case, seed=B + N + D)
            g = np.random.default_rng(N).normal(size=(B, N)).astype(np.float32)
            for sigma in (None, 3.0):
                out = run(p, sigma, g)
                worst = max(worst, check_against_oracle(p, sigma, *out, g))
            if B == 3:                                          # the row that is all padding: zeros in every bit, status 0
                e, det, dverts, dcam = out
                assert (bits(e[1]) == 0).all() and (bits(dverts[1]) == 0).all() and int(det["status"][1]) == 0
                assert dcam is None or (bits(dcam[1]) == 0).all()
            if case == "corner" and kind != "tri":              # bary = (1, 0, 0): the other corners get exact +-0
                f = p["faces"]
                never_first = np.setdiff1d(f[:, 1:].reshape(-1), f[:, 0])               # vertices that are no face's corner 0
                assert len(never_first) and (out[2][:, torch.as_tensor(never_first).to(dev())] == 0).all()
            if N >= 63 and case == "random":                    # residuals on both sides of sigma, some entries uncounted
                d2 = out[1]["d2"].cpu().numpy()[(p["conf"] > 0) & (p["face"] >= 0)]
                assert (d2 < 9.0).any() and (d2 > 9.0).any() and np.isnan(p["target"]).any()
    print("D = %d, B = %d, N = %d: worst error / bar over all topologies and cases = %.3g" % (D, B, N, worst))


def full_topology():
    """6 890 vertices, 13 776 seeded faces of distinct, nearby vertices (SMPL's counts; the synthetic model carries no faces)."""
    rng = np.random.default_rng(77)
    a = rng.integers(0, 6890, 13776)
    f = np.stack([a, (a + rng.integers(1, 40, 13776)) % 6890, (a + rng.integers(40, 80, 13776)) % 6890], 1).astype(np.int32)
    return MeshTopology(f, 6890), f


@pytest.fixture(scope="module")
def full_case(smpl_model):
    """V = 6 890, F = 13 776, B = 3, N = 4 096 with correspondences from `scan.sample_surface`, image targets on both sides
    of sigma; the oracle's rows for one cotangent, computed once."""
    from ilps_amd.scan import sample_surface
    topo, f = full_topology()
    rng = np.random.default_rng(9)
    B, V, N = 3, 6890, 4096
    verts = (np.asarray(smpl_model.v_template, np.float32).reshape(1, V, 3) + rng.normal(0, 0.01, (B, V, 3))).astype(np.float32)
    cam = np.stack([rng.uniform(18, 24, B), rng.uniform(18, 24, B), rng.uniform(20, 28, B), rng.uniform(20, 28, B)], 1).astype(np.float32)
    gen = torch.Generator(device=dev())
    gen.manual_seed(3)
    pts, face, bary = sample_surface(t(verts), topo, N, generator=gen)
    face, bary = face.cpu().numpy().astype(np.int32), bary.cpu().numpy().astype(np.float32)
    face[2, 4000:] = -1                                          # a ragged row
    proj = np.stack([cam[:, 2, None] + cam[:, 0, None] * pts.cpu().numpy()[..., 0],
                     cam[:, 3, None] + cam[:, 1, None] * pts.cpu().numpy()[..., 1]], -1)
    far = rng.uniform(size=(B, N, 1)) < 0.5
    off = np.where(far, rng.uniform(4.0, 9.0, (B, N, 2)), rng.uniform(0.1, 1.5, (B, N, 2))) * rng.choice([-1.0, 1.0], (B, N, 2))
    conf = rng.uniform(0.2, 1.0, (B, N)).astype(np.float32)
    conf[:, ::7] = 0.0
    p = dict(faces=f, V=V, verts=verts, cam=cam, face=face, bary=bary, target=(proj + off).astype(np.float32), conf=conf)
    g = rng.normal(size=(B, N)).astype(np.float32)
    refs = []
    for b in range(B):
        fw, gr = oracle_row(p, b, 3.0, g)
        fw["A"] = (fw["A"] != 0).any(0)[None]                    # (what the checks read of the two dense (N, V) matrices,
        del fw["W"]                                              # 226 MB each: they are not kept)
        refs.append((fw, gr))
    return p, g, refs


def test_full_size_against_the_oracle(full_case):
    p, g, refs = full_case
    out = run(p, 3.0, g)
    worst = check_against_oracle(p, 3.0, *out, g, refs=refs)
    print("full size: worst error / bar = %.3g" % worst)
    assert (out[2] != 0).any(2).sum(1).min() > 3000             # (the gradient reaches most of the mesh)


def test_launches_repeat_and_a_row_does_not_see_its_batch(full_case):
    p, g, _ = full_case
    a, b = run(p, 3.0, g), run(p, 3.0, g)
    flat = lambda o: [o[0], o[1]["d2"], o[1]["point"], o[2], o[3]]
    for x, y in zip(flat(a), flat(b)):
        assert torch.equal(bits(x), bits(y))
    for row in (0, 2):
        alone = run(p, 3.0, g, rows=[row])
        for x, y in zip(flat(a), flat(alone)):
            assert torch.equal(bits(x[row]), bits(y[0]))
        assert int(alone[1]["status"][0]) == 0


def test_permuting_a_row_permutes_e_and_keeps_the_gradient_within_the_bar(full_case):
    """The caller's order of a row's correspondences is not the kernels' order: e follows the permutation bit for bit (each
    entry is computed alone); dverts and dcam are sums over the row in SORTED order, where a stable sort keeps the caller's
    order among the correspondences of one face - so their bits MAY differ between the two orders, and both are held to the
    oracle's bar instead."""
    p, g, refs = full_case
    perm = np.random.default_rng(4).permutation(p["face"].shape[1])
    q = dict(p, **{k: p[k][:, perm] for k in ("face", "bary", "target", "conf")})
    a, b = run(p, 3.0, g), run(q, 3.0, g[:, perm])
    assert torch.equal(bits(a[0][:, torch.as_tensor(perm).to(dev())]), bits(b[0]))
    worst = 0.0
    for r in range(3):
        gr = refs[r][1]
        worst = max(worst, check_bar(b[2][r].cpu().numpy(), gr["dverts"], gr["T_dverts"], "dverts (permuted)"),
                    check_bar(b[3][r].cpu().numpy(), gr["dcam"], gr["T_dcam"], "dcam (permuted)"))
    print("permuted rows: worst error / bar = %.3g; dverts bits equal: %s" % (worst, bool(torch.equal(bits(a[2]), bits(b[2])))))


@pytest.mark.parametrize("D", [2, 3])
def test_hostile_rows(D):
    B, N = 7, 65
    p = problem(B, "v65", N, D, "perface", seed=4)
    f = p["faces"]
    p["conf"][:, :8] = 1.0
    p["target"][:, :8] = 1.0
    p["conf"][:, 9] = 0.0
    p["conf"][:, 20], p["target"][:, 20] = 0.7, 1.0
    g = np.ones((B, N), np.float32)
    clean = run(p, 3.0, g)
    h = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in p.items()}
    h["verts"][0, f[2, 1], 1] = np.nan                          # row 0: a NaN vertex under a counted correspondence -> status
    lone = [n for n in range(N) if n != 9 and f[9, 0] in f[n]]
    h["conf"][1, lone] = 0.0
    c1 = run(take(h, [1]), 3.0, g[[1]])                         # (row 1 with those confidences, before the NaN)
    h["verts"][1, f[9, 0], 0] = np.nan                          # row 1: a NaN vertex only uncounted ones use -> nothing
    h["verts"][1, 62, 2] = np.inf                               # ... and one in no face at all
    if D == 2:
        h["cam"][2, 1] = np.inf                                 # row 2: an Inf cam column -> status
    else:
        h["bary"][2, 3, 2] = np.inf                             # (D = 3 has no camera: an Inf weight under conf > 0)
    h["target"][3, 9, 0] = np.nan                               # row 3: a NaN target under conf 0 -> harmless
    h["target"][4, 1, 1] = np.nan                               # row 4: a NaN target under conf > 0 -> status
    h["conf"][5] = 0.0                                          # row 5: nothing counts
    h["conf"][6, 20] = np.nan                                   # row 6: a NaN conf does not count
    e, det, dverts, dcam = run(h, 3.0, g)
    assert det["status"].cpu().tolist() == [1, 0, 1, 0, 1, 0, 0]
    outs = [e, det["d2"], det["point"], dverts] + ([dcam] if D == 2 else [])
    for b in (0, 2, 4):
        for x in outs:
            assert torch.isnan(x[b]).all()
    for x in outs:                                              # status 0: every output finite
        assert torch.isfinite(x[[1, 3, 5, 6]]).all()
    cl = [clean[0], clean[1]["d2"], clean[1]["point"], clean[2]] + ([clean[3]] if D == 2 else [])
    for x, y in zip(outs, cl):                                  # a good row beside hostile ones: the bits of the clean run
        assert torch.equal(bits(x[3]), bits(y[3]))
    for x, y in zip(outs, [c1[0], c1[1]["d2"], c1[1]["point"], c1[2]] + ([c1[3]] if D == 2 else [])):
        assert torch.equal(bits(x[1]), bits(y[0]))              # ... and of the same row run alone, without the NaN
    for x in outs:
        assert (bits(x[5]) == 0).all()
    assert int(bits(e[6])[20]) == 0 and float(clean[0][6, 20]) > 0


def test_device_torch_restatement_agrees(full_case):
    """`surface_energy_torch` on the device - the stock composition tools/surface_time.py times the kernels against -
    computes the same numbers (its float64 sums have their own order: compared under the oracle's bar)."""
    p, g, refs = full_case
    verts, cam, targets = tens(p, dev(), grad=True)
    out = surface_energy_torch(verts, cam, targets, 3.0)
    (out["e"] * t(g, torch.float64)).sum().backward()
    worst = 0.0
    for b in range(3):
        fw, gr = refs[b]
        worst = max(worst, check_bar(out["e"][b].detach().to(torch.float32).cpu().numpy(), fw["e"], fw["T_e"], "torch e"),
                    check_bar(verts.grad[b].cpu().numpy(), gr["dverts"], gr["T_dverts"], "torch dverts"),
                    check_bar(cam.grad[b].cpu().numpy(), gr["dcam"], gr["T_dcam"], "torch dcam"))
    print("device restatement: worst error / bar = %.3g" % worst)


# ---- the chain through SMPLLayer -------------------------------------------------------------------------------------------

def grad_close(a, b, rtol=2e-3, name="", elem_rtol=None, elem_atol=2e-4, per_column=True):
    """tests/test_gpu_parity.py's two bars, as test_gpu_keypoints.py's chain test uses them.  (1) max-norm: max|a-b| <= rtol *
    max|b|.  (2) element-wise: |a-b| <= elem_rtol*|b| + elem_atol*scale, scale the RMS of the reference over the batch axis
    per trailing index (a parameter's own typical size)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, "%s: shapes %s vs %s" % (name, a.shape, b.shape)
    if b.size == 0:
        return
    scale = np.abs(b).max() + 1e-30
    err = np.abs(a - b).max() / scale
    assert err <= rtol, "%s: max|diff|/max|ref| = %.3e > %.1e" % (name, err, rtol)
    er = rtol if elem_rtol is None else elem_rtol
    col = np.sqrt(np.mean(b * b, axis=0, keepdims=True)) if (b.ndim >= 2 and per_column) else np.sqrt(np.mean(b * b))
    col = np.maximum(col, 1e-3 * np.sqrt(np.mean(b * b)) + 1e-30)
    bad = np.abs(a - b) > er * np.abs(b) + elem_atol * col
    assert not bad.any(), "%s: %d of %d entries outside |d| <= %.1e|ref| + %.1e*rms; worst %.3e vs ref %.3e" % (
        name, int(bad.sum()), b.size, er, elem_atol, float(np.abs(a - b)[bad].max()),
        float(np.abs(b)[bad][np.abs(a - b)[bad].argmax()]))


@functools.lru_cache(maxsize=None)
def body_topology():
    """An open triangle soup over the synthetic model's 6 890 vertices (the model carries no faces): consecutive vertices of
    the part tables, three at a time - small faces, each inside one body part."""
    from ilps_amd.smpl_model import load_part_tables
    ids, _ = load_part_tables(1)
    f = np.asarray(ids[:(len(ids) // 3) * 3], np.int32).reshape(-1, 3)
    return MeshTopology(f, 6890)


def test_chain_through_the_smpl_layer(smpl_model):
    """d (sum g e) / dx through SMPLLayer -> surface_energy (cam = x[:, :4]) against the float64 SMPL oracle chained with
    float64 autograd of `surface_energy_torch`, under the bars of test_gpu_keypoints.py's chain test per column block."""
    from _inputs import make_x
    from oracle.torch_oracle import TorchSMPL
    from ilps_amd.keras_smpl.batch_smpl import SMPLLayer
    from ilps_amd.scan import sample_surface
    topo = body_topology()
    layer = SMPLLayer(smpl_model)
    B, N = 3, 600
    x = make_x(B, 48, seed=5)
    rng = np.random.default_rng(6)
    xo = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    vo, _, _ = TorchSMPL(smpl_model)(xo, return_all=True)
    gen = torch.Generator()
    gen.manual_seed(8)
    pts, face, bary = sample_surface(vo.detach().to(torch.float32), topo, N, generator=gen)
    face, bary = face.to(torch.int32), bary.to(torch.float32)
    c = xo.detach()[:, :4]
    p0 = torch.stack([c[:, 2, None] + c[:, 0, None] * pts[..., 0].double(), c[:, 3, None] + c[:, 1, None] * pts[..., 1].double()], -1).numpy()
    target = torch.tensor((p0 + rng.uniform(1.0, 6.0, (B, N, 2)) * rng.choice([-1.0, 1.0], (B, N, 2))).astype(np.float32))
    conf = rng.uniform(0.3, 1.0, (B, N)).astype(np.float32)
    conf[:, ::5] = 0.0
    conf = torch.tensor(conf)
    g = rng.uniform(0.5, 1.5, (B, N)).astype(np.float32)
    eo = surface_energy_torch(vo, xo[:, :4], SurfaceTargets(topo, face, bary, target, conf), 3.0)["e"]
    (eo * torch.tensor(g, dtype=torch.float64)).sum().backward()
    xg = t(x).requires_grad_(True)
    verts = layer(xg)
    targets = SurfaceTargets(topo, face.to(dev()), bary.to(dev()), target.to(dev()), conf.to(dev()))
    e, det = surface_energy(verts, xg[:, :4], targets, 3.0, return_details=True)
    e.backward(t(g))
    assert det["status"].cpu().tolist() == [0] * B
    got, want = xg.grad.cpu().numpy(), xo.grad.numpy()
    np.testing.assert_allclose(e.detach().cpu().numpy(), eo.detach().numpy(), rtol=2e-3, atol=1e-4)
    grad_close(got[:, :4], want[:, :4], name="dcam")
    grad_close(got[:, 4:76], want[:, 4:76], name="dtheta")
    grad_close(got[:, 76:], want[:, 76:], name="dbeta")


# ---- the fitters -----------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def param_case(smpl_model):
    """A `with_surface(ParamFitter)` with the term (the body soup, sigma = 3 px), one without it, labels, a start, and correspondences rendered
    from the parameters the labels were made from."""
    import importlib.util
    from ilps_amd.fitting import ParamFitter, with_surface
    s = importlib.util.spec_from_file_location("fit_time", os.path.join(ROOT, "tools", "fit_time.py"))
    fit_time = importlib.util.module_from_spec(s)
    s.loader.exec_module(fit_time)
    topo = body_topology()
    with_sc = with_surface(ParamFitter)(smpl_model, img_wh=48, deterministic=True, surface=topo, sc_sigma=3.0)
    plain = ParamFitter(smpl_model, img_wh=48, deterministic=True)
    labels, x0, xs = fit_time.problem(plain, 3, 48, seed=0, pose_sigma=0.05, cam_shift=1.5)
    with torch.no_grad():
        verts = with_sc.decoder(xs)["verts"]
    face, bary, target = correspondences_from_render(verts, topo, xs[:, :4].contiguous(), 48)
    assert int((face >= 0).sum(1).min()) >= 20
    conf = torch.linspace(0.3, 1.0, face.numel(), device=dev()).reshape(face.shape).clone()
    conf[:, 5] = 0.0
    return with_sc, plain, labels, x0, SurfaceTargets(topo, face, bary, target, conf)


def test_param_fitter_one_iteration_is_the_hand_written_composition(param_case):
    from ilps_amd.fitting import FitState, fit_step
    fitter, _, labels, x0, tg = param_case
    w, B, NP, N = 0.5, 3, 48 * 48, tg.N
    r = fitter.fit(labels, init=x0, steps=1, lr=1e-2, history=True, surface=tg, sc_weight=w)
    state = FitState.new(x0)
    x = state.x.detach().requires_grad_(True)
    out = fitter.decoder(x, labels.to(torch.int32).reshape(B, 48, 48))
    e = surface_energy(out["verts"], x[:, :4], tg, 3.0)
    assert float(e.detach().sum()) > 0
    (g,) = torch.autograd.grad([out["seg_loss"], e], [x], grad_outputs=[torch.full((B, NP), 1.0 / NP, device=dev()),
                                                                       torch.full((B, N), w / N, device=dev())])
    loss = out["seg_loss"].detach() + (torch.full((1,), w, device=dev()) * e.detach().mean(1))[:, None]
    hist = torch.empty((1, B), device=dev())
    fit_step(state, g.contiguous(), loss, None, 1.0, None, hist, lr=1e-2)
    assert torch.equal(bits(r.final_x), bits(state.x)) and torch.equal(bits(r.history), bits(hist))
    assert torch.equal(bits(r.loss), bits(state.best_loss)) and torch.equal(bits(r.state.m), bits(state.m))
    assert not torch.equal(r.final_x, x0)
    assert torch.equal(bits(fitter.losses(x0, labels, surface=tg, sc_weight=w)), bits(hist[0]))


def test_param_fitter_replay_stage_weights_and_weight_zero(param_case):
    from ilps_amd.fitting import column_scale
    fitter, plain, labels, x0, tg = param_case
    cs = column_scale(cam=10.0, pose=1.0, shape=0.0)
    kw = dict(init=x0, stages=[(5, cs), (6, cs)], lr=1e-2, history=True)
    a = fitter.fit(labels, surface=tg, sc_weight=[0.5, 2.0], **kw)
    b = fitter.fit(labels, surface=tg, sc_weight=[0.5, 2.0], graph=True, graph_steps=2, **kw)
    for k in ("final_x", "history", "x", "loss"):
        assert torch.equal(bits(getattr(a, k)), bits(getattr(b, k))), k
    assert torch.equal(a.step, b.step)
    # the weights take effect under replay: another second-stage weight changes the second stage's losses only
    c = fitter.fit(labels, surface=tg, sc_weight=[0.5, 0.25], graph=True, graph_steps=2, **kw)
    assert torch.equal(bits(c.history[:5]), bits(b.history[:5])) and (c.history[5] < b.history[5]).all()
    # weight 0 in every stage: the term is left out - the launches, and so the bits, of a fitter built without it
    z = fitter.fit(labels, surface=tg, sc_weight=0.0, **kw)
    p = plain.fit(labels, **kw)
    for k in ("final_x", "history", "x", "loss"):
        assert torch.equal(bits(getattr(z, k)), bits(getattr(p, k))), k
    assert torch.equal(bits(fitter.losses(x0, labels, surface=tg, sc_weight=0.0)), bits(plain.losses(x0, labels)))
    with pytest.raises(ValueError, match="sc_weight lists"):
        fitter.fit(labels, surface=tg, sc_weight=[1.0], **kw)


def test_pairing_errors_come_before_any_launch(param_case, smpl_model):
    from ilps_amd.fitting import KeypointFitter, LabelDistanceFitter, ParamFitter, ScanFitter, SurfaceFitter, with_surface
    fitter, plain, labels, x0, tg = param_case
    nowhere = labels.cpu()                                      # (a fit that got as far as its data would refuse these)
    without = with_surface(ParamFitter)(smpl_model, img_wh=48)  # (the class takes the arguments; this fitter has no term)
    with pytest.raises(ValueError, match="go with a fitter built with surface"):
        without.fit(nowhere, sc_weight=1.0)
    with pytest.raises(ValueError, match="go with a fitter built with surface"):
        without.fit(nowhere, surface=tg)
    with pytest.raises(TypeError):
        plain.fit(nowhere, surface=tg)                          # (`ParamFitter.fit` keeps its signature)
    with pytest.raises(ValueError, match="pass surface=SurfaceTargets"):
        fitter.fit(nowhere)
    with pytest.raises(ValueError, match="pass surface=SurfaceTargets"):
        fitter.losses(x0, nowhere)
    with pytest.raises(ValueError, match="sc_sigma goes with"):
        with_surface(ParamFitter)(smpl_model, sc_sigma=3.0)
    topo = body_topology()
    scan = with_surface(ScanFitter)(smpl_model, topo, surface=True)
    with pytest.raises(ValueError, match="D in"):               # markers are 3D: image targets are refused
        scan.fit(torch.zeros((3, 10, 3), device=dev()), surface=tg, steps=1)
    assert with_surface(KeypointFitter)(smpl_model, surface=topo)._sc is not None
    assert with_surface(LabelDistanceFitter)(smpl_model, surface=topo, label_distance=None)._sc is not None
    assert with_surface(ParamFitter) is with_surface(ParamFitter) and issubclass(with_surface(ScanFitter), ScanFitter)
    with pytest.raises(TypeError):
        with_surface(SurfaceFitter)


@pytest.fixture(scope="module")
def sc_fit_case(smpl_model):
    """SurfaceFitter over the body soup, sigma = 6 px, B = 4, W = 48: correspondences rendered from the true bodies, the start
    perturbed."""
    from ilps_amd.fitting import SurfaceFitter
    topo = body_topology()
    fitter = SurfaceFitter(smpl_model, topo=topo, sigma=6.0, img_wh=48)
    B = 4
    rng = np.random.default_rng(12)
    xs = fitter.initial(B, device=dev())
    d = np.zeros((B, 86), np.float32)
    d[:, 2:4] = rng.normal(0, 1.5, (B, 2))
    d[:, 0:2] = rng.normal(0, 0.5, (B, 2))
    d[:, 4:76] = rng.normal(0, 0.1, (B, 72))
    d[:, 76:] = rng.normal(0, 0.7, (B, 10))
    x0 = xs + t(d)
    with torch.no_grad():
        verts = fitter.layer(xs)
    face, bary, target = correspondences_from_render(verts, topo, xs[:, :4].contiguous(), 48)
    assert int((face >= 0).sum(1).min()) >= 20
    return fitter, SurfaceTargets(topo, face, bary, target), x0


def test_surface_fitter_lowers_the_loss_and_the_pixel_error(sc_fit_case):
    from ilps_amd.evaluation import evaluate_surface
    fitter, tg, x0 = sc_fit_case
    kw = dict(init=x0, steps=60, lr=2e-2, history=True)
    r = fitter.fit(tg, **kw)
    first = fitter.losses(x0, tg)
    assert torch.equal(bits(r.history[0]), bits(first))
    assert (r.loss < first).all() and (first > 0).all()
    err = []
    for x in (x0, r.x):
        with torch.no_grad():
            _, det, _ = fitter.terms(x, tg)
        err.append(evaluate_surface(det, tg, thresholds=(2.0,)))
    print("SurfaceFitter: loss %s -> %s, mean pixel error %.3f -> %.3f, median %.3f -> %.3f, within 2 px %.2f -> %.2f"
          % (first.tolist(), r.loss.tolist(), err[0]["mean_error"], err[1]["mean_error"], err[0]["median_error"],
             err[1]["median_error"], err[0]["within"][2.0], err[1]["within"][2.0]))
    assert err[1]["mean_error"] < err[0]["mean_error"] and err[0]["nonfinite"] == 0
    assert err[0]["count"] == int(tg.counted().sum())
    # two fits from one start: the same bits; graph replay: the same bits again
    r2 = fitter.fit(tg, **kw)
    r3 = fitter.fit(tg, graph=True, graph_steps=4, **kw)
    for other in (r2, r3):
        assert torch.equal(bits(r.final_x), bits(other.final_x)) and torch.equal(bits(r.history), bits(other.history))


def test_surface_fitter_lbfgs_lowers_the_loss(sc_fit_case):
    fitter, tg, x0 = sc_fit_case
    first = fitter.losses(x0, tg)
    r = fitter.fit(tg, init=x0, steps=30, mode="lbfgs", history=True)
    assert r.optimizer == "lbfgs" and (r.loss < first).all()
    print("SurfaceFitter, lbfgs: loss %s -> %s" % (first.tolist(), r.loss.tolist()))


def test_surface_fitter_nonfinite_row_is_a_bad_call(sc_fit_case):
    fitter, tg, x0 = sc_fit_case
    bad = tg.target.clone()
    n = int(torch.nonzero(tg.counted()[1])[0])
    bad[1, n, 0] = float("nan")
    tb = SurfaceTargets(tg.topo, tg.face, tg.bary, bad, tg.conf)
    r = fitter.fit(tb, init=x0, steps=3, lr=2e-2, history=True)
    good = fitter.fit(tg, init=x0, steps=3, lr=2e-2, history=True)
    assert r.nonfinite.tolist() == [0, 3, 0, 0] and torch.equal(bits(r.final_x[1]), bits(x0[1])) and torch.isnan(r.history[:, 1]).all()
    for b in (0, 2, 3):
        assert torch.equal(bits(r.final_x[b]), bits(good.final_x[b]))
