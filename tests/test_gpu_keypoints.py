"""The 2D keypoint term on the GPU (csrc/keypoints.hip through ilps_amd/keypoints.py) against tests/_keypoint_oracle.py under
its rounding bar |got - want| <= 2^-24 |want| + 2^-28 T: small shapes (every combination of B in {1, 3}, V in {1, 65, 300},
K in {1, 5, 64}, with and without joint sources, with and without the robust function; rows that are empty, a single entry
of weight 1, dense over all V, one vertex shared by every row), the full size, bit-equality between launches and between a
row alone and inside a batch, hostile rows, the chain through `SMPLLayer`, and the two fitters."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _keypoint_oracle as orc  # noqa: E402
from test_keypoints_cpu import check_bar, problem, tens  # noqa: E402
from ilps_amd.keypoints import KeypointSpec, keypoint_energy, keypoint_energy_torch  # noqa: E402

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda:0")


def t(a, dtype=torch.float32):
    return torch.as_tensor(np.asarray(a), dtype=dtype).to(dev())


def bits(a):
    return a.detach().contiguous().view(torch.int32)


def run(p, spec, sigma, g=None, rows=None):
    """The op on the device for problem p (rows: a list of row indices, None = all) -> (e, details, dverts, dcam, djtr), the
    gradients for the cotangent g (B, K) numpy (None: no backward)."""
    q = p if rows is None else {k: (v if v is None or k == "R" else v[rows]) for k, v in p.items()}
    verts, cam, jtr, target, conf = tens(q, dev(), grad=g is not None)
    e, det = keypoint_energy(verts, cam, spec, target, conf, sigma, jtr, return_details=True)
    if g is None:
        return e, det, None, None, None
    e.backward(t(g if rows is None else g[rows]))
    torch.cuda.synchronize()
    return e.detach(), det, verts.grad, cam.grad, None if jtr is None else jtr.grad


def check_against_oracle(p, sigma, e, det, dverts, dcam, djtr, g):
    B, V = p["verts"].shape[:2]
    assert det["status"].cpu().tolist() == [0] * B
    for b in range(B):
        j = None if p["jtr"] is None else p["jtr"][b]
        fw = orc.forward(p["R"], p["verts"][b], p["cam"][b], p["target"][b], p["conf"][b], sigma, j)
        gr = orc.grads(p["R"], fw, p["cam"][b], p["conf"][b], g[b], sigma)
        check_bar(e[b].cpu().numpy(), fw["e"], fw["T_e"], "e")
        check_bar(det["d2"][b].cpu().numpy(), fw["d2"], fw["T_d2"], "d2")
        check_bar(det["proj"][b].cpu().numpy(), fw["proj"], fw["T_proj"], "proj")
        check_bar(det["joints"][b].cpu().numpy(), fw["J"], fw["T_J"], "joints")
        check_bar(dverts[b].cpu().numpy(), gr["dsrc"][:V], gr["T_dsrc"][:V], "dverts")
        check_bar(dcam[b].cpu().numpy(), gr["dcam"], gr["T_dcam"], "dcam")
        if j is not None:
            check_bar(djtr[b].cpu().numpy(), gr["dsrc"][V:], gr["T_dsrc"][V:], "djoints")
        assert (e[b].cpu().numpy()[~fw["counted"]] == 0).all()
        unused = ~(p["R"][:, :V] != 0).any(0)
        assert (dverts[b].cpu().numpy()[unused] == 0).all() and (dverts[b, :, 2] == 0).all()


# ---- values and gradients --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K", [1, 5, 64])
@pytest.mark.parametrize("V", [1, 65, 300])
@pytest.mark.parametrize("B", [1, 3])
def test_small_shapes_against_the_oracle(B, V, K):
    for with_joints in (False, True):
        p = problem(B, V, K, with_joints, seed=B + V + K)
        spec = KeypointSpec(p["R"], V, with_joints)
        if K >= 3:                                               # the rows the packing must get right
            assert spec.off[1] == spec.off[0] and spec.off[2] - spec.off[1] == 1 and spec.off[3] - spec.off[2] == V
            assert spec.t_off[V // 2 + 1] - spec.t_off[V // 2] == K - 1
        g = np.random.default_rng(K).normal(size=(B, K)).astype(np.float32)
        for sigma in (None, 3.0):
            out = run(p, spec, sigma, g)
            check_against_oracle(p, sigma, *out, g)
            if K >= 5 and B == 3:                                # residuals on both sides of sigma among the counted joints
                d2 = out[1]["d2"].cpu().numpy()[p["conf"] > 0]
                assert (d2 < 9.0).any() and (d2 > 9.0).any()


@pytest.fixture(scope="module")
def full_case(smpl_model):
    """V = 6 890 with the synthetic model's cocoplus spec, B = 5: seeded vertices around a body's size, a camera of the
    decoder's scale, targets on both sides of sigma."""
    spec = KeypointSpec.from_model(smpl_model)
    rng = np.random.default_rng(9)
    B, V, K = 5, 6890, spec.K
    R = spec.dense()
    verts = (np.asarray(smpl_model.v_template, np.float32).reshape(1, V, 3) + rng.normal(0, 0.01, (B, V, 3))).astype(np.float32)
    cam = np.stack([rng.uniform(18, 24, B), rng.uniform(18, 24, B), rng.uniform(20, 28, B), rng.uniform(20, 28, B)], 1).astype(np.float32)
    proj = np.stack([orc.forward(R, verts[b], cam[b], np.zeros((K, 2)), np.ones(K))["proj"] for b in range(B)])
    far = rng.uniform(size=(B, K, 1)) < 0.5
    off = np.where(far, rng.uniform(4.0, 9.0, (B, K, 2)), rng.uniform(0.1, 1.5, (B, K, 2))) * rng.choice([-1.0, 1.0], (B, K, 2))
    conf = rng.uniform(0.2, 1.0, (B, K)).astype(np.float32)
    conf[:, 4] = 0.0
    return dict(R=R, verts=verts, jtr=None, cam=cam, target=(proj + off).astype(np.float32), conf=conf), spec


def test_full_size_against_the_oracle(full_case):
    p, spec = full_case
    p4 = {k: (v if v is None or k == "R" else v[:4]) for k, v in p.items()}
    g = np.random.default_rng(1).normal(size=(4, spec.K)).astype(np.float32)
    out = run(p4, spec, 3.0, g)
    check_against_oracle(p4, 3.0, *out, g)
    assert (out[2] != 0).any(2).sum(1).cpu().tolist() == [int((p["R"][[k for k in range(spec.K) if k != 4]] != 0).any(0).sum())] * 4


@pytest.mark.parametrize("with_joints", [False, True])
def test_launches_repeat_and_a_row_does_not_see_its_batch(full_case, with_joints):
    if with_joints:
        p = problem(5, 300, 64, True, seed=21)
        spec = KeypointSpec(p["R"], 300, True)
    else:
        p, spec = full_case
    g = np.random.default_rng(2).normal(size=(5, spec.K)).astype(np.float32)
    a, b = run(p, spec, 3.0, g), run(p, spec, 3.0, g)
    flat = lambda o: [o[0], o[1]["d2"], o[1]["proj"], o[1]["joints"]] + [x for x in o[2:] if x is not None]
    for x, y in zip(flat(a), flat(b)):
        assert torch.equal(bits(x), bits(y))
    for row in (0, 3):
        alone = run(p, spec, 3.0, g, rows=[row])
        for x, y in zip(flat(a), flat(alone)):
            assert torch.equal(bits(x[row]), bits(y[0]))
        assert int(alone[1]["status"][0]) == 0


def test_hostile_rows():
    B, V, K = 7, 65, 5
    p = problem(B, V, K, True, seed=4)
    p["conf"][:, 3] = 0.0                                       # joint 3 never counts
    R = p["R"]
    R[:, 7] = 0.0                                               # vertex 7: a source no joint uses
    i3 = [i for i in np.nonzero(R[3, :V])[0] if i not in (V // 2, 7)][0]
    R[[0, 1, 2, 4], i3] = 0.0                                   # vertex i3: a source only the uncounted joint uses
    R[4, V + 2] = 0.25                                          # a joint source under a counted joint
    spec = KeypointSpec(R, V, True)
    g = np.ones((B, K), np.float32)
    clean = run(p, spec, 3.0, g)
    used = np.nonzero(R[1])[0][0]
    h = {k: (None if v is None else v.copy()) for k, v in p.items()}
    h["verts"][0, used, 1] = np.nan                             # row 0: a NaN in a used source -> status
    h["verts"][1, 7, 0] = np.nan                                # row 1: a NaN in an unused source -> nothing
    h["verts"][1, i3, 2] = np.inf                               # ... and in a source only an uncounted joint uses
    h["cam"][2, 1] = np.inf                                     # row 2: Inf cam -> status
    h["target"][3, 3, 0] = np.nan                               # row 3: NaN target under conf 0 -> harmless
    h["target"][4, 1, 1] = np.nan                               # row 4: NaN target under conf > 0 -> status
    h["conf"][5] = 0.0                                          # row 5: nothing counts
    jsrc = [j for j in range(24) if R[[0, 1, 2, 4], V + j].any()][0]
    h["jtr"][6, jsrc, 0] = np.inf                               # row 6: Inf in a used joint source -> status
    e, det, dverts, dcam, djtr = run(h, spec, 3.0, g)
    assert det["status"].cpu().tolist() == [1, 0, 1, 0, 1, 0, 1]
    for b in (0, 2, 4, 6):
        for x in (e, det["d2"], det["proj"], det["joints"], dverts, dcam, djtr):
            assert torch.isnan(x[b]).all()
    for b in (1, 3):                                            # neighbours of hostile rows: the bits of the clean run
        assert torch.equal(bits(e[b]), bits(clean[0][b])) and torch.equal(bits(dcam[b]), bits(clean[3][b]))
        assert torch.equal(bits(djtr[b]), bits(clean[4][b]))
        assert torch.equal(bits(dverts[b]), bits(clean[2][b]))
    keep = [0, 1, 2, 4]
    assert torch.equal(bits(det["d2"][1][keep]), bits(clean[1]["d2"][1][keep])) and not torch.isfinite(det["joints"][1, 3]).all()
    assert torch.equal(bits(det["d2"][3][keep]), bits(clean[1]["d2"][3][keep])) and torch.isnan(det["d2"][3, 3])
    assert (bits(e[5]) == 0).all() and (bits(dverts[5]) == 0).all() and (bits(dcam[5]) == 0).all() and (bits(djtr[5]) == 0).all()


def test_device_torch_restatement_agrees(full_case):
    """`keypoint_energy_torch` on the device - the stock composition tools/keypoint_time.py times the kernels against -
    computes the same numbers (its float64 einsum has its own order: compared under the oracle's bar)."""
    p, spec = full_case
    verts, cam, _, target, conf = tens(p, dev())
    out = keypoint_energy_torch(verts, cam, spec, target, conf, 3.0)
    e = keypoint_energy(verts, cam, spec, target, conf, 3.0)
    for b in range(5):
        fw = orc.forward(p["R"], p["verts"][b], p["cam"][b], p["target"][b], p["conf"][b], 3.0)
        check_bar(out["e"][b].to(torch.float32).cpu().numpy(), fw["e"], fw["T_e"], "torch e")
        check_bar(e[b].cpu().numpy(), fw["e"], fw["T_e"], "kernel e")


# ---- the chain through SMPLLayer -------------------------------------------------------------------------------------------

def mixed_spec(smpl_model):
    """OpenPose style: the 19 cocoplus rows over the vertices, then 5 rows that are posed joints (with_joints)."""
    R = np.zeros((24, 6890 + 24), np.float32)
    R[:19, :6890] = np.asarray(smpl_model.cocoplus_regressor, np.float32)
    for r, j in enumerate((0, 4, 7, 15, 20)):
        R[19 + r, 6890 + j] = 1.0
    return KeypointSpec(R, 6890, with_joints=True)


def test_chain_through_the_smpl_layer(smpl_model):
    """d (sum g e) / dx through SMPLLayer -> keypoint_energy (cam = x[:, :4], sources verts and J_transformed) against the
    float64 SMPL oracle chained with float64 autograd of `keypoint_energy_torch`, under test_gpu_parity's `grad_close` bars
    per column block."""
    from _inputs import make_x
    from oracle.torch_oracle import TorchSMPL
    from test_gpu_parity import grad_close
    from ilps_amd.keras_smpl.batch_smpl import SMPLLayer
    spec = mixed_spec(smpl_model)
    layer = SMPLLayer(smpl_model)
    B, K = 3, spec.K
    x = make_x(B, 48, seed=5)
    rng = np.random.default_rng(6)
    xo = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    vo, jo, _ = TorchSMPL(smpl_model)(xo, return_all=True)
    conf = rng.uniform(0.3, 1.0, (B, K)).astype(np.float32)
    conf[:, 2] = 0.0
    g = rng.uniform(0.5, 1.5, (B, K)).astype(np.float32)
    with torch.no_grad():
        p0 = keypoint_energy_torch(vo, xo[:, :4], spec, torch.zeros(B, K, 2), torch.ones(B, K), None, jo)["proj"].numpy()
    target = (p0 + rng.uniform(1.0, 6.0, (B, K, 2)) * rng.choice([-1.0, 1.0], (B, K, 2))).astype(np.float32)
    eo = keypoint_energy_torch(vo, xo[:, :4], spec, torch.tensor(target), torch.tensor(conf), 3.0, jo)["e"]
    (eo * torch.tensor(g, dtype=torch.float64)).sum().backward()
    xg = t(x).requires_grad_(True)
    verts = layer(xg)
    e, det = keypoint_energy(verts, xg[:, :4], spec, t(target), t(conf), 3.0, layer.J_transformed, return_details=True)
    e.backward(t(g))
    assert det["status"].cpu().tolist() == [0] * B
    got, want = xg.grad.cpu().numpy(), xo.grad.numpy()
    np.testing.assert_allclose(e.detach().cpu().numpy(), eo.detach().numpy(), rtol=2e-3, atol=1e-4)
    grad_close(got[:, :4], want[:, :4], name="dcam")
    grad_close(got[:, 4:76], want[:, 4:76], name="dtheta")
    grad_close(got[:, 76:], want[:, 76:], name="dbeta")
    # each source kind alone carries gradient: the joint rows only, then the vertex rows only
    for rows in (slice(19, 24), slice(0, 19)):
        c2 = np.zeros_like(conf)
        c2[:, rows] = np.maximum(conf[:, rows], 0.3)
        xo2 = torch.tensor(x, dtype=torch.float64, requires_grad=True)
        v2, j2, _ = TorchSMPL(smpl_model)(xo2, return_all=True)
        (keypoint_energy_torch(v2, xo2[:, :4], spec, torch.tensor(target), torch.tensor(c2), 3.0, j2)["e"]
         * torch.tensor(g, dtype=torch.float64)).sum().backward()
        xg2 = t(x).requires_grad_(True)
        v = layer(xg2)
        keypoint_energy(v, xg2[:, :4], spec, t(target), t(c2), 3.0, layer.J_transformed).backward(t(g))
        grad_close(xg2.grad.cpu().numpy()[:, 4:76], xo2.grad.numpy()[:, 4:76], name="dtheta (one source kind)")
        grad_close(xg2.grad.cpu().numpy()[:, 76:], xo2.grad.numpy()[:, 76:], name="dbeta (one source kind)")


# ---- the fitters -----------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def param_case(smpl_model):
    """A ParamFitter with the term (the mixed spec, sigma = 3 px), one without it, labels, a start, and detections made at
    the parameters the labels were made from."""
    import importlib.util
    from ilps_amd.fitting import ParamFitter
    s = importlib.util.spec_from_file_location("fit_time", os.path.join(ROOT, "tools", "fit_time.py"))
    fit_time = importlib.util.module_from_spec(s)
    s.loader.exec_module(fit_time)
    spec = mixed_spec(smpl_model)
    with_kp = ParamFitter(smpl_model, img_wh=48, deterministic=True, keypoints=spec, kp_sigma=3.0)
    plain = ParamFitter(smpl_model, img_wh=48, deterministic=True)
    labels, x0, xs = fit_time.problem(plain, 3, 48, seed=0, pose_sigma=0.05, cam_shift=1.5)
    with torch.no_grad():
        out = with_kp.decoder(xs)
        K = spec.K
        z = torch.zeros((3, K, 2), device=dev())
        _, det = keypoint_energy(out["verts"], xs[:, :4].contiguous(), spec, z, torch.ones((3, K), device=dev()), None,
                                 out["J_transformed"], return_details=True)
    conf = torch.linspace(0.3, 1.0, 3 * K, device=dev()).reshape(3, K).clone()
    conf[:, 5] = 0.0
    return with_kp, plain, labels, x0, (det["proj"].clone(), conf)


def test_param_fitter_one_iteration_is_the_hand_written_composition(param_case):
    from ilps_amd.fitting import FitState, fit_step
    fitter, _, labels, x0, kp = param_case
    w, B, N, K = 0.5, 3, 48 * 48, fitter.kp_spec.K
    r = fitter.fit(labels, init=x0, steps=1, lr=1e-2, history=True, keypoints=kp, kp_weight=w)
    state = FitState.new(x0)
    x = state.x.detach().requires_grad_(True)
    out = fitter.decoder(x, labels.to(torch.int32).reshape(B, 48, 48))
    e = keypoint_energy(out["verts"], x[:, :4], fitter.kp_spec, kp[0], kp[1], 3.0, out["J_transformed"])
    assert float(e.detach().sum()) > 0
    (g,) = torch.autograd.grad([out["seg_loss"], e], [x], grad_outputs=[torch.full((B, N), 1.0 / N, device=dev()),
                                                                       torch.full((B, K), w / K, device=dev())])
    loss = out["seg_loss"].detach() + (torch.full((1,), w, device=dev()) * e.detach().mean(1))[:, None]
    hist = torch.empty((1, B), device=dev())
    fit_step(state, g.contiguous(), loss, None, 1.0, None, hist, lr=1e-2)
    assert torch.equal(bits(r.final_x), bits(state.x)) and torch.equal(bits(r.history), bits(hist))
    assert torch.equal(bits(r.loss), bits(state.best_loss)) and torch.equal(bits(r.state.m), bits(state.m))
    assert not torch.equal(r.final_x, x0)
    assert torch.equal(bits(fitter.losses(x0, labels, keypoints=kp, kp_weight=w)), bits(hist[0]))


def test_param_fitter_replay_stage_weights_and_weight_zero(param_case):
    from ilps_amd.fitting import column_scale
    fitter, plain, labels, x0, kp = param_case
    cs = column_scale(cam=10.0, pose=1.0, shape=0.0)
    stages = [(5, cs), (6, cs)]
    kw = dict(init=x0, stages=stages, lr=1e-2, history=True)
    a = fitter.fit(labels, keypoints=kp, kp_weight=[0.0, 2.0], **kw)
    b = fitter.fit(labels, keypoints=kp, kp_weight=[0.0, 2.0], graph=True, graph_steps=2, **kw)
    for k in ("final_x", "history", "x", "loss"):
        assert torch.equal(bits(getattr(a, k)), bits(getattr(b, k))), k
    assert torch.equal(a.step, b.step)
    # the weights take effect under replay: another second-stage weight changes the second stage's losses only
    c = fitter.fit(labels, keypoints=kp, kp_weight=[0.0, 0.25], graph=True, graph_steps=2, **kw)
    assert torch.equal(bits(c.history[:5]), bits(b.history[:5])) and (c.history[5] < b.history[5]).all()
    # weight 0: the loss a fit built without the term records, plus zero - the same bits at the same x.  At the start that
    # is history[0]; at a later iterate `losses` of both fitters.  The two trajectories themselves part by an ulp from the
    # second update on: with a cotangent on verts, even a zero one, the decoder's backward runs its per-vertex skinning
    # kernel in place of the record-driven one (launch_skin_bwd_partials), whose sums round in another order - as with the
    # self-penetration term.  The weight-0 stage of `a` and a whole weight-0 fit take the same launches: the same bits.
    z = fitter.fit(labels, keypoints=kp, kp_weight=0.0, **kw)
    p = plain.fit(labels, **kw)
    assert torch.equal(bits(z.history[0]), bits(p.history[0])) and torch.equal(bits(a.history[:5]), bits(z.history[:5]))
    assert torch.equal(bits(fitter.losses(x0, labels, keypoints=kp, kp_weight=0.0)), bits(p.history[0]))
    for x in (z.final_x, p.final_x):
        assert torch.equal(bits(fitter.losses(x, labels, keypoints=kp, kp_weight=0.0)), bits(plain.losses(x, labels)))
    print("weight 0 against no term: max |history difference| %.3g" % float((z.history - p.history).abs().max()))
    with pytest.raises(ValueError, match="kp_weight lists"):
        fitter.fit(labels, keypoints=kp, kp_weight=[1.0], **kw)


@pytest.fixture(scope="module")
def both_case(param_case, smpl_model):
    """`param_case`'s labels, start and detections with a ParamFitter that carries BOTH side terms: the self-penetration
    term over the soup of test_gpu_scan.body_topology and the keypoint term (the mixed spec, sigma = 3 px)."""
    from test_gpu_scan import body_topology
    from ilps_amd.fitting import ParamFitter
    _, _, labels, x0, kp = param_case
    fitter = ParamFitter(smpl_model, img_wh=48, deterministic=True, penetration=body_topology()[0],
                         keypoints=mixed_spec(smpl_model), kp_sigma=3.0)
    return fitter, labels, x0, kp


def side_energies(fitter, x, labels, kp):
    """-> (the decoder's dict, e_pen (B, V), e_kp (B, K)) of x, by the ops themselves."""
    from ilps_amd.penetration import self_penetration
    out = fitter.decoder(x, labels.to(torch.int32).reshape(3, 48, 48))
    e_pen = self_penetration(out["verts"], fitter.pen_topo, fitter.pen_collide)
    e_kp = keypoint_energy(out["verts"], x[:, :4], fitter.kp_spec, kp[0], kp[1], 3.0, out["J_transformed"])
    return out, e_pen, e_kp


def test_param_fitter_with_both_side_terms_one_iteration_is_the_hand_written_composition(both_case):
    """The order a fitter keeps its side terms in: penetration, then keypoints - in the list `autograd.grad` accumulates
    over and in the sum of the loss's columns."""
    from ilps_amd.fitting import FitState, fit_step
    fitter, labels, x0, kp = both_case
    wp, wk, B, N, V, K = 30.0, 0.5, 3, 48 * 48, 6890, fitter.kp_spec.K
    r = fitter.fit(labels, init=x0, steps=1, lr=1e-2, history=True, pen_weight=wp, keypoints=kp, kp_weight=wk)
    state = FitState.new(x0)
    x = state.x.detach().requires_grad_(True)
    out, e_pen, e_kp = side_energies(fitter, x, labels, kp)
    assert float(e_pen.detach().sum()) > 0 and float(e_kp.detach().sum()) > 0
    f32 = lambda n, val: torch.full((B, n), val, device=dev())
    (g,) = torch.autograd.grad([out["seg_loss"], e_pen, e_kp], [x], grad_outputs=[f32(N, 1.0 / N), f32(V, wp / V), f32(K, wk / K)])
    loss = out["seg_loss"].detach() + (torch.full((1,), wp, device=dev()) * e_pen.detach().mean(1))[:, None]
    loss = loss + (torch.full((1,), wk, device=dev()) * e_kp.detach().mean(1))[:, None]
    hist = torch.empty((1, B), device=dev())
    fit_step(state, g.contiguous(), loss, None, 1.0, None, hist, lr=1e-2)
    assert torch.equal(bits(r.final_x), bits(state.x)) and torch.equal(bits(r.history), bits(hist))
    assert torch.equal(bits(r.loss), bits(state.best_loss)) and torch.equal(bits(r.state.m), bits(state.m))
    assert not torch.equal(r.final_x, x0)
    assert torch.equal(bits(fitter.losses(x0, labels, pen_weight=wp, keypoints=kp, kp_weight=wk)), bits(hist[0]))


def test_param_fitter_with_both_side_terms_replay_equals_eager_over_two_stages(both_case):
    from ilps_amd.fitting import column_scale
    fitter, labels, x0, kp = both_case
    with torch.no_grad():
        _, e_pen, _ = side_energies(fitter, x0, labels, kp)
    assert float(e_pen.sum()) > 0                               # (else the term's place in the order could not show)
    cs = column_scale(cam=10.0, pose=1.0, shape=0.0)
    kw = dict(init=x0, stages=[(3, cs), (4, cs)], lr=1e-2, history=True, pen_weight=[0.0, 30.0], keypoints=kp, kp_weight=[0.5, 0.0])
    a = fitter.fit(labels, **kw)
    b = fitter.fit(labels, graph=True, graph_steps=2, **kw)
    assert a.steps == b.steps == 7
    for k in ("final_x", "history", "x", "loss"):
        assert torch.equal(bits(getattr(a, k)), bits(getattr(b, k))), k
    assert torch.equal(a.step, b.step) and torch.equal(bits(a.state.m), bits(b.state.m))


@pytest.fixture(scope="module")
def kp_fit_case(smpl_model):
    """KeypointFitter on the cocoplus joints, sigma = 6 px; detections made from perturbed parameters, the last row's
    confidences all zero."""
    from ilps_amd.fitting import KeypointFitter
    fitter = KeypointFitter(smpl_model, sigma=6.0, img_wh=48)
    B, K = 4, fitter.spec.K
    rng = np.random.default_rng(12)
    x0 = fitter.initial(B, device=dev())
    d = np.zeros((B, 86), np.float32)
    d[:, 2:4] = rng.normal(0, 1.5, (B, 2))
    d[:, 0:2] = rng.normal(0, 0.5, (B, 2))
    d[:, 4:76] = rng.normal(0, 0.15, (B, 72))
    d[:, 76:] = rng.normal(0, 0.7, (B, 10))
    xs = x0 + t(d)
    with torch.no_grad():
        _, det, _ = fitter.terms(xs, torch.zeros((B, K, 2), device=dev()), torch.ones((B, K), device=dev()))
    conf = t(rng.uniform(0.3, 1.0, (B, K)))
    conf[:, 7] = 0.0
    conf[3] = 0.0
    return fitter, det["proj"].clone(), conf, x0


def test_keypoint_fitter_lowers_the_loss_and_the_pixel_error(kp_fit_case):
    from ilps_amd.evaluation import evaluate_keypoints
    fitter, target, conf, x0 = kp_fit_case
    kw = dict(init=x0, steps=60, lr=2e-2, history=True)
    r = fitter.fit(target, conf, **kw)
    first = fitter.losses(x0, target, conf)
    assert torch.equal(bits(r.history[0]), bits(first))
    assert (r.loss[:3] < first[:3]).all() and (r.history[-1, :3] < first[:3]).all() and (first[:3] > 0).all()
    err = []
    for x in (x0, r.x):
        with torch.no_grad():
            _, det, _ = fitter.terms(x, target, conf)
        err.append(evaluate_keypoints(det, target, conf, thresholds=(2.0,)))
    print("KeypointFitter: loss %s -> %s, mean pixel error %.3f -> %.3f, PCK@2px %.2f -> %.2f"
          % (first[:3].tolist(), r.loss[:3].tolist(), err[0]["mean_error"], err[1]["mean_error"], err[0]["pck"][2.0], err[1]["pck"][2.0]))
    assert err[1]["mean_error"] < err[0]["mean_error"] and err[0]["nonfinite"] == 0 and err[0]["count"] == 3 * (fitter.spec.K - 1)
    # two fits from one start: the same bits; graph replay: the same bits again
    r2 = fitter.fit(target, conf, **kw)
    r3 = fitter.fit(target, conf, graph=True, graph_steps=4, **kw)
    for other in (r2, r3):
        assert torch.equal(bits(r.final_x), bits(other.final_x)) and torch.equal(bits(r.history), bits(other.history))
    # the row without a counted joint and without a prior: loss 0, x unchanged
    assert torch.equal(bits(r.final_x[3]), bits(x0[3])) and (r.history[:, 3] == 0).all()
    assert not torch.equal(r.final_x[0], x0[0])


def test_keypoint_fitter_nonfinite_row_is_a_bad_call(kp_fit_case):
    fitter, target, conf, x0 = kp_fit_case
    bad = target.clone()
    bad[1, 0, 0] = float("nan")                                 # (conf[1, 0] > 0)
    r = fitter.fit(bad, conf, init=x0, steps=3, lr=2e-2, history=True)
    good = fitter.fit(target, conf, init=x0, steps=3, lr=2e-2, history=True)
    assert r.nonfinite.tolist() == [0, 3, 0, 0] and torch.equal(bits(r.final_x[1]), bits(x0[1])) and torch.isnan(r.history[:, 1]).all()
    for b in (0, 2, 3):
        assert torch.equal(bits(r.final_x[b]), bits(good.final_x[b]))
