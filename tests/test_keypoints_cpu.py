"""The 2D keypoint term without a GPU: the oracle's closed-form gradient (tests/_keypoint_oracle.py) against float64 autograd
of `keypoint_energy_torch`; `KeypointSpec`'s packing (an empty row, a dense row, one vertex in every row, the transposed CSR,
`from_model` against `SMPLLayer.joints`, the refusals); the package's CPU path against the oracle, values, gradient and
hostile rows; `evaluation.evaluate_keypoints` by hand; argument errors of the op and of the fitters; the C ABI of the two
launchers (no launch); the kernels' registers, LDS and scratch from the built code object."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ilps_amd  # noqa: E402,F401
from ilps_amd import keypoints  # noqa: E402
from ilps_amd.keypoints import KeypointSpec, keypoint_energy, keypoint_energy_torch  # noqa: E402
import _keypoint_oracle as orc  # noqa: E402


def regressor(K, V, with_joints, seed=0):
    """(K, S) float32 with the rows the issue names: row 0 empty, row 1 a single entry of weight 1, row 2 dense over all V
    (when K allows), vertex V // 2 in every row but the empty one, the rest a few random entries; with joint sources the
    later rows also use some."""
    rng = np.random.default_rng(seed)
    S = V + (24 if with_joints else 0)
    R = np.zeros((K, S))
    for k in range(K):
        if k == 0 and K > 1:
            continue
        if k == 1:
            R[k, V // 2] = 1.0
            continue
        if k == 2:
            R[k, :V] = rng.dirichlet(np.ones(V))
            continue
        n = min(V, int(rng.integers(1, 9)))
        R[k, rng.choice(V, n, replace=False)] = rng.normal(size=n)
        R[k, V // 2] = rng.uniform(0.1, 1.0)
        if with_joints and k % 2:
            R[k, V + rng.choice(24, 3, replace=False)] = rng.uniform(0.1, 0.5, 3)
    if K == 1:
        R[0, V // 2] = 1.0
        if with_joints:
            R[0, V + 3] = 0.5
    return R.astype(np.float32)


def problem(B, V, K, with_joints, seed=0, near_px=2.0):
    """Seeded verts, cam, joints, targets on both sides of sigma = 3 px (half the joints within near_px, half far), conf with
    some zeros.  -> dict of float32 numpy arrays and R."""
    rng = np.random.default_rng(seed + 17)
    R = regressor(K, V, with_joints, seed)
    verts = rng.normal(0, 0.4, (B, V, 3)).astype(np.float32)
    jtr = rng.normal(0, 0.4, (B, 24, 3)).astype(np.float32) if with_joints else None
    cam = np.stack([rng.uniform(18, 24, B), rng.uniform(18, 24, B), rng.uniform(20, 28, B), rng.uniform(20, 28, B)], 1).astype(np.float32)
    proj = np.stack([orc.forward(R, verts[b], cam[b], np.zeros((K, 2)), np.ones(K), None, None if jtr is None else jtr[b])["proj"]
                     for b in range(B)])
    far = (np.arange(K)[None, :] + np.arange(B)[:, None]) % 2 == 0
    off = np.where(far[..., None], rng.uniform(4.0, 9.0, (B, K, 2)), rng.uniform(0.1, near_px / 1.5, (B, K, 2)))
    target = (proj + off * rng.choice([-1.0, 1.0], (B, K, 2))).astype(np.float32)
    conf = rng.uniform(0.2, 1.0, (B, K)).astype(np.float32)
    conf[rng.uniform(size=(B, K)) < 0.2] = 0.0
    if K > 1:
        conf[:, 1] = np.maximum(conf[:, 1], 0.5)
    else:
        conf[:] = 0.7
    return dict(R=R, verts=verts, jtr=jtr, cam=cam, target=target, conf=conf)


def tens(p, device="cpu", grad=False):
    f = lambda a: None if a is None else torch.tensor(a, device=device)
    verts, cam, jtr = f(p["verts"]), f(p["cam"]), f(p["jtr"])
    if grad:
        for a in (verts, cam, jtr):
            if a is not None:
                a.requires_grad_(True)
    return verts, cam, jtr, f(p["target"]), f(p["conf"])


def check_bar(got, want, T, what):
    ok, worst = orc.within(got, want, T)
    print("%s: worst error / bar = %.3g" % (what, worst))
    assert ok, "%s: error %.3g times the bar" % (what, worst)


# ---- the oracle ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sigma", [None, 3.0])
@pytest.mark.parametrize("with_joints", [False, True])
def test_oracle_gradient_equals_float64_autograd_of_the_torch_restatement(sigma, with_joints):
    B, V, K = 2, 65, 5
    p = problem(B, V, K, with_joints, seed=3)
    spec = KeypointSpec(p["R"], V, with_joints)
    g = np.random.default_rng(5).normal(size=(B, K))
    f64 = lambda a: None if a is None else torch.tensor(a, dtype=torch.float64, requires_grad=True)
    verts, cam, jtr = f64(p["verts"]), f64(p["cam"]), f64(p["jtr"])
    out = keypoint_energy_torch(verts, cam, spec, torch.tensor(p["target"]), torch.tensor(p["conf"]), sigma, jtr)
    assert out["e"].dtype == torch.float64 and (out["status"] == 0).all()
    (out["e"] * torch.tensor(g)).sum().backward()
    for b in range(B):
        fw = orc.forward(p["R"], p["verts"][b], p["cam"][b], p["target"][b], p["conf"][b], sigma, None if jtr is None else p["jtr"][b])
        gr = orc.grads(p["R"], fw, p["cam"][b], p["conf"][b], g[b], sigma)
        np.testing.assert_allclose(out["e"][b].detach().numpy(), fw["e"], rtol=1e-13, atol=1e-13)
        np.testing.assert_allclose(out["d2"][b].detach().numpy(), fw["d2"], rtol=1e-13, atol=1e-13)
        np.testing.assert_allclose(verts.grad[b].numpy(), gr["dsrc"][:V], rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(cam.grad[b].numpy(), gr["dcam"], rtol=1e-12, atol=1e-12)
        if with_joints:
            np.testing.assert_allclose(jtr.grad[b].numpy(), gr["dsrc"][V:], rtol=1e-12, atol=1e-12)
            assert np.abs(gr["dsrc"][V:]).max() > 0
        assert np.abs(gr["dsrc"][:V]).max() > 0 and (gr["dsrc"][:, 2] == 0).all()
        sig = 3.0 if sigma is None else sigma
        cnt = fw["counted"]
        assert (fw["d2"][cnt] < sig ** 2).any() and (fw["d2"][cnt] > sig ** 2).any()      # residuals on both sides of sigma


def test_oracle_on_known_answers():
    # one joint = vertex 0 at (1, 2, 5), cam (10, 20, 3, 4): p = (13, 44); target (10, 40): d2 = 25; conf 0.5
    R = np.array([[1.0, 0.0]])
    v = np.array([[1.0, 2.0, 5.0], [9.0, 9.0, 9.0]])
    fw = orc.forward(R, v, [10, 20, 3, 4], [[10, 40]], [0.5])
    assert fw["proj"].tolist() == [[13.0, 44.0]] and fw["d2"].tolist() == [25.0] and fw["e"].tolist() == [12.5]
    fw3 = orc.forward(R, v, [10, 20, 3, 4], [[10, 40]], [0.5], sigma=5.0)
    assert fw3["e"].tolist() == [0.5 * 25.0 * 25.0 / 50.0]
    gr = orc.grads(R, fw, [10, 20, 3, 4], [0.5], [2.0])
    # q = 2 * 0.5 * 1 * 2 r = (6, 8); dJ = (60, 160, 0); dcam = (6 * 1, 8 * 2, 6, 8)
    assert gr["dsrc"].tolist() == [[60.0, 160.0, 0.0], [0.0, 0.0, 0.0]] and gr["dcam"].tolist() == [6.0, 16.0, 6.0, 8.0]
    # conf 0 and a NaN conf do not count, whatever the target holds; a NaN in the unused vertex does not matter
    v[1, 0] = np.nan
    for c in (0.0, np.nan, -1.0):
        fw0 = orc.forward(R, v, [10, 20, 3, 4], [[np.nan, 40]], [c])
        assert fw0["status"] == 0 and fw0["e"].tolist() == [0.0]
        g0 = orc.grads(R, fw0, [10, 20, 3, 4], [c], [2.0])
        assert (g0["dsrc"] == 0).all() and (g0["dcam"] == 0).all()
    assert orc.forward(R, v, [10, 20, 3, 4], [[np.nan, 40]], [0.5])["status"] == orc.NONFINITE
    assert orc.forward(R, v, [10, np.inf, 3, 4], [[10, 40]], [0.0])["status"] == orc.NONFINITE
    v[0, 2] = np.inf
    assert orc.forward(R, v, [10, 20, 3, 4], [[10, 40]], [0.5])["status"] == orc.NONFINITE


# ---- KeypointSpec ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("V, K, with_joints", [(1, 1, False), (65, 5, False), (65, 5, True), (300, 64, True)])
def test_spec_packing(V, K, with_joints):
    R = regressor(K, V, with_joints, seed=2)
    spec = KeypointSpec(R, V, with_joints)
    S = V + (24 if with_joints else 0)
    assert (spec.K, spec.num_verts, spec.S, spec.nnz) == (K, V, S, int((R != 0).sum()))
    assert spec.off.dtype == spec.idx.dtype == spec.t_off.dtype == spec.t_joint.dtype == np.int32 and spec.w.dtype == spec.t_w.dtype == np.float32
    assert len(spec.off) == K + 1 and len(spec.t_off) == S + 1 and spec.off[-1] == spec.t_off[-1] == spec.nnz
    for k in range(K):
        row = slice(spec.off[k], spec.off[k + 1])
        assert np.array_equal(spec.idx[row], np.nonzero(R[k])[0]) and np.array_equal(spec.w[row], R[k][R[k] != 0])
        assert (np.diff(spec.idx[row]) > 0).all()
    for i in range(S):                                           # the transposed CSR against regressor.T
        col = slice(spec.t_off[i], spec.t_off[i + 1])
        assert np.array_equal(spec.t_joint[col], np.nonzero(R.T[i])[0]) and np.array_equal(spec.t_w[col], R.T[i][R.T[i] != 0])
    assert np.array_equal(spec.dense(), R)
    if K > 2:
        assert spec.off[1] == spec.off[0]                        # the empty row
        assert spec.off[3] - spec.off[2] == V                    # the dense row
        assert spec.t_off[V // 2 + 1] - spec.t_off[V // 2] == K - 1      # one vertex in every row but the empty one
    # scipy-sparse input gives the same spec
    try:
        import scipy.sparse as sp
    except ImportError:
        sp = None
    if sp is not None:
        s2 = KeypointSpec(sp.csr_matrix(R), V, with_joints)
        assert all(np.array_equal(getattr(spec, n), getattr(s2, n)) for n in ("off", "idx", "w", "t_off", "t_joint", "t_w"))
    d = spec.to("cpu").on("cpu")
    assert d is spec.on(torch.device("cpu")) and d["idx"].dtype == torch.int32 and d["w"].dtype == torch.float32


def test_spec_refusals_and_constructors(smpl_model):
    V = 20
    with pytest.raises(ValueError, match="K = 0"):
        KeypointSpec(np.zeros((0, V)), V)
    with pytest.raises(ValueError, match="K = 65"):
        KeypointSpec(np.ones((65, V)), V)
    KeypointSpec(np.ones((64, V)), V)
    bad = np.ones((2, V))
    bad[1, 3] = np.nan
    with pytest.raises(ValueError, match="non-finite"):
        KeypointSpec(bad, V)
    bad[1, 3] = np.inf
    with pytest.raises(ValueError, match="non-finite"):
        KeypointSpec(bad, V)
    with pytest.raises(ValueError, match="float32"):
        KeypointSpec(np.full((2, V), 1e300), V)
    withj = np.zeros((2, V + 24))
    withj[0, 1] = withj[1, V + 2] = 1.0
    with pytest.raises(ValueError, match="with_joints"):
        KeypointSpec(withj, V)
    assert KeypointSpec(withj, V, with_joints=True).idx.tolist() == [1, V + 2]
    withj[1, V + 2] = 0.0
    assert KeypointSpec(withj, V).S == V                          # joint columns that are all zero are no joint sources
    with pytest.raises(ValueError, match="columns"):
        KeypointSpec(np.ones((2, V + 1)), V)
    with pytest.raises(ValueError, match="num_verts"):
        KeypointSpec(np.ones((2, 1)), 0)
    ident = KeypointSpec.smpl_joints()
    assert (ident.K, ident.num_verts, ident.S, ident.nnz, ident.with_joints) == (24, 6890, 6914, 24, True)
    assert ident.idx.tolist() == list(range(6890, 6914)) and (ident.w == 1).all() and (ident.t_off[:6891] == 0).all()
    with pytest.raises(ValueError, match="joint_type"):
        KeypointSpec.from_model(smpl_model, "coco")
    import dataclasses
    with pytest.raises(ValueError, match="cocoplus_regressor"):
        KeypointSpec.from_model(dataclasses.replace(smpl_model, cocoplus_regressor=None))


@pytest.mark.parametrize("joint_type, K", [("cocoplus", 19), ("lsp", 14)])
def test_from_model_equals_the_layers_joints_on_cpu(smpl_model, joint_type, K):
    from ilps_amd.keras_smpl.batch_smpl import SMPLLayer
    layer = SMPLLayer(smpl_model, joint_type=joint_type)
    spec = KeypointSpec.from_model(layer, joint_type)
    assert spec.K == K and spec.num_verts == 6890 and not spec.with_joints
    assert np.array_equal(spec.dense(), np.asarray(smpl_model.cocoplus_regressor, np.float32)[:K])
    assert np.array_equal(KeypointSpec.from_model(smpl_model, joint_type).idx, spec.idx)
    rng = np.random.default_rng(0)
    verts = torch.tensor(rng.normal(0, 0.5, (2, 6890, 3)), dtype=torch.float32)
    want = layer.joints(verts)                                   # (the fp32 einsum)
    cam = torch.tensor([[1.0, 1.0, 0.0, 0.0]] * 2)
    _, det = keypoint_energy(verts, cam, spec, torch.zeros(2, K, 2), torch.ones(2, K), return_details=True)
    assert det["joints"].shape == (2, K, 3)
    np.testing.assert_allclose(det["joints"].numpy(), want.numpy(), rtol=0, atol=2e-6)
    assert torch.equal(det["proj"], det["joints"][..., :2])      # the unit camera


# ---- the CPU path ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sigma", [None, 3.0])
@pytest.mark.parametrize("B, V, K, with_joints", [(1, 1, 1, False), (3, 65, 5, True), (3, 300, 64, False)])
def test_cpu_path_equals_the_oracle(B, V, K, with_joints, sigma):
    p = problem(B, V, K, with_joints, seed=1)
    spec = KeypointSpec(p["R"], V, with_joints)
    verts, cam, jtr, target, conf = tens(p, grad=True)
    e, det = keypoint_energy(verts, cam, spec, target, conf, sigma, jtr, return_details=True)
    assert e.dtype == torch.float32 and det["status"].dtype == torch.int32 and det["status"].tolist() == [0] * B
    g = np.random.default_rng(2).normal(size=(B, K)).astype(np.float32)
    e.backward(torch.tensor(g))
    for b in range(B):
        fw = orc.forward(p["R"], p["verts"][b], p["cam"][b], p["target"][b], p["conf"][b], sigma, None if jtr is None else p["jtr"][b])
        gr = orc.grads(p["R"], fw, p["cam"][b], p["conf"][b], g[b], sigma)
        check_bar(e[b].detach().numpy(), fw["e"], fw["T_e"], "e")
        check_bar(det["d2"][b].numpy(), fw["d2"], fw["T_d2"], "d2")
        check_bar(det["proj"][b].numpy(), fw["proj"], fw["T_proj"], "proj")
        check_bar(det["joints"][b].numpy(), fw["J"], fw["T_J"], "joints")
        check_bar(verts.grad[b].numpy(), gr["dsrc"][:V], gr["T_dsrc"][:V], "dverts")
        check_bar(cam.grad[b].numpy(), gr["dcam"], gr["T_dcam"], "dcam")
        if with_joints:
            check_bar(jtr.grad[b].numpy(), gr["dsrc"][V:], gr["T_dsrc"][V:], "djoints")
        assert (e[b].detach().numpy()[~fw["counted"]] == 0).all()


def test_cpu_path_hostile_rows():
    B, V, K = 6, 65, 5
    p = problem(B, V, K, True, seed=4)
    p["conf"][:, 3] = 0.0                                       # joint 3 never counts
    R = p["R"]
    R[:, 7] = 0.0                                               # vertex 7: a source no joint uses
    i3 = [i for i in np.nonzero(R[3, :V])[0] if i not in (V // 2, 7)][0]
    R[[0, 1, 2, 4], i3] = 0.0                                   # vertex i3: a source only the uncounted joint uses
    spec = KeypointSpec(R, V, True)
    clean = keypoint_energy(*tens(p)[:2], spec, *tens(p)[3:], 3.0, tens(p)[2], return_details=True)
    used = np.nonzero(p["R"][1])[0][0]
    unused, only3 = 7, [i3]
    h = {k: (None if v is None else v.copy()) for k, v in p.items()}
    h["verts"][0, used, 1] = np.nan                             # row 0: a NaN in a used source -> status
    h["verts"][1, unused, 0] = np.nan                           # row 1: a NaN in an unused source -> nothing
    if only3:
        h["verts"][1, only3[0], 2] = np.inf                     # ... and in a source only an uncounted joint uses
    h["cam"][2, 1] = np.inf                                     # row 2: Inf cam -> status
    h["target"][3, 3, 0] = np.nan                               # row 3: NaN target under conf 0 -> harmless
    h["target"][4, 1, 1] = np.nan                               # row 4: NaN target under conf > 0 -> status
    h["conf"][5] = 0.0                                          # row 5: nothing counts
    verts, cam, jtr, target, conf = tens(h, grad=True)
    e, det = keypoint_energy(verts, cam, spec, target, conf, 3.0, jtr, return_details=True)
    assert det["status"].tolist() == [1, 0, 1, 0, 1, 0]
    e.backward(torch.ones_like(e))
    for b in (0, 2, 4):
        assert torch.isnan(e[b]).all() and torch.isnan(det["d2"][b]).all() and torch.isnan(det["proj"][b]).all()
        assert torch.isnan(det["joints"][b]).all() and torch.isnan(verts.grad[b]).all() and torch.isnan(cam.grad[b]).all()
        assert torch.isnan(jtr.grad[b]).all()
    for b in (1, 3):
        assert torch.equal(e[b], clean[0][b]) and torch.isfinite(verts.grad[b]).all() and torch.isfinite(cam.grad[b]).all()
    assert torch.equal(det["d2"][3, [0, 1, 2, 4]], clean[1]["d2"][3, [0, 1, 2, 4]])
    assert (e[5] == 0).all() and (verts.grad[5] == 0).all() and (cam.grad[5] == 0).all() and (jtr.grad[5] == 0).all()


def test_argument_errors_are_raised_without_a_launch():
    p = problem(2, 20, 3, False)
    spec = KeypointSpec(p["R"], 20)
    verts, cam, _, target, conf = tens(p)
    with pytest.raises(TypeError, match="KeypointSpec"):
        keypoint_energy(verts, cam, p["R"], target, conf)
    with pytest.raises(ValueError, match="verts"):
        keypoint_energy(verts[0], cam, spec, target, conf)
    with pytest.raises(ValueError, match="vertices"):
        keypoint_energy(verts[:, :10], cam, spec, target, conf)
    with pytest.raises(ValueError, match="cam"):
        keypoint_energy(verts, cam[:, :3], spec, target, conf)
    with pytest.raises(ValueError, match="target"):
        keypoint_energy(verts, cam, spec, target[:, :2], conf)
    with pytest.raises(ValueError, match="conf"):
        keypoint_energy(verts, cam, spec, target, conf[:1])
    with pytest.raises(RuntimeError, match="float32"):
        keypoint_energy(verts.double(), cam, spec, target, conf)
    with pytest.raises(ValueError, match="with_joints"):
        keypoint_energy(verts, cam, spec, target, conf, joints=torch.zeros(2, 24, 3))
    with pytest.raises(ValueError, match="with_joints"):
        keypoint_energy(verts, cam, KeypointSpec(p["R"], 20, with_joints=True), target, conf)
    for s in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="sigma"):
            keypoint_energy(verts, cam, spec, target, conf, sigma=s)


def test_fitter_argument_checks_need_no_gpu(smpl_model):
    from ilps_amd.fitting import KeypointFitter, ParamFitter
    spec = KeypointSpec.from_model(smpl_model)
    with pytest.raises(ValueError, match="vertex_sampling"):
        ParamFitter(smpl_model, keypoints=spec, vertex_sampling=5)
    with pytest.raises(TypeError, match="KeypointSpec"):
        ParamFitter(smpl_model, keypoints=np.ones((3, 6890)))
    with pytest.raises(ValueError, match="vertices"):
        ParamFitter(smpl_model, keypoints=KeypointSpec(np.ones((3, 100)), 100))
    with pytest.raises(ValueError, match="kp_sigma"):
        ParamFitter(smpl_model, kp_sigma=3.0)
    with pytest.raises(ValueError, match="sigma"):
        ParamFitter(smpl_model, keypoints=spec, kp_sigma=-1.0)
    labels = torch.zeros((1, 48, 48), dtype=torch.int32)
    kp = (torch.zeros(1, 19, 2), torch.ones(1, 19))
    plain, withkp = ParamFitter(smpl_model), ParamFitter(smpl_model, keypoints=spec, kp_sigma=3.0)
    assert withkp.kp_spec is spec and withkp.kp_sigma == 3.0 and withkp.decoder.outputs == ("verts",) and plain.kp_spec is None
    with pytest.raises(ValueError, match="built with keypoints"):
        plain.fit(labels, steps=1, keypoints=kp)
    with pytest.raises(ValueError, match="built with keypoints"):
        plain.fit(labels, steps=1, kp_weight=2.0)
    with pytest.raises(ValueError, match="built with keypoints"):
        plain.losses(torch.zeros(1, 86), labels, kp_weight=2.0)
    with pytest.raises(ValueError, match=r"keypoints=\(target, conf\)"):
        withkp.fit(labels, steps=1)
    with pytest.raises(ValueError, match=r"keypoints=\(target, conf\)"):
        withkp.losses(torch.zeros(1, 86), labels)
    with pytest.raises(TypeError, match="KeypointSpec"):
        KeypointFitter(smpl_model, spec=np.ones((3, 6890)))
    with pytest.raises(ValueError, match="vertices"):
        KeypointFitter(smpl_model, spec=KeypointSpec(np.ones((3, 100)), 100))
    with pytest.raises(ValueError, match="sigma"):
        KeypointFitter(smpl_model, sigma=0.0)
    kf = KeypointFitter(smpl_model, sigma=3.0)
    assert kf.spec.K == 19 and kf.P == 86 and tuple(kf.initial(2).shape) == (2, 86)
    with pytest.raises(ValueError, match="target"):
        kf.fit(torch.zeros(1, 18, 2), torch.ones(1, 19))
    with pytest.raises(ValueError, match="conf"):
        kf.fit(torch.zeros(1, 19, 2), torch.ones(1, 18))
    with pytest.raises(RuntimeError, match="HIP device"):
        kf.fit(torch.zeros(1, 19, 2), torch.ones(1, 19))


# ---- evaluation ----------------------------------------------------------------------------------------------------------------

def test_evaluate_keypoints_by_hand():
    from ilps_amd.evaluation import evaluate_keypoints
    nan = float("nan")
    target = torch.tensor([[[0.0, 0.0], [0.0, 0.0], [nan, 0.0]], [[0.0, 0.0], [0.0, 0.0], [0.0, 0.0]], [[0.0, 0.0]] * 3])
    proj = torch.tensor([[[3.0, 4.0], [0.0, 1.0], [7.0, 7.0]], [[6.0, 8.0], [0.0, 2.0], [0.0, 0.0]], [[nan, 0.0], [1.0, 1.0], [1.0, 1.0]]])
    conf = torch.tensor([[1.0, 0.5, 0.0], [1.0, 1.0, 1.0], [1.0, 1.0, 1.0]])      # row 0: a conf = 0 joint with a NaN target; row 2: NaN
    res = evaluate_keypoints(proj, target, conf, thresholds=(1.0, 5.0), scale=None)
    # counted distances: row 0: 5, 1; row 1: 10, 2, 0; row 2 left out
    assert res["count"] == 5 and res["nonfinite"] == 1 and res["rows"] == 2
    assert res["mean_error"] == pytest.approx(18.0 / 5)
    assert res["per_joint"].tolist() == [7.5, 1.5, 0.0] and res["per_joint_count"].tolist() == [2, 2, 1]
    assert res["pck"] == {1.0: 2 / 5, 5.0: 4 / 5}
    res = evaluate_keypoints(proj, target, conf, thresholds=(1.0,), scale=torch.tensor([5.0, 1.0, 1.0]))
    assert res["pck"] == {1.0: 3 / 5}                           # row 0's threshold is 5 px: both its joints pass
    # from the op's details: the same numbers through d2 and status
    spec = KeypointSpec(np.eye(3, dtype=np.float32), 3)
    verts = torch.cat([proj, torch.zeros(3, 3, 1)], -1)
    cam = torch.tensor([[1.0, 1.0, 0.0, 0.0]] * 3)
    _, det = keypoint_energy(verts, cam, spec, target, conf, return_details=True)
    assert det["status"].tolist() == [0, 0, 1]
    res2 = evaluate_keypoints(det, target, conf, thresholds=(1.0, 5.0))
    assert res2["count"] == 5 and res2["nonfinite"] == 1 and res2["mean_error"] == pytest.approx(18.0 / 5)
    assert res2["pck"] == {1.0: 2 / 5, 5.0: 4 / 5} and res2["per_joint"].tolist() == [7.5, 1.5, 0.0]
    empty = evaluate_keypoints(proj, target, torch.zeros(3, 3))
    assert empty["count"] == 0 and np.isnan(empty["mean_error"]) and torch.isnan(empty["per_joint"]).all() and empty["nonfinite"] == 0


# ---- the C ABI and the built kernels ---------------------------------------------------------------------------------------

def test_abi_symbols_and_launchers_refuse_bad_arguments_without_launching():
    from ilps_amd import _lib
    lib = _lib.load()
    for name in ("smplr_kp_fwd", "smplr_kp_bwd"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    one = 1                                            # (a non-null pointer value that is never dereferenced: no launch)
    fwd = lambda verts=one, B=2, V=42, K=5, nnz=30, e=one, sigma=0.0: lib.smplr_kp_fwd(verts, None, one, one, one, one, one, one, B, V, K,
                                                                                       nnz, sigma, e, one, one, one, one, one, None)
    bwd = lambda verts=one, B=2, V=42, K=5, nnz=30, e=one, sigma=0.0: lib.smplr_kp_bwd(verts, one, one, one, one, one, one, one, B, V, K,
                                                                                       nnz, sigma, e, None, None, None)
    for fn, name in ((fwd, b"smplr_kp_fwd"), (bwd, b"smplr_kp_bwd")):
        assert fn(verts=None) == -1 and b"null" in lib.smplr_last_error() and name in lib.smplr_last_error()
        assert fn(e=None) == -1 and b"null" in lib.smplr_last_error()
        assert fn(V=0) == -1 and b"V=0" in lib.smplr_last_error() and name in lib.smplr_last_error()
        assert fn(V=(1 << 24) + 1) == -1 and fn(B=-1) == -1 and b"B=-1" in lib.smplr_last_error()
        assert fn(K=0) == -1 and b"K=0" in lib.smplr_last_error()
        assert fn(K=65) == -1 and b"K=65" in lib.smplr_last_error()
        assert fn(nnz=(1 << 24) + 1) == -1 and b"nnz=16777217" in lib.smplr_last_error() and fn(nnz=-1) == -1
        assert fn(sigma=-1.0) == -1 and b"sigma" in lib.smplr_last_error() and fn(sigma=float("nan")) == -1
        assert fn(sigma=float("inf")) == -1
        assert fn(B=0, verts=None) == 0                 # an empty batch is a no-op
    assert bwd(B=65536) == -1 and b"65535" in lib.smplr_last_error()
    header = open(os.path.join(ROOT, "include", "smplraster.h")).read()
    assert all("int %s(" % n in header for n in ("smplr_kp_fwd", "smplr_kp_bwd"))
    assert "#define SMPLR_ABI_VERSION 7" in header and "#define SMPLR_KP_NONFINITE 1" in header
    assert keypoints.NONFINITE == 1 and "TRUST" in header      # the header says who checks the index arrays


def test_kernels_fit_their_launch():
    """Registers, LDS and scratch from the built code object: no scratch, static LDS below 64 KB, 256 lanes per workgroup."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr
    ks = {n: k for n, k in kr.kernels().items() if "kp_fwd_kernel" in n or "kp_bwd_kernel" in n}
    assert len(ks) == 2
    for name, k in ks.items():
        assert k["scratch"] == 0, "%s spills %d B per lane" % (name, k["scratch"])
        assert k["lds"] <= 64 * 1024
        assert k["max_threads"] >= 256
        print(name, k, "waves per SIMD", kr.waves_per_simd(k))
