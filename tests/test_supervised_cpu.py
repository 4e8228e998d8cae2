"""The supervised 3D terms without a GPU: the oracle's hand-written gradients (tests/_supervised_oracle.py) against float64
autograd of the definition (`supervised_terms_torch`) - theta rows that are exactly 0, angles of 1e-6, pi - 1e-3 and
2 pi + 0.3, root at -1, 0 and K - 1, a row_w holding zeros over NaN targets; `UncertaintyWeights`; the refusals of the Python
surface; the C ABI of the two launchers (no launch); the kernels' registers and scratch from the built code object."""
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ilps_amd  # noqa: E402,F401
from ilps_amd import supervised  # noqa: E402
from ilps_amd.keypoints import KeypointSpec  # noqa: E402
from ilps_amd.supervised import UncertaintyWeights, supervised_terms, supervised_terms_torch  # noqa: E402
import _supervised_oracle as orc  # noqa: E402
from test_keypoints_cpu import regressor  # noqa: E402

ANGLES = (0.0, 1e-6, math.pi - 1e-3, 2.0 * math.pi + 0.3)        # the first four joints of every row, in turn on either side


def problem(B, V, K, with_joints, seed=0, num_cam=4, cols=None, zero_w=True):
    """Seeded float32 operands.  R: the packing cases of test_keypoints_cpu.regressor (an empty row, a single weight-1 entry,
    a dense row, one vertex shared by every row).  theta: joint j < 4 of the prediction has angle ANGLES[j] about a random
    axis (joint 0 exactly 0), joint j + 4 of the truth likewise; the rest N(0, 0.3).  row_w in (0.5, 1.5) with zeros, and NaN
    in the targets those zeros cover."""
    rng = np.random.default_rng(seed + 31)
    C = num_cam + 82 if cols is None else cols
    R = regressor(K, V, with_joints, seed) if K else None
    f32 = lambda a: a.astype(np.float32)
    verts = f32(rng.normal(0, 0.4, (B, V, 3)))
    verts_t = f32(verts + rng.normal(0, 0.03, (B, V, 3)))
    jtr = f32(rng.normal(0, 0.4, (B, 24, 3))) if with_joints else None
    jtr_t = f32(jtr + rng.normal(0, 0.03, (B, 24, 3))) if with_joints else None
    x, x_t = rng.normal(0, 0.3, (B, C)), None
    x[:, :num_cam] = rng.uniform(18, 28, (B, num_cam))
    x_t = x + rng.normal(0, 0.1, (B, C))
    for b in range(B):
        for j, ang in enumerate(ANGLES):
            for arr, jj in ((x, j), (x_t, j + 4)):
                ax = rng.normal(size=3)
                arr[b, num_cam + 3 * jj:num_cam + 3 * jj + 3] = ang * ax / np.linalg.norm(ax)
    x, x_t = f32(x), f32(x_t)
    row_w = f32(rng.uniform(0.5, 1.5, (B, 5)))
    if zero_w:
        for b in range(B):
            row_w[b, (b + np.arange(2)) % 5] = 0.0                 # (row 0: terms 0 and 1; row 1: 1 and 2; ...)
    g = f32(rng.normal(size=(B, 5)))
    cam_scale = f32(rng.uniform(0.02, 0.06, num_cam))
    return dict(R=R, x=x, x_t=x_t, verts=verts, verts_t=verts_t, jtr=jtr, jtr_t=jtr_t, row_w=row_w, g=g, cam_scale=cam_scale,
                num_cam=num_cam, V=V, K=K, with_joints=with_joints)


def poison(p):
    """NaN into the targets that only terms with a row_w of 0 read (a copy)."""
    q = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in p.items()}
    nc = p["num_cam"]
    for b in range(len(p["x"])):
        off = p["row_w"][b] == 0
        if off[0] and (off[1] or not p["K"]):                       # (the joints of term 1 read the true vertices too)
            q["verts_t"][b, ::3] = np.nan
        if off[1] and p["jtr_t"] is not None:
            q["jtr_t"][b, 0] = np.nan
        if off[2]:
            q["x_t"][b, nc + 5] = np.nan
        if off[3]:
            q["x_t"][b, nc + 75] = np.inf
        if off[4] and nc:
            q["x_t"][b, 0] = np.nan
    return q


def spec_of(p):
    return None if p["R"] is None else KeypointSpec(p["R"], p["V"], p["with_joints"])


def oracle_rows(p, root, use_row_w=True, g=None):
    """[(forward dict, grads dict)] per row."""
    out = []
    for b in range(len(p["x"])):
        j = (p["jtr"][b], p["jtr_t"][b]) if p["with_joints"] else (None, None)
        fw = orc.forward(p["R"], p["x"][b], p["x_t"][b], p["verts"][b], p["verts_t"][b], j[0], j[1], root,
                         p["row_w"][b] if use_row_w else None, p["cam_scale"], p["num_cam"])
        gr = orc.grads(fw, (p["g"] if g is None else g)[b], p["with_joints"]) if fw["status"] == 0 else None
        out.append((fw, gr))
    return out


def tensors(p, device="cpu", dtype=torch.float32, grad=False, root=None):
    f = lambda a: None if a is None else torch.tensor(a, dtype=dtype, device=device)
    x, verts, jtr = f(p["x"]), f(p["verts"]), f(p["jtr"])
    if grad:
        for a in (x, verts, jtr):
            if a is not None:
                a.requires_grad_(True)
    truth = {"x": f(p["x_t"]), "verts": f(p["verts_t"]), "J_transformed": f(p["jtr_t"])}
    return x, verts, jtr, truth, torch.tensor(p["row_w"], device=device), torch.tensor(p["cam_scale"], device=device)


# ---- the oracle against autograd of the definition ---------------------------------------------------------------------

@pytest.mark.parametrize("root", [-1, 0, 4])
@pytest.mark.parametrize("with_joints", [False, True])
def test_oracle_gradient_equals_float64_autograd_of_the_definition(root, with_joints):
    B, V, K = 3, 65, 5
    p = poison(problem(B, V, K, with_joints, seed=2))
    assert (p["row_w"] == 0).any() and (p["x"][:, 4:7] == 0).all() and np.isnan(p["verts_t"][0]).any()
    x, verts, jtr, truth, row_w, cam_scale = tensors(p, dtype=torch.float64, grad=True)
    terms = supervised_terms_torch(x, verts, jtr, truth, spec_of(p), root, row_w, cam_scale)
    assert terms.dtype == torch.float64 and terms.shape == (B, 5)
    (terms * torch.tensor(p["g"], dtype=torch.float64)).sum().backward()
    for b, (fw, gr) in enumerate(oracle_rows(p, root)):
        assert fw["status"] == 0
        np.testing.assert_allclose(terms[b].detach().numpy(), fw["terms"], rtol=1e-11, atol=1e-14)
        assert (fw["terms"][p["row_w"][b] == 0] == 0).all() and (fw["terms"][p["row_w"][b] > 0] > 0).all()
        np.testing.assert_allclose(verts.grad[b].numpy(), gr["dverts"], rtol=1e-10, atol=1e-13)
        np.testing.assert_allclose(x.grad[b].numpy(), gr["dx"], rtol=1e-9, atol=1e-12)
        if with_joints:
            np.testing.assert_allclose(jtr.grad[b].numpy(), gr["djtr"], rtol=1e-10, atol=1e-13)
            assert p["row_w"][b, 1] == 0 or np.abs(gr["djtr"]).max() > 0
        if p["row_w"][b, 2] > 0:
            assert (np.abs(gr["dx"][4:16].reshape(4, 3)).max(1) > 0).all()       # every special angle has a gradient
        assert np.isfinite(gr["dx"]).all() and np.isfinite(gr["dverts"]).all()
        if root >= 0 and p["row_w"][b, 1] > 0:
            assert (fw["r"][root] == 0).all()


def test_oracle_pose_gradient_equals_central_differences_at_the_special_angles():
    """The hand-written dR / dtheta against central differences of R in float64, at the four angles and at a plain one."""
    rng = np.random.default_rng(0)
    for ang in ANGLES[1:] + (0.7,):
        ax = rng.normal(size=3)
        th = np.float32(ang * ax / np.linalg.norm(ax)).astype(np.float64)
        dR, TdR = orc.rodrigues_jac(th)
        h = 1e-6 * max(ang, 1e-3)
        for m in range(3):
            e = np.zeros(3)
            e[m] = h
            num = (orc.rodrigues(th + e)[0] - orc.rodrigues(th - e)[0]) / (2 * h)
            np.testing.assert_allclose(dR[:, :, m], num, rtol=0, atol=2e-7 * max(1.0, 1.0 / ang * 1e-3))
        assert (TdR >= np.abs(dR) * (1 - 1e-12)).all()


def test_oracle_on_known_answers():
    V, nc = 2, 4
    x, x_t = np.zeros(86), np.zeros(86)
    x[76], x_t[76] = 3.0, 1.0                                      # beta_0: (3 - 1)^2 / 10
    x[0], x_t[0] = 10.0, 8.0                                       # cam_0 with scale 0.5: (0.5 * 2)^2 / 4
    x[4 + 3:4 + 6] = [math.pi, 0, 0]                               # joint 1: half a turn about x against the identity
    verts, verts_t = np.array([[1.0, 2, 3], [0, 0, 0]]), np.array([[0.0, 2, 3], [0, 0, 2]])
    R = np.array([[1.0, 0.0], [0.5, 0.5]])
    fw = orc.forward(R, x, x_t, verts, verts_t, cam_scale=[0.5, 1, 1, 1])
    np.testing.assert_allclose(fw["terms"], [(1 + 4) / 2, ((1) + (0.25 + 1)) / 2, 8.0 / 24, 0.4, 0.25], rtol=1e-7)
    fw0 = orc.forward(R, x, x_t, verts, verts_t, root=0)
    np.testing.assert_allclose(fw0["terms"][1], (0.25 + 1) / 2, rtol=1e-12)      # r_1 = (0.5, 0, -1) - (1, 0, 0)
    gr = orc.grads(fw0, [0, 1, 0, 0, 0])
    np.testing.assert_allclose(gr["dverts"].sum(0), 0, atol=1e-15)              # root-relative: translation-free
    # a weight of 0 (or NaN, or below 0) hides NaN targets; a weight above 0 does not
    verts_t[1, 1] = np.nan
    for w0 in (0.0, np.nan, -1.0):
        f = orc.forward(None, x, x_t, verts, verts_t, row_w=[w0, 1, 1, 1, 1])
        assert f["status"] == 0 and f["terms"][0] == 0 and f["terms"][1] == 0 and np.isfinite(f["terms"]).all()
        assert (orc.grads(f, np.ones(5))["dverts"] == 0).all()
    assert orc.forward(None, x, x_t, verts, verts_t)["status"] == orc.NONFINITE
    assert np.isnan(orc.forward(None, x, x_t, verts, verts_t)["terms"]).all()
    assert orc.forward(R, x, x_t, verts, verts_t, row_w=[0, 1, 1, 1, 1])["status"] == orc.NONFINITE     # joint 1 uses vertex 1


def full_turn_problem(seed=4):
    """One row (V = 4, no joints) whose truth theta* has angles of 2 pi + (0.02 .. 0.25) about random axes and whose
    prediction is the nearest float32 to theta* (1 - 2 pi / |theta*|), the same rotations without the full turn.  The small
    side carries the rounding: its components are below 0.25, half an ulp is 7.5e-9 at most, so the two rotation matrices
    differ by about 1e-8 per entry - inside the bar around 0, which 2 |D| T_D puts near 4e-8 per entry."""
    p = problem(1, 4, 0, False, seed=seed, zero_w=False)
    rng = np.random.default_rng(seed)
    ax = rng.normal(size=(24, 3))
    ax /= np.linalg.norm(ax, axis=1, keepdims=True)
    th_t = (ax * (2 * math.pi + rng.uniform(0.02, 0.25, (24, 1)))).astype(np.float32)
    n = np.linalg.norm(th_t.astype(np.float64), axis=1, keepdims=True)
    p["x_t"][0, 4:76] = th_t.reshape(-1)
    p["x"][0, 4:76] = (th_t.astype(np.float64) * (1 - 2 * math.pi / n)).astype(np.float32).reshape(-1)
    return p


def test_rotation_matrices_do_not_see_a_further_full_turn():
    """theta and theta rotated by a further 2 pi about its own axis: the pose term is inside the bar around 0, the
    parameter error is not small."""
    p = full_turn_problem()
    fw = orc.forward(None, p["x"][0], p["x_t"][0], p["verts"][0], p["verts_t"][0])
    print("T2 %.3g, bar %.3g" % (fw["terms"][2], 2.0 ** -28 * fw["T_terms"][2]))
    assert fw["terms"][2] <= 2.0 ** -28 * fw["T_terms"][2]
    assert ((p["x"][0, 4:76] - p["x_t"][0, 4:76]) ** 2).mean() > 10.0


# ---- the Python surface ------------------------------------------------------------------------------------------------

def test_uncertainty_weights():
    terms = torch.tensor([[1.0, 2, 3, 4, 5], [0.5, 0, 0, 1, 2]])
    uw = UncertaintyWeights()
    assert [n for n, _ in uw.named_parameters()] == ["s"] and uw.s.shape == (5,) and (uw.s == 0).all() and uw.learned
    assert uw(terms).tolist() == [15.0, 3.5]
    with torch.no_grad():
        uw.s.copy_(torch.tensor([0.0, math.log(2.0), 0, 0, -math.log(2.0)]))
    row_w = torch.tensor([[1.0, 1, 0, 0, 1], [0.0, float("nan"), 1, 1, 0]])
    want0 = 1.0 + (0.5 * 2 + math.log(2.0)) + (2.0 * 5 - math.log(2.0))
    np.testing.assert_allclose(uw(terms, row_w).detach().numpy(), [want0, 1.0], rtol=1e-6)
    uw(terms, row_w).sum().backward()
    np.testing.assert_allclose(uw.s.grad.numpy(), [-1.0 + 1, -0.5 * 2 + 1, -0.0 + 1, -1.0 + 1, -2.0 * 5 + 1], rtol=1e-6, atol=1e-7)
    fx = UncertaintyWeights(fixed=(1, 0, 2, 0, 0.5))
    assert list(fx.parameters()) == [] and not fx.learned and fx(terms).tolist() == [9.5, 1.5]
    assert fx(terms, row_w).tolist() == [3.5, 0.0]
    with pytest.raises(ValueError):
        UncertaintyWeights(fixed=(1, 2))
    assert supervised.TERM_NAMES == ("verts", "joints3d", "pose", "shape", "cam")


def test_cpu_tensors_and_bad_arguments_raise():
    p = problem(2, 9, 5, True, seed=1)
    x, verts, jtr, truth, row_w, cam_scale = tensors(p)
    spec = spec_of(p)
    with pytest.raises(RuntimeError, match="HIP device"):
        supervised_terms(x, verts, jtr, truth, spec)
    with pytest.raises(ValueError, match="root"):
        supervised_terms_torch(x, verts, jtr, truth, spec, root=5)
    with pytest.raises(ValueError, match="root"):
        supervised_terms_torch(x, verts, None, truth, None, root=0)
    with pytest.raises(ValueError, match="jtr"):
        supervised_terms_torch(x, verts, None, truth, spec)
    with pytest.raises(ValueError, match="J_transformed"):
        supervised_terms_torch(x, verts, jtr, {"x": truth["x"], "verts": truth["verts"]}, spec)
    with pytest.raises(ValueError, match="truth"):
        supervised_terms_torch(x, verts, jtr, {"x": truth["x"]}, spec)
    with pytest.raises(ValueError):
        supervised_terms_torch(x[:, :80], verts, jtr, truth, spec)
    with pytest.raises(ValueError, match="num_cam"):
        supervised_terms_torch(x, verts, jtr, truth, spec, num_cam=9)
    with pytest.raises(ValueError, match="vertices"):
        supervised_terms_torch(x, verts[:, :8], jtr, truth, spec)
    with pytest.raises(TypeError):
        supervised_terms_torch(x, verts, jtr, truth, spec="cocoplus")
    # a spec without joint sources ignores jtr; no spec turns term 1 off
    t = supervised_terms_torch(x, verts, jtr, truth, None)
    assert (t[:, 1] == 0).all() and (t[:, [0, 2, 3, 4]] > 0).all()


# ---- the C ABI and the built kernels -----------------------------------------------------------------------------------

def check_abi_refusals():
    """Every SMPLR_EINVAL case of the two launchers, with pointer values that are never dereferenced: nothing is launched."""
    from ilps_amd import _lib
    lib = _lib.load()
    one = 1

    def fwd(x=one, stride=86, verts=one, jtr=None, jtr_t=None, off=one, idx=one, root=-1, cam_scale=one, B=2, V=42, K=5, nnz=30,
            num_cam=4, terms=one, ws=one):
        return lib.smplr_sup_fwd(x, one, stride, verts, one, jtr, jtr_t, off, idx, one, root, None, cam_scale, B, V, K, nnz,
                                 num_cam, terms, one, ws, None)

    def bwd(x=one, stride=86, verts=one, jtr=None, jtr_t=None, off=one, idx=one, root=-1, cam_scale=one, B=2, V=42, K=5, nnz=30,
            num_cam=4, terms=one, ws=one):
        return lib.smplr_sup_bwd(x, one, stride, verts, one, off, idx, one, root, None, cam_scale, one, ws, one, B, V, K, nnz,
                                 num_cam, terms, None, one, None)
    err = lib.smplr_last_error
    for fn, name in ((fwd, b"smplr_sup_fwd"), (bwd, b"smplr_sup_bwd")):
        assert fn(x=None) == -1 and b"null" in err() and name in err()
        assert fn(verts=None) == -1 and fn(terms=None) == -1 and fn(ws=None) == -1 and b"null" in err()
        assert fn(off=None) == -1 and fn(idx=None) == -1 and fn(cam_scale=None) == -1 and b"null" in err()
        assert fn(V=0) == -1 and b"V=0" in err() and name in err()
        assert fn(V=(1 << 24) + 1) == -1 and fn(B=-1) == -1 and b"B=-1" in err()
        assert fn(K=-1) == -1 and fn(K=65) == -1 and b"K=65" in err()
        assert fn(nnz=-1) == -1 and fn(nnz=(1 << 24) + 1) == -1 and b"nnz=16777217" in err()
        assert fn(num_cam=-1) == -1 and fn(num_cam=9) == -1 and b"num_cam=9" in err()
        assert fn(stride=85) == -1 and b"x_stride=85" in err()
        assert fn(root=5) == -1 and b"root=5" in err() and fn(root=-2) == -1 and fn(K=0, nnz=0, root=0) == -1
        assert fn(B=0, x=None, verts=None, terms=None) == 0          # an empty batch is a no-op
    assert fwd(jtr=one) == -1 and fwd(jtr_t=one) == -1 and b"null" in err()      # jtr and jtr_t go together
    assert bwd(B=65536) == -1 and b"65535" in err()


def test_abi_symbols_and_launchers_refuse_bad_arguments_without_launching():
    from ilps_amd import _lib
    lib = _lib.load()
    for name in ("smplr_sup_fwd", "smplr_sup_bwd"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    check_abi_refusals()
    header = open(os.path.join(ROOT, "include", "smplraster.h")).read()
    assert all("int %s(" % n in header for n in ("smplr_sup_fwd", "smplr_sup_bwd"))
    assert "#define SMPLR_ABI_VERSION 7" in header and "#define SMPLR_SUP_NONFINITE 1" in header
    assert "#define SMPLR_SUP_WS_DOUBLES %d" % supervised.WS_DOUBLES in header and supervised.NONFINITE == 1


def test_torch_ops_have_meta_kernels():
    from ilps_amd import torch_ops
    ns = torch_ops.load()
    m = lambda *s, dt=torch.float32: torch.empty(*s, dtype=dt, device="meta")
    i32 = torch.int32
    terms, status, ws = ns.sup_fwd(m(2, 90), m(2, 90), m(2, 65, 3), m(2, 65, 3), None, None, m(6, dt=i32), m(30, dt=i32), m(30), 5, 0,
                                   None, m(4))
    assert terms.shape == (2, 5) and status.shape == (2,) and status.dtype == i32 and ws.shape == (2, 408) and ws.dtype == torch.float64
    dv, dj, dx = ns.sup_bwd(m(2, 90), m(2, 90), m(2, 65, 3), m(2, 65, 3), m(90, dt=i32), m(30, dt=i32), m(30), 5, 0, None, m(4),
                            status, ws, m(2, 5), True)
    assert dv.shape == (2, 65, 3) and dj.shape == (2, 24, 3) and dx.shape == (2, 90)
    with pytest.raises((RuntimeError, NotImplementedError)):
        ns.sup_fwd(torch.zeros(1, 86), torch.zeros(1, 86), torch.zeros(1, 3, 3), torch.zeros(1, 3, 3), None, None, None, None, None,
                   0, -1, None, torch.ones(4))


def test_supervised_kernels_use_no_scratch():
    """Registers, LDS and scratch from the built code object (tools/kernel_resources.py): no spills, no scratch, the
    forward's 1024 lanes and the backward's 256 fit their launch."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr
    ks = {n: k for n, k in kr.kernels().items() if "sup_fwd_kernel" in n or "sup_bwd_kernel" in n}
    assert len(ks) == 2, sorted(ks)
    for name, k in ks.items():
        assert k["scratch"] == 0, "%s spills %d B per lane" % (name, k["scratch"])
        assert k.get("sgpr_spills", 0) == 0 and k.get("vgpr_spills", 0) == 0, (name, k)
        assert k["lds"] <= 8 * 1024
        assert k["max_threads"] >= (1024 if "fwd" in name else 256), (name, k)
        assert kr.waves_per_simd(k) >= (4 if "fwd" in name else 1), (name, k)
        print(name, k, "waves per SIMD", kr.waves_per_simd(k))
