"""3D evaluation on the device (csrc/eval3d.hip) against the float64 NumPy oracle (tests/_eval3d_oracle.py), through the C
ABI (`eval3d.point_errors`) and the torch op (`torch.ops.smplraster.point_errors`).

The bar is the project's own vertex bar: 1e-4 m absolute on every per-point error and every per-mesh mean (README,
DESIGN section 0 - these are distances between vertices that are themselves held to it).  The similarity transform is
compared where the oracle's gap = (S2 + d S3) / S1 >= 0.02, and every parity case asserts that its inputs are there.  Its
bounds, from the number formats: the inputs are fp32 and the moments are summed in fp64 from centred fp32 coordinates, so
M carries a relative error of about 1e-7; a perturbation E of M turns R by |E| / (S1 gap) <= 1e-7 / 0.02 = 5e-6 -> R to
2e-5 absolute (4x); s is a ratio of two such sums written as fp32 -> 1e-6 relative; t = mean(g) - s R mean(p) inherits
|mean(p)| s dR <= 16 m x 2 x 2e-5 x sqrt(3) -> 1e-3 m, while the point it is there for - the aligned centroid
s R mean(p) + t = mean(g) - holds to 1e-5 m (a few fp32 ulps at 16 m)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _eval3d_oracle as orc  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-4            # metres
GAP_MIN = 0.02
R_ATOL, S_RTOL, T_ATOL, CENTROID_ATOL = 2e-5, 1e-6, 1e-3, 1e-5


def _dev():
    return torch.device("cuda", 0)


def _run(pred, gt, **kw):
    from ilps_amd.eval3d import point_errors
    out = point_errors(torch.as_tensor(pred, device=_dev()), torch.as_tensor(gt, device=_dev()), **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize("N", [14, 19, 24, 1378, 6890])
@pytest.mark.parametrize("B", [1, 3, 128, 1024])
def test_parity_with_the_oracle(B, N):
    pred, gt = orc.make_case(B, N, seed=1000 * B + N)
    want = orc.align(pred, gt)
    assert want["gap"].min() >= GAP_MIN, "the recipe must give well-determined rotations (gap %.3f)" % want["gap"].min()
    if B >= 3:
        assert (want["d"][1::3] < 0).all() and (want["d"][0::3] > 0).all()      # the reflection branch is exercised
        assert gt[2::3, :, 2].mean(1).min() >= 3.5                               # and the 5-10 m depth
    worst_pp, worst_mean = 0.0, 0.0
    for mode in range(4):
        got = _run(pred, gt, per_point=mode, transform=(mode == 3))
        assert (got["status"] == 0).all()
        worst_pp = max(worst_pp, float(np.abs(got["per_point"] - want["per_point"][:, mode]).max()))
        worst_mean = max(worst_mean, float(np.abs(got["mean_err"] - want["mean"]).max()))
    tr = got["transform"].astype(np.float64)
    s, R, t = tr[:, 0], tr[:, 1:10].reshape(B, 3, 3), tr[:, 10:]
    ds = float(np.abs(s / want["s"] - 1).max())
    dR = float(np.abs(R - want["R"]).max())
    dt = float(np.abs(t - want["t"]).max())
    mp, mg = pred.astype(np.float64).mean(1), gt.astype(np.float64).mean(1)
    dc = float(np.abs(s[:, None] * np.einsum("brc,bc->br", R, mp) + t - mg).max())
    print("eval3d parity B=%d N=%d: per-point %.2e m, mean %.2e m, s rel %.2e, R %.2e, t %.2e m, centroid %.2e m, "
          "gap >= %.3f" % (B, N, worst_pp, worst_mean, ds, dR, dt, dc, want["gap"].min()))
    assert worst_pp <= TOL and worst_mean <= TOL
    assert ds <= S_RTOL and dR <= R_ATOL and dt <= T_ATOL and dc <= CENTROID_ATOL
    assert np.abs(np.linalg.det(R) - 1).max() < 1e-5


@pytest.mark.parametrize("N", [65, 512, 513, 1536, 1537, 7168, 7169, 9000])
def test_sizes_at_the_edges_of_the_kernel_forms(N):
    """Each form at its largest N and the next at its smallest, and the form that re-reads memory (N > 7 168)."""
    pred, gt = orc.make_case(2, N, seed=N)
    want = orc.align(pred, gt)
    got = _run(pred, gt, per_point=3)
    assert np.abs(got["per_point"] - want["per_point"][:, 3]).max() <= TOL
    assert np.abs(got["mean_err"] - want["mean"]).max() <= TOL


def test_degenerate_rows():
    from ilps_amd import eval3d
    rng = np.random.default_rng(3)
    N = 24
    g = rng.normal(size=(7, N, 3)).astype(np.float32) * 0.4
    p = (g + rng.normal(size=g.shape) * 0.02).astype(np.float32)
    p[1] = p[1, :1]                                                 # coincident prediction: sum |pc|^2 = 0
    lin = np.linspace(-1, 1, N)
    p[2] = np.outer(lin, [1, 2, 3]) + 0.5                           # both sets collinear
    g[2] = np.outer(lin, [3, 1, -2]) * 1.5 - 1.0
    p[3] = g[3]                                                     # pred == gt exactly
    p[4] = np.outer(lin, [0.3, -0.2, 0.9])                          # a collinear prediction against a full cloud
    g[5] = g[5, :1]                                                 # the target is one point: M = 0, s = 0
    g[6] = g[6] * [1, 1, 0]                                         # planar sets (rank 2): unique up to the flip
    p[6] = p[6] * [1, 1, 0]
    got = _run(p, g, transform=True, per_point=3)
    want = orc.align(p, g)
    st, m = got["status"], got["mean_err"]
    print("eval3d degenerate rows: status", st.tolist(), "max mean diff %.2e" % np.abs(m - want["mean"]).max())
    assert np.isfinite(m).all() and np.isfinite(got["transform"]).all() and np.isfinite(got["per_point"]).all()
    assert st[0] == 0 and st[3] == 0 and st[6] == 0
    assert st[1] == eval3d.DEGENERATE and m[1, 1] == m[1, 2] == m[1, 3]      # the fall-back: translation only
    assert st[2] == eval3d.RANK_DEFICIENT and st[4] == eval3d.RANK_DEFICIENT and st[5] == eval3d.RANK_DEFICIENT
    assert (m[3, :2] == 0).all() and (m[3, 2:] <= 1e-6).all() and abs(got["transform"][3, 0] - 1) <= 1e-6
    # the minimal error, whatever rotation was picked among the optimal ones
    assert np.abs(m - want["mean"]).max() <= TOL
    assert m[2, 3] <= 1e-5                                          # a line maps onto a line
    R = got["transform"][:, 1:10].reshape(-1, 3, 3).astype(np.float64)
    assert np.abs(np.einsum("bij,bkj->bik", R, R) - np.eye(3)).max() <= 1e-5 and np.abs(np.linalg.det(R) - 1).max() <= 1e-5
    for n in (1, 2, 3):
        pn, gn = p[:1, :n].copy(), g[:1, :n].copy()
        o = _run(pn, gn, transform=True, per_point=3)
        w = orc.align(pn, gn)
        assert np.isfinite(o["mean_err"]).all() and np.abs(o["mean_err"] - w["mean"]).max() <= TOL, n
        Rn = o["transform"][0, 1:10].reshape(3, 3).astype(np.float64)
        assert np.abs(Rn @ Rn.T - np.eye(3)).max() <= 1e-5 and abs(np.linalg.det(Rn) - 1) <= 1e-5, n
        assert int(o["status"][0]) == {1: eval3d.DEGENERATE, 2: eval3d.RANK_DEFICIENT, 3: 0}[n]
        if n == 1:
            assert o["mean_err"][0, 1] == 0 and o["transform"][0, 0] == 1
        if n == 2:
            assert o["mean_err"][0, 3] <= 1e-6                       # two points always align exactly


@pytest.mark.parametrize("N", [24, 1378])
@pytest.mark.parametrize("offset", [0.0, 10.0])
def test_collinear_prediction_in_fp32_is_flagged(N, offset):
    """A prediction on a line against a full cloud, at the origin and 10 m out: the fp32 rounding of the line's points
    leaves S2 / S1 of 1e-8 to 1e-6, which the flag must take for zero (the threshold comes from the inputs' precision:
    1e-5), while 1 cm off a 1 m line is a real second direction.  The error is the minimal one in both rows."""
    from ilps_amd import eval3d
    rng = np.random.default_rng(4)
    g = (rng.normal(size=(2, N, 3)) * 0.4 + offset).astype(np.float32)
    lin = np.linspace(-1, 1, N)
    p = np.stack([np.outer(lin, [0.3, -0.2, 0.9]), np.outer(lin, [0.3, -0.2, 0.9])]) + offset
    p[1] += np.outer(np.cos(7 * lin), [0.9, 0, -0.3]) * 0.01
    p = p.astype(np.float32)
    want = orc.align(p, g)
    got = _run(p, g, transform=True)
    pc, gc = p.astype(np.float64) - p.astype(np.float64).mean(1, keepdims=True), g - g.astype(np.float64).mean(1, keepdims=True)
    S = np.linalg.svd(np.einsum("bnr,bnc->brc", gc, pc), compute_uv=False)
    print("eval3d collinear N=%d offset=%g: S2/S1 %.1e %.1e, status %s, max mean diff %.2e" % (
        N, offset, *(S[:, 1] / S[:, 0]), got["status"].tolist(), np.abs(got["mean_err"] - want["mean"]).max()))
    assert got["status"].tolist() == [eval3d.RANK_DEFICIENT, 0]
    assert np.abs(got["mean_err"] - want["mean"]).max() <= TOL


@pytest.mark.parametrize("N", [19, 6890])
def test_hostile_rows_stay_in_their_row(N):
    from ilps_amd import eval3d
    pred, gt = orc.make_case(8, N, seed=77)
    pred[3, N // 2, 1] = np.nan
    gt[4, 0, 0] = np.inf
    pred[5] *= 1e30
    gt[5] *= 1e30
    kw = dict(per_point=3, transform=True)
    got = _run(pred, gt, **kw)
    for b in (3, 4, 5):
        assert np.isnan(got["mean_err"][b]).all() and got["status"][b] & eval3d.NONFINITE
    for b in (3, 4):
        assert np.isnan(got["per_point"][b]).all() and np.isnan(got["transform"][b]).all()
    for b in (0, 1, 2, 6, 7):
        alone = _run(pred[b:b + 1], gt[b:b + 1], **kw)
        assert got["status"][b] == 0
        for k in ("mean_err", "per_point", "transform", "status"):
            assert np.array_equal(got[k][b], alone[k][0]), "%s of row %d changed beside hostile rows" % (k, b)


@pytest.mark.parametrize("N", [19, 1378, 6890])
def test_determinism(N):
    pred, gt = orc.make_case(128, N, seed=5)
    kw = dict(per_point=3, transform=True)
    a, b = _run(pred, gt, **kw), _run(pred, gt, **kw)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    for i in (0, 1, 63, 64, 127):
        one = _run(pred[i:i + 1], gt[i:i + 1], **kw)
        for k in a:
            assert np.array_equal(a[k][i], one[k][0]), "%s of mesh %d differs between B = 128 and B = 1" % (k, i)


@pytest.mark.parametrize("N,root", [(19, 0), (19, 18), (24, 7), (1378, 1000)])
def test_root_mode(N, root):
    pred, gt = orc.make_case(5, N, seed=9)
    got = _run(pred, gt, root=root, per_point=1)
    host = _run(pred - pred[:, root:root + 1], gt - gt[:, root:root + 1], per_point=0)
    assert np.abs(got["per_point"] - host["per_point"]).max() <= 1e-6
    assert np.abs(got["mean_err"][:, 1] - host["mean_err"][:, 0]).max() <= 1e-6
    want = orc.align(pred, gt, root=root)
    assert np.abs(got["per_point"] - want["per_point"][:, 1]).max() <= TOL
    assert np.abs(got["mean_err"] - want["mean"]).max() <= TOL
    assert (got["per_point"][:, root] == 0).all()
    # the root changes the translation mode alone
    plain = _run(pred, gt)
    assert np.array_equal(plain["mean_err"][:, [0, 2, 3]], got["mean_err"][:, [0, 2, 3]])


def test_torch_op_and_ctypes_give_identical_bits():
    from ilps_amd import torch_ops
    ns = torch_ops.load()
    for N in (19, 1378, 6890):
        pred, gt = orc.make_case(6, N, seed=N + 1)
        p, g = torch.as_tensor(pred, device=_dev()), torch.as_tensor(gt, device=_dev())
        for mode in (0, 3):
            c = _run(pred, gt, root=2, per_point=mode, transform=True)
            mean, status, pp, tr = ns.point_errors(p, g, 2, mode, True)
            assert np.array_equal(mean.cpu().numpy(), c["mean_err"]) and np.array_equal(status.cpu().numpy(), c["status"])
            assert np.array_equal(pp.cpu().numpy(), c["per_point"]) and np.array_equal(tr.cpu().numpy(), c["transform"])
        mean, status, pp, tr = ns.point_errors(p, g)
        assert pp.numel() == 0 and tr.numel() == 0 and np.array_equal(mean.cpu().numpy()[:, [0, 2, 3]], c["mean_err"][:, [0, 2, 3]])
    e = ns.point_errors(torch.empty(0, 19, 3, device=_dev()), torch.empty(0, 19, 3, device=_dev()))
    assert e[0].shape == (0, 4)


def test_bad_arguments_raise_instead_of_faulting():
    from ilps_amd import _lib, torch_ops
    from ilps_amd.eval3d import point_errors
    ns = torch_ops.load()
    d = _dev()
    p = torch.zeros(2, 19, 3, device=d)
    with pytest.raises(RuntimeError, match="shape"):
        ns.point_errors(p, torch.zeros(2, 18, 3, device=d))
    with pytest.raises(RuntimeError, match="shape"):
        point_errors(p, torch.zeros(3, 19, 3, device=d))
    with pytest.raises((RuntimeError, NotImplementedError)):
        ns.point_errors(torch.zeros(2, 19, 3), torch.zeros(2, 19, 3))
    with pytest.raises(RuntimeError):
        ns.point_errors(p, torch.zeros(2, 19, 3))                  # gt on the CPU
    with pytest.raises(RuntimeError, match="lives on"):
        point_errors(p, torch.zeros(2, 19, 3))
    with pytest.raises(RuntimeError, match="root"):
        ns.point_errors(p, p, 19)
    with pytest.raises(RuntimeError, match="root"):
        point_errors(p, p, root=-2)
    with pytest.raises(RuntimeError, match="float32"):
        ns.point_errors(p.double(), p.double())
    with pytest.raises(RuntimeError, match="contiguous"):
        ns.point_errors(torch.zeros(2, 3, 19, device=d).transpose(1, 2), p)
    lib = _lib.load()
    mean = torch.zeros(2, 4, device=d)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    assert lib.smplr_point_errors(vp(p), vp(p), 2, 19, 19, 0, vp(mean), None, None, None, None) == -1
    assert b"root=19" in lib.smplr_last_error()
    assert lib.smplr_point_errors(vp(p), None, 2, 19, 0, 0, vp(mean), None, None, None, None) == -1
    # the Python front makes strided and double inputs contiguous fp32 itself
    q = torch.rand(2, 3, 19, device=d, dtype=torch.float64).transpose(1, 2)
    a = point_errors(q, q * 1.5 + 0.25)["mean_err"]
    b = point_errors(q.float().contiguous(), (q * 1.5 + 0.25).float().contiguous())["mean_err"]
    assert torch.equal(a, b) and float(a[:, 3].max()) <= 1e-6


class _Identity(torch.nn.Module):
    """The regressor's stand-in: the 'image' is the (N, 86) answer."""

    def forward(self, images):
        return images


def test_eval3d_and_evaluate_3d_on_decoder_outputs(smpl_model):
    """`Eval3D` and `evaluate_3d` on SMPLLayer vertices and joints for perturbed parameters against the oracle's dataset
    means (taken over the same decoded point sets)."""
    from _inputs import make_x
    from ilps_amd.eval3d import Eval3D
    from ilps_amd.evaluation import evaluate_3d, evaluate_pose_param_mse
    from ilps_amd.keras_smpl.batch_smpl import SMPLLayer
    d = _dev()
    layer = SMPLLayer(smpl_model, device=d)
    rng = np.random.default_rng(21)
    sizes = (5, 16, 3)
    xs, ys = [], []
    for i, n in enumerate(sizes):
        x = make_x(n, 48, seed=30 + i).astype(np.float32)
        y = x.copy()
        y[:, 4:76] += rng.normal(0, 0.08, (n, 72)).astype(np.float32)
        y[:, 76:] += rng.normal(0, 0.5, (n, 10)).astype(np.float32)
        xs.append(torch.as_tensor(x, device=d))
        ys.append(torch.as_tensor(y, device=d))
    root = 2
    res = evaluate_3d(_Identity(), layer, [(x, (y[:, 4:76], y[:, 76:86])) for x, y in zip(xs, ys)], root_joint=root)
    pv = np.concatenate([layer(x).cpu().numpy() for x in xs])
    gv = np.concatenate([layer(torch.cat([x[:, :4], y[:, 4:]], 1)).cpu().numpy() for x, y in zip(xs, ys)])
    jr = layer.constants(d).joint_regressor
    pj = torch.einsum("bvc,vj->bjc", torch.as_tensor(pv, device=d), jr).cpu().numpy()
    gj = torch.einsum("bvc,vj->bjc", torch.as_tensor(gv, device=d), jr).cpu().numpy()
    wv, wj = orc.align(pv, gv)["mean"].mean(0), orc.align(pj, gj, root=root)["mean"].mean(0)
    print("evaluate_3d:", {k: (round(v, 6) if isinstance(v, float) else v) for k, v in res.items()})
    assert res["count"] == sum(sizes) and res["joint_count"] == sum(sizes) and res["nonfinite"] == 0
    for key, w in (("pve", wv[0]), ("pve_t", wv[1]), ("pve_sc", wv[2]), ("pve_pa", wv[3]), ("mpjpe", wj[0]),
                   ("mpjpe_root", wj[1]), ("mpjpe_pa", wj[3])):
        assert abs(res[key] - w) <= TOL, (key, res[key], w)
    assert res["pve"] > res["pve_pa"] > 1e-4
    want_mse = evaluate_pose_param_mse(_Identity(), [(x, y[:, 4:76]) for x, y in zip(xs, ys)])
    assert abs(res["pose_mse"] - want_mse) <= 1e-12
    # ground-truth vertices instead of parameters, and the accumulator by itself
    lo = np.cumsum((0,) + sizes)
    res_v = evaluate_3d(_Identity(), layer, [(x, torch.as_tensor(gv[a:b], device=d)) for x, a, b in zip(xs, lo[:-1], lo[1:])])
    for key in ("pve", "pve_t", "pve_sc", "pve_pa"):
        assert res_v[key] == res[key], key
    for key in ("mpjpe", "mpjpe_pa"):
        assert abs(res_v[key] - res[key]) <= 1e-6, key
    assert res_v["pose_mse"] is None
    m = Eval3D(d, keep_per_mesh=True)
    for a, b in zip(lo[:-1], lo[1:]):
        m.update(torch.as_tensor(pv[a:b], device=d), torch.as_tensor(gv[a:b], device=d))
    r = m.result()
    assert r["count"] == sum(sizes) and abs(r["similarity"] - wv[3]) <= TOL and abs(r["none"] - res["pve"]) <= 1e-9
    assert m.per_mesh().shape == (sum(sizes), 4)
