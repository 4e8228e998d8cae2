"""3D evaluation without a GPU: the float64 torch path of `eval3d.point_errors` against the NumPy oracle, the `Eval3D`
accumulator (uneven batches, two gloo ranks), `evaluation.evaluate_3d` on the synthetic SMPL model with a stub regressor
and a CPU stand-in for the SMPL layer, argument errors, the ABI / torch-op surface and the kernels' resources."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ilps_amd  # noqa: E402,F401
from ilps_amd import eval3d  # noqa: E402
from ilps_amd.eval3d import Eval3D, point_errors  # noqa: E402
import _eval3d_oracle as orc  # noqa: E402


@pytest.mark.parametrize("B,N", [(1, 14), (5, 19), (4, 24), (3, 300), (2, 1378)])
def test_cpu_path_matches_the_oracle(B, N):
    pred, gt = orc.make_case(B, N, seed=100 + N)
    want = orc.align(pred, gt)
    assert want["gap"].min() >= 0.02
    assert (want["d"][1::3] < 0).all() and (want["d"][0::3] > 0).all()      # the mirrored sets take the reflection branch
    for mode in range(4):
        got = point_errors(torch.from_numpy(pred), torch.from_numpy(gt), per_point=mode, transform=True)
        assert got["mean_err"].dtype == torch.float32 and got["mean_err"].shape == (B, 4)
        np.testing.assert_allclose(got["mean_err"].numpy(), want["mean"], rtol=0, atol=1e-6)
        np.testing.assert_allclose(got["per_point"].numpy(), want["per_point"][:, mode], rtol=0, atol=1e-6)
        assert int(got["status"].abs().sum()) == 0
    tr = got["transform"].numpy().astype(np.float64)
    np.testing.assert_allclose(tr[:, 0], want["s"], rtol=1e-6)
    np.testing.assert_allclose(tr[:, 1:10].reshape(B, 3, 3), want["R"], atol=1e-6)
    np.testing.assert_allclose(tr[:, 10:], want["t"], atol=1e-5)
    assert point_errors(torch.from_numpy(pred), torch.from_numpy(gt), per_point="similarity")["per_point"].shape == (B, N)


def test_root_relative_mode():
    pred, gt = orc.make_case(4, 19, seed=7)
    want = orc.align(pred, gt, root=3)
    got = point_errors(torch.from_numpy(pred), torch.from_numpy(gt), root=3, per_point="translation")
    np.testing.assert_allclose(got["per_point"].numpy(), want["per_point"][:, 1], atol=1e-6)
    np.testing.assert_allclose(got["mean_err"].numpy(), want["mean"], atol=1e-6)
    assert float(got["per_point"][:, 3].abs().max()) == 0.0                 # the root itself


@pytest.mark.parametrize("offset", [0.0, 1.0, 10.0])
def test_collinear_prediction_in_fp32_is_flagged(offset):
    """A prediction on a line against a full cloud: M has rank 1 in exact arithmetic, but the fp32 rounding of the line's
    points leaves S2 / S1 of 1e-8 (at the origin) to 1e-6 (10 m out).  The flag follows the inputs' precision, not
    float64's; the error is still the minimal one, and a thin but real second direction (1 cm on 1 m) is not flagged."""
    rng = np.random.default_rng(4)
    g = (rng.normal(size=(2, 24, 3)) * 0.4 + offset).astype(np.float32)
    lin = np.linspace(-1, 1, 24)
    p = np.stack([np.outer(lin, [0.3, -0.2, 0.9]), np.outer(lin, [0.3, -0.2, 0.9])]) + offset
    p[1] += np.outer(np.cos(7 * lin), [0.9, 0, -0.3]) * 0.01          # 1 cm off the line
    p = p.astype(np.float32)
    want = orc.align(p, g)
    got = point_errors(torch.from_numpy(p), torch.from_numpy(g), transform=True)
    assert got["status"].tolist() == [eval3d.RANK_DEFICIENT, 0]
    np.testing.assert_allclose(got["mean_err"].numpy(), want["mean"], rtol=0, atol=1e-6)


def test_degenerate_and_hostile_rows_cpu():
    rng = np.random.default_rng(3)
    g = rng.normal(size=(6, 8, 3)).astype(np.float32)
    p = (g + rng.normal(size=g.shape) * 0.01).astype(np.float32)
    p[1] = p[1, :1]                                   # coincident prediction: sum |pc|^2 = 0
    p[2] = np.outer(np.linspace(-1, 1, 8), [1, 2, 3])  # collinear in both sets
    g[2] = np.outer(np.linspace(-1, 1, 8), [3, 1, -2]) * 1.5
    p[3, 4, 1] = np.nan
    p[4] = g[4]                                       # exact
    got = point_errors(torch.from_numpy(p), torch.from_numpy(g), transform=True)
    st = got["status"].numpy()
    assert st[0] == 0 and st[1] == eval3d.DEGENERATE and st[2] == eval3d.RANK_DEFICIENT and st[3] == eval3d.NONFINITE
    m = got["mean_err"].numpy()
    assert np.isnan(m[3]).all() and np.isfinite(np.delete(m, 3, 0)).all()
    assert m[1, 2] == m[1, 1] == m[1, 3]              # the fall-back: translation only
    assert m[2, 3] < 1e-6                             # a line maps onto a line exactly
    assert (m[4, :2] == 0).all() and (m[4, 2:] < 1e-6).all() and abs(float(got["transform"][4, 0]) - 1) < 1e-6
    R = got["transform"][2, 1:10].reshape(3, 3).double().numpy()
    np.testing.assert_allclose(R @ R.T, np.eye(3), atol=1e-6)
    assert abs(np.linalg.det(R) - 1) < 1e-6
    one = point_errors(torch.from_numpy(p[:1, :1]), torch.from_numpy(g[:1, :1]))
    assert int(one["status"][0]) == eval3d.DEGENERATE and float(one["mean_err"][0, 1]) == 0.0


def test_accumulation_over_uneven_batches_equals_one_pass():
    pred, gt = orc.make_case(23, 19, seed=11)
    pred[5, 2, 0] = np.inf                             # one mesh left out, and counted as such
    p, g = torch.from_numpy(pred), torch.from_numpy(gt)
    whole = Eval3D(keep_per_mesh=True).update(p, g)
    parts = Eval3D(keep_per_mesh=True)
    for lo, hi in ((0, 1), (1, 8), (8, 20), (20, 23)):
        parts.update(p[lo:hi], g[lo:hi])
    a, b = whole.result(), parts.result()
    assert a["count"] == b["count"] == 22 and a["nonfinite"] == b["nonfinite"] == 1
    keep = np.delete(np.arange(23), 5)
    want = orc.align(pred[keep], gt[keep])["mean"].mean(0)
    for i, name in enumerate(eval3d.MODES):
        assert abs(a[name] - b[name]) < 1e-12
        assert abs(a[name] - want[i]) < 1e-6
    assert torch.equal(whole.per_mesh()[keep], parts.per_mesh()[keep]) and parts.per_mesh().shape == (23, 4)
    assert parts.reset().result()["count"] == 0 and np.isnan(parts.result()["none"])
    with pytest.raises(RuntimeError, match="keep_per_mesh"):
        Eval3D().per_mesh()


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import ilps_amd  # noqa: F401
    from ilps_amd.eval3d import Eval3D
    import _eval3d_oracle as orc
    dist.init_process_group("gloo", rank=rank, world_size=world)
    pred, gt = orc.make_case(10, 14, seed=5)
    lo, hi = (0, 3) if rank == 0 else (3, 10)
    m = Eval3D().update(torch.from_numpy(pred[lo:hi]), torch.from_numpy(gt[lo:hi])).all_reduce()
    if rank == 0:
        out.put(m.result())
    dist.barrier()
    dist.destroy_process_group()


def test_all_reduce_two_ranks_gloo():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = q.get(timeout=120)
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    pred, gt = orc.make_case(10, 14, seed=5)
    want = orc.align(pred, gt)["mean"].mean(0)
    assert res["count"] == 10 and res["nonfinite"] == 0
    for i, name in enumerate(eval3d.MODES):
        assert abs(res[name] - want[i]) < 1e-6


class _CpuLayer:
    """A CPU stand-in for SMPLLayer (which has no CPU path): the float64 NumPy oracle of the SMPL forward."""

    num_cam = 4

    def __init__(self, model):
        self.model = model

    def constants(self, device):
        class C:
            joint_regressor = torch.from_numpy(np.asarray(self.model.cocoplus_regressor, np.float64).T.copy()).float()
        return C

    def __call__(self, x):
        from oracle import np_oracle as o
        return torch.from_numpy(o.smpl_layer_call(x.numpy().astype(np.float64), self.model).astype(np.float32))

    def joints(self, verts):
        return torch.einsum("bvc,vj->bjc", verts, self.constants(None).joint_regressor)


class _StubRegressor(torch.nn.Module):
    """images (N, 86): the 'image' is the answer."""

    def forward(self, images):
        return images


def _params(n, seed):
    from ilps_amd.smpl_model import mean86
    rng = np.random.default_rng(seed)
    x = np.tile(mean86(48), (n, 1))
    x[:, 4:76] += rng.normal(0, 0.2, (n, 72))
    x[:, 76:] += rng.normal(0, 1.0, (n, 10))
    return torch.from_numpy(x.astype(np.float32))


def test_evaluate_3d_on_the_synthetic_model():
    from ilps_amd.evaluation import evaluate_3d, evaluate_pose_param_mse
    from ilps_amd.smpl_model import synthetic_smpl_model
    sys.path.insert(0, ROOT)
    model = synthetic_smpl_model(1234, num_verts=600)
    layer, reg = _CpuLayer(model), _StubRegressor()
    xs = [_params(2, 1), _params(3, 2)]
    # ground truth = the prediction's own parameters: every error is zero
    res = evaluate_3d(reg, layer, [(x, (x[:, 4:76], x[:, 76:86])) for x in xs], root_joint=0)
    assert res["count"] == 5 and res["joint_count"] == 5 and res["nonfinite"] == 0
    for k in ("pve", "pve_t", "mpjpe", "mpjpe_root", "pose_mse"):
        assert res[k] == 0.0, k
    for k in ("pve_sc", "pve_pa", "mpjpe_pa"):            # (s and R come out of an SVD: 1 and I to rounding)
        assert res[k] < 1e-7, k
    # ground-truth vertices with a planted rigid offset: pve = the offset where it is a pure translation, and only the
    # Procrustes mode removes a rotation
    t0 = torch.tensor([0.3, -0.4, 1.2])
    res = evaluate_3d(reg, layer, [(x, layer(x) + t0) for x in xs])
    assert abs(res["pve"] - 1.3) < 1e-5 and abs(res["mpjpe"] - 1.3) < 1e-5
    assert res["pve_t"] < 1e-6 and res["pve_pa"] < 1e-6 and res["mpjpe_root"] < 1e-6 and res["pose_mse"] is None
    Rz = torch.from_numpy(orc.random_rotation(np.random.default_rng(4))).float()
    res = evaluate_3d(reg, layer, [(x, layer(x) @ Rz.T * 1.0 + t0) for x in xs])
    assert res["pve_pa"] < 1e-5 and res["mpjpe_pa"] < 1e-5 and res["pve_t"] > 1e-2 and res["pve_sc"] > 1e-2
    # other parameters as ground truth: the pose MSE is evaluate_pose_param_mse's number
    ys = [_params(2, 8), _params(3, 9)]
    res = evaluate_3d(reg, layer, [(x, (y[:, 4:76], y[:, 76:86])) for x, y in zip(xs, ys)])
    assert abs(res["pose_mse"] - evaluate_pose_param_mse(reg, [(x, y[:, 4:76]) for x, y in zip(xs, ys)])) < 1e-12
    assert res["pve"] > res["pve_pa"] > 0
    with pytest.raises(ValueError, match="no batches"):
        evaluate_3d(reg, layer, [])
    with pytest.raises(ValueError, match="gt_pose"):
        evaluate_3d(reg, layer, [(xs[0], (xs[0][:, 4:70], xs[0][:, 76:86]))])


def test_argument_errors_are_reported():
    p = torch.zeros(2, 5, 3)
    with pytest.raises(RuntimeError, match="shape"):
        point_errors(p, torch.zeros(2, 4, 3))
    with pytest.raises(RuntimeError, match=r"\(B, N, 3\)"):
        point_errors(torch.zeros(2, 5, 2), torch.zeros(2, 5, 2))
    with pytest.raises(RuntimeError, match="root"):
        point_errors(p, p, root=5)
    with pytest.raises(RuntimeError, match="at least one point"):
        point_errors(torch.zeros(2, 0, 3), torch.zeros(2, 0, 3))
    with pytest.raises(ValueError, match="mode"):
        point_errors(p, p, per_point="rigid")
    with pytest.raises(ValueError, match="mode"):
        point_errors(p, p, per_point=4)
    assert point_errors(torch.zeros(0, 5, 3), torch.zeros(0, 5, 3))["mean_err"].shape == (0, 4)
    # the C entry point: argument errors come back through smplr_last_error, without a launch
    from ilps_amd import _lib
    lib = _lib.load()
    f = lib.smplr_point_errors
    one = 1                                            # (a non-null pointer value that is never dereferenced: no launch)
    assert f(one, one, 2, 0, -1, 0, one, None, None, None, None) == -1 and b"N=0" in lib.smplr_last_error()
    assert f(one, one, 2, 19, 19, 0, one, None, None, None, None) == -1 and b"root=19" in lib.smplr_last_error()
    assert f(one, one, 2, 19, -2, 0, one, None, None, None, None) == -1 and b"root" in lib.smplr_last_error()
    assert f(one, one, 2, 19, 0, 4, one, None, None, None, None) == -1 and b"mode" in lib.smplr_last_error()
    assert f(None, one, 2, 19, 0, 0, one, None, None, None, None) == -1 and b"null" in lib.smplr_last_error()
    assert f(one, one, 2, 19, 0, 0, None, None, None, None, None) == -1 and b"null" in lib.smplr_last_error()
    assert f(one, one, -1, 19, 0, 0, one, None, None, None, None) == -1
    assert f(None, None, 0, 19, 0, 0, None, None, None, None, None) == 0        # an empty batch is a no-op


def test_abi_symbol_and_torch_op_schema():
    from ilps_amd import _lib, torch_ops
    assert "smplr_point_errors" in _lib.SIGNATURES and len(_lib.SIGNATURES["smplr_point_errors"][1]) == 11
    header = open(os.path.join(ROOT, "include", "smplraster.h")).read()
    assert "int smplr_point_errors(" in header and "#define SMPLR_ABI_VERSION 7" in header
    for name, bit in (("DEGENERATE", 1), ("NONFINITE", 2), ("RANK_DEFICIENT", 4)):
        assert "#define SMPLR_PE_%s %d" % (name, bit) in header and getattr(eval3d, name) == bit
    ns = torch_ops.load()
    assert str(ns.point_errors.default._schema) == torch_ops.SCHEMAS["point_errors"]
    m = lambda *s: torch.empty(*s, device="meta")
    mean, status, pp, tr = ns.point_errors(m(3, 19, 3), m(3, 19, 3), 0, 3, True)
    assert mean.shape == (3, 4) and status.shape == (3,) and status.dtype == torch.int32
    assert pp.shape == (3, 19) and tr.shape == (3, 13)
    mean, status, pp, tr = ns.point_errors(m(3, 19, 3), m(3, 19, 3))
    assert pp.numel() == 0 and tr.numel() == 0
    with pytest.raises(RuntimeError, match="shape"):
        ns.point_errors(m(3, 19, 3), m(3, 18, 3))
    with pytest.raises(RuntimeError, match="root"):
        ns.point_errors(m(3, 19, 3), m(3, 19, 3), 19)
    with pytest.raises((RuntimeError, NotImplementedError)):
        ns.point_errors(torch.zeros(1, 4, 3), torch.zeros(1, 4, 3))           # CPU tensors: no kernel registered


def test_eval3d_kernels_fit_the_budget():
    """No scratch in any form; the vertex form's 84 KB of LDS (gt) leaves one 512-thread workgroup per CU its 256
    registers per lane, the smaller forms at least 3 waves per SIMD."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr
    ks = {n: k for n, k in kr.kernels().items() if "point_errors_kernel" in n}
    assert len(ks) == 5, sorted(ks)
    for name, k in ks.items():
        assert k["scratch"] == 0, "%s spills %d B per lane" % (name, k["scratch"])
        assert k["lds"] <= 160 * 1024 // 1, name
        if "ILi512ELi14E" in name:
            assert k["max_threads"] == 512 and 512 * 14 * 12 <= k["lds"] <= 96 * 1024 and kr.waves_per_simd(k) >= 2, name
        elif "ILi1024E" in name:
            assert kr.waves_per_simd(k) >= 4, name
        else:
            assert k["max_threads"] == 256 and kr.waves_per_simd(k) >= 3, name


def test_timing_tool_counts_and_trace_summary(tmp_path):
    """tools/eval3d_time.py: the compulsory bytes are both point sets read once, and a kernel trace is summarised per
    (kernel form, workgroups)."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import eval3d_time as et
    assert et.compulsory_bytes(1024, 6890) == 2 * 1024 * 6890 * 12 == 169328640
    assert (1, 19) in et.SIZES and (1024, 6890) in et.SIZES and len(et.SIZES) == 6
    csv = tmp_path / "k.csv"
    name = "void smplr::point_errors_kernel<512, 14, false>(float const*, float const*, int)"
    rows = ["Kernel_Name,Workgroup_Size_X,Grid_Size_X,Start_Timestamp,End_Timestamp"]
    rows += ['"%s",512,%d,%d,%d' % (name, 512 * 128, 1000 * i, 1000 * i + 40000 + 1000 * i) for i in range(3)]
    rows += ['"other_kernel",256,256,0,5']
    csv.write_text("\n".join(rows) + "\n")
    out = et.trace_medians(str(csv))
    assert out == {"<512, 14, false> workgroups 128": {"n": 3, "median_us": 41.0, "min_us": 40.0}}
