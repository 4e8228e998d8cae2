"""The fused silhouette loss head without a GPU: its ABI and torch-op surface, what the compiler says about its kernels,
the float64 restatement of its formula (tests/_silh_loss_oracle.py) against the oracle's Keras losses and against finite
differences, the constructors' refusals and the timing tool's host-side parts."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

import _silh_loss_oracle as slo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "smplraster.h")
sys.path.insert(0, os.path.join(ROOT, "tools"))

ENTRY_POINTS = {"smplr_silh_loss_fwd": 10, "smplr_silh_fwd_loss": 15, "smplr_silh_loss_bwd": 11}


def test_abi_has_the_three_entry_points_and_stays_version_7():
    from ilps_amd import _lib
    src = open(HEADER).read()
    assert "#define SMPLR_ABI_VERSION 7" in src
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs in ENTRY_POINTS.items():
        m = re.search(r"\b%s\s*\(([^)]*)\)" % name, code)
        assert m, "%s is not declared in the header" % name
        assert m.group(1).count(",") + 1 == nargs == len(_lib.SIGNATURES[name][1]), name
        assert hasattr(lib, name), "%s is not exported" % name
    assert _lib.load().smplr_abi_version() == _lib.ABI_VERSION == 7


def test_argument_errors_are_reported_without_a_launch():
    from ilps_amd import _lib
    lib = _lib.load()
    assert lib.smplr_silh_loss_fwd(None, None, None, 0.0, 1, 48, None, None, None, None) == -1
    assert b"smplr_silh_loss_fwd" in lib.smplr_last_error()
    assert lib.smplr_silh_loss_fwd(None, None, None, -1.0, 1, 48, None, None, None, None) == -1
    assert b"gamma" in lib.smplr_last_error()
    assert lib.smplr_silh_loss_fwd(None, None, None, 0.0, 0, 48, None, None, None, None) == 0      # empty batch: a no-op
    assert lib.smplr_silh_fwd_loss(None, None, None, None, 0.0, 1, 6890, 48, None, None, None, None, None, None, None) == -1
    assert b"smplr_silh_fwd_loss" in lib.smplr_last_error()
    assert lib.smplr_silh_fwd_loss(None, None, None, None, 0.0, 1, 6890, 0, None, None, None, None, None, None, None) == -1
    assert lib.smplr_silh_fwd_loss(None, None, None, None, 0.0, 0, 6890, 48, None, None, None, None, None, None, None) == 0
    assert lib.smplr_silh_loss_bwd(None, None, None, None, None, 1, 6890, 48, None, 0, None) == -1
    assert b"smplr_silh_loss_bwd" in lib.smplr_last_error()
    assert lib.smplr_silh_loss_bwd(None, None, None, None, None, 0, 6890, 48, None, 1, None) == 0


def test_torch_op_schemas_and_meta_kernels():
    import torch
    from ilps_amd import torch_ops
    ns = torch_ops.load()
    for name in ("silh_loss_fwd", "silh_fwd_loss", "silh_loss_bwd"):
        assert str(getattr(ns, name).default._schema) == torch_ops.SCHEMAS[name], name
    m = lambda *s, dt=torch.float32: torch.empty(*s, dtype=dt, device="meta")
    loss, k = ns.silh_loss_fwd(m(2, 50, 50, 2), m(2, 50, 50, dt=torch.int32), None, 0.0, None)
    assert loss.shape == k.shape == (2, 2500)
    silh, arg, loss, k = ns.silh_fwd_loss(m(2, 6890, 3), None, m(2, 48, 48, dt=torch.int32), m(2), 2.0, 48, None)
    assert silh.shape == (2, 48, 48, 2) and arg.shape == (2, 48, 48) and arg.dtype == torch.int32
    assert loss.shape == k.shape == (2, 2304)
    assert ns.silh_loss_bwd(loss, k, silh, arg, m(2, 6890, 3), True).shape == (2, 6890, 3)
    with pytest.raises((RuntimeError, NotImplementedError)):
        ns.silh_loss_fwd(torch.zeros(1, 4, 4, 2), torch.zeros(1, 4, 4, dtype=torch.int32), None, 0.0, None)   # CPU tensors


def test_kernel_resources():
    import kernel_resources as kr
    ks = kr.kernels()
    pick = lambda pat: {n: k for n, k in ks.items() if pat in n}
    fwd, bwd, px = pick("silh_loss_fwd_kernel"), pick("silh_loss_bwd_kernel"), pick("silh_px_kernel")
    assert len(fwd) == 1 and len(bwd) == 2 and len(px) == 2, (list(fwd), list(bwd), list(px))
    for name, k in fwd.items():
        assert k["scratch"] == 0 and kr.waves_per_simd(k) >= 8, (name, k)
    for name, k in bwd.items():
        assert k["scratch"] == 0 and k["max_threads"] >= 1024 and kr.waves_per_simd(k) >= 4, (name, k)
    for name, k in px.items():
        assert k["scratch"] == 0 and k["max_threads"] >= 1024 and kr.waves_per_simd(k) >= 4, (name, k)
        assert k["lds"] <= 160 * 1024 - 159 * 1024, "%s: %d B of static LDS beside the layout's 159 KB" % (name, k["lds"])


# ---------------------------------------------------------------------------------------------------------- formula
def _case(seed, n=4000):
    rng = np.random.default_rng(seed)
    s = np.concatenate([rng.uniform(0.0, 1.0, n - 3), [0.0, 0.5, 1.0]])
    t = rng.integers(0, 2, n)
    return s, t


@pytest.mark.parametrize("gamma,weighted", [(0.0, False), (0.0, True), (1.5, False), (1.5, True), (2.0, False), (2.0, True)])
def test_formula_is_the_keras_loss_on_the_softmax(gamma, weighted):
    from oracle import np_oracle as o
    s, t = _case(int(gamma * 10) + weighted)
    z = np.stack([1.0 - s, s], axis=-1)[None]                    # (1, n, 2)
    y = np.eye(2)[t][None]
    p = o.softmax_last(z)
    L, _ = slo.silh_loss(s, t, gamma, slo.FOCAL_W2 if weighted else None)
    assert tuple(o.FOCAL_CLASS_WEIGHTS[:2]) == slo.FOCAL_W2
    want = o.categorical_focal_loss(y, p, gamma, weighted)[0]
    err = float(np.abs(L - want).max())
    print("gamma %g weighted %s: max |L - categorical_focal_loss| %.2e" % (gamma, weighted, err))
    assert err <= 1e-12
    if gamma == 0.0 and not weighted:
        err = float(np.abs(L - o.categorical_crossentropy(y, p)[0]).max())
        print("max |L - categorical_crossentropy| %.2e" % err)
        assert err <= 1e-12


def test_the_clip_cannot_bind():
    """p lies in [0.2689, 0.7311] for s in [0, 1]: the reference's clip to [1e-7, 1 - 1e-7] is the identity."""
    from oracle import np_oracle as o
    s = np.linspace(0.0, 1.0, 101)
    p = o.softmax_last(np.stack([1.0 - s, s], axis=-1)[None])
    assert 0.2689 < p.min() and p.max() < 0.7311


@pytest.mark.parametrize("gamma,weighted", [(0.0, False), (1.5, True), (2.0, False), (2.0, True)])
def test_k_is_the_derivative_of_the_loss(gamma, weighted):
    """Central differences of L(s) over s in linspace(0, 1, 101), h = 1e-6: truncation h^2 |L'''| / 6 ~ 1e-12 and
    rounding eps |L| / h ~ 2e-10, against a bar of 1e-8."""
    s = np.linspace(0.0, 1.0, 101)
    w = slo.FOCAL_W2 if weighted else None
    h = 1e-6
    for t in (0, 1):
        lab = np.full(s.shape, t)
        _, k = slo.silh_loss(s, lab, gamma, w)
        fd = (slo.silh_loss(s + h, lab, gamma, w)[0] - slo.silh_loss(s - h, lab, gamma, w)[0]) / (2 * h)
        err = float(np.abs(k - fd).max())
        print("gamma %g weighted %s t=%d: max |k - finite difference| %.2e" % (gamma, weighted, t, err))
        assert err <= 1e-8
        if gamma == 0.0 and not weighted:          # the closed form: -2 p0 for t = 1, +2 p1 for t = 0
            p1 = 1.0 / (1.0 + np.exp(1.0 - 2.0 * s))
            assert np.abs(k - (-2.0 * (1.0 - p1) if t else 2.0 * p1)).max() <= 1e-14


def test_labels_outside_the_classes_and_nan_scores():
    s = np.array([0.3, 0.3, 0.3, 0.3, np.nan, np.nan])
    t = np.array([-1, 2, 255, 1, 0, 7])
    L, k = slo.silh_loss(s, t, 2.0, slo.FOCAL_W2)
    assert np.all(L[:3] == 0) and np.all(k[:3] == 0) and L[3] > 0 and k[3] < 0
    assert np.isnan(L[4]) and np.isnan(k[4]) and L[5] == 0 and k[5] == 0
    silh = np.stack([1.0 - s, s], axis=-1)
    assert slo.confusion(silh, t).tolist() == [[1, 0], [1, 0], [4, 0]]
    assert slo.confusion(np.array([[0.5, 0.5], [0.4, 0.6]]), np.array([1, 1])).tolist() == [[0, 0], [1, 1], [0, 0]]


# ----------------------------------------------------------------------------------------------------- constructors
def test_constructors_refuse_a_silhouette_loss_without_its_head(smpl_model):
    from ilps_amd.decoder import SMPLDecoder
    from ilps_amd.focal_loss import softmax_focal_loss
    from ilps_amd.training import SegTrainer
    ce = softmax_focal_loss(0.0, False)
    with pytest.raises(ValueError, match="silhouette"):
        SMPLDecoder(smpl_model, heads=("seg",), silh_loss=ce)
    with pytest.raises(ValueError, match="softmax_focal_loss"):
        SMPLDecoder(smpl_model, heads=("silhouette",), silh_loss=lambda y, s: s)
    dec = SMPLDecoder(smpl_model, heads=("seg", "silhouette"), silh_loss=ce)
    assert dec.silh_loss is ce and dec.loss is None
    with pytest.raises(ValueError, match="with_silhouette"):
        SegTrainer(smpl_model, fused_silh_loss=True, with_silhouette=False, device="cpu")


def test_decoder_opts_defaults_leave_the_silhouette_head_unfused():
    from ilps_amd import ops
    o = ops.DecoderOpts()
    assert o.silh_loss is None and o.silh_confusion is None
    for name in ("_silh_loss_fwd", "_silh_fwd_loss", "_silh_loss_bwd"):
        assert callable(getattr(ops, name))


# -------------------------------------------------------------------------------------------------------------- tool
def test_timing_tool_arguments_and_trace_summary(tmp_path):
    import silh_loss_time as st
    a = st.parse_args([])
    assert a.iters >= 200 and a.blocks >= 4 and a.batches == [128, 512] and a.wh == 48
    assert st.VARIANTS == ("unfused", "standalone", "epilogue") and st.PASSES == ("silh", "both")
    with pytest.raises(SystemExit):
        st.parse_args(["--iters", "50"])
    with pytest.raises(SystemExit):
        st.parse_args(["--blocks", "2"])
    assert st.parse_args(["--kernels-only", "--batches", "128"]).batches == [128]
    s = st.summarise([10.0, 12.0, 11.0, 11.5])
    assert s == {"median_us": 11.25, "spread_us": 2.0, "blocks_us": [10.0, 12.0, 11.0, 11.5]}
    fast, slow = st.summarise([5.0, 5.5, 5.2, 5.1]), st.summarise([7.0, 7.2, 7.1, 7.3])
    assert st.verdict(fast, slow) == "faster" and st.verdict(slow, fast) == "slower" and st.verdict(s, st.summarise([11, 12, 10, 13])) == "same"
    csv = tmp_path / "k.csv"
    rows = ['"Kernel_Name","Workgroup_Size_X","Grid_Size_X","Start_Timestamp","End_Timestamp"']
    rows += ['"void smplr::silh_px_kernel<true>(float const*, int)",1024,%d,%d,%d' % (1024 * 256, 1000 * i, 1000 * i + 30000 + 1000 * i)
             for i in range(3)]
    rows += ['"smplr::silh_loss_fwd_kernel(float const*, smplr::SilhLossIO, long long)",256,%d,0,4000' % (256 * 1024)]
    rows += ['"void smplr::silh_loss_bwd_kernel<false>(float const*)",1024,%d,0,9500' % (1024 * 256)]
    rows += ['"other_kernel",256,256,0,5']
    csv.write_text("\n".join(rows) + "\n")
    assert st.trace_medians(str(csv)) == {
        "silh_loss_bwd_kernel<false> workgroups 256": {"n": 1, "median_us": 9.5, "min_us": 9.5},
        "silh_loss_fwd_kernel workgroups 1024": {"n": 1, "median_us": 4.0, "min_us": 4.0},
        "silh_px_kernel<true> workgroups 256": {"n": 3, "median_us": 31.0, "min_us": 30.0}}
