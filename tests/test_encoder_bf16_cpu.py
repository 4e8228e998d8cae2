"""The bf16 forms of the encoder kernels and the `amp` option, as far as they can be checked without a GPU: the bars of
tests/_encoder_bf16.py are fair (a sound bf16 implementation built from torch's CPU modules stays inside them on every
case the GPU test runs), `training.amp_dtype` validates, the regressor under CPU autocast keeps fp32 at its boundary, the
six smplr_*_bf16 entry points are declared, exported and bound, and their kernels fit the hardware as their fp32 twins do."""
import ctypes
import os
import re
import sys

import pytest
import torch

import _encoder_bf16 as eb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF16_ENTRIES = ("smplr_prelu_fwd_bf16", "smplr_prelu_bwd_bf16", "smplr_bn_fwd_bf16", "smplr_bn_bwd_bf16",
                "smplr_bn_res_fwd_bf16", "smplr_bn_res_bwd_bf16")


@pytest.mark.parametrize("form", eb.FORMS)
@pytest.mark.parametrize("hw", eb.PLANES)
def test_sound_bf16_model_is_inside_every_bar(hw, form):
    """torch fp32 on the bf16 values, outputs rounded once: at most one bar out of one everywhere, on the GPU test's seed
    and two more (the half-ulp term of the bar is reached by construction: the worst figure lies just under 1)."""
    for seed in (eb.SEED, eb.SEED + 1, eb.SEED + 2):
        x, p, gy, other, scale = eb.case(hw, form, seed)
        assert torch.equal(x, eb.bf(x)) and torch.equal(gy, eb.bf(gy))             # the inputs ARE bf16 values
        worst = eb.check(eb.sound_model(x, p, gy, form, other, scale), hw, form, seed, tag="sound model")
        assert worst > 0.5, "a bf16 output that is nowhere half a bar from float64 was not rounded to bf16"


def test_bf16_ties_round_to_even():
    """The two products the GPU test plants: -(1 + 2^-8) lies halfway between -1 and -(1 + 2^-7) and goes to the even -1
    (truncation too, round-half-away does not); -(1 + 3 2^-8) lies halfway between -(1 + 2^-7) and -(1 + 2^-6) and goes to
    the even -(1 + 2^-6) = -1.015625 (truncation does not)."""
    x = torch.tensor([-1.0])
    for w, want in ((1 + 2.0 ** -8, -1.0), (1 + 3 * 2.0 ** -8, -1.015625)):
        y = torch.nn.functional.prelu(x, torch.tensor([w]))
        assert float(y) == -w and float(y.bfloat16()) == want


def test_amp_dtype_validates():
    from ilps_amd.training import amp_dtype
    assert amp_dtype(None) is None
    assert amp_dtype("bf16") is torch.bfloat16 and amp_dtype(torch.bfloat16) is torch.bfloat16
    for bad in ("fp32", "bfloat16", "BF16", "", 16, True, torch.float32, torch.float64):
        with pytest.raises(ValueError, match="amp must be"):
            amp_dtype(bad)
    for half in ("fp16", torch.float16):
        with pytest.raises(ValueError, match="no loss scaling"):
            amp_dtype(half)
    from ilps_amd.training import SegTrainer
    with pytest.raises(ValueError, match="no loss scaling"):
        SegTrainer(None, amp="fp16", device="cpu")                    # refused before anything is built


def test_fusable_admits_bf16_planes_only_dense_and_with_fp32_parameters(monkeypatch):
    """`ops._bn_fusable` on meta-free stand-ins (no device: is_cuda is patched): fp32 and bf16 dense NCHW planes of >= 256
    elements are admitted, fp16 / float64, channels_last, small planes and modules with non-fp32 parameters are not."""
    from ilps_amd import ops

    class OnDevice(torch.Tensor):
        is_cuda = True

    def t(dtype, shape=(2, 4, 16, 16), channels_last=False):
        x = torch.zeros(shape, dtype=dtype)
        if channels_last:
            x = x.contiguous(memory_format=torch.channels_last)
        return x.as_subclass(OnDevice)
    bn = torch.nn.BatchNorm2d(4).train()
    assert ops._bn_fusable(t(torch.float32), bn) and ops._bn_fusable(t(torch.bfloat16), bn)
    assert not ops._bn_fusable(t(torch.float16), bn) and not ops._bn_fusable(t(torch.float64), bn)
    assert not ops._bn_fusable(t(torch.bfloat16, channels_last=True), bn)
    assert not ops._bn_fusable(t(torch.bfloat16, (2, 4, 15, 15)), bn)
    assert not ops._bn_fusable(torch.zeros(2, 4, 16, 16, dtype=torch.bfloat16), bn)          # a CPU tensor
    assert not ops._bn_fusable(t(torch.bfloat16), torch.nn.BatchNorm2d(4).train().bfloat16())
    assert not ops._bn_fusable(t(torch.bfloat16), torch.nn.BatchNorm2d(4).eval())
    act, act16 = torch.nn.PReLU(4), torch.nn.PReLU(4).bfloat16()
    assert ops._slope_fusable(act, t(torch.bfloat16)) and not ops._slope_fusable(act16, t(torch.bfloat16))
    assert not ops._slope_fusable(torch.nn.PReLU(1), t(torch.bfloat16))
    # the opt-in channels_last encoder layout runs torch's own batch norm: refused together with amp
    from ilps_amd.training import SegTrainer
    monkeypatch.setenv("SMPLR_ENCODER_LAYOUT", "channels_last")
    with pytest.raises(ValueError, match="channels_last"):
        SegTrainer(None, amp="bf16", device="cpu")


@pytest.mark.parametrize("use_IEF", [True, False])
def test_regressor_under_cpu_autocast_keeps_fp32_at_its_boundary(use_IEF):
    """`training.regress(net, images, "bf16")` on the CPU (stock modules): an fp32 finite (2, 86) vector, fp32 parameter
    gradients, and bf16 in and out of every bottleneck - the residual stream stays bf16 from the initial block on."""
    from ilps_amd.model import SMPLRegressor
    from ilps_amd.training import regress
    torch.manual_seed(0)
    net = SMPLRegressor(48, "enet", use_IEF).train()
    images = torch.rand(2, 3, 256, 256)
    seen = []
    hooks = [b.register_forward_hook(lambda m, i, o: seen.append((i[0].dtype, o.dtype))) for b in net.backbone.enet.blocks]
    param = regress(net, images, "bf16")
    for h in hooks:
        h.remove()
    assert param.shape == (2, 86) and param.dtype == torch.float32 and bool(torch.isfinite(param).all())
    assert len(seen) == len(net.backbone.enet.blocks) and set(seen) == {(torch.bfloat16, torch.bfloat16)}
    param.square().sum().backward()
    grads = [q.grad for q in net.parameters()]
    assert all(g is not None and g.dtype == torch.float32 and bool(torch.isfinite(g).all()) for g in grads)
    assert all(q.dtype == torch.float32 for q in net.parameters())
    with torch.no_grad():
        assert regress(net, images, None).dtype == torch.float32          # amp = None: net(images) itself


def test_bf16_entry_points_are_declared_exported_and_bound():
    from ilps_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "smplraster.h")).read(), flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in BF16_ENTRIES:
        twin = name[:-len("_bf16")]
        assert hasattr(lib, name), "%s is not exported" % name
        m, t = (re.search(r"\b%s\s*\(([^)]*)\)" % n, src) for n in (name, twin))
        assert m and t, name
        n_params = m.group(1).count(",") + 1
        assert n_params == t.group(1).count(",") + 1 == len(_lib.SIGNATURES[name][1]) == len(_lib.SIGNATURES[twin][1])
        assert _lib.SIGNATURES[name] == _lib.SIGNATURES[twin]
    assert _lib.load().smplr_abi_version() == _lib.ABI_VERSION == 7


def test_bf16_entry_points_refuse_bad_arguments_without_a_launch():
    """The refusals of the fp32 calls: sizes past the grid limit and null pointers give a nonzero code and a message that
    names the call (every pointer is NULL: nothing can have been launched), an empty batch is a no-op."""
    from ilps_amd import _lib
    lib = _lib.load()
    calls = {"smplr_prelu_fwd_bf16": lambda N, C, HW: lib.smplr_prelu_fwd_bf16(None, None, N, C, HW, None, None),
             "smplr_bn_fwd_bf16": lambda N, C, HW: lib.smplr_bn_fwd_bf16(None, None, None, None, N, C, HW, 1e-3, 0.1, None,
                                                                         None, None, None, None, None, None),
             "smplr_bn_res_fwd_bf16": lambda N, C, HW: lib.smplr_bn_res_fwd_bf16(None, None, None, None, None, None, N, C,
                                                                                 HW, 1e-3, 0.1, None, None, None, None,
                                                                                 None, None, None),
             "smplr_prelu_bwd_bf16": lambda N, C, HW: lib.smplr_prelu_bwd_bf16(None, None, None, N, C, HW, None, None, None,
                                                                               None),
             "smplr_bn_bwd_bf16": lambda N, C, HW: lib.smplr_bn_bwd_bf16(None, None, None, None, None, None, None, N, C, HW,
                                                                         None, None, None, None, None, None),
             "smplr_bn_res_bwd_bf16": lambda N, C, HW: lib.smplr_bn_res_bwd_bf16(None, None, None, None, None, None, None,
                                                                                 None, None, N, C, HW, None, None, None,
                                                                                 None, None, None, None)}
    assert sorted(calls) == sorted(BF16_ENTRIES)
    for name, call in calls.items():
        assert call(1 << 31, 1, 4096) != 0, name
        msg = lib.smplr_last_error().decode()
        assert name in msg and "N=%d" % (1 << 31) in msg and "HW=4096" in msg, msg
        assert call(2, 3, 256) != 0, name
        assert name in lib.smplr_last_error().decode() and "null" in lib.smplr_last_error().decode()
        if name.endswith("fwd_bf16"):
            assert call(0, 3, 256) == 0, name


def test_bf16_kernels_fit_the_hardware_as_their_fp32_twins_do():
    """The bf16 entry points of a kernel body are named bnh_* / preluh_* beside the fp32 bn_* / prelu_*: each has no
    scratch, no AGPRs, and at least the waves per SIMD of its twin (8: the streams hide HBM latency by occupancy)."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr
    ks = {n: k for n, k in kr.kernels().items() if "smplr" in n}
    stem = lambda n: re.sub(r"^_ZN5smplr\d+", "", n)
    half = {n: k for n, k in ks.items() if re.match(r"_ZN5smplr\d+(bnh_|preluh_)", n)}
    assert len(half) == 12, sorted(half)          # stats, 3 apply, 3 bwd_stats, 3 bwd_apply; prelu fwd and bwd
    for n, k in half.items():
        want = stem(n).replace("bnh_", "bn_", 1).replace("preluh_", "prelu_", 1)
        want = want[:want.index("kernel") + len("kernel")] + (re.search(r"ILNS_6BnFormE\dE", want) or [""])[0]
        twins = [t for t in ks if t not in half and stem(t).startswith(want)]
        assert len(twins) == 1, (n, want, twins)
        assert k["scratch"] == 0 and k["agpr"] == 0, (n, k)
        assert kr.waves_per_simd(k) >= kr.waves_per_simd(ks[twins[0]]), (n, k, ks[twins[0]])
