"""The encoder's batch-norm and PReLU kernels (csrc/norm.hip: smplr_bn_fwd/bwd, smplr_bn_res_fwd/bwd; csrc/act.hip:
smplr_prelu_fwd/bwd) against torch's own modules in float64 on the CPU, where such kernels go wrong: channels whose
offset is large against their spread, reductions long enough for a second trip of the finalize loops, planes that cross
a 4096-element chunk on the scalar path, the PReLU kink, gradients that are not dense NCHW, sizes past the grid limit.
Inputs and bars: tests/_encoder_inputs.py (torch's CPU fp32 passes the same bars: tests/test_encoder_regimes_cpu.py)."""
import pytest
import torch

import _encoder_inputs as ei

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = ei.REGIME_SEED


def _run(form, x, p, gy, eps=1e-3, momentum=0.1, other=None, plane_scale=None):
    """One forward + backward of ops.batch_norm_act ("bn", "bn_act") or ops.batch_norm_residual_act ("bn_res") on the
    stock modules, on the GPU.  Returns what _encoder_inputs.compare takes, as CPU tensors."""
    from ilps_amd import ops
    from ilps_amd.model import PReLU
    C = x.shape[1]
    bn = torch.nn.BatchNorm2d(C, eps=eps, momentum=momentum)
    act = PReLU(C) if form != "bn" else None
    with torch.no_grad():
        bn.weight.copy_(p["gamma"])
        bn.bias.copy_(p["beta"])
        bn.running_mean.copy_(p["running_mean"])
        bn.running_var.copy_(p["running_var"])
        if act is not None:
            act.weight.copy_(p["slope"])
    bn, act = bn.to(DEV).train(), (act.to(DEV) if act is not None else None)
    xd = x.to(DEV).requires_grad_(True)
    od = None
    if form == "bn_res":
        od = other.to(DEV).requires_grad_(True)
        drop = torch.nn.Dropout2d(0.3).train() if plane_scale is not None else None
        z = ops.batch_norm_residual_act(xd, bn, drop, od, act,
                                        plane_scale=plane_scale.to(DEV) if plane_scale is not None else None)
        assert "BatchNormResActFn" in type(z.grad_fn).__name__                      # the HIP op ran
        mean, rstd = z.grad_fn.saved_tensors[6:8]           # ops.BatchNormResActFn saves (x, other, gamma, beta, slope, plane_scale, mean, rstd)
    else:
        z = ops.batch_norm_act(xd, bn, act)
        assert "BatchNormActFn" in type(z.grad_fn).__name__
        mean, rstd = z.grad_fn.saved_tensors[4:6]           # ops.BatchNormActFn saves (x, gamma, beta, slope, mean, rstd)
    assert mean.shape == rstd.shape == (C,) and bool((rstd > 0).all()), "saved_tensors are not in the order read here"
    mean, rstd = mean.clone(), rstd.clone()
    z.backward(gy if gy.is_cuda else gy.to(DEV))
    got = {"z": z, "dx": xd.grad, "dgamma": bn.weight.grad, "dbeta": bn.bias.grad, "running_mean": bn.running_mean,
           "running_var": bn.running_var, "mean": mean, "rstd": rstd}
    if od is not None:
        got["dother"] = od.grad
    if act is not None:
        got["dslope"] = act.weight.grad
    got = {k: v.detach().cpu() for k, v in got.items()}
    got["num_batches_tracked"] = int(bn.num_batches_tracked)
    return got


def _check(form, x, p, gy, eps=1e-3, momentum=0.1, other=None, plane_scale=None, exempt=(), tag=""):
    got = _run(form, x, p, gy, eps, momentum, other, plane_scale)
    ref = ei.reference(x, p, gy, eps, momentum, with_act=form != "bn", other=other, plane_scale=plane_scale)
    ei.assert_finite(got)
    rep, left_out, total = ei.compare(got, ref, x, p, eps, plane_scale=plane_scale)
    ei.assert_report(rep, left_out, total, exempt=exempt, tag="%s %s eps=%g momentum=%g" % (tag, form, eps, momentum))
    assert got["num_batches_tracked"] == ref["num_batches_tracked"] == 1
    return got


def _same_bits(a, b):
    for k, v in a.items():
        if torch.is_tensor(v):
            assert torch.equal(v.view(torch.int32), b[k].view(torch.int32)), "%s differs between two runs" % k


def _prelu(x, w, gy):
    """ops.PReLUFn forward + backward on the GPU; y, gx, gw as CPU tensors."""
    from ilps_amd import ops
    xd, wd = x.to(DEV).requires_grad_(True), w.to(DEV).requires_grad_(True)
    y = ops.PReLUFn.apply(xd, wd)
    assert "PReLUFn" in type(y.grad_fn).__name__
    y.backward(gy if gy.is_cuda else gy.to(DEV))
    return y.detach().cpu(), xd.grad.cpu(), wd.grad.cpu()


def _prelu64(x, w, gy):
    x64, w64 = x.double().requires_grad_(True), w.double().requires_grad_(True)
    y64 = torch.nn.functional.prelu(x64, w64)
    y64.backward(gy.double())
    return y64.detach(), x64.grad, w64.grad


def _check_prelu(x, w, gy, tag=""):
    y, gx, gw = _prelu(x, w, gy)
    y64, gx64, gw64 = _prelu64(x, w, gy)
    # y and gx are one fp32 product each: half an ulp; gw is a sum: the dslope bar
    assert torch.allclose(y.double(), y64, rtol=1e-6, atol=1e-7), tag
    assert torch.allclose(gx.double(), gx64, rtol=1e-6, atol=1e-7), tag
    ratio = (gw.double() - gw64).abs() / (2e-4 * (1 + gw64.abs()))
    print("%s PReLUFn dslope error / bar: %s" % (tag, " ".join("%.3g" % v for v in ratio.tolist())))
    assert bool((ratio <= 1).all()) and bool(torch.isfinite(gw).all()), tag


# ---- 1. shifted statistics -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("momentum", [0.1, 0.01])
@pytest.mark.parametrize("eps", [1e-3, 1e-5])
@pytest.mark.parametrize("form", ["bn", "bn_act", "bn_res"])
def test_shifted_channels_match_float64(form, eps, momentum):
    """regime_tensor(4, 64, 65): HW = 4160 is two chunks, the second of 64 elements; offsets up to 1000 standard
    deviations.  Every output, gradient and statistic inside the bars of _encoder_inputs; two runs bit-equal."""
    x, p, gy, other, scale = ei.regime_case(form, SEED)
    got = _check(form, x, p, gy, eps, momentum, other, scale, exempt=(ei.CONSTANT_CHANNEL,), tag="regimes")
    _same_bits(got, _run(form, x, p, gy, eps, momentum, other, scale))


@pytest.mark.parametrize("form", ["bn", "bn_act", "bn_res"])
def test_scaled_control_channel(form):
    """The control channel as it is, times 1e4 and times 1e-4 (var = 4e-8, far below eps): no scale is special.  The
    residual form with the draw's dropout factors (zeros and 1 / 0.7) on these channels."""
    x8, p8, gy8, other8, scale8 = ei.regime_case(form, SEED)
    x = torch.stack([x8[:, 0], x8[:, 0] * 1e4, x8[:, 0] * 1e-4], 1).contiguous()
    p = {k: v[:3].clone() for k, v in p8.items()}
    gy = gy8[:, :3].contiguous()
    other = other8[:, :3].contiguous() if other8 is not None else None
    scale = scale8[:, :3].contiguous() if scale8 is not None else None
    for eps in (1e-3, 1e-5):
        _check(form, x, p, gy, eps, 0.1, other, scale, tag="scaled control")


# ---- 2. reductions whose finalize loops take a second trip -----------------------------------------------------------

def _plain_case(shape, seed, with_other=False):
    """randn * 2 + 0.5 planes, and a gradient whose mean differs per image (gy * (1 + n)): a partial sum dropped or
    added twice shows in dgamma, dbeta and dslope."""
    g = torch.Generator().manual_seed(seed)
    N, C = shape[0], shape[1]
    x = torch.randn(*shape, generator=g) * 2.0 + 0.5
    gy = torch.randn(*shape, generator=g) * (1.0 + torch.arange(N, dtype=torch.float32))[:, None, None, None]
    other = torch.randn(*shape, generator=g) if with_other else None
    scale = (torch.rand(N, C, generator=g) > 0.3).float() / 0.7 if with_other else None
    return x, ei.make_params(C, seed), gy, other, scale


@pytest.mark.parametrize("form,shape", [("bn_act", (300, 2, 16, 16)), ("bn", (300, 2, 16, 16)),
                                        ("bn_res", (300, 2, 16, 16)), ("bn", (70, 3, 128, 128))])
def test_batch_norm_reduces_more_partials_than_threads(form, shape):
    """300 and 280 chunk partials per channel: bn_finalize_kernel and bn_bwd_finalize_kernel stride 256 threads.
    (The 3.4 M-element shape runs without the PReLU: the element nearest the kink is typically 3e-7 from it there, within
    reach of fp32 rounding, and one element on the other branch is hundreds of dbeta bars.)"""
    x, p, gy, other, scale = _plain_case(shape, sum(shape), with_other=form == "bn_res")
    assert shape[0] * ((shape[2] * shape[3] + 4095) // 4096) > 256
    _check(form, x, p, gy, 1e-3, 0.1, other, scale, tag="partials %s" % (shape,))


@pytest.mark.parametrize("shape", [(70, 3, 20, 15), (20, 2, 128, 128)])
def test_prelu_reduces_more_partials_than_lanes(shape):
    """70 and 80 partials per channel: prelu_bwd_reduce_kernel strides 64 lanes."""
    x, p, gy, _, _ = _plain_case(shape, sum(shape))
    assert shape[0] * ((shape[2] * shape[3] + 4095) // 4096) > 64
    _check_prelu(x - 0.5, p["slope"], gy, tag="partials %s" % (shape,))


# ---- 3. chunk edges ------------------------------------------------------------------------------------------------

CHUNK_EDGES = [(1, 4096),      # exactly one chunk
               (1, 4097),      # scalar path, a second chunk of ONE element
               (1, 4100),      # vector path, a second chunk of one float4
               (65, 65),       # 4225: scalar path, a second chunk of 129 elements (fewer than the 256 threads)
               (1, 8191)]      # scalar path, the last chunk short by one


@pytest.mark.parametrize("hw", CHUNK_EDGES)
@pytest.mark.parametrize("form", ["bn", "bn_act", "bn_res", "prelu"])
def test_chunk_edges(form, hw):
    shape = (2, 3) + hw
    x, p, gy, other, scale = _plain_case(shape, hw[0] * hw[1], with_other=form == "bn_res")
    if form == "prelu":
        _check_prelu(x - 0.5, p["slope"], gy, tag="edge %s" % (hw,))
    else:
        _check(form, x, p, gy, 1e-3, 0.1, other, scale, tag="edge %s" % (hw,))


# ---- 4. the PReLU kink ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("hw", [(5, 7), (8, 8)])                       # scalar and float4 paths
def test_prelu_branch_convention(hw):
    """x = +0.0, -0.0 and denormals of both signs take the branches torch's PReLU takes (x > 0 ? x : a x: zero is on the
    slope side), with slopes 0, 1, negative and above 1.  Slopes are powers of two and the planted denormals even
    multiples of the smallest one, so every product is exact: y and gx must EQUAL the float64 result, signs of zero
    included; gw is a sum and gets the dslope bar."""
    g = torch.Generator().manual_seed(hw[0])
    w = torch.tensor([0.0, 1.0, -0.5, 2.0])
    x = torch.randn(2, 4, *hw, generator=g)
    gy = torch.randn(2, 4, *hw, generator=g)
    tiny = 2.0 ** -149
    planted = torch.tensor([0.0, -0.0, 2 * tiny, -2 * tiny, 6 * tiny, -6 * tiny, 2.0 ** -127, -(2.0 ** -127)])
    assert bool((planted[2:] != 0).all()) and bool((planted[2:].abs() < 2.0 ** -126).all())     # fp32 holds them
    flat = x.view(2, 4, -1)
    flat[:, :, 1:1 + len(planted)] = planted                              # (from 1 on: not aligned to a float4)
    flat[:, :, -len(planted):] = planted.flip(0)
    y, gx, gw = _prelu(x, w, gy)
    y64, gx64, gw64 = _prelu64(x, w, gy)
    assert torch.equal(y.double(), y64) and torch.equal(torch.signbit(y), torch.signbit(y64))
    assert torch.equal(gx.double(), gx64) and torch.equal(torch.signbit(gx), torch.signbit(gx64))
    assert bool(((gw.double() - gw64).abs() <= 2e-4 * (1 + gw64.abs())).all())
    # what the convention means at the planted places: +0.0 with slope 0 passes no gradient, with slope 2 twice it
    zero = (x == 0)
    assert bool(zero[:, 0].any()) and torch.equal(gx[:, 0][zero[:, 0]], torch.zeros_like(gx[:, 0][zero[:, 0]]))
    assert torch.equal(gx[:, 3][zero[:, 3]], 2 * gy[:, 3][zero[:, 3]])


# ---- 5. gradients that are not dense NCHW --------------------------------------------------------------------------

def _grad_layouts(shape):
    """The gradient of z.sum() (ones expanded with stride 0) and a channels_last gradient, each with its dense twin."""
    g = torch.Generator().manual_seed(5)
    ones = torch.ones((), device=DEV).expand(shape)
    assert ones.stride() == (0, 0, 0, 0)
    dense = torch.randn(*shape, generator=g).to(DEV)
    cl = dense.contiguous(memory_format=torch.channels_last)
    assert not cl.is_contiguous() and torch.equal(cl, dense)
    return [("expanded", ones, torch.ones(shape, device=DEV)), ("channels_last", cl, dense)]


@pytest.mark.parametrize("form", ["bn", "bn_act", "bn_res", "prelu"])
def test_gradient_layouts(form):
    shape = (3, 4, 17, 19)
    x, p, _, other, scale = _plain_case(shape, 11, with_other=form == "bn_res")
    for name, odd, dense in _grad_layouts(shape):
        if form == "prelu":
            a, b = _prelu(x - 0.5, p["slope"], odd), _prelu(x - 0.5, p["slope"], dense)
            for u, v in zip(a, b):
                assert torch.equal(u.view(torch.int32), v.view(torch.int32)), name
        else:
            _same_bits(_run(form, x, p, odd, other=other, plane_scale=scale),
                       _run(form, x, p, dense, other=other, plane_scale=scale))
    if form == "prelu":                                                  # z.sum().backward() itself
        from ilps_amd import ops
        xd, wd = (x - 0.5).to(DEV).requires_grad_(True), p["slope"].to(DEV).requires_grad_(True)
        ops.PReLUFn.apply(xd, wd).sum().backward()
        ref = _prelu(x - 0.5, p["slope"], torch.ones(shape))
        assert torch.equal(xd.grad.cpu(), ref[1]) and torch.equal(wd.grad.cpu(), ref[2])


# ---- 6. sizes past the grid limit ----------------------------------------------------------------------------------

@pytest.mark.parametrize("N,C,HW", [(1 << 20, 1 << 11, 1), (1 << 31, 1, 4096), (3, 1 << 29, 4097)])
def test_size_guard_refuses_before_touching_a_pointer(N, C, HW):
    """N C chunks >= 2^31 workgroups cannot be launched: a nonzero code and a message with the sizes, nothing launched
    (every pointer is NULL)."""
    from ilps_amd import _lib
    lib = _lib.load()
    assert N * C * ((HW + 4095) // 4096) >= 1 << 31
    calls = {"smplr_bn_fwd": lambda: lib.smplr_bn_fwd(None, None, None, None, N, C, HW, 1e-3, 0.1, None, None, None, None,
                                                      None, None, None),
             "smplr_bn_bwd": lambda: lib.smplr_bn_bwd(None, None, None, None, None, None, None, N, C, HW, None, None, None,
                                                      None, None, None),
             "smplr_prelu_fwd": lambda: lib.smplr_prelu_fwd(None, None, N, C, HW, None, None),
             "smplr_prelu_bwd": lambda: lib.smplr_prelu_bwd(None, None, None, N, C, HW, None, None, None, None)}
    for name, call in calls.items():
        assert call() != 0, name
        msg = lib.smplr_last_error().decode()
        assert name in msg and "N=%d" % N in msg and "C=%d" % C in msg and "HW=%d" % HW in msg, msg
