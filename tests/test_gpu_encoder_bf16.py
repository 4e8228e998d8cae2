"""The bf16 forms of the encoder's batch-norm / PReLU kernels (smplr_*_bf16 of csrc/norm.hip, csrc/act.hip) and the `amp`
option built on them, on the GPU.  Inputs, float64 references and bars: tests/_encoder_bf16.py (a sound bf16 model passes
the same bars: tests/test_encoder_bf16_cpu.py).  The plane sizes are the smallest at which the 8-wide walk can go wrong."""
import pytest
import torch

import _encoder_bf16 as eb

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16


def _modules(p, with_act):
    from ilps_amd.model import PReLU
    C = p["gamma"].numel()
    bn = torch.nn.BatchNorm2d(C, eps=eb.EPS, momentum=eb.MOMENTUM)
    act = PReLU(C) if with_act else None
    with torch.no_grad():
        bn.weight.copy_(p["gamma"])
        bn.bias.copy_(p["beta"])
        bn.running_mean.copy_(p["running_mean"])
        bn.running_var.copy_(p["running_var"])
        if act is not None:
            act.weight.copy_(p["slope"])
    return bn.to(DEV).train(), (act.to(DEV) if act is not None else None)


def _run(form, x, p, gy, other=None, plane_scale=None, x_dtype=BF, other_dtype=BF, backward=None):
    """One forward + backward of ops.batch_norm_act / ops.batch_norm_residual_act on stock modules with x (and other) in
    bf16, on the GPU.  backward: a function of z that runs the backward (default: z.backward(gy in bf16)).  Returns what
    _encoder_bf16.compare takes, as CPU tensors in the dtypes the ops gave them."""
    from ilps_amd import ops
    bn, act = _modules(p, form != "bn")
    xd = x.to(DEV, x_dtype).requires_grad_(True)
    od = None
    if form == "bn_res":
        od = other.to(DEV, other_dtype).requires_grad_(True)
        drop = torch.nn.Dropout2d(0.3).train() if plane_scale is not None else None
        z = ops.batch_norm_residual_act(xd, bn, drop, od, act,
                                        plane_scale=plane_scale.to(DEV) if plane_scale is not None else None)
        assert type(z.grad_fn).__name__ == "BatchNormResActFnBackward"                 # the package's Function ran
        saved = z.grad_fn.saved_tensors
        mean, rstd = saved[6:8]
    else:
        z = ops.batch_norm_act(xd, bn, act)
        assert type(z.grad_fn).__name__ == "BatchNormActFnBackward"
        saved = z.grad_fn.saved_tensors
        mean, rstd = saved[4:6]
    assert z.dtype == x_dtype and saved[0].dtype == x_dtype
    mean, rstd = mean.clone(), rstd.clone()
    if backward is None:
        z.backward(gy.to(DEV, x_dtype))
    else:
        backward(z)
    got = {"z": z, "dx": xd.grad, "dgamma": bn.weight.grad, "dbeta": bn.bias.grad, "running_mean": bn.running_mean,
           "running_var": bn.running_var, "mean": mean, "rstd": rstd}
    if od is not None:
        got["dother"] = od.grad
    if act is not None:
        got["dslope"] = act.weight.grad
    return {k: v.detach().cpu() for k, v in got.items()}


def _bits(t):
    return t.view(torch.int16) if t.dtype == BF else t.view(torch.int32)


def _same_bits(a, b, tag=""):
    assert sorted(a) == sorted(b)
    for k, v in a.items():
        assert v.dtype == b[k].dtype and torch.equal(_bits(v), _bits(b[k])), "%s: %s differs" % (tag, k)


# ---- 1. the bars ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", eb.FORMS)
@pytest.mark.parametrize("hw", eb.PLANES)
def test_bf16_forms_match_float64(hw, form):
    """Every output inside the bars of _encoder_bf16 (the fp32 bars, plus one bf16 rounding on z, dx, dother); the
    streamed results bf16, everything per channel fp32; two runs bit-equal."""
    x, p, gy, other, scale = eb.case(hw, form)
    got = _run(form, x, p, gy, other, scale)
    worst = eb.check(got, hw, form, tag="HIP")
    print("worst error / bar: %.3f" % worst)
    _same_bits(got, _run(form, x, p, gy, other, scale), "second run")


# ---- 2. PReLU: one rounding, to nearest even ------------------------------------------------------------------------

def _prelu(x, w, gy):
    """ops.PReLUFn on bf16 x, gy and an fp32 w, on the GPU -> y, gx (bf16), gw (fp32) on the CPU."""
    from ilps_amd import ops
    xd, wd = x.to(DEV).requires_grad_(True), w.to(DEV).requires_grad_(True)
    y = ops.PReLUFn.apply(xd, wd)
    assert type(y.grad_fn).__name__ == "PReLUFnBackward" and y.dtype == BF
    y.backward(gy.to(DEV))
    assert xd.grad.dtype == BF and wd.grad.dtype == torch.float32
    return y.detach().cpu(), xd.grad.cpu(), wd.grad.cpu()


def _prelu_cpu(x, w, gy):
    """torch's CPU PReLU in fp32 on the bf16 values, y and gx rounded to bf16 once; gw in float64."""
    x32 = x.float().requires_grad_(True)
    y32 = torch.nn.functional.prelu(x32, w)
    y32.backward(gy.float())
    x64, w64 = x.double(), w.double().requires_grad_(True)
    torch.nn.functional.prelu(x64, w64).backward(gy.double())
    return y32.detach().bfloat16(), x32.grad.bfloat16(), w64.grad


def _assert_bf16_equal(got, want, tag):
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan), "%s: NaN positions differ" % tag
    g, w = got.view(torch.int16), want.view(torch.int16)
    assert torch.equal(g[~nan], w[~nan]), "%s: %d elements differ" % (tag, int((g[~nan] != w[~nan]).sum()))


SPECIALS = [-1.0, -0.0, float("inf"), float("-inf"), float("nan"), 0.0]       # (no subnormal results: outside the contract)


@pytest.mark.parametrize("shape", [(2, 3, 16, 16), (2, 3, 17, 17), (1, 2, 54, 76)])
def test_prelu_bf16_is_the_fp32_product_rounded_once(shape):
    """y and gx EQUAL bf16(torch CPU fp32 PReLU on the bf16 values), bit for bit (NaN by position): -0.0, +-Inf and NaN
    pass through, and the two ties x = -1, w = 1 + 2^-8 -> -1.0 and w = 1 + 3 2^-8 -> -1.015625 tell round-to-nearest-even
    from truncation and from round-half-away (channels 0 and 1 carry these slopes; both in y and, with gy = -1 there, in gx).
    gw, a sum, is held to the 2e-4 (1 + |gw|) bar of the fp32 tests on the same tensors without their non-finite plants."""
    g = torch.Generator().manual_seed(shape[2])
    N, C = shape[0], shape[1]
    w = torch.tensor([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -0.375][:C])
    x = (torch.randn(shape, generator=g) * 2).bfloat16()
    gy = torch.randn(shape, generator=g).bfloat16()
    plants = torch.tensor(SPECIALS).bfloat16()
    xf, gf = x.view(N, C, -1), gy.view(N, C, -1)
    xf[:, :, 3:3 + len(plants)] = plants                                   # (from 3 on: not aligned to a vector)
    xf[:, :, -len(plants):] = plants.flip(0)
    gf[:, :, 3] = -1.0                                                     # the ties in gx: w * gy where x = -1 <= 0
    gf[:, :, 5:8] = torch.tensor([float("nan"), float("inf"), -0.0]).bfloat16()
    y, gx, gw = _prelu(x, w, gy)
    y_ref, gx_ref, _ = _prelu_cpu(x, w, gy)
    _assert_bf16_equal(y, y_ref, "y")
    _assert_bf16_equal(gx, gx_ref, "gx")
    for t in (y, gx):
        assert float(t[0, 0].flatten()[3]) == -1.0 and float(t[0, 1].flatten()[3]) == -1.015625      # the ties
    assert bool(torch.signbit(y[0, 0].flatten()[4])) and float(y[0, 0].flatten()[4]) == 0.0         # -0.0 * w = -0.0
    assert float(y[0, 0].flatten()[5]) == float("inf") and float(y[0, 0].flatten()[6]) == float("-inf")
    # the slope gradient, on finite tensors
    fin = lambda t: torch.where(torch.isfinite(t.float()), t.float(), torch.ones(())).bfloat16()
    xq, gq = fin(x), fin(gy)
    y, gx, gw = _prelu(xq, w, gq)
    y_ref, gx_ref, gw64 = _prelu_cpu(xq, w, gq)
    _assert_bf16_equal(y, y_ref, "y (finite)")
    _assert_bf16_equal(gx, gx_ref, "gx (finite)")
    ratio = (gw.double() - gw64).abs() / (2e-4 * (1 + gw64.abs()))
    print("PReLUFn bf16 dslope error / bar: %s" % " ".join("%.3g" % v for v in ratio.tolist()))
    assert bool(torch.isfinite(gw).all()) and bool((ratio <= 1).all())


# ---- 3. mixed operands ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("hw", [(16, 16), (17, 17)])
def test_residual_of_another_dtype_is_converted_first(hw):
    """x bf16 with an fp32 `other` that is NOT a bf16 value: out is bf16 and bit-equal to the run with other rounded
    beforehand; dother comes back fp32 and equals the bf16 dother upcast."""
    x, p, gy, _, scale = eb.case(hw, "bn_res")
    other = torch.randn(x.shape, generator=torch.Generator().manual_seed(3))
    assert not torch.equal(other, eb.bf(other))
    mixed = _run("bn_res", x, p, gy, other, scale, other_dtype=torch.float32)
    ref = _run("bn_res", x, p, gy, eb.bf(other), scale)
    assert mixed["z"].dtype == BF and mixed["dother"].dtype == torch.float32 and ref["dother"].dtype == BF
    assert torch.equal(mixed["dother"], ref["dother"].float())
    mixed["dother"] = mixed["dother"].bfloat16()
    _same_bits(mixed, ref, "fp32 other")


# ---- 4. a gradient that is neither dense nor bf16 ---------------------------------------------------------------------

@pytest.mark.parametrize("form", eb.FORMS)
def test_gradient_of_a_float_sum(form):
    """z.float().sum().backward(): the gradient arrives as expanded ones through a cast; the bits of a dense bf16 ones."""
    hw = (17, 17)
    x, p, gy, other, scale = eb.case(hw, form)
    odd = _run(form, x, p, gy, other, scale, backward=lambda z: z.float().sum().backward())
    dense = _run(form, x, p, torch.ones_like(gy), other, scale)
    _same_bits(odd, dense, "float sum")


# ---- 5. what the kernels do not take -----------------------------------------------------------------------------------

def test_small_bf16_planes_take_the_stock_modules():
    """Under autocast, bf16 planes below 256 elements run the stock modules, without error.  (A channels_last bf16 tensor
    takes the same branch of `ops._bn_fusable` - its is_contiguous() test, which tests/test_encoder_bf16_cpu.py checks
    without a device - but is not run here: with torch 2.10 / ROCm 7.0 torch's own training-mode batch norm ends the
    process on such a tensor, and SegTrainer refuses amp together with that layout.)"""
    from ilps_amd import ops
    shape = (2, 5, 15, 15)
    g = torch.Generator().manual_seed(9)
    p = eb.ei.make_params(5, 9)
    for form in eb.FORMS:
        bn, act = _modules(p, form != "bn")
        x = torch.randn(shape, generator=g).to(DEV, BF)
        other = torch.randn(shape, generator=g).to(DEV, BF)
        x.requires_grad_(True)
        with torch.autocast("cuda", dtype=BF):
            if form == "bn_res":
                z = ops.batch_norm_residual_act(x, bn, torch.nn.Dropout2d(0.3).train(), other, act)
            else:
                z = ops.batch_norm_act(x, bn, act)
        names = set()
        stack = [z.grad_fn]
        while stack:
            fn = stack.pop()
            if fn is not None and fn not in names:
                names.add(fn)
                stack += [n for n, _ in fn.next_functions]
        names = {type(fn).__name__ for fn in names}
        assert not any("BatchNormActFn" in n or "BatchNormResActFn" in n for n in names), names
        assert any("BatchNorm" in n for n in names), names                 # torch's own batch norm
        z.float().sum().backward()
        assert z.shape == shape and bool(torch.isfinite(z.float()).all()) and bool(torch.isfinite(x.grad.float()).all())
        assert bn.weight.grad.dtype == torch.float32 and int(bn.num_batches_tracked) == 1


# ---- 6. the trainer ------------------------------------------------------------------------------------------------

def _encoder_nodes(param):
    """The package's encoder Function nodes in the autograd graph under `param`: {class name: [node, ...]}."""
    found, seen, stack = {}, set(), [param.grad_fn]
    while stack:
        fn = stack.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        name = type(fn).__name__.replace("Backward", "")
        if name in ("BatchNormActFn", "BatchNormResActFn", "PReLUFn"):
            found.setdefault(name, []).append(fn)
        stack += [n for n, _ in fn.next_functions]
    return found


def test_trainer_steps_in_bf16(smpl_model):
    """Two steps of SegTrainer(amp="bf16") at B = 2: finite loss, parameters changed, parameters and gradients fp32; the
    regressor's graph holds as many of the package's batch-norm / PReLU nodes as the fp32 trainer's, each with a bf16 x."""
    from ilps_amd.training import SegTrainer, regress
    torch.manual_seed(0)
    g = torch.Generator().manual_seed(1)
    images = torch.rand(2, 3, 256, 256, generator=g).to(DEV)
    labels = torch.randint(0, 32, (2, 48, 48), generator=g).to(DEV)
    tr = SegTrainer(smpl_model, output_wh=48, encoder_architecture="enet", use_IEF=True, device=DEV, amp="bf16")
    before = [q.detach().clone() for q in tr.smpl_model.parameters()]
    for _ in range(2):
        loss = tr.step(images, labels)
        assert loss.dtype == torch.float32 and bool(torch.isfinite(loss))
    params = list(tr.smpl_model.parameters())
    assert all(q.dtype == torch.float32 and q.grad is not None and q.grad.dtype == torch.float32 for q in params)
    assert all(bool(torch.isfinite(q).all()) for q in params)
    assert sum(int(not torch.equal(a, b)) for a, b in zip(before, params)) > len(params) // 2
    assert all(v.dtype == torch.float32 for v in tr.state_dict().values() if v.is_floating_point())
    param = regress(tr.net, images, tr.amp)
    assert param.dtype == torch.float32 and param.shape == (2, 86)
    nodes = _encoder_nodes(param)
    plain = SegTrainer(smpl_model, output_wh=48, encoder_architecture="enet", use_IEF=True, device=DEV)
    assert plain.amp is None
    param32 = regress(plain.net, images, None)                            # (kept: the nodes' saved tensors live with it)
    nodes32 = _encoder_nodes(param32)
    count = lambda d: {k: len(v) for k, v in d.items()}
    print("encoder nodes: bf16 %s, fp32 %s" % (count(nodes), count(nodes32)))
    assert count(nodes) == count(nodes32) and sum(count(nodes).values()) >= 60
    for name, fns in nodes.items():
        assert all(fn.saved_tensors[0].dtype == BF for fn in fns), name
    for name, fns in nodes32.items():
        assert all(fn.saved_tensors[0].dtype == torch.float32 for fn in fns), name
    out = tr.monitor(images)
    assert out["smpl"].dtype == torch.float32 and out["seg"].dtype == torch.float32 and out["seg"].shape == (2, 48, 48, 32)


# ---- 7. inference --------------------------------------------------------------------------------------------------

def test_predict_batch_in_bf16(smpl_model):
    """predict_batch(..., amp="bf16"): fp32 finite outputs of the usual shapes.  The share of seg_maps pixels that agree with
    the fp32 prediction is printed, not asserted: no bar for a network's amplification of a rounding can be derived."""
    from ilps_amd.decoder import SMPLDecoder
    from ilps_amd.inference import predict_batch
    from ilps_amd.model import SMPLRegressor
    torch.manual_seed(0)
    reg = SMPLRegressor(48, "enet", True).to(DEV)
    dec = SMPLDecoder(smpl_model, img_wh=48)
    img = torch.rand(2, 3, 256, 256, device=DEV)
    ref = predict_batch(reg, dec, img)
    got = predict_batch(reg, dec, img, amp="bf16")
    assert sorted(got) == sorted(ref)
    for k, v in got.items():
        assert v.shape == ref[k].shape and v.dtype == ref[k].dtype, k
        assert bool(torch.isfinite(v).all()) if v.is_floating_point() else True, k
    assert got["smpl"].dtype == torch.float32 and got["segs"].dtype == torch.float32
    print("seg_maps pixels equal to the fp32 prediction's: %.4f; max |smpl - smpl32| = %.3g"
          % (float((got["seg_maps"] == ref["seg_maps"]).float().mean()), float((got["smpl"] - ref["smpl"]).abs().max())))
    assert reg.training                                                   # the mode is restored
    with pytest.raises(ValueError, match="no loss scaling"):
        predict_batch(reg, dec, img, amp="fp16")
