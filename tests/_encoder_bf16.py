"""Inputs, references and error bars for the bf16 forms of the encoder's batch-norm / PReLU kernels (csrc/norm.hip,
csrc/act.hip: the smplr_*_bf16 entry points), on top of tests/_encoder_inputs.py.

The kernels take bf16 tensors, widen every element to fp32 (exact), run the fp32 expressions and round a streamed result
(z, dx, dother) to bf16 once.  So the truth is torch's float64 modules on the bf16 INPUT VALUES upcast exactly, and the
bar of a bf16 output is the fp32 bar of `_encoder_inputs.compare` plus one bf16 rounding of the result, 2^-8 |ref| (half
an ulp of an 8-bit significand).  The fp32 outputs (dgamma, dbeta, dslope, the saved and the running statistics) keep
the fp32 bars as they are, and so does the kink exemption with its cap FLIP_CAP.  `sound_model` - torch's CPU fp32
modules on the same values with z, dx, dother rounded to bf16 - must pass these bars (tests/test_encoder_bf16_cpu.py);
the half-ulp term is reached by construction, so its worst error / bar lies just under 1."""
import functools

import torch

import _encoder_inputs as ei

U16 = 2.0 ** -8                      # half an ulp of bf16, relative
FORMS = ("bn", "bn_act", "bn_res")
# (H, W): the smallest planes at which the bf16 walk can go wrong
PLANES = [(16, 16),                  # 256: the smallest fusable plane, one partial trip of the 8-wide path
          (13, 20),                  # 260: a multiple of 4 but not of 8 - scalar path; plane bases only 8-B aligned
          (17, 17),                  # 289: odd - 2-B aligned planes, scalar path
          (54, 76),                  # 4104: the second chunk is exactly one 8-vector
          (64, 65)]                  # 4160: the regime shape of the fp32 tests, a second chunk of 64
SEED = 41
EPS, MOMENTUM = 1e-3, 0.1


def bf(t):
    """t rounded to bf16 (to nearest even), as fp32."""
    return t.bfloat16().float()


@functools.lru_cache(maxsize=None)
def case(hw, form, seed=SEED):
    """(x, p, gy, other, scale) for a (3, 5, H, W) tensor: fp32 tensors that hold bf16 values - x = bf16(randn 2 + 0.5),
    gy = bf16(randn (1 + n)), other = bf16(randn) - fp32 parameters, and dropout factors of which some are 0 and some
    1 / 0.7.  other and scale are None unless form is "bn_res".  Cached: treat as read-only."""
    N, C = 3, 5
    shape = (N, C) + tuple(hw)
    g = torch.Generator().manual_seed(seed)
    x = bf(torch.randn(shape, generator=g) * 2 + 0.5)
    gy = bf(torch.randn(shape, generator=g) * (1 + torch.arange(N).float())[:, None, None, None])
    p = ei.make_params(C, seed)
    other = scale = None
    if form == "bn_res":
        other = bf(torch.randn(shape, generator=g))
        scale = (torch.rand(N, C, generator=g) > 0.3).float() / 0.7
        assert bool((scale == 0).any()) and bool((scale > 0).any())
    return x, p, gy, other, scale


@functools.lru_cache(maxsize=None)
def truth(hw, form, seed=SEED):
    """float64 reference of case(hw, form, seed).  Cached: treat as read-only."""
    x, p, gy, other, scale = case(hw, form, seed)
    return ei.reference(x, p, gy, EPS, MOMENTUM, with_act=form != "bn", other=other, plane_scale=scale)


def sound_model(x, p, gy, form, other, scale):
    """A sound implementation of the bf16 contract: torch's CPU fp32 modules on the bf16 values, z / dx / dother rounded
    to bf16 once, everything else left in fp32."""
    r = ei.reference(x, p, gy, EPS, MOMENTUM, with_act=form != "bn", other=other, plane_scale=scale, dtype=torch.float32)
    got = {k: v.float() for k, v in r.items() if torch.is_tensor(v) and k != "pre"}
    for k in ("z", "dx", "dother"):
        if k in got:
            got[k] = got[k].bfloat16()
    return got


def compare(got, ref, x, p, plane_scale=None):
    """_encoder_inputs.compare with 2^-8 |ref| added to the bars of the tensors stored in bf16 (z, dx, dother); every
    other bar, and the kink exemption (float64 `pre` within the fp32 z bar of 0), exactly as there.  got: z, dx, dother
    in bf16 (or anything .double() takes), the rest fp32.  -> (report, elements left out of dx / dother, elements)."""
    mean, rstd, floor = ei.batch_stats(x, EPS)
    fl = (p["gamma"].double().abs() * floor)[None, :, None, None]
    if plane_scale is not None:
        fl = fl * plane_scale.double().abs()[:, :, None, None]
    zbar = 2e-5 * (1 + ref["z"].abs()) + fl + U16 * ref["z"].abs()
    rep = {"z": ei._per_channel(ei._ratio(got["z"], ref["z"], zbar))}
    keep = torch.ones_like(ref["pre"], dtype=torch.bool)
    if "dslope" in ref:
        keep = ref["pre"].abs() > 2e-5 * (1 + ref["pre"].abs()) + fl
    for k in ("dx", "dother"):
        if k in ref:
            r = ref[k]
            bar = (2e-4 + U16) * r.abs() + 2e-4 * r.pow(2).mean((0, 2, 3), keepdim=True).sqrt()
            rep[k] = ei._per_channel(ei._ratio(got[k], r, bar), keep)
    rep["dgamma"] = ei._ratio(got["dgamma"], ref["dgamma"], 2e-4 * (1 + ref["dgamma"].abs()) + floor * ref["dbeta"].abs())
    for k in ("dbeta", "dslope"):
        if k in ref:
            rep[k] = ei._ratio(got[k], ref[k], 2e-4 * (1 + ref[k].abs()))
    stats = dict(ref, mean=mean, rstd=rstd)
    for k in ("running_mean", "running_var", "mean", "rstd"):
        if k in got:
            rep[k] = ei._ratio(got[k], stats[k], 1e-5 + 1e-5 * stats[k].abs())
    return rep, int((~keep).sum()), keep.numel()


def check(got, hw, form, seed=SEED, tag=""):
    """Assert `got` inside the bars for case(hw, form, seed); prints the worst error / bar per channel first.
    -> the worst figure."""
    x, p, gy, other, scale = case(hw, form, seed)
    for k in ("z", "dx", "dother"):
        if k in got:
            assert got[k].dtype == torch.bfloat16, "%s is %s" % (k, got[k].dtype)
    for k in ("dgamma", "dbeta", "dslope", "running_mean", "running_var", "mean", "rstd"):
        if k in got:
            assert got[k].dtype == torch.float32, "%s is %s" % (k, got[k].dtype)
    ei.assert_finite(got)
    rep, left_out, total = compare(got, truth(hw, form, seed), x, p, scale)
    ei.assert_report(rep, left_out, total, tag="%s bf16 %s HW=%d seed %d" % (tag, form, hw[0] * hw[1], seed))
    return max(float(v.max()) for v in rep.values())
