"""Inputs, references and error bars for the encoder's batch-norm / PReLU kernels (csrc/norm.hip, csrc/act.hip).

`regime_tensor` builds planes whose offset is large against their spread - what a biased convolution or a sparse
input produces - next to the well-centred kind.  `reference` runs torch's own modules on the CPU (float64: the truth;
float32: a sound fp32 implementation, which must pass the same bars - tests/test_encoder_regimes_cpu.py).  `compare`
turns a result and the float64 truth into worst-error-over-bar figures per channel, and `assert_report` asserts them.

The bars are derived, not tuned.  floor_c = 2^-23 |mean_c| rstd_c is one fp32 ulp of the saved mean in x_hat units:
a kernel that keeps `mean` in fp32 cannot beat half of it, so it is granted wherever x_hat enters linearly
(z through gamma, dgamma through sum(dy) = dbeta); every other term is the suite's usual 2e-5 / 2e-4 / 1e-5."""
import torch

# (mean, std) of channel c of regime_tensor
REGIMES = [(0.5, 2.0), (10.0, 0.1), (100.0, 0.1), (-100.0, 0.1), (127.5, 1.0), (5.0, 0.01), (100.0, 0.0), (3000.0, 30.0)]
CONSTANT_CHANNEL = 6          # std 0: x_hat is rounding noise times 1 / sqrt(eps) - no relative bar for dgamma, dslope, dx
FLIP_CAP = 1e-3               # share of a tensor that may sit within the z bar of the PReLU kink
ULP = 2.0 ** -23
# The draw both test files use.  One element on the other PReLU branch than float64 moves dbeta by |dz| (1 - slope),
# hundreds of its bars, and with floor_c up to 1e-4 in x_hat units a draw of 133 120 elements per channel often holds one
# for a sound fp32 implementation (torch's CPU fp32 has one in most draws).  On this draw torch fp32 has none, and the
# float64 pre-activation stays 4e-6 away from 0 everywhere.  The GPU test leans on the same: a later reordering of a
# kernel's arithmetic, harmless in itself, could put an element of this draw on the other branch; then the draw is what
# to change (test_encoder_regimes_cpu.py must still pass on the new one), not a bar.
REGIME_SEED = 31


def regime_tensor(N, H, W, seed=0):
    """fp32 (N, 8, H, W) with channel c drawn as mean_c + std_c * randn, and the list of (mean, std)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, len(REGIMES), H, W, generator=g, dtype=torch.float64)
    for c, (m, s) in enumerate(REGIMES):
        x[:, c] = x[:, c] * s + m
    return x.float(), list(REGIMES)


def make_params(C, seed=0, slope=None):
    """gamma, beta, slope and the running statistics before the step (fp32, seeded)."""
    g = torch.Generator().manual_seed(1000 + seed)
    p = {"gamma": torch.rand(C, generator=g) + 0.5, "beta": torch.randn(C, generator=g) * 0.3,
         "slope": torch.rand(C, generator=g) * 0.6 - 0.2,                     # some slopes negative
         "running_mean": torch.randn(C, generator=g), "running_var": torch.rand(C, generator=g) + 0.5}
    if slope is not None:
        p["slope"] = torch.as_tensor(slope, dtype=torch.float32)
    return p


def regime_case(form, seed, N=4, H=64, W=65):
    """The shifted-statistics case of both test files: x = regime_tensor, parameters, a gradient and, for form "bn_res",
    the other branch and dropout factors of which some are 0.  form: "bn", "bn_act" or "bn_res"."""
    x, _ = regime_tensor(N, H, W, seed)
    C = x.shape[1]
    p = make_params(C, seed)
    g = torch.Generator().manual_seed(seed + 7)
    gy = torch.randn(x.shape, generator=g)
    other = scale = None
    if form == "bn_res":
        other = torch.randn(x.shape, generator=g)
        scale = (torch.rand(N, C, generator=g) > 0.3).float() / 0.7
        assert bool((scale == 0).any()) and bool((scale > 0).any())
    return x, p, gy, other, scale


def reference(x, p, gy, eps, momentum, with_act=True, other=None, plane_scale=None, dtype=torch.float64):
    """torch.nn.BatchNorm2d in training mode (+ PReLU; with `other`: prelu(plane_scale * bn(x) + other)) on the CPU in
    `dtype`, forward and backward.  Everything comes back as float64: z, pre (the PReLU's argument), dx, dother, dgamma,
    dbeta, dslope, running_mean, running_var, num_batches_tracked."""
    C = x.shape[1]
    bn = torch.nn.BatchNorm2d(C, eps=eps, momentum=momentum).to(dtype).train()
    with torch.no_grad():
        bn.weight.copy_(p["gamma"])
        bn.bias.copy_(p["beta"])
        bn.running_mean.copy_(p["running_mean"])
        bn.running_var.copy_(p["running_var"])
    act = with_act or other is not None
    slope = p["slope"].detach().to(dtype).clone().requires_grad_(True) if act else None
    xr = x.detach().to(dtype).clone().requires_grad_(True)      # (clone: .to() of the same dtype is the caller's tensor)
    orr = None
    pre = bn(xr)
    if other is not None:
        orr = other.detach().to(dtype).clone().requires_grad_(True)
        if plane_scale is not None:
            pre = pre * plane_scale.to(dtype)[:, :, None, None]
        pre = pre + orr
    z = torch.nn.functional.prelu(pre, slope) if act else pre
    z.backward(gy.to(dtype))
    out = {"z": z, "pre": pre, "dx": xr.grad, "dgamma": bn.weight.grad, "dbeta": bn.bias.grad,
           "running_mean": bn.running_mean, "running_var": bn.running_var}
    if orr is not None:
        out["dother"] = orr.grad
    if act:
        out["dslope"] = slope.grad
    out = {k: v.detach().double() for k, v in out.items()}
    out["num_batches_tracked"] = int(bn.num_batches_tracked)
    return out


def batch_stats(x, eps):
    """float64 mean, rstd and floor_c = 2^-23 |mean_c| rstd_c of the batch, per channel."""
    x64 = x.double()
    mean = x64.mean((0, 2, 3))
    rstd = (x64.var((0, 2, 3), unbiased=False) + eps).rsqrt()
    return mean, rstd, ULP * mean.abs() * rstd


def _per_channel(ratio, keep=None):
    if keep is not None:
        ratio = torch.where(keep, ratio, torch.zeros_like(ratio))
    return ratio.amax((0, 2, 3)) if ratio.dim() == 4 else ratio


def _ratio(got, ref, bar):
    err = (got.double() - ref).abs()
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))
    return torch.where(err == 0, torch.zeros_like(err), err / bar)         # (a zero bar admits a zero error only)


def compare(got, ref, x, p, eps, plane_scale=None):
    """Worst |got - ref| over its bar, per channel, for every quantity that `got` holds; ref = reference(float64).
    Returns (report {name: (C,) float64}, elements left out of dx / dother, elements in all).  got may also hold
    `mean` and `rstd` (the saved statistics).  Elements whose float64 `pre` lies within the z bar of 0 may take
    the other PReLU branch: they are left out of dx / dother, nothing else."""
    mean, rstd, floor = batch_stats(x, eps)
    fl = (p["gamma"].double().abs() * floor)[None, :, None, None]
    if plane_scale is not None:
        fl = fl * plane_scale.double().abs()[:, :, None, None]
    rep = {"z": _per_channel(_ratio(got["z"], ref["z"], 2e-5 * (1 + ref["z"].abs()) + fl))}
    keep = torch.ones_like(ref["pre"], dtype=torch.bool)
    if "dslope" in ref:
        keep = ref["pre"].abs() > 2e-5 * (1 + ref["pre"].abs()) + fl
    for k in ("dx", "dother"):
        if k in ref:
            r = ref[k]
            bar = 2e-4 * r.abs() + 2e-4 * r.pow(2).mean((0, 2, 3), keepdim=True).sqrt()
            rep[k] = _per_channel(_ratio(got[k], r, bar), keep)
    rep["dgamma"] = _ratio(got["dgamma"], ref["dgamma"], 2e-4 * (1 + ref["dgamma"].abs()) + floor * ref["dbeta"].abs())
    for k in ("dbeta", "dslope"):
        if k in ref:
            rep[k] = _ratio(got[k], ref[k], 2e-4 * (1 + ref[k].abs()))
    stats = dict(ref, mean=mean, rstd=rstd)
    for k in ("running_mean", "running_var", "mean", "rstd"):
        if k in got:
            rep[k] = _ratio(got[k], stats[k], 1e-5 + 1e-5 * stats[k].abs())
    return rep, int((~keep).sum()), keep.numel()


def format_report(rep):
    return "\n".join("%-13s %s" % (k, " ".join("%9.3g" % float(v) for v in r)) for k, r in rep.items())


def assert_report(rep, left_out, total, exempt=(), tag=""):
    """Every figure of compare() at most 1, the left-out share within FLIP_CAP.  `exempt`: constant channels, which are
    held to z, dbeta and the statistics only (regime_tensor: CONSTANT_CHANNEL)."""
    print("%s  worst error / bar per channel (%d of %d elements near the kink)\n%s" % (tag, left_out, total, format_report(rep)))
    assert left_out <= FLIP_CAP * total, "%s: %d of %d elements within the z bar of the PReLU kink" % (tag, left_out, total)
    for k, r in rep.items():
        for c, v in enumerate(r.tolist()):
            if c in exempt and k in ("dx", "dother", "dgamma", "dslope"):
                continue
            assert v <= 1.0, "%s: %s of channel %d is %.3g bars out" % (tag, k, c, v)


def assert_finite(got):
    for k, v in got.items():
        if torch.is_tensor(v):
            assert bool(torch.isfinite(v).all()), "%s is not finite" % k
