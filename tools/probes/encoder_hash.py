"""Hashes of every output of the encoder's batch-norm / PReLU kernels (csrc/norm.hip, csrc/act.hip) for fixed seeded
inputs: run under two builds of the library (SMPLR_LIB_PATH) to show a kernel change is bit-exact.  One sha256 line per
(form, shape, output) on stdout; `HASH_PROBE=tools/probes/encoder_hash.py bash tools/hash_ab.sh ENV_A ENV_B` or diff the
stdout of two runs.  The inputs are the shifted channels of tests/_encoder_inputs.py: a sum taken in another order shows
there first.  The shapes are the smallest that reach each way the plane walk can go.  GPU only."""
import hashlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _encoder_inputs as ei  # noqa: E402
from ilps_amd import ops  # noqa: E402

SHAPES = [(3, 5, 7, 9),        # HW = 63: tail path, one chunk
          (2, 3, 8, 8),        # float4 path
          (2, 2, 63, 67),      # HW = 4221: tail path across a chunk boundary
          (2, 2, 64, 72),      # HW = 4608: float4 path across a chunk boundary
          (300, 2, 16, 16),    # more chunk partials per channel than the finalize kernels have threads
          (70, 3, 20, 15)]     # more partials than prelu_bwd_reduce_kernel has lanes
FORMS = ["bn", "bn_act", "bn_res", "bn_res_scaled", "prelu"]
CHANNELS = [7, 1, 0, 3, 5]     # of ei.REGIMES, for a tensor of C <= 5 channels: the widest offsets first
EPS, MOMENTUM = 1e-3, 0.1


def case(shape, seed):
    """x, parameters, gradient, other branch and dropout factors (some 0) of one shape, on the CPU."""
    N, C, H, W = shape
    x = ei.regime_tensor(N, H, W, seed)[0][:, CHANNELS[:C]].contiguous()
    p = ei.make_params(C, seed)
    g = torch.Generator().manual_seed(seed + 7)
    gy = torch.randn(x.shape, generator=g)
    other = torch.randn(x.shape, generator=g)
    scale = (torch.rand(N, C, generator=g) > 0.3).float() / 0.7
    scale[0, 0], scale[-1, -1] = 0.0, 1.0 / 0.7                  # both kinds whatever the draw
    return x, p, gy, other, scale


def run(form, x, p, gy, other, scale, dev):
    """{output name: tensor} of one forward + backward of the form's autograd Function."""
    d = lambda t: t.to(dev)  # noqa: E731
    xd = d(x).requires_grad_(True)
    if form == "prelu":                                          # (centred: both branches in every channel)
        centre = torch.tensor([ei.REGIMES[c][0] for c in CHANNELS[:x.shape[1]]])
        xd = d(x - centre[None, :, None, None]).requires_grad_(True)
        w = d(p["slope"]).requires_grad_(True)
        y = ops.PReLUFn.apply(xd, w)
        y.backward(d(gy))
        return {"y": y, "gx": xd.grad, "gw": w.grad}
    gamma, beta = d(p["gamma"]).requires_grad_(True), d(p["beta"]).requires_grad_(True)
    slope = d(p["slope"]).requires_grad_(True) if form != "bn" else None
    rm, rv = d(p["running_mean"]), d(p["running_var"])
    out = {}
    if form.startswith("bn_res"):
        od = d(other).requires_grad_(True)
        z = ops.BatchNormResActFn.apply(xd, od, gamma, beta, slope, d(scale) if form == "bn_res_scaled" else None, rm, rv,
                                        EPS, MOMENTUM)
        mean, rstd = z.grad_fn.saved_tensors[6:8]
    else:
        z = ops.BatchNormActFn.apply(xd, gamma, beta, slope, rm, rv, EPS, MOMENTUM)
        mean, rstd = z.grad_fn.saved_tensors[4:6]
    out.update(mean=mean.clone(), rstd=rstd.clone())
    z.backward(d(gy))
    out.update(z=z, dx=xd.grad, dgamma=gamma.grad, dbeta=beta.grad, running_mean=rm, running_var=rv)
    if form.startswith("bn_res"):
        out["dother"] = od.grad
    if slope is not None:
        out["dslope"] = slope.grad
    return out


def main():
    dev = torch.device("cuda", 0)
    for si, shape in enumerate(SHAPES):
        x, p, gy, other, scale = case(shape, ei.REGIME_SEED + si)
        for form in FORMS:
            outs = run(form, x, p, gy, other, scale, dev)
            torch.cuda.synchronize()
            for name in sorted(outs):
                t = outs[name].detach().cpu().contiguous()
                assert bool(torch.isfinite(t).all()), (form, shape, name)
                print("%-13s %-18s %-12s %s" % (form, "x".join(map(str, shape)), name,
                                                hashlib.sha256(t.numpy().tobytes()).hexdigest()))


if __name__ == "__main__":
    main()
