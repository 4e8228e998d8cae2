"""Timing of the 6D rotation pose head (ilps_amd.rot6d over csrc/rot6d.hip), one GPU:
    timeout -k 10 300 python tools/rot6d_time.py [--batches 128 2048]
Inputs: the mean pose in 6D (`mean_rot6d_row`) plus Gaussian noise, as a regressor's early output.  Legs, per call and batch:
    rot6d_hip     `params_from_rot6d` forward + backward (one launch each: rot6d_fwd_kernel, rot6d_bwd_kernel) for a random
                  cotangent
    rot6d_torch   `params_from_rot6d_torch` in fp32 on the device, forward + backward by autograd: the stock composition (a cat,
                  a Gram-Schmidt, a matrix logarithm)
Each figure is device-event time around back-to-back calls, after untimed calls of the same shape; the calls per window come
from one timed call (at least --window seconds per window, 1 to 5000 calls).  The two legs alternate --rounds times in the same
run, every round is printed and the median reported.  `kernels` counts the device kernels of one forward + backward of each
leg, from torch.profiler (copies and memsets are listed apart).  No bar is asserted: the tool reports."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import ilps_amd  # noqa: E402,F401


def event_ms(fn, iters):
    """Device-event milliseconds per call over `iters` back-to-back calls."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def count_kernels(fn):
    """Device kernels (and copies / memsets) one call of fn launches, by torch.profiler."""
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    kernels = other = 0
    names = {}
    for ev in prof.events():
        if ev.device_type != torch.autograd.DeviceType.CUDA:
            continue
        if ev.name.lower().startswith(("memcpy", "memset")):
            other += 1
        else:
            kernels += 1
            names[ev.name] = names.get(ev.name, 0) + 1
    return kernels, other, names


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[128, 2048])
    ap.add_argument("--output", type=int, default=48)
    ap.add_argument("--sigma", type=float, default=0.1, help="noise on the mean's six-vectors")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("rot6d_time.py needs a HIP device: a CPU run gives no timing")
    from ilps_amd import _lib
    from ilps_amd.rot6d import mean_rot6d_row, params_from_rot6d, params_from_rot6d_torch
    dev = torch.device("cuda", torch.cuda.current_device())
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    res = {"build_id": _lib.build_id()[:16], "batches": {}}
    for B in a.batches:
        y = mean_rot6d_row(a.output, dev).repeat(B, 1)
        y[:, 4:148] += a.sigma * torch.randn((B, 144), generator=gen, device=dev)
        y.requires_grad_(True)
        g = torch.randn((B, 86), generator=gen, device=dev)

        def leg(fn):
            def run():
                y.grad = None
                fn(y).backward(g)
            return run
        legs = {"rot6d_hip": leg(params_from_rot6d), "rot6d_torch": leg(params_from_rot6d_torch)}
        out = {}
        grads = {}
        for k, fn in legs.items():
            fn()
            grads[k] = y.grad.clone()
        with torch.no_grad():
            out["x_max_abs_diff_hip_torch"] = float((params_from_rot6d(y) - params_from_rot6d_torch(y)).abs().max())
        out["dy_max_rel_diff_hip_torch"] = float((grads["rot6d_hip"] - grads["rot6d_torch"]).abs().max() / grads["rot6d_hip"].abs().max())
        out["kernels"], out["copies_memsets"], iters = {}, {}, {}
        for k, fn in legs.items():
            kernels, other, names = count_kernels(fn)
            out["kernels"][k], out["copies_memsets"][k] = kernels, other
            if k == "rot6d_hip":
                out["hip_kernel_names"] = names
            fn()                                                           # untimed
            one = event_ms(fn, 1)
            iters[k] = int(min(5000, max(1, np.ceil(a.window * 1e3 / max(one, 1e-3)))))
        ms = {k: [] for k in legs}
        for _ in range(a.rounds):                                          # the two legs, alternated
            for k in legs:
                ms[k].append(event_ms(legs[k], iters[k]))
        out["iters"] = iters
        out["ms_per_call_rounds"] = {k: [round(v, 5) for v in vs] for k, vs in ms.items()}
        out["ms_per_call"] = {k: round(statistics.median(vs), 5) for k, vs in ms.items()}
        out["torch_over_hip"] = round(out["ms_per_call"]["rot6d_torch"] / out["ms_per_call"]["rot6d_hip"], 2)
        out["hip_faster_than_torch"] = bool(max(ms["rot6d_hip"]) < min(ms["rot6d_torch"]))
        res["batches"][str(B)] = out
    print(json.dumps(res))


if __name__ == "__main__":
    main()
