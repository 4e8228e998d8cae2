"""Timing of the probabilistic head (ilps_amd.prob over csrc/prob.hip) against its torch restatements, one GPU:
    timeout -k 10 300 python tools/prob_time.py [--legs samples nll spread] [--rounds 20]
Each pair of legs is a step of its own (--legs picks them, so that each can run under its own time limit):
    samples   `gaussian_samples` forward + backward for a random cotangent (prob_sample_fwd_kernel, prob_sample_bwd_kernel)
              against `gaussian_samples_torch` in fp32 by autograd, at B = 128, S = 32, D = 86, camera columns masked
    nll       `gaussian_nll` forward + backward (prob_nll_fwd_kernel, prob_nll_bwd_kernel) against `gaussian_nll_torch`, at
              B = 128, D = 86, the groups (camera out, pose, shape)
    spread    `sample_spread` (prob_spread_kernel: one pass) against `sample_spread_torch` (a mean, a difference, a reduction:
              three passes) at B = 16, S = 64, N = 6890; `read_bytes` = B S N 12 is what one pass reads, `hip_TBps` and
              `torch_TBps` are that over each leg's time - the rate of the call as a user sees it, host work included, not a
              kernel's share of peak
Tools: tools/_timing.py.  After untimed calls of the same shape, the calls that fill --window seconds are timed back to back
with the host clock around a device synchronise; the two legs of a pair alternate --rounds times (at least 20) in the same run
and the medians are reported with every round.  The tool exits non-zero when a HIP leg's median is slower than its torch
leg's."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _timing  # noqa: E402
import ilps_amd  # noqa: E402,F401


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", nargs="+", default=["samples", "nll", "spread"], choices=["samples", "nll", "spread"])
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--samples", type=int, default=32)
    ap.add_argument("--width", type=int, default=86)
    ap.add_argument("--spread", type=int, nargs=3, default=[16, 64, 6890], metavar=("B", "S", "N"))
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--window", type=float, default=0.05)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("prob_time.py needs a HIP device: a CPU run gives no timing")
    if a.rounds < 20:
        sys.exit("--rounds: at least 20 timed rounds per leg")
    from ilps_amd import _lib, prob
    dev = torch.device("cuda", torch.cuda.current_device())
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    rn = lambda *s: torch.randn(s, generator=gen, device=dev)
    B, S, D = a.batch, a.samples, a.width
    res = {"build_id": _lib.build_id()[:16], "B": B, "S": S, "D": D, "rounds": a.rounds}
    slower = []

    def pair(name, legs, per=None):
        iters = _timing.calls_per_window(legs, a.window, warm=3, cap=2000)
        out = _timing.rounds(legs, iters, a.rounds)
        out["iters"] = iters
        us = out["us_per_call"]
        out["torch_over_hip"] = round(us[name + "_torch"] / us[name + "_hip"], 2)
        if us[name + "_hip"] > us[name + "_torch"]:
            slower.append(name)
        res[name] = out
        return out

    mu, s = rn(B, D).requires_grad_(True), (0.5 * rn(B, D) - 4.0).requires_grad_(True)
    if "samples" in a.legs:
        eps, g = rn(B, S, D), rn(B, S, D)
        mask = [0] * 4 + [1] * (D - 4)

        def leg(fn):
            def run():
                mu.grad = s.grad = None
                fn(mu, s, eps, mask, True).backward(g)
            return run
        with torch.no_grad():
            d = (prob.gaussian_samples(mu, s, eps, mask, True) - prob.gaussian_samples_torch(mu, s, eps, mask, True)).abs().max()
        pair("samples", {"samples_hip": leg(prob.gaussian_samples), "samples_torch": leg(prob.gaussian_samples_torch)})
        res["samples"]["x_max_abs_diff_hip_torch"] = float(d)
    if "nll" in a.legs:
        target, g = rn(B, D), rn(B, 2)
        groups = [-1] * 4 + [0] * (D - 14) + [1] * 10

        def leg(fn):
            def run():
                mu.grad = s.grad = None
                fn(mu, s, target, groups).backward(g)
            return run
        with torch.no_grad():
            h, r = prob.gaussian_nll(mu, s, target, groups), prob.gaussian_nll_torch(mu, s, target, groups)
        pair("nll", {"nll_hip": leg(prob.gaussian_nll), "nll_torch": leg(prob.gaussian_nll_torch)})
        res["nll"]["nll_max_rel_diff_hip_torch"] = float(((h - r).abs() / r.abs()).max())
    if "spread" in a.legs:
        b, ns, n = a.spread
        points = 0.3 * rn(b, 1, n, 3) + 0.01 * rn(b, ns, n, 3)
        points = points.reshape(b * ns, n, 3).contiguous()
        h, r = prob.sample_spread(points, ns), prob.sample_spread_torch(points, ns)
        out = pair("spread", {"spread_hip": lambda: prob.sample_spread(points, ns),
                              "spread_torch": lambda: prob.sample_spread_torch(points, ns)})
        read = b * ns * n * 12
        out.update(shape=[b, ns, n], read_bytes=read, rms_max_abs_diff_hip_torch=float((h[1] - r[1]).abs().max()),
                   hip_TBps=round(read / (out["us_per_call"]["spread_hip"] * 1e-6) / 1e12, 3),
                   torch_TBps=round(read / (out["us_per_call"]["spread_torch"] * 1e-6) / 1e12, 3))
    print(json.dumps(res))
    if slower:
        sys.exit("slower than the torch composition: %s" % ", ".join(slower))


if __name__ == "__main__":
    main()
