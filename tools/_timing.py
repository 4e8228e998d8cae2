"""What the side terms' timing scripts (scan_time.py, penetration_time.py, meshreg_time.py, measure_time.py, labeldist_time.py,
keypoint_time.py) share: the host clock around back-to-back calls, the calls per window, the alternating rounds and the
torch.profiler count of kernels per call."""
import statistics
import time

import torch


def wall(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / iters


def calls_per_window(legs, window, warm=1, cap=200):
    """Per leg: `warm` untimed calls (code objects, allocator pools), then one timed call -> the calls that fill about
    `window` seconds, 2 to `cap`."""
    iters = {}
    for k, fn in legs.items():
        for _ in range(warm):
            fn()
        iters[k] = int(min(cap, max(2, window * 1e6 / max(wall(fn, 1), 1.0))))
    return iters


def rounds(legs, iters, n, per=1, key="us_per_call"):
    """The legs alternate n times, iters (one number, or one per leg) calls each -> every round and the median, in us per
    call / `per`, under key + "_rounds" and key."""
    us = {k: [] for k in legs}
    for _ in range(n):
        for k, fn in legs.items():
            us[k].append(wall(fn, iters[k] if isinstance(iters, dict) else iters) / per)
    return {key + "_rounds": {k: [round(v, 1) for v in vs] for k, vs in us.items()},
            key: {k: round(statistics.median(vs), 1) for k, vs in us.items()}}


def profile_calls(fn, iters, kernels, label):
    """-> kernels per call and their summed device time per call (us), those named in `kernels` by name under `label`, from
    a torch.profiler trace."""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
    ev = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "memcpy" not in e.name.lower()
          and "memset" not in e.name.lower()]
    ours = {}
    for e in ev:
        for key in kernels:
            if key in e.name:
                ours.setdefault(key, []).append(e.device_time)
    return {"kernels_per_call": round(len(ev) / iters, 2), "device_us_per_call": round(sum(e.device_time for e in ev) / iters, 1),
            label: {k: round(statistics.median(v), 1) for k, v in ours.items()}}
