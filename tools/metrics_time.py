"""Timing of the segmentation metrics (csrc/metrics.hip and the rasteriser's metrics epilogue), one GPU:
    python tools/metrics_time.py [--iters N]
(a) the confusion kernel on (B, 48, 48, 32) fp32 scores + int32 labels at B = 128 and 2 048: us per call and the bytes
    it must read per us; (b) the fused-loss decoder forward (gradient-free, outputs=()) with and without
    `confusion` at B = 128 and 2 048.  Event pairs around N back-to-back calls (dispatch gaps included); for the kernel
    durations alone run it under `rocprofv3 --kernel-trace --stats -- python tools/metrics_time.py`."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ilps_amd  # noqa: E402,F401


def timed(fn, iters, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1000.0 / iters          # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    a = ap.parse_args()
    from _inputs import make_x
    from ilps_amd.decoder import SMPLDecoder
    from ilps_amd.focal_loss import softmax_focal_loss
    from ilps_amd.metrics import seg_confusion
    from ilps_amd.smpl_model import synthetic_smpl_model
    dev = torch.device("cuda:0")
    W, C = 48, 32
    res = {}
    for B in (128, 2048):
        g = torch.Generator(device=dev).manual_seed(B)
        scores = torch.rand(B, W, W, C, device=dev, generator=g)
        labels = torch.randint(0, C, (B, W, W), device=dev, generator=g, dtype=torch.int32)
        conf = torch.zeros(C + 1, C, dtype=torch.int64, device=dev)
        us = timed(lambda: seg_confusion(scores, labels, conf), a.iters)
        mb = (scores.numel() * 4 + labels.numel() * 4) / 1e6
        res["confusion_B%d" % B] = {"us": round(us, 2), "MB": round(mb, 1), "GB_per_s": round(mb * 1e3 / us, 1)}
        del scores
    model = synthetic_smpl_model(1234)
    dec = None
    for B in (128, 2048):
        x = torch.as_tensor(make_x(B, W, seed=3), device=dev)
        lab = torch.randint(0, 32, (B, W, W), device=dev)
        if dec is None:
            dec = SMPLDecoder(model, img_wh=W, outputs=(), loss=softmax_focal_loss(2.0, True))
        conf = torch.zeros(33, 32, dtype=torch.int64, device=dev)
        with torch.no_grad():
            t0 = timed(lambda: dec(x, lab), a.iters)
            t1 = timed(lambda: dec(x, lab, confusion=conf), a.iters)
            t2 = timed(lambda: dec(x, lab), a.iters)
        res["decoder_fwd_B%d" % B] = {"us_without": round((t0 + t2) / 2, 2), "us_with_confusion": round(t1, 2),
                                      "us_without_runs": [round(t0, 2), round(t2, 2)]}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
