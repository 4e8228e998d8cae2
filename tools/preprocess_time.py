"""Timing of the input preprocessing (csrc/preprocess.hip through preprocess.load_images / load_labels), one GPU:
    python tools/preprocess_time.py [--iters N]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/preprocess_time.py --kernels-only      # kernel times, own run
    python tools/preprocess_time.py --trace-csv DIR/.../*_kernel_trace.csv    # median us per (resize kernel, grid) of that run
Three workloads:
  images   128 ragged 3-channel images, sides drawn from 200..1000 (seed 0) -> 256 x 256 x 3 fp32, pad, bilinear, quantised;
  masks    the matching 128 one-channel masks -> 48 x 48 int32, pad, nearest;
  frame    one 720 x 1280 x 3 frame, centre crop of the middle half of its columns, pad -> 256 x 256 x 3.
Per workload it prints
  hip_us     one launch (event pairs around N back-to-back calls with `out=` given, profiler off);
  stock_us   what a caller does today on the same device and inputs, timed in alternation with the above: per image
             `F.pad` + `F.interpolate` (bilinear, or nearest for the masks) + round half up + rescale, then `torch.stack`
             (it interpolates in fp32, so its rounding differs from the exact form at ties: timed, not compared);
  bytes      computed from the shapes, the least the algorithm needs: per sample the smaller of the view's bytes and the
             taps it takes (4 per output pixel and channel for bilinear, 1 for nearest), 32 B of descriptor, and the
             fp32 / int32 output written.  A reduction touches only part of its source, in runs shorter than a cache
             line, so the memory system moves more than this count: the rate printed is a lower bound of the traffic.
Every time printed here is measured on the device this runs on; the byte counts are arithmetic."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]

import gather_timing  # noqa: E402

N_IMAGES, LO, HI, S, W = 128, 200, 1000, 256, 48
FRAME = (720, 1280)


def ragged_sizes(n=N_IMAGES, lo=LO, hi=HI, seed=0):
    """[(h, w)] drawn from lo..hi inclusive."""
    rng = np.random.default_rng(seed)
    return [(int(h), int(w)) for h, w in rng.integers(lo, hi + 1, (n, 2))]


def frame_crop(frame=FRAME, lo=0.25, hi=0.75):
    """(h, w) of the centre crop predict_realtime.py:54 takes."""
    return frame[0], int(hi * frame[1]) - int(lo * frame[1])


def hip_bytes(sizes, C, out_hw, taps):
    """(read, written) of one launch over views of `sizes`, the least the algorithm needs: per sample
    min(h w C, taps H W C) source bytes (taps = 4 bilinear, 1 nearest) + 32 B of descriptor; C planes of H x W
    4-byte items written."""
    H, W = out_hw
    read = sum(min(h * w * C, taps * H * W * C) for h, w in sizes) + 32 * len(sizes)
    return read, len(sizes) * C * H * W * 4


def workloads():
    sizes = ragged_sizes()
    return {"images": (sizes, 3, (S, S), 4), "masks": (sizes, 1, (W, W), 1), "frame": ([frame_crop()], 3, (S, S), 4)}


def trace_medians(path):
    """Median duration (us) and count of the resize_pad dispatches of a rocprofv3 kernel trace, per (kernel, grid)."""
    return gather_timing.trace_medians(path, "resize_pad_kernel")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--kernels-only", action="store_true", help="20 launches per workload, nothing else (for a kernel trace)")
    ap.add_argument("--trace-csv", help="summarise the resize kernels of a rocprofv3 kernel trace (no GPU needed)")
    a = ap.parse_args()
    if a.trace_csv:
        print(json.dumps(trace_medians(a.trace_csv), indent=1))
        return
    import ilps_amd  # noqa: F401
    from ilps_amd import preprocess as pp
    F = torch.nn.functional
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(1)
    sizes = ragged_sizes()
    imgs_np = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in sizes]
    masks_np = [rng.integers(0, 32, (h, w), dtype=np.uint8) for h, w in sizes]
    imgs, masks = pp.RaggedImages.from_arrays(imgs_np, dev), pp.RaggedImages.from_arrays(masks_np, dev)
    frame = pp.RaggedImages.from_dense(torch.from_numpy(rng.integers(0, 256, (1,) + FRAME + (3,), dtype=np.uint8)).to(dev))
    crop = frame.center_crop_width()
    # the same pixels as separate tensors, which is what a caller holds today
    t_imgs = [torch.from_numpy(x).to(dev) for x in imgs_np]
    t_masks = [torch.from_numpy(x).to(dev) for x in masks_np]
    t_frame = frame.data.view(FRAME + (3,))
    o_img = torch.empty(N_IMAGES, 3, S, S, device=dev)
    o_lab = torch.empty(N_IMAGES, W, W, dtype=torch.int32, device=dev)
    o_frm = torch.empty(1, 3, S, S, device=dev)

    def stock_image(x):                                   # (h, w, 3) uint8 -> (3, S, S) fp32
        h, w = x.shape[:2]
        _, _, top, left = pp.pad_geometry(h, w)
        p = F.pad(x.permute(2, 0, 1)[None].float(), (left, left, top, top))
        y = F.interpolate(p, size=(S, S), mode="bilinear", align_corners=False)
        return (torch.floor(y + 0.5) * (1 / 255.))[0]

    def stock_mask(x):
        h, w = x.shape
        _, _, top, left = pp.pad_geometry(h, w)
        p = F.pad(x[None, None].float(), (left, left, top, top))
        return F.interpolate(p, size=(W, W), mode="nearest")[0, 0].to(torch.int32)

    lo, hi = int(0.25 * FRAME[1]), int(0.75 * FRAME[1])
    runs = {
        "images": (lambda: pp.load_images(imgs, S, pad=True, out=o_img), lambda: torch.stack([stock_image(x) for x in t_imgs])),
        "masks": (lambda: pp.load_labels(masks, W, pad=True, out=o_lab), lambda: torch.stack([stock_mask(x) for x in t_masks])),
        "frame": (lambda: pp.load_images(crop, S, pad=True, out=o_frm), lambda: torch.stack([stock_image(t_frame[:, lo:hi])])),
    }
    if a.kernels_only:
        for hip, _ in runs.values():
            for _ in range(20):
                hip()
        torch.cuda.synchronize()
        print("kernels-only run done")
        return
    res = {}
    for name, args in workloads().items():
        r, w = hip_bytes(*args)
        us, stock_us = gather_timing.timed_pair(runs[name][0], runs[name][1], a.iters, warm=3)
        res[name] = {"MB_read_min": round(r / 1e6, 3), "MB_written": round(w / 1e6, 3), "hip_us": round(us, 1),
                     "stock_us": round(stock_us, 1), "TB_per_s_min": round((r + w) / us / 1e6, 3),
                     "stock_over_hip": round(stock_us / us, 1)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
