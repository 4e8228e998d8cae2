"""Timing of the data generator (csrc/augment.hip through augment.warp_images / warp_labels / DeviceBatches), one GPU:
    python tools/augment_time.py [--iters N] [--no-step]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/augment_time.py --kernels-only      # kernel times, own run
    python tools/augment_time.py --trace-csv DIR/.../*_kernel_trace.csv       # median us per (warp kernel, grid) of that run
256 x 256 x 3 images + 48 x 48 labels out of a 256-row uint8 pool, the reference's draws (10 deg / 0.05 / 0.15 / 0.15),
B in {32, 128, 256, 1024}, nearest and bilinear.  Per B it prints
  warps_us      the two launches with the matrices given (event pairs around N back-to-back calls, profiler off);
  batch_us      one `next(DeviceBatches)`: index stream, draws, three matrix builds' worth of small torch ops, the launches;
  stock_us      the stock-torch formulation a user would otherwise write, on the same device and inputs, timed in
                alternation with the above: pool[index].permute(0, 3, 1, 2).float() * rescale -> F.affine_grid ->
                F.grid_sample(mode='nearest', padding_mode='border'), labels likewise (it rounds halves to even and
                uses another pixel convention, and only the linear part of each matrix is carried over: timed, not compared);
  bytes         computed from the shapes: uint8 read at most once per output pixel, fp32 / int32 written; the stock
                path's bytes count every tensor it reads and writes (gathered uint8 copy, fp32 copy, grid, output);
and, unless --no-step, `SegTrainer.step_timed` at B = 128 and 256 with the generator's share of it.
Every time printed here is measured on the device this runs on; the byte counts and the 6.3 TB/s share are arithmetic."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]

import ilps_amd  # noqa: E402,F401
from ilps_amd import augment  # noqa: E402
import gather_timing  # noqa: E402

HBM_TBPS = 6.3                     # achievable HBM rate of an MI355X
REF = dict(rotation_range=10, width_shift_range=0.05, height_shift_range=0.05, shear_range=0.15, zoom_range=0.15)
S, W, NPOOL = 256, 48, 256


def hip_bytes(B):
    """(read, written): at most one uint8 texel per channel and output pixel, fp32 image planes, int32 label map."""
    return B * (S * S * 3 + W * W), B * (S * S * 3 * 4 + W * W * 4)


def stock_bytes(B):
    img = B * S * S * 3 * (1 + 1) + B * S * S * 3 * (1 + 4) + B * S * S * 3 * (4 + 4)      # gather, float, scale
    img += B * S * S * 2 * 4 * 2 + B * S * S * 3 * (4 + 4)                                # grid written + read, sample
    lab = B * S * S * (1 + 1) + B * S * S * (1 + 4) + B * W * W * 2 * 4 * 2 + B * W * W * (4 + 4) + B * W * W * (4 + 4)
    return img + lab


def trace_medians(path):
    """Median duration (us) and count of the affine_warp dispatches of a rocprofv3 kernel trace, per (kernel, grid):
    the grid tells the batch (B * ceil(H * W / 1024) workgroups of 256 threads)."""
    return gather_timing.trace_medians(path, "affine_warp_kernel")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--kernels-only", action="store_true", help="20 launches per size and mode, nothing else (for a kernel trace)")
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--trace-csv", help="summarise the warp kernels of a rocprofv3 kernel trace (no GPU needed)")
    a = ap.parse_args()
    if a.trace_csv:
        print(json.dumps(trace_medians(a.trace_csv), indent=1))
        return
    F = torch.nn.functional
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    pool_i = torch.randint(0, 256, (NPOOL, S, S, 3), dtype=torch.uint8, device=dev, generator=g)
    pool_l = torch.randint(0, 32, (NPOOL, S, S), dtype=torch.uint8, device=dev, generator=g)
    gen = augment.ImageDataGenerator(rescale=1 / 255., **REF)
    res = {}
    for B in (32, 128, 256, 1024):
        d = gen.random_draws(B, g)
        Mi, Ml = augment.affine_matrices(d, S), augment.affine_matrices(d, W)
        idx = torch.randint(0, NPOOL, (B,), device=dev, generator=g)
        oi = torch.empty(B, 3, S, S, device=dev)
        ol = torch.empty(B, W, W, dtype=torch.int32, device=dev)

        def warps(mode="nearest"):
            augment.warp_images(pool_i, Mi, S, idx, 1 / 255., mode, out=oi)
            augment.warp_labels(pool_l, Ml, W, idx, out=ol)

        if a.kernels_only:
            for mode in ("nearest", "bilinear"):
                for _ in range(20):
                    warps(mode)
            torch.cuda.synchronize()
            continue
        theta_i = torch.stack([Mi[:, 1, [1, 0]], Mi[:, 0, [1, 0]]], 1)
        theta_i = torch.cat([theta_i, torch.zeros(B, 2, 1, device=dev)], 2).contiguous()

        def stock():
            x = pool_i[idx].permute(0, 3, 1, 2).float() * (1 / 255.)
            im = F.grid_sample(x, F.affine_grid(theta_i, (B, 3, S, S), align_corners=False), mode="nearest",
                               padding_mode="border", align_corners=False)
            y = pool_l[idx][:, None].float()
            lb = F.grid_sample(y, F.affine_grid(theta_i, (B, 1, W, W), align_corners=False), mode="nearest",
                               padding_mode="border", align_corners=False)
            return im, lb[:, 0].to(torch.int32)

        batches = iter(augment.DeviceBatches(pool_i, pool_l, B, S, W, gen, generator=g))
        r, w = hip_bytes(B)
        row = {"MB_read_max": round(r / 1e6, 2), "MB_written": round(w / 1e6, 2), "stock_MB_moved": round(stock_bytes(B) / 1e6, 1)}
        us, stock_us = gather_timing.timed_pair(warps, stock, a.iters, warm=10)
        us_bl, batch_us = gather_timing.timed_pair(lambda: warps("bilinear"), lambda: next(batches), a.iters, warm=10)
        row.update(warps_us=round(us, 1), warps_bilinear_us=round(us_bl, 1), batch_us=round(batch_us, 1),
                   stock_us=round(stock_us, 1), TB_per_s=round((r + w) / us / 1e6, 3),
                   share_of_6p3=round((r + w) / us / 1e6 / HBM_TBPS, 3), stock_over_hip=round(stock_us / us, 1),
                   stock_bytes_over_hip=round(stock_bytes(B) / (r + w), 2))
        res["B%d" % B] = row
    if a.kernels_only:
        print("kernels-only run done")
        return
    if not a.no_step:
        from ilps_amd.smpl_model import synthetic_smpl_model
        from ilps_amd.training import SegTrainer
        torch.manual_seed(0)
        tr = SegTrainer(synthetic_smpl_model(1234), output_wh=W, encoder_architecture="enet", use_IEF=True, device=dev)
        tr.smpl_model.train()
        for B in (128, 256):
            batches = iter(augment.DeviceBatches(pool_i, pool_l, B, S, W, gen, generator=g))
            for _ in range(3):
                tr.step(*next(batches))
            ms = sorted(tr.step_timed(*next(batches))["total_ms"] for _ in range(10))
            step_ms = ms[len(ms) // 2]
            res["B%d" % B].update(step_ms=round(step_ms, 2),
                                  batch_over_step=round(res["B%d" % B]["batch_us"] / 1e3 / step_ms, 4),
                                  warps_over_step=round(res["B%d" % B]["warps_us"] / 1e3 / step_ms, 5))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
