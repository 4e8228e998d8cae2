"""Timing of the 3D evaluation kernel (csrc/eval3d.hip through eval3d.point_errors), one GPU:
    python tools/eval3d_time.py [--iters N]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/eval3d_time.py --kernels-only      # kernel times, own run
    python tools/eval3d_time.py --trace-csv DIR/.../*_kernel_trace.csv        # median us per (kernel form, grid) of that run
At B in {1, 128, 1 024} x N in {19, 6 890} it prints
  hip_us     one call (means + status; event pairs around N back-to-back calls, profiler off);
  stock_us   the composition a caller writes today, on the same device and inputs, timed in alternation with the above:
             elementwise ops and reductions for the four modes plus a batched `torch.linalg.svd` of the 3 x 3 covariances;
  MB         the compulsory traffic 2 B N 12 bytes (both point sets read once; the outputs are 20 B per mesh);
  bound_us   MB at 5 TB/s, the HBM rate DESIGN.md section 8 uses for its lower bounds.
Every time printed here is measured on the device this runs on; the byte counts and the bound are arithmetic."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = [(B, N) for N in (19, 6890) for B in (1, 128, 1024)]
HBM_TB_S = 5.0


def compulsory_bytes(B, N):
    return 2 * B * N * 12


def trace_medians(path):
    """Median duration (us) and count of the point_errors dispatches of a rocprofv3 kernel trace, per (form, workgroups)."""
    import csv
    groups = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row.get("Kernel_Name", "")
            if "point_errors_kernel" not in name:
                continue
            form = name.split("point_errors_kernel")[1].split(">")[0] + ">"
            wg = int(row.get("Workgroup_Size_X", row.get("Workgroup_Size", 1)) or 1)
            grid = int(row.get("Grid_Size_X", row.get("Grid_Size", 0))) // max(wg, 1)
            groups.setdefault((form, grid), []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    out = {}
    for (form, grid), v in sorted(groups.items()):
        v.sort()
        out["%s workgroups %d" % (form, grid)] = {"n": len(v), "median_us": round(v[len(v) // 2], 2), "min_us": round(v[0], 2)}
    return out


def stock_point_errors(p, g):
    """The four per-mesh mean errors in stock torch (fp32 on the device, as a caller would write them)."""
    mp, mg = p.mean(1, keepdim=True), g.mean(1, keepdim=True)
    pc, gc = p - mp, g - mg
    spp = pc.square().sum((1, 2))
    M = gc.transpose(1, 2) @ pc
    U, S, Vh = torch.linalg.svd(M)
    d = torch.sign(torch.linalg.det(U) * torch.linalg.det(Vh))
    D = torch.ones_like(S)
    D[:, 2] = d
    R = (U * D[:, None, :]) @ Vh
    s2 = torch.diagonal(M, dim1=1, dim2=2).sum(1) / spp
    s3 = (S * D).sum(1) / spp
    return torch.stack([(p - g).norm(dim=2).mean(1), (pc - gc).norm(dim=2).mean(1),
                        (s2[:, None, None] * pc - gc).norm(dim=2).mean(1),
                        (s3[:, None, None] * (pc @ R.transpose(1, 2)) - gc).norm(dim=2).mean(1)], 1)


def timed_pair(fa, fb, iters, warm=3):
    """us per call of fa and fb, measured in alternating blocks of iters / 4 calls."""
    for _ in range(warm):
        fa()
        fb()
    torch.cuda.synchronize()
    tot = [0.0, 0.0]
    blocks, n = 4, max(1, iters // 4)
    for _ in range(blocks):
        for k, fn in enumerate((fa, fb)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(n):
                fn()
            e1.record()
            torch.cuda.synchronize()
            tot[k] += e0.elapsed_time(e1) * 1000.0
    return tot[0] / (blocks * n), tot[1] / (blocks * n)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--kernels-only", action="store_true", help="20 launches per size, nothing else (for a kernel trace)")
    ap.add_argument("--trace-csv", help="summarise the point_errors kernels of a rocprofv3 kernel trace (no GPU needed)")
    a = ap.parse_args()
    if a.trace_csv:
        print(json.dumps(trace_medians(a.trace_csv), indent=1))
        return
    import ilps_amd  # noqa: F401
    from ilps_amd.eval3d import point_errors
    dev = torch.device("cuda:0")
    res = {}
    for B, N in SIZES:
        gen = torch.Generator(device=dev).manual_seed(B * 7919 + N)
        g = torch.randn(B, N, 3, device=dev, generator=gen) * torch.tensor([0.3, 0.6, 0.15], device=dev)
        p = 1.1 * g.roll(1, 2) + 0.02 * torch.randn(B, N, 3, device=dev, generator=gen) + 0.5
        hip = lambda: point_errors(p, g)
        if a.kernels_only:
            for _ in range(20):
                hip()
            continue
        us, stock_us = timed_pair(hip, lambda: stock_point_errors(p, g), a.iters)
        diff = float((point_errors(p, g)["mean_err"] - stock_point_errors(p, g)).abs().max())
        mb = compulsory_bytes(B, N) / 1e6
        res["B%d_N%d" % (B, N)] = {"MB": round(mb, 3), "bound_us": round(mb / HBM_TB_S, 2), "hip_us": round(us, 1),
                                   "stock_us": round(stock_us, 1), "stock_over_hip": round(stock_us / us, 1),
                                   "TB_per_s": round(mb / us, 3), "max_diff_m": float("%.2e" % diff)}
    torch.cuda.synchronize()
    print("kernels-only run done" if a.kernels_only else json.dumps(res))


if __name__ == "__main__":
    main()
