"""Kernel times of the encoder's batch-norm / PReLU kernels, fp32 against bf16, on ENet's three plane sizes:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/encoder_kernel_time.py      # the run
    python tools/encoder_kernel_time.py --trace-csv DIR/*/*_kernel_trace.csv [--batch 128]                  # the table
The run calls, per shape (B, 16, 128, 128), (B, 64, 64, 64), (B, 128, 32, 32) and per dtype, forward + backward of
ops.BatchNormActFn, ops.BatchNormResActFn and ops.PReLUFn --reps times (the first one included: these kernels pick no
solver and the figure is a median).  The table reads the dispatches back in launch order - the same (shape, dtype, op)
sequence - and gives the median us, the bytes a kernel must move (its streamed tensors once each: a count, not a
counter) and the TB/s that makes, fp32 beside bf16.  No timing is taken by the run itself."""
import argparse
import csv
import os
import re
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.append(ROOT)

SHAPES = [(16, 128, 128), (64, 64, 64), (128, 32, 32)]
DTYPES = ("fp32", "bf16")
# op -> its kernels in launch order (finalize / reduce kernels work on per-channel partials: not tabled), and per kernel
# the tensors it reads + writes once each
OPS = [("bn_act", [("bn_stats", 1), ("bn_apply<ACT>", 2), ("bn_bwd_stats<ACT>", 2), ("bn_bwd_apply<ACT>", 3)]),
       ("bn_res", [("bn_stats", 1), ("bn_apply<RES>", 3), ("bn_bwd_stats<RES>", 3), ("bn_bwd_apply<RES>", 5)]),
       ("prelu", [("prelu_fwd", 2), ("prelu_bwd", 3)])]
STREAMING = re.compile(r"smplr(?:::|\d+)(bnh?_stats|bnh?_apply|bnh?_bwd_stats|bnh?_bwd_apply|preluh?_fwd|preluh?_bwd)_kernel")


def run(B, reps):
    import torch
    import ilps_amd  # noqa: F401
    from ilps_amd import ops
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    for C, H, W in SHAPES:
        par = [torch.rand(C, device=dev, generator=g) + 0.5 for _ in range(2)] + [torch.rand(C, device=dev, generator=g) * 0.5]
        rm, rv = torch.zeros(C, device=dev), torch.ones(C, device=dev)
        scale = (torch.rand(B, C, device=dev, generator=g) > 0.1).float() / 0.9
        for dt in (torch.float32, torch.bfloat16):
            x = torch.randn(B, C, H, W, device=dev, generator=g).to(dt).requires_grad_(True)
            other = torch.randn(B, C, H, W, device=dev, generator=g).to(dt).requires_grad_(True)
            gy = torch.randn(B, C, H, W, device=dev, generator=g).to(dt)
            gamma, beta, slope = (p.clone().requires_grad_(True) for p in par)
            for _ in range(reps):
                ops.BatchNormActFn.apply(x, gamma, beta, slope, rm, rv, 1e-3, 0.1).backward(gy)
            for _ in range(reps):
                ops.BatchNormResActFn.apply(x, other, gamma, beta, slope, scale, rm, rv, 1e-3, 0.1).backward(gy)
            for _ in range(reps):
                ops.PReLUFn.apply(x, slope).backward(gy)
            torch.cuda.synchronize()
            del x, other, gy
    print("encoder_kernel_time: %d shapes x %d dtypes x %d reps done" % (len(SHAPES), len(DTYPES), reps))


def table(path, B, reps):
    rows = [(int(r["Start_Timestamp"]), (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3, r["Kernel_Name"])
            for r in csv.DictReader(open(path)) if STREAMING.search(r["Kernel_Name"])]
    rows.sort()
    per_seg = reps * sum(len(ks) for _, ks in OPS)
    assert len(rows) == per_seg * len(SHAPES) * len(DTYPES), "%d streaming dispatches, expected %d" % (
        len(rows), per_seg * len(SHAPES) * len(DTYPES))
    us, i = {}, 0
    for shape in SHAPES:
        for dt in DTYPES:
            for op, ks in OPS:
                acc = {k: [] for k, _ in ks}
                for _ in range(reps):
                    for k, _ in ks:
                        stem = k.split("<")[0]
                        name = rows[i][2]
                        want = (stem.replace("bn_", "bnh_", 1).replace("prelu_", "preluh_", 1) if dt == "bf16" else stem) + "_kernel"
                        assert re.search(r"(::|\d)" + want, name), "dispatch %d is %s, expected %s" % (i, name, want)
                        acc[k].append(rows[i][1])
                        i += 1
                for k, v in acc.items():
                    us[(shape, dt, op, k)] = statistics.median(v)
    print("| plane (B = %d) | op | kernel | fp32 us | fp32 MB | fp32 TB/s | bf16 us | bf16 MB | bf16 TB/s | bf16 / fp32 time |" % B)
    print("|---|---|---|---|---|---|---|---|---|---|")
    for shape in SHAPES:
        C, H, W = shape
        for op, ks in OPS:
            for k, tensors in ks:
                cells = []
                for dt, size in (("fp32", 4), ("bf16", 2)):
                    t, b = us[(shape, dt, op, k)], tensors * size * B * C * H * W
                    cells += ["%.1f" % t, "%.1f" % (b / 1e6), "%.2f" % (b / t / 1e6)]
                print("| %d x %d x %d | %s | %s | %s | %.2f |" % (C, H, W, op, k, " | ".join(cells),
                                                             us[(shape, "bf16", op, k)] / us[(shape, "fp32", op, k)]))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--trace-csv")
    a = ap.parse_args()
    if a.trace_csv:
        table(a.trace_csv, a.batch, a.reps)
    else:
        run(a.batch, a.reps)
