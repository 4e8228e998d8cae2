"""What tools/augment_time.py and tools/preprocess_time.py share: the alternating event timer and the summary of a
rocprofv3 kernel trace.  Not a tool of its own."""


def timed_pair(fa, fb, iters, warm):
    """us per call of fa and fb, measured in alternating blocks of iters / 4 calls."""
    import torch
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


def trace_medians(path, kernel_name):
    """Median duration (us) and count of the dispatches of kernel_name's instantiations in a rocprofv3 kernel trace, per
    (template arguments, grid)."""
    import csv
    groups = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row.get("Kernel_Name", "")
            if kernel_name not in name:
                continue
            key = (name.split(kernel_name)[1].split(">")[0] + ">", int(row.get("Grid_Size_X", row.get("Grid_Size", 0))))
            groups.setdefault(key, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    out = {}
    for (name, grid), v in sorted(groups.items()):
        v.sort()
        out["%s grid %d" % (name, grid)] = {"n": len(v), "median_us": round(v[len(v) // 2], 2), "min_us": round(v[0], 2)}
    return out
