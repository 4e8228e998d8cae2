"""Timing of the fused silhouette loss head (csrc/silh_loss.hip, SMPLDecoder(silh_loss=...)), one GPU:
    python tools/silh_loss_time.py [--iters N] [--blocks K] [--batches 128,512] [--wh 48]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/silh_loss_time.py --kernels-only   # kernel times, own run
    python tools/silh_loss_time.py --trace-csv DIR/.../*_kernel_trace.csv       # median us per silhouette kernel of that run
What is timed: the decoder part of a train pass - decoder forward, loss mean, backward down to the gradient of the
86-vector - for
  silh   the silhouette-only pass of the alternating schedule (train_stage2_silhouette.py:262-270),
  both   the 31-part head (loss fused into the rasteriser) + the silhouette head in one pass,
each with and without the silhouette accuracy counts (`conf`), in three variants:
  unfused     what SegTrainer runs without fused_silh_loss: silhouette written, softmax + cross-entropy kernel, its
              backward through a (B, W, W, 2) gradient, the confusion kernel - no code of the fused head runs: the comparator;
  standalone  SMPLDecoder(silh_loss=...) with SMPLR_SILH_LOSS_EPILOGUE=0: silhouette forward, then silh_loss_fwd_kernel;
  epilogue    the same with SMPLR_SILH_LOSS_EPILOGUE=1: the loss head inside silh_px_kernel.
Device events around `--iters` calls per block (>= 200), the variants alternating over `--blocks` blocks each (>= 4), every
shape warmed up first, profiler off.  Per variant: the median block (us per pass) and the block-to-block spread
(max - min); a variant is called faster than another only where the gap of the medians exceeds both spreads."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VARIANTS = ("unfused", "standalone", "epilogue")
PASSES = ("silh", "both")
KERNELS = ("silh_px_kernel", "silh_fused_kernel", "silh_loss_fwd_kernel", "silh_loss_bwd_kernel", "silh_bwd_kernel",
           "focal_kernel", "confusion")


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--iters", type=int, default=200, help="calls per block (at least 200)")
    ap.add_argument("--blocks", type=int, default=4, help="blocks per variant (at least 4), variants alternating")
    ap.add_argument("--batches", default="128,512")
    ap.add_argument("--wh", type=int, default=48)
    ap.add_argument("--kernels-only", action="store_true", help="20 passes per case, nothing else (for a kernel trace)")
    ap.add_argument("--trace-csv", help="summarise the silhouette kernels of a rocprofv3 kernel trace (no GPU needed)")
    a = ap.parse_args(argv)
    a.batches = [int(b) for b in str(a.batches).split(",") if b]
    if not a.trace_csv and not a.kernels_only and (a.iters < 200 or a.blocks < 4):
        ap.error("--iters >= 200 and --blocks >= 4: fewer calls do not average the launch jitter out")
    return a


def trace_medians(path):
    """Median / min duration (us) and count of the silhouette path's dispatches in a rocprofv3 kernel trace, per
    (kernel, template arguments, workgroups)."""
    import csv
    groups = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row.get("Kernel_Name", "")
            hit = next((k for k in KERNELS if k in name), None)
            if hit is None:
                continue
            targs = name.split(hit, 1)[1]
            targs = targs[:targs.index(">") + 1] if targs.startswith("<") and ">" in targs else ""
            wg = int(row.get("Workgroup_Size_X", row.get("Workgroup_Size", 1)) or 1)
            grid = int(row.get("Grid_Size_X", row.get("Grid_Size", 0))) // max(wg, 1)
            groups.setdefault((hit + targs, grid), []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    out = {}
    for (kern, grid), v in sorted(groups.items()):
        v.sort()
        out["%s workgroups %d" % (kern, grid)] = {"n": len(v), "median_us": round(v[len(v) // 2], 2), "min_us": round(v[0], 2)}
    return out


def summarise(blocks_us):
    """Per-variant block times (us per pass) -> median, spread (max - min) and the blocks themselves."""
    v = sorted(blocks_us)
    med = v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])
    return {"median_us": round(med, 2), "spread_us": round(v[-1] - v[0], 2), "blocks_us": [round(b, 2) for b in blocks_us]}


def verdict(a, b):
    """'faster' / 'slower' / 'same' for summary a against summary b: only a gap beyond both spreads counts."""
    gap = b["median_us"] - a["median_us"]
    noise = max(a["spread_us"], b["spread_us"])
    return "faster" if gap > noise else ("slower" if -gap > noise else "same")


_BASE = []


def build_pass(kind, variant, with_conf, B, W, model, dev, seed):
    """-> a callable running one pass (forward, loss mean, backward)."""
    import torch
    import bench
    from ilps_amd.decoder import SMPLDecoder
    from ilps_amd.focal_loss import softmax_focal_loss
    from ilps_amd.metrics import SegConfusion
    heads = ("silhouette",) if kind == "silh" else ("seg", "silhouette")
    ce = softmax_focal_loss(0.0, False)
    fused = variant != "unfused"
    dec = SMPLDecoder(model, img_wh=W, heads=heads, outputs=(), loss=softmax_focal_loss(2.0, True) if kind == "both" else None,
                      silh_loss=ce if fused else None)
    if _BASE:
        dec.share_constants(_BASE[0])         # one upload of the SMPL constants for all the decoders
    else:
        _BASE.append(dec)
    x = torch.tensor(bench.make_x(B, W, seed), device=dev, requires_grad=True)
    gen = torch.Generator().manual_seed(seed)
    sl = torch.randint(0, 2, (B, W, W), generator=gen, dtype=torch.int32).to(dev)
    lab = torch.randint(0, 32, (B, W, W), generator=gen, dtype=torch.int32).to(dev) if kind == "both" else None
    conf = SegConfusion(2, dev) if with_conf else None
    epi = "1" if variant == "epilogue" else "0"

    def run():
        x.grad = None
        if fused:
            out = dec(x, lab, silh_labels=sl, silh_confusion=conf)
            loss = out["silh_loss"].mean()
        else:
            out = dec(x, lab)
            loss = ce(sl, out["silhouette"]).mean()
            if conf is not None:
                conf.update(out["silhouette"], sl)
        if kind == "both":
            loss = loss + out["seg_loss"].mean()
        loss.backward()
    run.epilogue = epi              # what SMPLR_SILH_LOSS_EPILOGUE holds while this variant runs (set per block, not per call)
    return run


def run_n(fn, n):
    os.environ["SMPLR_SILH_LOSS_EPILOGUE"] = fn.epilogue
    for _ in range(n):
        fn()


def time_case(fns, iters, blocks, warm=10):
    """fns: variant -> callable; -> variant -> list of per-block us per call, the variants alternating block by block."""
    import torch
    for fn in fns.values():
        run_n(fn, warm)
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(blocks):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            os.environ["SMPLR_SILH_LOSS_EPILOGUE"] = fn.epilogue
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            out[k].append(e0.elapsed_time(e1) * 1000.0 / iters)
    return out


def main(argv=None):
    a = parse_args(argv)
    if a.trace_csv:
        print(json.dumps(trace_medians(a.trace_csv), indent=1))
        return
    import torch
    import ilps_amd  # noqa: F401
    from ilps_amd.smpl_model import synthetic_smpl_model
    dev = torch.device("cuda:0")
    model = synthetic_smpl_model(1234)
    prev = os.environ.get("SMPLR_SILH_LOSS_EPILOGUE")
    res = {}
    try:
        for B in a.batches:
            for kind in PASSES:
                for with_conf in (False, True):
                    fns = {v: build_pass(kind, v, with_conf, B, a.wh, model, dev, 1000 + B) for v in VARIANTS}
                    key = "B%d_%s%s" % (B, kind, "_conf" if with_conf else "")
                    if a.kernels_only:
                        for fn in fns.values():
                            run_n(fn, 20)
                        continue
                    s = {v: summarise(t) for v, t in time_case(fns, a.iters, a.blocks).items()}
                    s["standalone_vs_unfused"] = verdict(s["standalone"], s["unfused"])
                    s["epilogue_vs_unfused"] = verdict(s["epilogue"], s["unfused"])
                    s["epilogue_vs_standalone"] = verdict(s["epilogue"], s["standalone"])
                    res[key] = s
                    print(key, json.dumps(s), flush=True)
    finally:
        if prev is None:
            os.environ.pop("SMPLR_SILH_LOSS_EPILOGUE", None)
        else:
            os.environ["SMPLR_SILH_LOSS_EPILOGUE"] = prev
    torch.cuda.synchronize()
    print("kernels-only run done" if a.kernels_only else json.dumps(res))


if __name__ == "__main__":
    main()
