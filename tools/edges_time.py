"""Timing of the edge detector (ilps_amd.edges over csrc/edges.hip), one GPU:
    timeout -k 10 600 python tools/edges_time.py [--batch 128 --size 256 --no-loop]
The source is a Lambert render of sampled bodies on white (the synthetic SMPL model's hull surface unless --smpl names a model
file), form RGB_F32_HWC, blur on, L2, thresholds 100 / 200.  Legs, per call:
    classify      `edge_classes`: one launch of edge_classify_kernel<RGB_F32_HWC, 1, 1>
    link          `link_edges` on that class map: one launch of edge_link_kernel
    canny_hip     `canny_edges`: the pair
    canny_torch   `canny_edges_torch` on the same source on the device: the stock composition, with its `.any()` per pass
    next_edges / next_silhouette   one whole `next(SyntheticBatches(seg=...))` at --input / --output, with 17 joints
Each figure is device-event time around back-to-back calls, after untimed calls of the same shape; the calls per window come
from one timed call (at least --window seconds per window, 1 to 2000 calls).  canny_hip and canny_torch alternate --rounds
times in the same run, every round is printed and the median reported.  The expectation is a comparison only: the pair should
not be slower than the composition it replaces."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--input", type=int, default=256)
    ap.add_argument("--output", type=int, default=48)
    ap.add_argument("--joints", type=int, default=17)
    ap.add_argument("--smpl", default=None, help="an SMPL model file (default: the synthetic model)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--no-loop", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("edges_time.py needs a HIP device: a CPU run gives no timing")
    from ilps_amd import _lib, edges as ed, synthetic as syn
    from ilps_amd.keras_smpl.batch_smpl import SMPLLayer
    from ilps_amd.keypoints import KeypointSpec
    from ilps_amd.render import render_mesh
    dev = torch.device("cuda", torch.cuda.current_device())
    B, S = a.batch, a.size
    layer = SMPLLayer(a.smpl)
    model = layer._model
    topo = syn.hull_topology(model) if model.faces is None else None
    rng = np.random.default_rng(0)
    R = np.zeros((a.joints, model.num_verts), np.float32)
    for k in range(a.joints):
        R[k, rng.choice(model.num_verts, 8, replace=False)] = rng.dirichlet(np.ones(8))
    spec = KeypointSpec(R, model.num_verts)
    kw = dict(spec=spec, corruption={}, topology=topo, device=dev)
    loops = {seg: syn.SyntheticBatches(layer, B, a.input, a.output, seg=seg, **kw) for seg in ("edges", "silhouette")}
    first = loops["edges"]
    s = first.sampler.sample(B, a.output, first.generator)
    rgb = render_mesh(s["verts"], first.topo, s["x"][:, :4], mode="ortho", img_wh=S, scale=float(S) / a.output)["rgb"]
    canny = dict(low=100, high=200, blur=True, l2=True)
    classes = ed.edge_classes(rgb, **canny)
    out = torch.empty_like(classes)
    got, ref = ed.canny_edges(rgb, **canny), ed.canny_edges_torch(rgb, **canny)
    res = {"build_id": _lib.build_id()[:16], "device": torch.cuda.get_device_name(dev), "B": B, "size": S,
           "form": "RGB_F32_HWC", "blur": 1, "l2": 1, "hip_equals_torch": bool(torch.equal(got, ref)),
           "edge_share": round(float(got.float().mean()), 4), "strong_share": round(float((classes == 2).float().mean()), 4)}
    del got, ref
    legs = {"classify": lambda: ed.edge_classes(rgb, **canny), "link": lambda: ed.link_edges(classes, out=out),
            "canny_hip": lambda: ed.canny_edges(rgb, out=out, **canny), "canny_torch": lambda: ed.canny_edges_torch(rgb, **canny)}
    if not a.no_loop:
        legs["next_edges"] = lambda: next(loops["edges"])
        legs["next_silhouette"] = lambda: next(loops["silhouette"])
    iters = {}
    for k, fn in legs.items():
        fn()
        fn()                                                            # untimed
        one = event_ms(fn, 1)
        iters[k] = int(min(2000, max(1, np.ceil(a.window * 1e3 / max(one, 1e-3)))))
    res["iters"] = iters
    ms = {k: [] for k in legs}
    for k in legs:
        if not k.startswith("canny_"):
            ms[k].append(event_ms(legs[k], iters[k]))
    for _ in range(a.rounds):                                           # the two canny legs, alternated
        for k in ("canny_hip", "canny_torch"):
            ms[k].append(event_ms(legs[k], iters[k]))
    res["ms_per_call_rounds"] = {k: [round(v, 4) for v in vs] for k, vs in ms.items()}
    res["ms_per_call"] = {k: round(statistics.median(vs), 4) for k, vs in ms.items()}
    res.update(canny_torch_over_hip=round(res["ms_per_call"]["canny_torch"] / res["ms_per_call"]["canny_hip"], 2),
               hip_not_slower_than_torch=bool(max(ms["canny_hip"]) <= min(ms["canny_torch"])))
    print(json.dumps(res))
    if not res["hip_equals_torch"]:
        sys.exit("canny_edges and canny_edges_torch differ")


if __name__ == "__main__":
    main()
