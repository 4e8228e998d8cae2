"""Timing of the self-penetration term (csrc/penetration.hip through penetration.self_penetration), one GPU, one shape per run:
    timeout -k 10 300 python tools/penetration_time.py --batch 1 && timeout -k 10 300 python tools/penetration_time.py --batch 128
    timeout -k 10 300 python tools/penetration_time.py --batch 128 --fit
    timeout -k 10 300 python tools/penetration_time.py --batch 128 --launches
V = 6 890: the synthetic SMPL model's vertices at seeded poses (each body part a blob around a bone), the part tables of the package, an open soup of small faces inside the parts for the normals, and the
default part-pair table (no face joins two parts here, so every pair of distinct parts collides: the most pairs a table can
ask for).  Per call:
    hip        `self_penetration(verts, topo)`: one forward launch (the pruned walk); with the backward of sum(e) one backward
               launch more (+ torch's own kernels for the sum and the cotangent)
    hip_plain  the same with SMPLR_PEN_UNPRUNED=1: natural order, every tile - the same bits
    stock      `penetration.self_penetration_torch` on device tensors - the package's float64 torch restatement, chunked so
               that no (B, V, V) tensor exists - followed by the gradient definition in torch (index_add_).  It is timed on
               --stock-meshes meshes of the same problem and its figure is for THAT sub-problem; nothing is extrapolated.
--shrink S scales every part about its own centroid: the synthetic model's parts are blobs of about 0.2 m radius on a body
0.9 m wide, fatter than limbs, and what the pruned walk skips depends on how compact the parts are.
Each figure is a host clock around back-to-back calls that ends in a device synchronise, after untimed calls of the same
shape; the calls per window come from one timed call (about --window seconds per window, 2 to 200 calls); the legs
alternate --rounds times, every round is printed, the median is reported.
--fit times `ParamFitter.fit(graph=True)` per iteration with and without the term on tools/fit_time.py's problem (the same
loop as its "graph" leg: run that tool on the same box for the figure without the term as DESIGN.md section 14 has it).
--launches counts the device kernels per call and sums their device time with torch.profiler, in a run of its own."""
import argparse
import contextlib
import importlib.util
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ilps_amd  # noqa: E402,F401
from _timing import calls_per_window, profile_calls, rounds  # noqa: E402

KERNELS = ("pen_fwd_kernel", "pen_bwd_kernel")


@contextlib.contextmanager
def plain_walk():
    os.environ["SMPLR_PEN_UNPRUNED"] = "1"
    try:
        yield
    finally:
        del os.environ["SMPLR_PEN_UNPRUNED"]


def soup_topology():
    """Consecutive vertices of the part tables, three at a time: 2 293 small faces, each inside one body part."""
    from ilps_amd.render import MeshTopology
    from ilps_amd.smpl_model import load_part_tables
    ids, _ = load_part_tables(1)
    return MeshTopology(np.asarray(ids[:(len(ids) // 3) * 3], np.int32).reshape(-1, 3), 6890)


def problem(B, seed=0, shrink=1.0):
    from _inputs import make_x
    from ilps_amd.keras_smpl.batch_smpl import SMPLLayer
    from ilps_amd.smpl_model import synthetic_smpl_model
    layer = SMPLLayer(synthetic_smpl_model(1234))
    x = torch.from_numpy(make_x(B, 48, seed=seed)).cuda()
    with torch.no_grad():
        verts = layer(x).contiguous()
    topo = soup_topology()
    if shrink != 1.0:
        # every part pulled towards its own centroid: parts as compact as limbs (the synthetic model's are blobs of 0.2 m radius)
        part = torch.from_numpy(topo.vertex_part).to(verts.device)
        for p in range(int(part.max()) + 1):
            m = part == p
            c = verts[:, m].mean(1, keepdim=True)
            verts[:, m] = c + shrink * (verts[:, m] - c)
    return verts, topo


def fit_legs(B, iters, G):
    """us per `ParamFitter.fit(graph=True)` iteration without the term, with it, and with it on the plain walk."""
    from ilps_amd.fitting import ParamFitter
    spec = importlib.util.spec_from_file_location("fit_time", os.path.join(ROOT, "tools", "fit_time.py"))
    fit_time = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fit_time)
    plain = ParamFitter(None, img_wh=48)
    with_pen = ParamFitter(None, img_wh=48, penetration=soup_topology())
    labels, x0, _ = fit_time.problem(plain, B, 48)
    n = iters - iters % G
    kw = dict(init=x0, steps=n, graph=True, graph_steps=G)

    def pen_plain():
        with plain_walk():
            with_pen.fit(labels, pen_weight=10.0, **kw)
    return n, {"fit": lambda: plain.fit(labels, **kw), "fit_pen": lambda: with_pen.fit(labels, pen_weight=10.0, **kw),
               "fit_pen_plain_walk": pen_plain}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--window", type=float, default=0.4)
    ap.add_argument("--stock-meshes", type=int, default=1)
    ap.add_argument("--no-stock", action="store_true")
    ap.add_argument("--shrink", type=float, default=1.0, help="scale every part about its centroid (1: the model's own blobs)")
    ap.add_argument("--launches", action="store_true")
    ap.add_argument("--fit", action="store_true")
    ap.add_argument("--fit-iters", type=int, default=400)
    ap.add_argument("--graph-steps", type=int, default=10)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("penetration_time.py needs a HIP device: a CPU run gives no timing")
    from ilps_amd import _lib
    from ilps_amd.penetration import _backward_torch, self_penetration, self_penetration_torch
    B = a.batch
    res = {"build_id": _lib.build_id()[:16], "B": B, "V": 6890}
    if a.fit:
        n, legs = fit_legs(B, a.fit_iters, a.graph_steps)
        for fn in legs.values():
            fn()                                                    # untimed: code objects, allocator pools, capture
        res.update(iters=n, graph_steps=a.graph_steps, **rounds(legs, 1, a.rounds, per=n, key="us_per_iteration"))
        print(json.dumps(res))
        return
    verts, topo = problem(B, shrink=a.shrink)
    res["shrink"] = a.shrink
    sb = min(B, a.stock_meshes)
    sv = verts[:sb].contiguous()

    def hip(grad):
        v = verts.detach().requires_grad_(grad)
        e = self_penetration(v, topo)
        if grad:
            e.sum().backward()

    def hip_plain(grad):
        with plain_walk():
            hip(grad)

    def stock(grad):
        o = self_penetration_torch(sv, topo)
        if grad:
            _backward_torch(sv, o["near"], o["inside"], o["status"], torch.ones_like(o["e"]))

    legs = {"hip_fwd": lambda: hip(False), "hip_fwd_bwd": lambda: hip(True), "hip_plain_fwd": lambda: hip_plain(False),
            "hip_plain_fwd_bwd": lambda: hip_plain(True)}
    if not a.no_stock:
        legs.update({"stock_fwd": lambda: stock(False), "stock_fwd_bwd": lambda: stock(True)})
    with torch.no_grad():
        e, det = self_penetration(verts, topo, return_details=True)
    res.update(pairs=B * 6890 * 6890, stock_meshes=sb, stock_pairs=sb * 6890 * 6890,
               with_candidates=float((det["near"] >= 0).float().mean()), inside=float(det["inside"].float().mean()))
    iters = calls_per_window(legs, a.window)
    res["iters"] = iters
    if a.launches:
        res["profile"] = {k: profile_calls(fn, 3, KERNELS, "pen_kernels_us") for k, fn in legs.items() if k.startswith("hip")}
        print(json.dumps(res))
        return
    if not a.no_stock:
        s = self_penetration_torch(sv, topo)
        res["max_abs_diff_hip_stock"] = float((e[:sb] - s["e"]).abs().max())
        res["index_agreement"] = float((det["near"][:sb] == s["near"]).float().mean())
    res.update(rounds(legs, iters, a.rounds))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
