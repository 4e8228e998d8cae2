"""Timing of the mesh measurements (csrc/measure.hip through measure.mesh_measures), one GPU, one batch size per run:
    timeout -k 10 300 python tools/measure_time.py --batch 128 && timeout -k 10 900 python tools/measure_time.py --batch 2048
    timeout -k 10 300 python tools/measure_time.py --batch 128 --launches
V = 6 890, F = 13 776 (the generated sphere at SMPL's counts, posed), K = 3 planes on every part, per call:
    hip       `mesh_measures(verts, spec)`: one forward launch; with the backward of sum(volume + area + extent + girth), one
              backward launch more (+ torch's own kernels for the sums and the cotangents)
    stock     `measure.measures_torch` on the same device tensors - the package's float64 torch restatement of the
              definitions, which is what a user without the kernels would write - with autograd's backward; in chunks of
              --stock-chunk meshes (its (B, K, F, 3, 3) float64 intermediates are 3 MB per mesh and plane)
Each figure is a host clock around --iters back-to-back calls that ends in a device synchronise, after untimed calls of
the same shape; hip and stock alternate --rounds times, every round is printed, the median is reported.  Each batch size
is a run of its own under its own time limit, chained with && (a leg that fails or hangs ends the chain).
--launches counts the device kernels per call and sums their device time with torch.profiler, in a run of its own (tracing
slows the host: no wall time is taken from it)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ilps_amd  # noqa: E402,F401
from _timing import profile_calls, rounds  # noqa: E402

KERNELS = ("measure_fwd_kernel", "measure_bwd_kernel")


def problem(B, K, seed=0):
    """B posed spheres at SMPL's counts (cycled from 8 seeded ones with a per-mesh scale), the topology with its own face
    parts, K planes near the middle."""
    from _render_oracle import posed_sphere
    from ilps_amd.measure import MeasureSpec
    from ilps_amd.render import MeshTopology
    base, f = posed_sphere(seed, 8)
    rng = np.random.default_rng(seed + 1)
    verts = base[np.arange(B) % 8] * rng.uniform(0.9, 1.1, (B, 1, 1)).astype(np.float32)
    planes = np.concatenate([rng.normal(size=(K, 3)), rng.uniform(-0.1, 0.1, (K, 1))], 1).astype(np.float32)
    topo = MeshTopology(f, verts.shape[1])
    return torch.from_numpy(verts).cuda(), MeasureSpec(topo, planes=planes)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--planes", type=int, default=3)
    ap.add_argument("--iters", type=int, default=0, help="calls per timed window (default: 200 at B <= 256, else 20)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--stock-chunk", type=int, default=256)
    ap.add_argument("--launches", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("measure_time.py needs a HIP device: a CPU run gives no timing")
    from ilps_amd import _lib
    from ilps_amd.measure import measures_torch, mesh_measures
    B, K = a.batch, a.planes
    iters = a.iters or (200 if B <= 256 else 20)
    verts, spec = problem(B, K)
    d = spec.on(verts.device)
    mask64 = torch.from_numpy(spec.part_mask.astype(np.int64)).to(verts.device)
    total = lambda o: o[0].sum() + o[1].sum() + o[2].sum() + o[3].sum()

    def hip(grad):
        v = verts.detach().requires_grad_(grad)
        o = mesh_measures(v, spec)
        if grad:
            total((o["volume"], o["area"], o["extent"], o["girth"])).backward()

    def stock(grad):
        for s in range(0, B, a.stock_chunk):
            v = verts[s:s + a.stock_chunk].detach().requires_grad_(grad)
            pl = d["planes"][None].expand(v.shape[0], K, 4)
            o = measures_torch(v, d["faces"], d["face_part"], pl, mask64)
            if grad:
                total(o).backward()

    legs = {"hip_fwd": lambda: hip(False), "stock_fwd": lambda: stock(False), "hip_fwd_bwd": lambda: hip(True),
            "stock_fwd_bwd": lambda: stock(True)}
    res = {"build_id": _lib.build_id()[:16], "B": B, "V": int(verts.shape[1]), "F": spec.topo.num_faces, "K": K, "iters": iters,
           "stock_chunk": a.stock_chunk}
    for fn in legs.values():
        fn()
        fn()                                                    # untimed: code objects, allocator pools
    if a.launches:
        res["profile"] = {k: profile_calls(fn, 5, KERNELS, "measure_kernels_us") for k, fn in legs.items()}
        print(json.dumps(res))
        return
    with torch.no_grad():
        o = mesh_measures(verts, spec)
        s = measures_torch(verts[:a.stock_chunk], d["faces"], d["face_part"], d["planes"][None].expand(min(B, a.stock_chunk), K, 4), mask64)
    res["max_abs_diff_hip_stock"] = {k: float((o[k][:a.stock_chunk] - s[i]).abs().max()) for i, k in enumerate(("volume", "area", "extent", "girth"))}
    res.update(rounds(legs, {k: iters if k.startswith("hip") else max(2, iters // 10) for k in legs}, a.rounds))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
