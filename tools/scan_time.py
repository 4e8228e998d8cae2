"""Timing of the scan distances (csrc/scan.hip through scan.surface_distance), one GPU, one shape per run:
    timeout -k 10 300 python tools/scan_time.py --batch 1 --points 2048 && timeout -k 10 300 python tools/scan_time.py --batch 1 --points 2048 --morton
    timeout -k 10 300 python tools/scan_time.py --batch 128 --points 16384 --launches
V = 6 890, F = 13 776 (the generated sphere at SMPL's counts, posed), N points per mesh sampled from the mesh's own surface
by `sample_surface` with 5 mm of Gaussian noise - in the sampler's random order, or with --morton sorted per mesh along a
Morton curve (10 bits per axis over the cloud's bounding box): neighbouring lanes then hold neighbouring points, and the
sphere test prunes the same faces for a whole wave.  Per call:
    hip       `surface_distance(verts, topo, points)`: one p2m and one m2p launch; with the backward of sum(d2) + sum(vd2) one
              backward launch more (+ torch's own kernels for the sums and the cotangents)
    stock     `scan.surface_distance_torch` on device tensors - the package's float64 torch restatement, chunked so that no
              (B, N, F) tensor exists - followed by the gradient definition in torch (index_add_).  It evaluates every (point,
              face) pair, so it is timed on --stock-meshes meshes and --stock-points points of the same problem and its
              figure is for THAT sub-problem (the pair count of both is in the output); nothing is extrapolated here.
Each figure is a host clock around back-to-back calls that ends in a device synchronise, after untimed calls of the same
shape; the calls per window come from one timed call (about --window seconds per window, 2 to 200 calls); hip and stock
alternate --rounds times, every round is printed, the median is reported.  Each shape is a run of its own under its own
time limit, chained with && (a leg that fails or hangs ends the chain).
--launches counts the device kernels per call and sums their device time with torch.profiler, in a run of its own."""
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
from _timing import calls_per_window, profile_calls, rounds  # noqa: E402

KERNELS = ("scan_p2m_kernel", "scan_m2p_kernel", "scan_bwd_kernel")


def morton_order(points):
    """points (B, N, 3) -> (B, N) int64 permutation that sorts each mesh's points along a 30-bit Morton curve."""
    lo, hi = points.amin(1, keepdim=True), points.amax(1, keepdim=True)
    q = ((points - lo) / (hi - lo).clamp(min=1e-20) * 1023.0).long().clamp(0, 1023)
    code = torch.zeros(points.shape[:2], dtype=torch.long, device=points.device)
    for bit in range(10):
        for axis in range(3):
            code |= ((q[..., axis] >> bit) & 1) << (3 * bit + axis)
    return code.argsort(1)


def problem(B, N, morton, seed=0):
    from _render_oracle import posed_sphere
    from ilps_amd.render import MeshTopology
    from ilps_amd.scan import sample_surface
    base, f = posed_sphere(seed, 8)
    rng = np.random.default_rng(seed + 1)
    verts = torch.from_numpy(base[np.arange(B) % 8] * rng.uniform(0.9, 1.1, (B, 1, 1)).astype(np.float32)).cuda()
    topo = MeshTopology(f, verts.shape[1])
    g = torch.Generator(device=verts.device).manual_seed(seed + 2)
    pts, _, _ = sample_surface(verts, topo, N, g)
    pts = pts + 0.005 * torch.randn(pts.shape, device=pts.device, generator=g)
    if morton:
        pts = pts.gather(1, morton_order(pts)[..., None].expand(-1, -1, 3))
    return verts, topo, pts.contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--points", type=int, default=2048)
    ap.add_argument("--morton", action="store_true")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--window", type=float, default=0.4)
    ap.add_argument("--stock-meshes", type=int, default=1)
    ap.add_argument("--stock-points", type=int, default=2048)
    ap.add_argument("--no-stock", action="store_true")
    ap.add_argument("--launches", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("scan_time.py needs a HIP device: a CPU run gives no timing")
    from ilps_amd import _lib
    from ilps_amd.scan import _backward_torch, surface_distance, surface_distance_torch
    B, N = a.batch, a.points
    verts, topo, pts = problem(B, N, a.morton)
    faces = topo.on(verts.device)["faces"]
    sb, sn = min(B, a.stock_meshes), min(N, a.stock_points)
    sv, sp = verts[:sb].contiguous(), pts[:sb, :sn].contiguous()

    def hip(grad):
        v = verts.detach().requires_grad_(grad)
        o = surface_distance(v, topo, pts)
        if grad:
            (o["d2"].sum() + o["vd2"].sum()).backward()

    def stock(grad):
        o = surface_distance_torch(sv, faces, sp)
        if grad:
            _backward_torch(sv, faces, sp, o["face"], o["bary"], o["resid"], o["vpoint"], o["status"], torch.ones_like(o["d2"]),
                            torch.ones_like(o["vd2"]), True, False)

    legs = {"hip_fwd": lambda: hip(False), "hip_fwd_bwd": lambda: hip(True)}
    if not a.no_stock:
        legs.update({"stock_fwd": lambda: stock(False), "stock_fwd_bwd": lambda: stock(True)})
    res = {"build_id": _lib.build_id()[:16], "B": B, "V": int(verts.shape[1]), "F": topo.num_faces, "N": N, "morton": a.morton,
           "hip_pairs": B * N * topo.num_faces + B * int(verts.shape[1]) * N,
           "stock_meshes": sb, "stock_points": sn, "stock_pairs": sb * sn * topo.num_faces + sb * int(verts.shape[1]) * sn}
    iters = calls_per_window(legs, a.window)
    res["iters"] = iters
    if a.launches:
        res["profile"] = {k: profile_calls(fn, 3, KERNELS, "scan_kernels_us") for k, fn in legs.items() if k.startswith("hip")}
        print(json.dumps(res))
        return
    if not a.no_stock:
        with torch.no_grad():
            o, s = surface_distance(sv, topo, sp), surface_distance_torch(sv, faces, sp)
        res["max_abs_diff_hip_stock"] = {k: float((o[k] - s[k]).abs().max()) for k in ("d2", "vd2")}
        res["index_agreement"] = {k: float((o[k] == s[k]).float().mean()) for k in ("face", "vpoint")}
    res.update(rounds(legs, iters, a.rounds))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
