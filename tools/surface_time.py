"""Timing of the dense surface-correspondence term (csrc/surface.hip through surface.surface_energy), one GPU, one leg set per
run, each under its own time limit:
    timeout -k 10 300 python tools/surface_time.py --batch 1 --n 16384 && timeout -k 10 300 python tools/surface_time.py --batch 128 --n 4096
    timeout -k 10 300 python tools/surface_time.py --batch 128 --n 4096 --launches
    timeout -k 10 300 python tools/surface_time.py --batch 128 --fit
V = 6 890: the synthetic SMPL model's vertices at seeded poses over a seeded topology of SMPL's 13 776 faces (the synthetic
model carries none), N correspondences per row from `scan.sample_surface`, image targets a few pixels from the projected
points, sigma = 3 px.  Per call:
    hip        `surface_energy(verts, cam, targets, sigma)`: one forward launch; with the backward of sum(e) one backward
               launch more (+ torch's own kernels for the sum and the cotangent)
    stock      `surface.surface_energy_torch` on device tensors - the package's float64 torch restatement, a face gather, a
               (B, N, 3, 3) intermediate and element-wise launches - and, for the backward, torch.autograd through it
Each figure is a host clock around back-to-back calls that ends in a device synchronise, after untimed calls of the same
shape; the calls per window come from one timed call (about --window seconds per window, 2 to 2000 calls); the legs
alternate --rounds times, every round is printed, the median is reported.
--fit times one iteration of `SurfaceFitter.fit(graph=True)`, and of `ParamFitter.fit(graph=True)` with and without the term on
tools/fit_time.py's problem, the correspondences rendered from the true bodies (`correspondences_from_render`).
--launches counts the device kernels per call and sums their device time with torch.profiler, in a run of its own."""
import argparse
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

KERNELS = ("sc_fwd_kernel", "sc_bwd_kernel")


def smpl_sized_topology(seed=77):
    """6 890 vertices, 13 776 seeded faces of distinct, nearby vertices."""
    from ilps_amd.render import MeshTopology
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 6890, 13776)
    f = np.stack([a, (a + rng.integers(1, 40, 13776)) % 6890, (a + rng.integers(40, 80, 13776)) % 6890], 1).astype(np.int32)
    return MeshTopology(f, 6890)


def soup_topology():
    """The open triangle soup of the part tables: consecutive vertices, three at a time."""
    from ilps_amd.render import MeshTopology
    from ilps_amd.smpl_model import load_part_tables
    ids, _ = load_part_tables(1)
    return MeshTopology(np.asarray(ids[:(len(ids) // 3) * 3], np.int32).reshape(-1, 3), 6890)


def problem(B, N, seed=0):
    """-> verts (B, 6890, 3), cam (B, 4), targets (a SurfaceTargets of N image correspondences per row) on the device."""
    from _inputs import make_x
    from ilps_amd.keras_smpl.batch_smpl import SMPLLayer
    from ilps_amd.scan import sample_surface
    from ilps_amd.smpl_model import synthetic_smpl_model
    from ilps_amd.surface import SurfaceTargets
    layer = SMPLLayer(synthetic_smpl_model(1234))
    topo = smpl_sized_topology()
    x = torch.from_numpy(make_x(B, 48, seed=seed)).cuda()
    gen = torch.Generator(device="cuda").manual_seed(seed)
    with torch.no_grad():
        verts = layer(x).contiguous()
        cam = x[:, :4].contiguous()
        pts, face, bary = sample_surface(verts, topo, N, generator=gen)
    proj = torch.stack([cam[:, 2, None] + cam[:, 0, None] * pts[..., 0], cam[:, 3, None] + cam[:, 1, None] * pts[..., 1]], -1)
    target = proj + (torch.rand((B, N, 2), generator=gen, device="cuda") * 8.0 - 4.0)
    conf = torch.rand((B, N), generator=gen, device="cuda") * 0.8 + 0.2
    conf[:, ::9] = 0.0
    return verts, cam, SurfaceTargets(topo, face.to(torch.int32), bary.to(torch.float32), target.contiguous(), conf)


def fit_legs(B, iters, G):
    """us per graph-replayed iteration: SurfaceFitter, ParamFitter without the term, ParamFitter with it."""
    from ilps_amd.fitting import ParamFitter, SurfaceFitter, with_surface
    from ilps_amd.smpl_model import synthetic_smpl_model
    from ilps_amd.surface import SurfaceTargets, correspondences_from_render
    s = importlib.util.spec_from_file_location("fit_time", os.path.join(ROOT, "tools", "fit_time.py"))
    fit_time = importlib.util.module_from_spec(s)
    s.loader.exec_module(fit_time)
    model = synthetic_smpl_model(1234)
    topo = soup_topology()
    plain = ParamFitter(model, img_wh=48)
    with_sc = with_surface(ParamFitter)(model, img_wh=48, surface=topo, sc_sigma=3.0)
    sfit = SurfaceFitter(model, topo=topo, sigma=3.0, img_wh=48)
    labels, x0, xs = fit_time.problem(plain, B, 48)
    with torch.no_grad():
        verts = sfit.layer(xs)
    targets = SurfaceTargets(topo, *correspondences_from_render(verts, topo, xs[:, :4].contiguous(), 48))
    n = iters - iters % G
    kw = dict(init=x0, steps=n, graph=True, graph_steps=G)
    return n, targets.N, {"param_fit": lambda: plain.fit(labels, **kw),
                          "param_fit_sc": lambda: with_sc.fit(labels, surface=targets, sc_weight=1.0, **kw),
                          "surface_fit": lambda: sfit.fit(targets, **kw)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--window", type=float, default=0.4)
    ap.add_argument("--launches", action="store_true")
    ap.add_argument("--fit", action="store_true")
    ap.add_argument("--fit-iters", type=int, default=400)
    ap.add_argument("--graph-steps", type=int, default=10)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("surface_time.py needs a HIP device: a CPU run gives no timing")
    from ilps_amd import _lib
    from ilps_amd.surface import surface_energy, surface_energy_torch
    B = a.batch
    res = {"build_id": _lib.build_id()[:16], "B": B, "V": 6890}
    if a.fit:
        n, N, legs = fit_legs(B, a.fit_iters, a.graph_steps)
        for fn in legs.values():
            fn()                                                    # untimed: code objects, allocator pools, capture
        res.update(iters=n, N=N, graph_steps=a.graph_steps, **rounds(legs, 1, a.rounds, per=n, key="us_per_iteration"))
        print(json.dumps(res))
        return
    verts, cam, targets = problem(B, a.n)
    res.update(N=targets.N, F=targets.topo.num_faces, sigma=3.0)

    def hip(grad):
        v, c = verts.detach().requires_grad_(grad), cam.detach().requires_grad_(grad)
        e = surface_energy(v, c, targets, 3.0)
        if grad:
            e.sum().backward()

    def stock(grad):
        v, c = verts.detach().requires_grad_(grad), cam.detach().requires_grad_(grad)
        e = surface_energy_torch(v, c, targets, 3.0)["e"]
        if grad:
            e.sum().backward()

    legs = {"hip_fwd": lambda: hip(False), "hip_fwd_bwd": lambda: hip(True), "stock_fwd": lambda: stock(False),
            "stock_fwd_bwd": lambda: stock(True)}
    iters = calls_per_window(legs, a.window, cap=2000)
    res["iters"] = iters
    if a.launches:
        res["profile"] = {k: profile_calls(fn, 3, KERNELS, "sc_kernels_us") for k, fn in legs.items()}
        print(json.dumps(res))
        return
    with torch.no_grad():
        e = surface_energy(verts, cam, targets, 3.0)
        s = surface_energy_torch(verts, cam, targets, 3.0)["e"]
    res["max_abs_diff_hip_stock"] = float((e.double() - s).abs().max())
    res.update(rounds(legs, iters, a.rounds))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
