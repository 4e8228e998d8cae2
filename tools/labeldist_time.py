"""Timing of the label-map distance term (csrc/labeldist.hip through labeldist.label_distance), one GPU, one leg set per run,
each under its own time limit:
    timeout -k 10 300 python tools/labeldist_time.py --batch 128 && timeout -k 10 300 python tools/labeldist_time.py --batch 128 --fit
    timeout -k 10 300 python tools/labeldist_time.py --batch 128 --launches
    timeout -k 10 300 python tools/labeldist_time.py --batch 8 --wh 160
V = 6 890: the synthetic SMPL model's vertices at seeded poses with the camera a few pixels off, 32 classes from the part
tables, sigma = 8 px, slack 0.5.  At W = 48 the labels are the arg-max of the decoder's scores at the unshifted parameters; at
another W (the 160 leg) the camera is scaled by W / 48 and the label map is painted from the unshifted vertices themselves
(every vertex's class at its pixel, grown by one pixel), since the part rasteriser's fused path stops below that width.
Per call:
    hip        `label_distance(verts, cam, spec, targets, sigma=8)`: one forward launch for both directions; with the backward
               of sum(e) one backward launch and the small dcam reduction more (+ torch's own kernels for the sums);
               hip_fwd_m2i / hip_fwd_i2m: the forward of one direction alone
    stock      `labeldist.label_distance_torch` on device tensors - the package's float64 torch restatement, chunked so that
               no (B, V, W^2) tensor exists - and, for the backward, torch.autograd through it
    prep       `LabelTargets(labels, 32)`: the one launch per label batch, outside the iteration
Each figure is a host clock around back-to-back calls that ends in a device synchronise, after untimed calls of the same
shape; the calls per window come from one timed call (about --window seconds per window, 2 to 2000 calls); the legs
alternate --rounds times, every round is printed, the median is reported.
--fit times one iteration of `ParamFitter.fit(graph=True)` and of `LabelDistanceFitter.fit(graph=True)`, the same loop with the term, on tools/fit_time.py's problem.
--launches counts the device kernels per call and sums their device time with torch.profiler, in a run of its own."""
import argparse
import importlib.util
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ilps_amd  # noqa: E402,F401
from _timing import calls_per_window, profile_calls, rounds  # noqa: E402

KERNELS = ("ld_prep_kernel", "ld_fwd_kernel", "ld_bwd_kernel", "ld_dcam_kernel")


def problem(B, W, seed=0, shift=4.0):
    """-> verts (B, 6890, 3), cam (B, 4), spec, labels (B, W, W) int32 on the device."""
    from _inputs import make_x
    from ilps_amd.decoder import SMPLDecoder
    from ilps_amd.labeldist import LabelDistanceSpec
    from ilps_amd.smpl_model import load_part_tables, synthetic_smpl_model
    model = synthetic_smpl_model(1234)
    spec = LabelDistanceSpec.from_parts(load_part_tables(1), model.num_verts)
    dec = SMPLDecoder(model, img_wh=48)
    x = torch.from_numpy(make_x(B, 48, seed=seed)).cuda()
    with torch.no_grad():
        out = dec(x)
    verts, cam = out["verts"].contiguous(), x[:, :4].clone()
    if W == 48:
        labels = out["seg"].argmax(-1).to(torch.int32)
    else:
        cam = cam * (W / 48.0)
        u = (cam[:, 2, None] + cam[:, 0, None] * verts[..., 0]).round().long()
        v = (cam[:, 3, None] + cam[:, 1, None] * verts[..., 1]).round().long()
        cls = spec.on(verts.device)["vclass"].long()[None].expand(B, -1)
        ok = (u >= 0) & (u < W) & (v >= 0) & (v < W) & (cls > 0)
        flat = torch.zeros((B, W * W), dtype=torch.long, device=verts.device)
        stored = (W - 1 - v) * W + u                                 # (row r of the stored map is v = W - 1 - r)
        flat.scatter_(1, torch.where(ok, stored, torch.zeros_like(stored)), torch.where(ok, cls, flat[:, :1].expand(-1, cls.shape[1])))
        labels = torch.nn.functional.max_pool2d(flat.reshape(B, 1, W, W).float(), 3, 1, 1).reshape(B, W, W).to(torch.int32)
    cam[:, 2:] += shift
    return verts, cam.contiguous(), spec, labels.contiguous()


def fit_legs(B, iters, G):
    """us per graph-replayed iteration of ParamFitter without the term and with it (both directions, sigma = 8 px)."""
    from ilps_amd.fitting import LabelDistanceFitter, ParamFitter
    from ilps_amd.smpl_model import synthetic_smpl_model
    s = importlib.util.spec_from_file_location("fit_time", os.path.join(ROOT, "tools", "fit_time.py"))
    fit_time = importlib.util.module_from_spec(s)
    s.loader.exec_module(fit_time)
    model = synthetic_smpl_model(1234)
    plain = ParamFitter(model, img_wh=48)
    with_ld = LabelDistanceFitter(model, img_wh=48, label_distance=True, ld_sigma=8.0)
    labels, x0, _ = fit_time.problem(plain, B, 48)
    n = iters - iters % G
    kw = dict(init=x0, steps=n, graph=True, graph_steps=G)
    return n, {"param_fit": lambda: plain.fit(labels, **kw), "param_fit_ld": lambda: with_ld.fit(labels, ld_weight=1.0, **kw)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--wh", type=int, default=48)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--window", type=float, default=0.4)
    ap.add_argument("--launches", action="store_true")
    ap.add_argument("--fit", action="store_true")
    ap.add_argument("--fit-iters", type=int, default=400)
    ap.add_argument("--graph-steps", type=int, default=10)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("labeldist_time.py needs a HIP device: a CPU run gives no timing")
    from ilps_amd import _lib
    from ilps_amd.labeldist import LabelTargets, label_distance, label_distance_torch
    B, W = a.batch, a.wh
    res = {"build_id": _lib.build_id()[:16], "B": B, "V": 6890, "W": W}
    if a.fit:
        n, legs = fit_legs(B, a.fit_iters, a.graph_steps)
        for fn in legs.values():
            fn()                                                    # untimed: code objects, allocator pools, capture
        res.update(iters=n, graph_steps=a.graph_steps, **rounds(legs, 1, a.rounds, per=n, key="us_per_iteration"))
        print(json.dumps(res))
        return
    verts, cam, spec, labels = problem(B, W)
    targets = LabelTargets(labels, spec.num_classes)
    off = targets.off[:, 1:].long() - targets.off[:, :-1].long()
    res.update(C=spec.num_classes, sigma=8.0, slack=0.5, labelled_pixels_per_image=round(float(off[:, 1:].sum(1).float().mean()), 1))

    def hip(grad, directions=("m2i", "i2m")):
        v, c = verts.detach().requires_grad_(grad), cam.detach().requires_grad_(grad)
        e = label_distance(v, c, spec, targets, None, 8.0, directions=directions)
        if grad:
            (e[0].sum() + e[1].sum()).backward()

    def stock(grad):
        v, c = verts.detach().requires_grad_(grad), cam.detach().requires_grad_(grad)
        o = label_distance_torch(v, c, spec, targets, None, 8.0)
        if grad:
            (o["e_m2i"].sum() + o["e_i2m"].sum()).backward()

    legs = {"hip_fwd": lambda: hip(False), "hip_fwd_bwd": lambda: hip(True), "stock_fwd": lambda: stock(False),
            "stock_fwd_bwd": lambda: stock(True), "prep": lambda: LabelTargets(labels, spec.num_classes),
            "hip_fwd_m2i": lambda: hip(False, "m2i"), "hip_fwd_i2m": lambda: hip(False, "i2m")}
    iters = calls_per_window(legs, a.window, cap=2000)
    res["iters"] = iters
    if a.launches:
        res["profile"] = {k: profile_calls(fn, 3, KERNELS, "ld_kernels_us") for k, fn in legs.items()}
        print(json.dumps(res))
        return
    with torch.no_grad():
        (e_v, e_p), det = label_distance(verts, cam, spec, targets, None, 8.0, return_details=True)
        s = label_distance_torch(verts, cam, spec, targets, None, 8.0)
    res["max_abs_diff_hip_stock"] = max(float((e_v.double() - s["e_m2i"]).abs().max()), float((e_p.double() - s["e_i2m"]).abs().max()))
    res["winners_equal"] = bool(torch.equal(det["near_pix"], s["near_pix"]) and torch.equal(det["near_vert"], s["near_vert"]))
    res.update(rounds(legs, iters, a.rounds))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
