"""Timing of the 2D keypoint term (csrc/keypoints.hip through keypoints.keypoint_energy), one GPU, one leg set per run, each
under its own time limit:
    timeout -k 10 300 python tools/keypoint_time.py --batch 128 && timeout -k 10 300 python tools/keypoint_time.py --batch 128 --fit
    timeout -k 10 300 python tools/keypoint_time.py --batch 128 --launches
V = 6 890: the synthetic SMPL model's vertices at seeded poses, its cocoplus spec (19 joints of 8 vertices each), cameras of
the decoder's scale, detections a few pixels from the projected joints, sigma = 3 px.  Per call:
    hip        `keypoint_energy(verts, cam, spec, target, conf, sigma)`: one forward launch; with the backward of sum(e) one
               backward launch more (+ torch's own kernels for the sum and the cotangent)
    stock      `keypoints.keypoint_energy_torch` on device tensors - the package's float64 torch restatement, a dense einsum
               and element-wise launches - and, for the backward, torch.autograd through it
Each figure is a host clock around back-to-back calls that ends in a device synchronise, after untimed calls of the same
shape; the calls per window come from one timed call (about --window seconds per window, 2 to 2000 calls); the legs
alternate --rounds times, every round is printed, the median is reported.
--fit times one iteration of `KeypointFitter.fit(graph=True)`, and of `ParamFitter.fit(graph=True)` with and without the term
on tools/fit_time.py's problem.
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

KERNELS = ("kp_fwd_kernel", "kp_bwd_kernel")


def problem(B, seed=0):
    """-> verts (B, 6890, 3), cam (B, 4), spec, target (B, 19, 2), conf (B, 19) on the device."""
    from _inputs import make_x
    from ilps_amd.keras_smpl.batch_smpl import SMPLLayer
    from ilps_amd.keypoints import KeypointSpec, keypoint_energy
    from ilps_amd.smpl_model import synthetic_smpl_model
    model = synthetic_smpl_model(1234)
    layer = SMPLLayer(model)
    spec = KeypointSpec.from_model(model)
    x = torch.from_numpy(make_x(B, 48, seed=seed)).cuda()
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        verts = layer(x).contiguous()
        cam = x[:, :4].contiguous()
        K = spec.K
        _, det = keypoint_energy(verts, cam, spec, torch.zeros((B, K, 2)).cuda(), torch.ones((B, K)).cuda(), return_details=True)
    target = det["proj"] + (torch.rand((B, K, 2), generator=gen) * 8.0 - 4.0).cuda()
    conf = (torch.rand((B, K), generator=gen) * 0.8 + 0.2).cuda()
    conf[:, 3] = 0.0
    return verts, cam, spec, target.contiguous(), conf


def fit_legs(B, iters, G):
    """us per graph-replayed iteration: KeypointFitter, ParamFitter without the term, ParamFitter with it."""
    from ilps_amd.fitting import KeypointFitter, ParamFitter
    from ilps_amd.keypoints import KeypointSpec
    from ilps_amd.smpl_model import synthetic_smpl_model
    s = importlib.util.spec_from_file_location("fit_time", os.path.join(ROOT, "tools", "fit_time.py"))
    fit_time = importlib.util.module_from_spec(s)
    s.loader.exec_module(fit_time)
    model = synthetic_smpl_model(1234)
    spec = KeypointSpec.from_model(model)
    plain = ParamFitter(model, img_wh=48)
    with_kp = ParamFitter(model, img_wh=48, keypoints=spec, kp_sigma=3.0)
    kfit = KeypointFitter(model, spec, sigma=3.0, img_wh=48)
    labels, x0, xs = fit_time.problem(plain, B, 48)
    K = spec.K
    with torch.no_grad():
        _, det, _ = kfit.terms(xs, torch.zeros((B, K, 2)).cuda(), torch.ones((B, K)).cuda())
    target, conf = det["proj"].clone(), torch.ones((B, K)).cuda()
    n = iters - iters % G
    kw = dict(init=x0, steps=n, graph=True, graph_steps=G)
    return n, {"param_fit": lambda: plain.fit(labels, **kw),
               "param_fit_kp": lambda: with_kp.fit(labels, keypoints=(target, conf), kp_weight=1.0, **kw),
               "keypoint_fit": lambda: kfit.fit(target, conf, **kw)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--window", type=float, default=0.4)
    ap.add_argument("--launches", action="store_true")
    ap.add_argument("--fit", action="store_true")
    ap.add_argument("--fit-iters", type=int, default=400)
    ap.add_argument("--graph-steps", type=int, default=10)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("keypoint_time.py needs a HIP device: a CPU run gives no timing")
    from ilps_amd import _lib
    from ilps_amd.keypoints import keypoint_energy, keypoint_energy_torch
    B = a.batch
    res = {"build_id": _lib.build_id()[:16], "B": B, "V": 6890}
    if a.fit:
        n, legs = fit_legs(B, a.fit_iters, a.graph_steps)
        for fn in legs.values():
            fn()                                                    # untimed: code objects, allocator pools, capture
        res.update(iters=n, graph_steps=a.graph_steps, **rounds(legs, 1, a.rounds, per=n, key="us_per_iteration"))
        print(json.dumps(res))
        return
    verts, cam, spec, target, conf = problem(B)
    res.update(K=spec.K, nnz=spec.nnz, sigma=3.0)

    def hip(grad):
        v, c = verts.detach().requires_grad_(grad), cam.detach().requires_grad_(grad)
        e = keypoint_energy(v, c, spec, target, conf, 3.0)
        if grad:
            e.sum().backward()

    def stock(grad):
        v, c = verts.detach().requires_grad_(grad), cam.detach().requires_grad_(grad)
        e = keypoint_energy_torch(v, c, spec, target, conf, 3.0)["e"]
        if grad:
            e.sum().backward()

    legs = {"hip_fwd": lambda: hip(False), "hip_fwd_bwd": lambda: hip(True), "stock_fwd": lambda: stock(False),
            "stock_fwd_bwd": lambda: stock(True)}
    iters = calls_per_window(legs, a.window, cap=2000)
    res["iters"] = iters
    if a.launches:
        res["profile"] = {k: profile_calls(fn, 3, KERNELS, "kp_kernels_us") for k, fn in legs.items()}
        print(json.dumps(res))
        return
    with torch.no_grad():
        e = keypoint_energy(verts, cam, spec, target, conf, 3.0)
        s = keypoint_energy_torch(verts, cam, spec, target, conf, 3.0)["e"]
    res["max_abs_diff_hip_stock"] = float((e.double() - s).abs().max())
    res.update(rounds(legs, iters, a.rounds))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
