"""Iterations per second of fitting SMPL parameters to label maps, three loops at the same commit, one GPU:
    python tools/fit_time.py [--batch 128] [--iters 1600] [--rounds 3] [--launches] [--prior K [--angles A]] [--group G [--smooth]] [--loops fitter,graph]
                             [--optimizer lbfgs [--memory M] [--evaluations]]
At B = 128, W = 48 (the reference's decoder_loss_debugging.py runs the loop at W = 48), targets = the arg-max part maps
of seeded parameters, start = those parameters with pose noise and a camera shift:
    stock     the loop a user of the decoder writes with stock torch: the same `SMPLDecoder(loss=...)`, `seg_loss.mean(1)`,
              `torch.optim.Adam([x])`, best-iterate tracking with torch.where (`stock_fit` below)
    fitter    `fitting.ParamFitter.fit`, eager: decoder forward + backward + ONE smplr_fit_step launch per iteration
    graph     `ParamFitter.fit(graph=True, graph_steps=G)`: G iterations per replay of one captured HIP graph
Each figure is a host clock around a whole `fit` / `stock_fit` call of --iters iterations that ends in a device
synchronise (set-up, warm-up and graph capture of that call included: they are part of what a user waits for), taken
after one untimed call per loop; the loops alternate --rounds times, every round is printed, the median is reported.
--prior K adds a seeded K-component pose prior with --angles A angle terms and a shape prior to the fitter's two loops (the
stock loop has none): the same single launch per iteration, smplr_fit_step_prior in place of smplr_fit_step.  --group G fits
the rows in groups of G consecutive rows with the shape tied within a group, --smooth adds the first-difference penalty between a
group's rows (the fitter's two loops; still one launch per iteration, smplr_fit_step_group; the problem's rows stay the seeded,
unrelated ones: the figure is a time, not a fit).  --loops picks
the loops to run.  --launches counts the device kernels per iteration of each loop with torch.profiler in a short run of its own (tracing
slows the host: no timing is taken from it).
--optimizer lbfgs [--memory M] adds the fitter's two loops with mode=Lbfgs(memory=M) - "fitter_lbfgs" and "graph_lbfgs", one
smplr_lbfgs_step launch per evaluation in smplr_fit_step's place - beside Adam's on the same build, and the step kernels' own
device time (the median over a short traced run, and one launch alone between two events on a state in mid-fit) next to the
whole iteration's.  With --evaluations it reports instead, for `KeypointFitter`, `ScanFitter` and `ParamFitter` on seeded
synthetic problems, how many evaluations L-BFGS needs to reach the loss Adam has after its first n = 25, 50, ... --iters
steps: per row the first evaluation whose loss is at or below Adam's best so far; the median over the rows that get there,
and how many do (--batch rows; 16 is plenty)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ilps_amd  # noqa: E402,F401


def stock_fit(decoder, labels, x0, steps, lr=1e-3, eps=1e-8, history=False):
    """The stock loop: torch.optim.Adam on x (B, 86) against the decoder's per-pixel loss, with the best iterate per row.
    -> (best_x, best_loss, final_x, history (steps, B) or None)."""
    x = x0.detach().clone().requires_grad_(True)
    opt = torch.optim.Adam([x], lr=lr, eps=eps)
    B = x.shape[0]
    best_loss = torch.full((B,), float("inf"), device=x.device)
    best_x = x.detach().clone()
    hist = torch.empty((steps, B), device=x.device) if history else None
    for k in range(steps):
        opt.zero_grad(set_to_none=True)
        L = decoder(x, labels)["seg_loss"].mean(1)
        L.sum().backward()
        with torch.no_grad():
            Ld = L.detach()
            if hist is not None:
                hist[k] = Ld
            better = Ld < best_loss
            best_loss = torch.where(better, Ld, best_loss)
            best_x = torch.where(better[:, None], x.detach(), best_x)
        opt.step()
    torch.cuda.synchronize()
    return best_x, best_loss, x.detach(), hist


def problem(fitter, B, W, seed=0, pose_sigma=0.05, cam_shift=1.5):
    """Seeded targets and a perturbed start: labels (B, W, W) int32 = arg-max of the decoder's scores at x*, x0 = x* with
    N(0, pose_sigma) on the pose columns and cam_shift pixels on the camera translation."""
    from _inputs import make_x
    from ilps_amd.decoder import SMPLDecoder
    dev = torch.device("cuda:0")
    xs = torch.from_numpy(make_x(B, W, seed=seed)).to(dev)
    plain = SMPLDecoder(fitter.decoder._model, img_wh=W, outputs=()).share_constants(fitter.decoder)
    with torch.no_grad():
        labels = plain(xs)["seg"].argmax(-1).to(torch.int32)
    rng = np.random.default_rng(seed + 1)
    d = np.zeros((B, 86), np.float32)
    d[:, 2:4] = cam_shift * rng.choice([-1.0, 1.0], (B, 2))
    d[:, 4:76] = rng.normal(0.0, pose_sigma, (B, 72))
    return labels, xs + torch.from_numpy(d).to(dev), xs


def group_problem(fitter, K, G, W, seed=0, turn=0.5, cam_shift=1.0):
    """K bodies seen G times each: xs (K G, 86) = seeded parameters with one beta and one body pose per group and, for view r,
    the global rotation turned by r `turn` radians about the vertical axis and the camera translation moved by r `cam_shift`
    pixels; labels (K G, W, W) int32 = arg-max of the decoder's scores at xs.  A group's rows are consecutive."""
    from _inputs import make_x
    from ilps_amd.decoder import SMPLDecoder
    dev = torch.device("cuda:0")
    x = np.repeat(make_x(K, W, seed=seed), G, axis=0)
    r = np.tile(np.arange(G, dtype=np.float32), K)
    x[:, 5] += turn * r
    x[:, 2] += cam_shift * r
    x[:, 3] -= cam_shift * r
    xs = torch.from_numpy(x.astype(np.float32)).to(dev)
    plain = SMPLDecoder(fitter.decoder._model, img_wh=W, outputs=()).share_constants(fitter.decoder)
    with torch.no_grad():
        labels = plain(xs)["seg"].argmax(-1).to(torch.int32)
    return labels, xs


def seeded_prior(K, A, seed=0):
    """A K-component mixture about the mean pose (means N(0, 0.3^2) away, upper-triangular factors with diagonal U[2, 6]), A
    angle terms on distinct theta indices, a shape prior about N(0, 0.5^2)."""
    from ilps_amd.fitting import PosePrior
    from ilps_amd.smpl_model import load_mean_params
    rng = np.random.default_rng(seed)
    mean = load_mean_params()[0][None, 3:] + rng.normal(0.0, 0.3, (K, 69))
    factor = np.triu(rng.normal(0.0, 0.3, (K, 69, 69)), 1)
    for k in range(K):
        factor[k][np.diag_indices(69)] = rng.uniform(2.0, 6.0, 69)
    return PosePrior(mean=mean, factor=factor, offset=rng.uniform(0.0, 3.0, K), angle_idx=rng.choice(np.arange(3, 72), A, replace=False),
                     angle_scale=rng.uniform(-2.0, 2.0, A), shape_mean=rng.normal(0.0, 0.5, 10))


def keypoint_problem(B, seed=0):
    """`KeypointFitter` on the cocoplus joints: targets = the joints' projections at seeded parameters, start = `problem`'s."""
    from _inputs import make_x
    from ilps_amd.fitting import KeypointFitter
    from ilps_amd.smpl_model import synthetic_smpl_model
    dev = torch.device("cuda:0")
    fitter = KeypointFitter(synthetic_smpl_model(1234), sigma=3.0, img_wh=48)
    xs = torch.from_numpy(make_x(B, 48, seed=seed)).to(dev)
    rng = np.random.default_rng(seed + 1)
    d = np.zeros((B, 86), np.float32)
    d[:, 2:4] = 1.5 * rng.choice([-1.0, 1.0], (B, 2))
    d[:, 4:76] = rng.normal(0.0, 0.05, (B, 72))
    K = fitter.spec.K
    with torch.no_grad():
        _, det, _ = fitter.terms(xs, torch.zeros((B, K, 2), device=dev), torch.ones((B, K), device=dev))
    return fitter, (det["proj"].clone(), torch.ones((B, K), device=dev)), xs + torch.from_numpy(d).to(dev)


def scan_problem(B, N=512, seed=0):
    """`ScanFitter` over an open triangle soup on the synthetic model's vertices (it carries no faces: consecutive vertices of
    the part table, three at a time): points sampled from the body at seeded parameters, start = those with pose noise and a
    shifted placement."""
    from _inputs import make_x
    from ilps_amd.fitting import ScanFitter
    from ilps_amd.render import MeshTopology
    from ilps_amd.scan import sample_surface
    from ilps_amd.smpl_model import load_part_tables, synthetic_smpl_model
    dev = torch.device("cuda:0")
    ids, _ = load_part_tables(1)
    faces = np.asarray(ids[:(len(ids) // 3) * 3], np.int32).reshape(-1, 3)
    fitter = ScanFitter(synthetic_smpl_model(1234), MeshTopology(faces, 6890))
    x = make_x(B, 48, seed=seed)
    x[:, :4] = (1.0, 0.0, 0.0, 0.0)
    xs = torch.from_numpy(x).to(dev)
    with torch.no_grad():
        pts, _, _ = sample_surface(fitter.place(xs).cpu(), fitter.topo, N, torch.Generator().manual_seed(seed + 2))
    rng = np.random.default_rng(seed + 1)
    d = np.zeros((B, 86), np.float32)
    d[:, 1:4] = (0.05, -0.04, 0.03)
    d[:, 4:76] = rng.normal(0.0, 0.05, (B, 72))
    return fitter, (pts.to(dev).contiguous(),), xs + torch.from_numpy(d).to(dev)


def evaluations_to_reach(history, goal):
    """history (n, B) losses of every evaluation, goal (B,) -> per row the 1-based evaluation whose loss is the first at or
    below the goal, 0 where none is."""
    hit = torch.nan_to_num(history, nan=float("inf")) <= goal[None]
    first = torch.where(hit.any(0), hit.float().argmax(0) + 1, torch.zeros_like(goal, dtype=torch.long))
    return first.cpu().tolist()


def evaluations_report(B, iters, memory):
    from ilps_amd.fitting import Lbfgs, ParamFitter
    param = ParamFitter(None, img_wh=48)
    labels, px0, _ = problem(param, B, 48)
    kfit, kdata, kx0 = keypoint_problem(B)
    sfit, sdata, sx0 = scan_problem(B)
    legs = {"KeypointFitter": (lambda **kw: kfit.fit(*kdata, init=kx0, **kw), dict(lr=2e-2)),
            "ScanFitter": (lambda **kw: sfit.fit(*sdata, init=sx0, **kw), dict(lr=1e-2)),
            "ParamFitter": (lambda **kw: param.fit(labels, init=px0, **kw), dict(lr=1e-3))}
    out = {}
    for name, (fit, adam_kw) in legs.items():
        adam = fit(steps=iters, history=True, **adam_kw)
        lb = fit(steps=iters, history=True, mode=Lbfgs(memory=memory))
        table = {}
        n = 25
        while n <= iters:                                           # Adam's best loss after its first n steps, n = 25, 50, ...
            goal = adam.history[:n].min(0).values
            got = sorted(k for k in evaluations_to_reach(lb.history, goal) if k > 0)
            table[n] = {"adam_mean_loss": float("%.4g" % float(goal.mean())), "rows_reaching": len(got),
                        "evaluations_median": statistics.median(got) if got else None, "evaluations_max": got[-1] if got else None}
            n = iters if n < iters < 2 * n else 2 * n
        out[name] = {"adam": dict(adam_kw, steps=iters), "rows": B,
                     "mean_loss": {"start": float("%.4g" % float(adam.history[0].mean())), "adam": float("%.4g" % float(adam.loss.mean())),
                                   "lbfgs": float("%.4g" % float(lb.loss.mean()))},
                     "after_adams_first_n_steps": table, "lbfgs_rows_stopped": int((~lb.active).sum()),
                     "lbfgs_accepted_steps_median": statistics.median(lb.state.t.cpu().tolist())}
    return out


def step_alone_us(B, memory, reps=40):
    """One step launch between two events, on a P = 86 state in mid-fit restored before every launch (L-BFGS: a full memory and
    an accepted trial, so the launch stores a pair and runs the whole recursion): the median over reps, us.  An upper bound
    on the kernel's own time: the events add the launch's gaps."""
    from dataclasses import fields
    from ilps_amd.fitting import FitState, LbfgsState, fit_step, lbfgs_step
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    a = torch.logspace(0, 2, 86, device=dev)
    x = torch.randn((B, 86), device=dev, generator=gen)
    fg = lambda x: ((0.5 * (a * x * x).sum(1))[:, None].contiguous(), (a * x).contiguous())
    lb = LbfgsState.new(x, memory)
    for _ in range(3 * memory):
        loss, grad = fg(lb.x)
        lbfgs_step(lb, grad, loss)
    ad = FitState.new(x)
    out = {}
    for name, st, step in (("lbfgs_step", lb, lbfgs_step), ("fit_step", ad, fit_step)):
        saved = st.clone()
        loss, grad = fg(st.x)
        us = []
        for _ in range(reps):
            for f in fields(st):
                getattr(st, f.name).copy_(getattr(saved, f.name))
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            step(st, grad, loss)
            e1.record()
            torch.cuda.synchronize()
            us.append(e0.elapsed_time(e1) * 1e3)
        out[name] = round(statistics.median(us), 2)
    out["lbfgs_pairs_median"] = statistics.median(lb.pairs.cpu().tolist())
    return out


def step_kernel_us(fn, iters):
    """Median device time (us) of the step kernels in a traced run of fn(iters): {kernel: us}."""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn(iters)
        torch.cuda.synchronize()
    seen = {}
    for e in prof.events():
        for key in ("lbfgs_step_kernel", "fit_step_kernel"):
            if e.device_type == torch.autograd.DeviceType.CUDA and key in e.name:
                seen.setdefault(key, []).append(e.device_time)
    return {k: round(statistics.median(v), 2) for k, v in seen.items()}


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def kernels_per_iteration(fn, iters):
    """Device kernels per iteration of fn(n): traced runs of n = iters, 2 iters and 3 iters; the slope between the first and
    the last (set-up launches cancel), with the raw counts beside it so that a trace that lost records shows."""
    from torch.profiler import ProfilerActivity, profile

    def count(n):
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn(n)
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "memcpy" not in e.name.lower()
                   and "memset" not in e.name.lower())
    counts = [count(k * iters) for k in (1, 2, 3)]
    return {"per_iteration": round((counts[2] - counts[0]) / (2.0 * iters), 2), "iterations": [iters, 2 * iters, 3 * iters],
            "kernels": counts}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--wh", type=int, default=48)
    ap.add_argument("--iters", type=int, default=1600)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--graph-steps", type=int, default=10)
    ap.add_argument("--launches", action="store_true")
    ap.add_argument("--prior", type=int, default=0, help="components of a seeded pose prior for the fitter's loops (0: none)")
    ap.add_argument("--angles", type=int, default=4)
    ap.add_argument("--loops", default="stock,fitter,graph")
    ap.add_argument("--group", type=int, default=1, help="rows per group for the fitter's loops: shape tied within a group (1: none)")
    ap.add_argument("--smooth", action="store_true", help="with --group: a first-difference penalty on camera, global rotation and pose")
    ap.add_argument("--optimizer", default="adam", choices=("adam", "lbfgs"), help="lbfgs: the fitter's loops with mode=Lbfgs too")
    ap.add_argument("--memory", type=int, default=8, help="pairs of L-BFGS memory per row")
    ap.add_argument("--evaluations", action="store_true", help="with --optimizer lbfgs: evaluations to reach Adam's loss, three fitters")
    a = ap.parse_args()
    from ilps_amd import _lib
    from ilps_amd.fitting import ParamFitter
    B, W, G = a.batch, a.wh, a.graph_steps
    fitter = ParamFitter(None, img_wh=W)
    labels, x0, _ = problem(fitter, B, W)
    pkw = dict(prior=seeded_prior(a.prior, a.angles), prior_weights=(1e-3, 1e-3, 1e-3)) if a.prior > 0 else {}
    if a.group > 1 or a.smooth:
        from ilps_amd.fitting import smooth_weights
        pkw.update(group_size=a.group, tie=("shape",))
        if a.smooth:
            pkw.update(smooth=smooth_weights(cam=0.01, global_rot=0.1, pose=0.1))
    loops = {"stock": lambda n: stock_fit(fitter.decoder, labels, x0, n),
             "fitter": lambda n: fitter.fit(labels, init=x0, steps=n, **pkw),
             "graph": lambda n: fitter.fit(labels, init=x0, steps=n, graph=True, graph_steps=G, **pkw)}
    if a.optimizer == "lbfgs":
        from ilps_amd.fitting import Lbfgs
        if a.group > 1 or a.smooth:
            ap.error("--optimizer lbfgs fits every row on its own: no --group, no --smooth")
        if a.evaluations:
            print(json.dumps({"build_id": _lib.build_id()[:16], "B": B, "iters": a.iters, "memory": a.memory,
                              "evaluations_to_adams_loss": evaluations_report(B, a.iters, a.memory)}))
            return
        lb = Lbfgs(memory=a.memory)
        loops["fitter_lbfgs"] = lambda n: fitter.fit(labels, init=x0, steps=n, mode=lb, **pkw)
        loops["graph_lbfgs"] = lambda n: fitter.fit(labels, init=x0, steps=n, graph=True, graph_steps=G, mode=lb, **pkw)
    loops = {k: fn for k, fn in loops.items() if k.split("_")[0] in a.loops.split(",")}
    res = {"build_id": _lib.build_id()[:16], "B": B, "W": W, "iters": a.iters, "graph_steps": G, "prior_K": a.prior,
           "prior_A": a.angles if a.prior > 0 else 0, "group": a.group, "smooth": bool(a.smooth)}
    if a.launches:
        for fn in loops.values():
            fn(2 * G)                                               # untimed and untraced: code objects loaded
        res["kernels"] = {k: kernels_per_iteration(fn, 4 * G) for k, fn in loops.items()}
        print(json.dumps(res))
        return
    n = a.iters - a.iters % G
    for fn in loops.values():
        fn(n)                                                   # untimed: code objects, allocator pools
    us = {k: [] for k in loops}
    for _ in range(a.rounds):
        for k, fn in loops.items():
            us[k].append(wall(lambda: fn(n)) * 1e6 / n)
    res["us_per_iteration_rounds"] = {k: [round(v, 1) for v in vs] for k, vs in us.items()}
    res["us_per_iteration"] = {k: round(statistics.median(vs), 1) for k, vs in us.items()}
    res["iterations_per_s"] = {k: round(1e6 / statistics.median(vs)) for k, vs in us.items()}
    if a.optimizer == "lbfgs":
        res["memory"] = a.memory
        res["step_kernel_us"] = {k: step_kernel_us(fn, 4 * G) for k, fn in loops.items() if k.startswith("fitter")}
        res["step_alone_us"] = step_alone_us(B, a.memory)
    # the three loops on the same problem: mean best loss against the start's (not the same optimiser: stock is torch's Adam)
    if "stock" in loops and "fitter" in loops and not pkw:
        s = stock_fit(fitter.decoder, labels, x0, n)
        f = fitter.fit(labels, init=x0, steps=n)
        res["mean_loss"] = {"start": round(float(fitter.losses(x0, labels).mean()), 6), "stock": round(float(s[1].mean()), 6),
                            "fitter": round(float(f.loss.mean()), 6)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
