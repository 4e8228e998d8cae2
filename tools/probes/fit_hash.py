"""Hashes of whole fits - `FitResult.x`, loss, step, final_x, nonfinite and history - for five seeded fits of 40 iterations,
each run eagerly and again with graph=True, graph_steps=10; run under two trees (two builds of the library, two versions of
fitting.py) to show that a change to the fit step's host side - launcher, bindings, the fitters' loop - leaves every bit.
`ParamFitter` (deterministic backward) at B = 8, W = 48: ungrouped; a seeded prior with two stages of annealed weights;
group_size = 4 with tied shape and `smooth`; with_silhouette.  `ScanFitter` at B = 4 with 512 seeded points per scan, ragged
counts, both directions.  One line per fit and loop, the library's build id first.
GPU only: python tools/probes/fit_hash.py"""
import hashlib
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ilps_amd  # noqa: E402,F401
from ilps_amd import _lib  # noqa: E402
from ilps_amd.fitting import ParamFitter, ScanFitter, column_scale, smooth_weights  # noqa: E402

FIELDS = ("x", "loss", "step", "final_x", "nonfinite", "history")
ITERS, B, W = 40, 8, 48


def digest(result):
    h = hashlib.sha256()
    for name in FIELDS:
        h.update(getattr(result, name).detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def fit_time():
    spec = importlib.util.spec_from_file_location("fit_time", os.path.join(ROOT, "tools", "fit_time.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def scan_case(model, dev):
    """Four scans of 512 points from the surface of seeded bodies placed by (s, t), ragged counts, a perturbed start."""
    from ilps_amd.keras_smpl.batch_smpl import SMPLLayer
    from ilps_amd.render import MeshTopology
    from ilps_amd.scan import sample_surface
    from ilps_amd.smpl_model import load_part_tables, mean86
    ids, _ = load_part_tables(1)
    topo = MeshTopology(np.asarray(ids[:(len(ids) // 3) * 3], np.int32).reshape(-1, 3), 6890)
    fitter = ScanFitter(SMPLLayer(model), topo)
    rng = np.random.default_rng(77)
    x_true = np.tile(mean86(1.0), (4, 1))
    x_true[:, 4:76] += rng.normal(0, 0.15, (4, 72))
    x_true[:, 76:] += rng.normal(0, 0.8, (4, 10))
    x_true[:, 0] = (1.0, 1.1, 0.9, 1.05)
    x_true[:, 1:4] = rng.normal(0, 0.1, (4, 3))
    x_true = torch.from_numpy(x_true.astype(np.float32)).to(dev)
    with torch.no_grad():
        verts = fitter.place(x_true).cpu()
    scans, _, _ = sample_surface(verts, topo, 512, torch.Generator().manual_seed(5))
    x0 = x_true.clone()
    x0[:, 4:76] += torch.from_numpy(rng.normal(0, 0.05, (4, 72)).astype(np.float32)).to(dev)
    x0[:, 1:4] += torch.tensor((0.05, -0.04, 0.03), device=dev)
    counts = torch.tensor([512, 200, 431, 512], dtype=torch.int32, device=dev)
    return fitter, scans.to(dev).contiguous(), counts, x0


def main():
    from ilps_amd.smpl_model import synthetic_smpl_model
    dev = torch.device("cuda", 0)
    ft = fit_time()
    model = synthetic_smpl_model(1234)
    fitter = ParamFitter(model, img_wh=W, deterministic=True)
    labels, x0, _ = ft.problem(fitter, B, W, seed=3)
    stages = [(20, column_scale(cam=20.0, pose=1.0, shape=0.0)), (20, column_scale(cam=5.0, pose=1.0, shape=1.0))]
    cases = [("plain", fitter, (labels,), dict(init=x0, steps=ITERS)),
             ("prior, two stages", fitter, (labels,), dict(init=x0, stages=stages, prior=ft.seeded_prior(8, 4, seed=2),
                                                          prior_weights=[(4e-3, 1.5e-2, 1e-3), (4e-4, 1.5e-3, 5e-4)], patience=15)),
             ("group 4, tie, smooth", fitter, (labels,), dict(init=x0, steps=ITERS, group_size=4, tie=("shape",), mode="torch",
                                                             smooth=smooth_weights(cam=0.01, global_rot=0.1, pose=0.1)))]
    silh = ParamFitter(model, img_wh=W, with_silhouette=True, deterministic=True)
    g = torch.Generator().manual_seed(9)
    silh_labels = torch.randint(0, 2, (B, silh.silh_wh, silh.silh_wh), generator=g, dtype=torch.int32).to(dev)
    cases.append(("silhouette", silh, (labels,), dict(init=x0, steps=ITERS, silh_labels=silh_labels, grad_scale=1.0 / B)))
    scan, points, counts, sx0 = scan_case(model, dev)
    cases.append(("scan, both directions", scan, (points, counts), dict(init=sx0, steps=ITERS, lr=0.01, mode="torch")))
    print("build %s" % _lib.build_id()[:16])
    for name, f, args, kw in cases:
        for loop, gkw in (("eager", {}), ("graph", dict(graph=True, graph_steps=10))):
            r = f.fit(*args, history=True, **kw, **gkw)
            assert r.steps == ITERS and tuple(r.history.shape)[0] == ITERS
            print("%-22s %-5s %s" % (name, loop, digest(r)))


if __name__ == "__main__":
    main()
