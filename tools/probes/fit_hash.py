"""Hashes of whole fits - `FitResult.x`, loss, step, final_x, nonfinite and history - for seeded fits of 40 iterations, each
run eagerly and again with graph=True, graph_steps=10; run under two trees (two builds of the library, two versions of
fitting.py) to show that a change to the fit step's host side - launcher, bindings, the fitters' loop - leaves every bit.
Only public names are used, so the file runs unchanged on both trees.
`ParamFitter` (deterministic backward) at B = 8, W = 48: ungrouped; a seeded prior with two stages of annealed weights;
group_size = 4 with tied shape and `smooth`; with_silhouette; with the self-penetration term, with the keypoint term and with
both, each over two stages with their own weights.  `ScanFitter` at B = 4 with 512 seeded points per scan, ragged counts: both
directions, both with penetration=True, and p2m alone.  `KeypointFitter` at B = 4, without and with the self-penetration term.
`OffsetFitter` at B = 2 (offsets, x, history, bad and t are hashed; graph=True replays one iteration per launch): x fixed, and
fit_params=True over two stages.  One line per fit and loop, the library's build id first.
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
from ilps_amd.fitting import KeypointFitter, OffsetFitter, ParamFitter, ScanFitter, column_scale, smooth_weights  # noqa: E402

FIELDS = ("x", "loss", "step", "final_x", "nonfinite", "history")
OFFSET_FIELDS = ("offsets", "x", "history", "bad", "t")
ITERS, B, W = 40, 8, 48
LOOPS = (("eager", {}), ("graph", dict(graph=True, graph_steps=10)))
OFFSET_LOOPS = (("eager", {}), ("graph", dict(graph=True)))


def digest(result, names=FIELDS):
    h = hashlib.sha256()
    for name in names:
        h.update(getattr(result, name).detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def fit_time():
    spec = importlib.util.spec_from_file_location("fit_time", os.path.join(ROOT, "tools", "fit_time.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def soup_topology():
    """An open triangle soup over the synthetic model's vertices (it carries no faces): the part tables, three at a time."""
    from ilps_amd.render import MeshTopology
    from ilps_amd.smpl_model import load_part_tables
    ids, _ = load_part_tables(1)
    return MeshTopology(np.asarray(ids[:(len(ids) // 3) * 3], np.int32).reshape(-1, 3), 6890)


def scan_case(model, dev, topo):
    """Four scans of 512 points from the surface of seeded bodies placed by (s, t), ragged counts, a perturbed start."""
    from ilps_amd.keras_smpl.batch_smpl import SMPLLayer
    from ilps_amd.scan import sample_surface
    from ilps_amd.smpl_model import mean86
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


def mixed_spec(model):
    """The 19 cocoplus rows over the vertices, then 5 rows that are posed joints (with_joints)."""
    from ilps_amd.keypoints import KeypointSpec
    R = np.zeros((24, 6890 + 24), np.float32)
    R[:19, :6890] = np.asarray(model.cocoplus_regressor, np.float32)
    for r, j in enumerate((0, 4, 7, 15, 20)):
        R[19 + r, 6890 + j] = 1.0
    return KeypointSpec(R, 6890, with_joints=True)


def detections(fitter, xs, spec):
    """(target, conf) for a ParamFitter built with `spec`: the projections at xs, seeded confidences, one joint uncounted."""
    from ilps_amd.keypoints import keypoint_energy
    n, K, dev = int(xs.shape[0]), spec.K, xs.device
    with torch.no_grad():
        out = fitter.decoder(xs)
        _, det = keypoint_energy(out["verts"], xs[:, :4].contiguous(), spec, torch.zeros((n, K, 2), device=dev),
                                 torch.ones((n, K), device=dev), None, out["J_transformed"], return_details=True)
    conf = torch.linspace(0.3, 1.0, n * K, device=dev).reshape(n, K).clone()
    conf[:, 5] = 0.0
    return det["proj"].clone(), conf


def keypoint_case(model, dev, topo):
    """KeypointFitters without and with the self-penetration term, detections made from perturbed parameters (the last
    row's confidences all zero), and the start."""
    plain, with_pen = KeypointFitter(model, sigma=6.0, img_wh=W), KeypointFitter(model, sigma=6.0, img_wh=W, penetration=topo)
    n, K = 4, plain.spec.K
    rng = np.random.default_rng(12)
    x0 = plain.initial(n, device=dev)
    d = np.zeros((n, 86), np.float32)
    d[:, 2:4] = rng.normal(0, 1.5, (n, 2))
    d[:, 0:2] = rng.normal(0, 0.5, (n, 2))
    d[:, 4:76] = rng.normal(0, 0.15, (n, 72))
    d[:, 76:] = rng.normal(0, 0.7, (n, 10))
    with torch.no_grad():
        _, det, _ = plain.terms(x0 + torch.from_numpy(d).to(dev), torch.zeros((n, K, 2), device=dev), torch.ones((n, K), device=dev))
    conf = torch.from_numpy(rng.uniform(0.3, 1.0, (n, K)).astype(np.float32)).to(dev)
    conf[:, 7] = 0.0
    conf[3] = 0.0
    return plain, with_pen, det["proj"].clone(), conf, x0


def offset_case(dev):
    """An `OffsetFitter` over the closed surface model of tests/_meshreg_oracle at B = 2: posed parameters, a scan of 512
    points from the surface moved by seeded offsets."""
    from _meshreg_oracle import surface_model
    from ilps_amd.keras_smpl.batch_smpl import SMPLLayer
    from ilps_amd.meshreg import MeshRegSpec
    from ilps_amd.render import MeshTopology
    from ilps_amd.scan import sample_surface
    model, _ = surface_model()
    V = model.num_verts
    topo = MeshTopology(model.faces, V)
    sf = ScanFitter(SMPLLayer(model), topo)
    fitter = OffsetFitter(sf, MeshRegSpec(topo, model.v_template, "cotangent"))
    rng = np.random.default_rng(31)
    x = np.zeros((2, 86), np.float32)
    x[:, 0] = 1.0
    x[:, 4:76] = rng.normal(0, 0.03, (2, 72))
    x = torch.from_numpy(x).to(dev)
    D = torch.from_numpy(rng.normal(0, 0.003, (2, V, 3)).astype(np.float32)).to(dev)
    with torch.no_grad():
        verts = sf.place(x, D).cpu()
    pts, _, _ = sample_surface(verts, topo, 512, torch.Generator().manual_seed(9))
    return fitter, pts.to(dev).contiguous(), x


def main():
    from ilps_amd.smpl_model import synthetic_smpl_model
    dev = torch.device("cuda", 0)
    ft = fit_time()
    model = synthetic_smpl_model(1234)
    topo = soup_topology()
    fitter = ParamFitter(model, img_wh=W, deterministic=True)
    labels, x0, xs = ft.problem(fitter, B, W, seed=3)
    stages = [(20, column_scale(cam=20.0, pose=1.0, shape=0.0)), (20, column_scale(cam=5.0, pose=1.0, shape=1.0))]
    # (name, fitter, positional arguments, keyword arguments, hashed fields, loops)
    cases = [("plain", fitter, (labels,), dict(init=x0, steps=ITERS)),
             ("prior, two stages", fitter, (labels,), dict(init=x0, stages=stages, prior=ft.seeded_prior(8, 4, seed=2),
                                                          prior_weights=[(4e-3, 1.5e-2, 1e-3), (4e-4, 1.5e-3, 5e-4)], patience=15)),
             ("group 4, tie, smooth", fitter, (labels,), dict(init=x0, steps=ITERS, group_size=4, tie=("shape",), mode="torch",
                                                             smooth=smooth_weights(cam=0.01, global_rot=0.1, pose=0.1)))]
    silh = ParamFitter(model, img_wh=W, with_silhouette=True, deterministic=True)
    g = torch.Generator().manual_seed(9)
    silh_labels = torch.randint(0, 2, (B, silh.silh_wh, silh.silh_wh), generator=g, dtype=torch.int32).to(dev)
    cases.append(("silhouette", silh, (labels,), dict(init=x0, steps=ITERS, silh_labels=silh_labels, grad_scale=1.0 / B)))
    spec = mixed_spec(model)
    with_pen = ParamFitter(model, img_wh=W, deterministic=True, penetration=topo)
    with_kp = ParamFitter(model, img_wh=W, deterministic=True, keypoints=spec, kp_sigma=3.0)
    with_both = ParamFitter(model, img_wh=W, deterministic=True, penetration=topo, keypoints=spec, kp_sigma=3.0)
    kp = detections(with_kp, xs, spec)
    cases += [("param + pen, 2 stages", with_pen, (labels,), dict(init=x0, stages=stages, pen_weight=[5.0, 30.0])),
              ("param + kp, 2 stages", with_kp, (labels,), dict(init=x0, stages=stages, keypoints=kp, kp_weight=[1.0, 0.25])),
              ("param + pen + kp", with_both, (labels,), dict(init=x0, stages=stages, pen_weight=[0.0, 30.0], keypoints=kp,
                                                            kp_weight=[0.5, 0.1]))]
    kfit, kfit_pen, target, conf, kx0 = keypoint_case(model, dev, topo)
    cases += [("keypoint fitter", kfit, (target, conf), dict(init=kx0, steps=ITERS, lr=0.02)),
              ("keypoint fitter + pen", kfit_pen, (target, conf), dict(init=kx0, stages=stages, lr=0.02, pen_weight=[10.0, 40.0]))]
    scan, points, counts, sx0 = scan_case(model, dev, topo)
    skw = dict(init=sx0, steps=ITERS, lr=0.01, mode="torch")
    cases += [("scan, both directions", scan, (points, counts), skw),
              ("scan + pen", ScanFitter(scan.layer, topo, penetration=True), (points, counts), dict(skw, pen_weight=20.0)),
              ("scan, p2m", ScanFitter(scan.layer, topo, directions="p2m"), (points, counts), skw)]
    reg, opts, ox = offset_case(dev)
    okw = dict(lr=2e-4, lap_weight=0.1, edge_weight=1e-6, offset_weight=1e-3, mode="torch")
    ones = torch.ones(86)
    cases += [("offsets", reg, (opts, None, ox), dict(okw, steps=ITERS), OFFSET_FIELDS, OFFSET_LOOPS),
              ("offsets + x, 2 stages", reg, (opts, None, ox), dict(okw, stages=[(20, ones), (20, 0.5 * ones)], fit_params=True,
                                                                    x_lr=1e-3, lap_weight=[0.1, 0.05]), OFFSET_FIELDS, OFFSET_LOOPS)]
    print("build %s" % _lib.build_id()[:16])
    for name, f, args, kw, *rest in cases:
        names, loops = rest if rest else (FIELDS, LOOPS)
        for loop, gkw in loops:
            r = f.fit(*args, history=True, **kw, **gkw)
            assert r.steps == ITERS and tuple(r.history.shape)[0] == ITERS
            print("%-22s %-5s %s" % (name, loop, digest(r, names)))


if __name__ == "__main__":
    main()
