"""Evaluation of the reference (`evaluate.py:59-127`, `evaluate_autoencoder.py:23-117`, `evaluate3d.py:32-65`) without its file, `cv2` and
printing I/O: per-part IoU over classes 1..31 and pixel accuracy of the arg-max part map against ground-truth maps, in the
style of `inference.predict_batch`.  With a decoder built with a fused loss (`SMPLDecoder(..., loss=softmax_focal_loss(..))`)
the counting runs inside the rasteriser's loss epilogue and the (N, W, W, 32) scores are never written; a decoder without
one writes them and the confusion kernel counts them.  `evaluate_3d` adds what `evaluate3d.py` leaves out: the distance between the
predicted and the ground-truth surface and joints in metres, raw and after translation, scale and Procrustes alignment
(eval3d.py, csrc/eval3d.hip), and the pose-parameter MSE in the same pass; `evaluate_measurements` compares what a tape
measure would: volume, surface area, extents and girths of the predicted and the ground-truth body (measure.py,
csrc/measure.hip), which needs ground-truth parameters but no ground-truth vertices; `evaluate_scans` compares with point clouds that have no
correspondences at all (scan.py, csrc/scan.hip)."""
from __future__ import annotations

import numpy as np
import torch

from .eval3d import Eval3D
from .measure import mesh_measures
from .metrics import SegConfusion


@torch.no_grad()
def evaluate_iou_and_acc(smpl_model, decoder, batches, num_classes=32):
    """batches: an iterable of (images (N,3,H,W) or (N,H,W,3), gt_maps (N,W,W) integer part maps laid out as the
    decoder's output) already on the HIP device.  -> dict(ious (num_classes - 1,) float64 = I / U per part,
    mean_iou = their plain mean (NaN when a part occurs in neither map, as np.mean in evaluate.py), accuracy = correct /
    pixels, counts (num_classes + 1, num_classes) int64 on the device, intersections, unions, correct, total = pixels
    counted (evaluate.py's W * W * num_images))."""
    m = None
    was_training = smpl_model.training
    smpl_model.eval()
    try:
        for images, gt in batches:
            if m is None:
                m = SegConfusion(num_classes, images.device)
            decoder(smpl_model(images), gt, confusion=m)
    finally:
        smpl_model.train(was_training)
    if m is None:
        raise ValueError("evaluate_iou_and_acc: no batches")
    return {"ious": m.iou(), "mean_iou": m.mean_iou(), "accuracy": m.pixel_accuracy(), "counts": m.counts,
            "intersections": m.intersections(), "unions": m.unions(), "correct": m.correct(), "total": m.total()}


@torch.no_grad()
def evaluate_pose_param_mse(smpl_model, batches):
    """`evaluate3d.py:32-65`: batches: an iterable of (images, gt_pose (N, 72) axis-angle pose parameters) on the model's
    device.  -> the mean of (gt_pose[:, 3:] - smpl[:, 7:76])^2 over all samples and the 69 parameters without the global
    rotation, as a float (accumulated in float64)."""
    total, count = None, 0
    was_training = smpl_model.training
    smpl_model.eval()
    try:
        for images, gt_pose in batches:
            smpl = smpl_model(images)
            gt = torch.as_tensor(gt_pose, device=smpl.device)
            if gt.dim() != 2 or gt.shape[1] != 72 or gt.shape[0] != smpl.shape[0]:
                raise ValueError("gt_pose must be (N, 72) with N = the batch's images")
            err = (gt[:, 3:].to(torch.float64) - smpl[:, 7:76].to(torch.float64)).square().sum()
            total = err if total is None else total + err
            count += int(smpl.shape[0]) * 69
    finally:
        smpl_model.train(was_training)
    if total is None:
        raise ValueError("evaluate_pose_param_mse: no batches")
    return float(total) / count


@torch.no_grad()
def evaluate_3d(smpl_model, smpl_layer, batches, root_joint=None):
    """The loop of `evaluate3d.py:32-65` with 3D errors in metres.  batches: an iterable of (images, gt) on the model's
    device, gt either (gt_pose (N, 72), gt_shape (N, 10)) - decoded by the same `smpl_layer` as the prediction - or
    ground-truth vertices (N, V, 3).  The predicted vertices are smpl_layer(smpl) with pose = smpl[:, 4:76] and shape =
    smpl[:, 76:86] (the layout `evaluate_pose_param_mse` assumes).
    -> dict(pve, pve_t, pve_sc, pve_pa: mean per-vertex error as given / centroids removed / + least-squares scale /
    Procrustes-aligned; with a joint regressor in the SMPL model also mpjpe, mpjpe_root (relative to joint `root_joint`,
    the joints' centroid when None) and mpjpe_pa over `smpl_layer.joints`; count = meshes counted, nonfinite = meshes left
    out because they held a NaN or Inf; pose_mse = `evaluate_pose_param_mse`'s number when gt carries the pose, else None)."""
    ev_v = ev_j = None
    mse_sum, mse_n = None, 0
    was_training = smpl_model.training
    smpl_model.eval()
    try:
        for images, gt in batches:
            smpl = smpl_model(images)
            dev = smpl.device
            if ev_v is None:
                ev_v = Eval3D(dev)
                has_j = smpl_layer.constants(dev).joint_regressor is not None
                ev_j = Eval3D(dev) if has_j else None
            pred_v = smpl_layer(smpl.float())
            if isinstance(gt, (tuple, list)):
                gt_pose, gt_shape = (torch.as_tensor(t, device=dev) for t in gt)
                if gt_pose.dim() != 2 or gt_pose.shape[1] != 72 or gt_pose.shape[0] != smpl.shape[0]:
                    raise ValueError("gt_pose must be (N, 72) with N = the batch's images")
                if gt_shape.shape != (smpl.shape[0], 10):
                    raise ValueError("gt_shape must be (N, 10) with N = the batch's images")
                x = torch.cat([smpl[:, :smpl_layer.num_cam].float(), gt_pose.float(), gt_shape.float()], 1)
                gt_v = smpl_layer(x)
                err = (gt_pose[:, 3:].to(torch.float64) - smpl[:, 7:76].to(torch.float64)).square().sum()
                mse_sum = err if mse_sum is None else mse_sum + err
                mse_n += int(smpl.shape[0]) * 69
            else:
                gt_v = torch.as_tensor(gt, device=dev).float()
                if gt_v.shape != pred_v.shape:
                    raise ValueError("ground-truth vertices must be %s, got %s" % (tuple(pred_v.shape), tuple(gt_v.shape)))
            ev_v.update(pred_v, gt_v)
            if ev_j is not None:
                pj, gj = smpl_layer.joints(pred_v).contiguous(), smpl_layer.joints(gt_v).contiguous()
                ev_j.update(pj, gj, root=root_joint)          # (the root only changes the translation mode)
    finally:
        smpl_model.train(was_training)
    if ev_v is None:
        raise ValueError("evaluate_3d: no batches")
    v = ev_v.result()
    out = {"pve": v["none"], "pve_t": v["translation"], "pve_sc": v["scale"], "pve_pa": v["similarity"],
           "count": v["count"], "nonfinite": v["nonfinite"],
           "pose_mse": float(mse_sum) / mse_n if mse_n else None}
    if ev_j is not None:
        j = ev_j.result()
        out.update(mpjpe=j["none"], mpjpe_root=j["translation"], mpjpe_pa=j["similarity"], joint_count=j["count"])
    return out


@torch.no_grad()
def evaluate_uncertainty(smpl_model, smpl_layer, batches, samples, generator=None):
    """Does the predicted spread say where the prediction is wrong?  smpl_model: an `SMPLRegressor(probabilistic=True)`;
    batches: an iterable of (images, truth) on the model's device, truth a dict with "verts" (N, V, 3) and "x" (N, 86) as
    `SyntheticBatches(truth=True)` yields it; samples = S >= 2 bodies are drawn per image (sample 0 the mean) from
    `generator`, decoded by `smpl_layer`, and `prob.sample_spread` gives every vertex its rms distance to the sample mean.
    -> dict(rms (V,) float64: the mean rms per vertex over all images; error (V,): the mean actual error per vertex of the
    mean prediction (`eval3d.point_errors(per_point="none")`); correlation: Pearson's r between rms and actual error over
    all (image, vertex) pairs; nll (2,): the mean pose and shape likelihood (`prob.gaussian_nll`); count: images counted)."""
    from .eval3d import point_errors
    from .prob import gaussian_nll, sample_spread
    S = int(samples)
    if S < 2:
        raise ValueError("samples must be at least 2: one body has no spread")
    if not getattr(smpl_model, "probabilistic", False):
        raise ValueError("evaluate_uncertainty needs an SMPLRegressor(probabilistic=True)")
    acc = None
    was_training = smpl_model.training
    smpl_model.eval()
    try:
        for images, truth in batches:
            smpl = smpl_model(images)
            dev, n = smpl.device, int(smpl.shape[0])
            eps = torch.randn((n, S, smpl_model.nout), generator=generator, device=dev)
            verts = smpl_layer(smpl_model.sample(eps, mean_first=True))
            _, rms = sample_spread(verts, S)
            pred = verts.reshape(n, S, -1, 3)[:, 0].contiguous()
            err = point_errors(pred, truth["verts"].float(), per_point="none")["per_point"]
            x_t = truth["x"].float()
            nc = smpl_layer.num_cam
            if smpl_model.pose_repr == "rot6d":
                from .rot6d import axis_angle_to_rot6d
                x_t = torch.cat([x_t[:, :nc], axis_angle_to_rot6d(x_t[:, nc:nc + 72].reshape(n, 24, 3)).reshape(n, 144),
                                 x_t[:, nc + 72:]], 1)
            groups = (-1,) * nc + (0,) * (smpl_model.nout - nc - 10) + (1,) * 10
            nll = gaussian_nll(smpl_model.mean, smpl_model.log_var, x_t, groups)
            r, e = rms.double(), err.double()
            ok = torch.isfinite(r).all(1) & torch.isfinite(e).all(1) & torch.isfinite(nll).all(1)
            r, e = r[ok], e[ok]
            part = [r.sum(0), e.sum(0), r.sum(), e.sum(), (r * r).sum(), (e * e).sum(), (r * e).sum(), nll[ok].double().sum(0),
                    ok.sum().double()]
            acc = part if acc is None else [a + p for a, p in zip(acc, part)]
    finally:
        smpl_model.train(was_training)
    if acc is None:
        raise ValueError("evaluate_uncertainty: no batches")
    count = int(acc[8])
    m = max(count, 1) * acc[0].numel()
    sr, se, srr, see, sre = (float(v) for v in acc[2:7])
    cov, vr, ve = sre / m - sr * se / m ** 2, srr / m - (sr / m) ** 2, see / m - (se / m) ** 2
    return {"rms": (acc[0] / max(count, 1)).cpu().numpy(), "error": (acc[1] / max(count, 1)).cpu().numpy(),
            "correlation": cov / np.sqrt(vr * ve) if vr > 0 and ve > 0 else float("nan"),
            "nll": (acc[7] / max(count, 1)).cpu().numpy(), "count": count}


@torch.no_grad()
def evaluate_measurements(smpl_model, smpl_layer, batches, spec, tpose=True):
    """The loop of `evaluate_3d` with gt = (gt_pose (N, 72), gt_shape (N, 10)), comparing body measurements instead of
    vertices: prediction and ground truth are decoded by the same `smpl_layer` and measured by `mesh_measures(verts, spec)`
    (`spec`: a `measure.MeasureSpec` on the layer's topology, with its planes).  tpose=True sets the pose to zero in both, so
    that fixed planes cut the same places of every body and only shape is compared.
    -> dict of mean absolute errors: volume (m^3), area (m^2), extent (3) and girth (K) (m), + names (the spec's), count =
    bodies counted, nonfinite = bodies left out because either mesh or a plane held a NaN or Inf.  Sums are float64 on the
    device; nothing synchronises before the end."""
    K = spec.num_planes
    state = None                                        # 1 + 1 + 3 + K sums, count, nonfinite
    was_training = smpl_model.training
    smpl_model.eval()
    try:
        for images, gt in batches:
            smpl = smpl_model(images)
            dev = smpl.device
            gt_pose, gt_shape = (torch.as_tensor(t, device=dev) for t in gt)
            n, nc = int(smpl.shape[0]), smpl_layer.num_cam
            if gt_pose.dim() != 2 or gt_pose.shape[1] != 72 or gt_pose.shape[0] != n:
                raise ValueError("gt_pose must be (N, 72) with N = the batch's images")
            if gt_shape.shape != (n, 10):
                raise ValueError("gt_shape must be (N, 10) with N = the batch's images")
            xp = smpl.float().clone()
            xg = torch.cat([smpl[:, :nc].float(), gt_pose.float(), gt_shape.float()], 1)
            if tpose:
                xp[:, nc:nc + 72] = 0
                xg[:, nc:nc + 72] = 0
            mp, mg = mesh_measures(smpl_layer(xp), spec), mesh_measures(smpl_layer(xg), spec)
            ok = (mp["status"] == 0) & (mg["status"] == 0)
            err = torch.cat([(mp[k] - mg[k]).abs().reshape(n, -1) for k in ("volume", "area", "extent", "girth")], 1)
            err = torch.where(ok[:, None], err, torch.zeros_like(err)).to(torch.float64).sum(0)
            n_ok = ok.sum().to(torch.float64)
            row = torch.cat([err, n_ok[None], (n - n_ok)[None]])
            state = row if state is None else state + row
    finally:
        smpl_model.train(was_training)
    if state is None:
        raise ValueError("evaluate_measurements: no batches")
    st = state.cpu()
    cnt = float(st[5 + K])
    mean = [(float(x) / cnt if cnt else float("nan")) for x in st[:5 + K]]
    return {"volume": mean[0], "area": mean[1], "extent": mean[2:5], "girth": mean[5:5 + K], "names": spec.names,
            "count": int(st[5 + K]), "nonfinite": int(st[6 + K])}


@torch.no_grad()
def evaluate_scans(smpl_model, smpl_layer, batches, topo):
    """The loop of `evaluate_3d` against point clouds: batches: an iterable of (images, (points (N, Np, 3), counts (N,) or
    None)) on the model's device, the points in the frame of smpl_layer's vertices (metres); `topo`: the layer's
    `render.MeshTopology`.  Per batch one `scan.surface_distance(smpl_layer(smpl), topo, points, counts)`.
    -> dict(scan_to_mesh = the mean over the used, finite points of their distance to the predicted surface, mesh_to_scan =
    the mean over the vertices of their distance to the nearest used, finite point (both in metres, the square roots of the
    op's d2 and vd2), points = points counted, vertices = vertices counted (those of meshes with a usable point), count =
    meshes counted, nonfinite = meshes left out because they held a NaN or Inf).  Sums are float64 on the device; nothing
    synchronises before the end."""
    from .scan import surface_distance
    state = None
    was_training = smpl_model.training
    smpl_model.eval()
    try:
        for images, gt in batches:
            smpl = smpl_model(images)
            dev = smpl.device
            points, counts = gt if isinstance(gt, (tuple, list)) else (gt, None)
            points = torch.as_tensor(points, device=dev).float()
            n = int(smpl.shape[0])
            if points.dim() != 3 or points.shape[0] != n or points.shape[2] != 3:
                raise ValueError("points must be (N, Np, 3) with N = the batch's images")
            if counts is not None:
                counts = torch.as_tensor(counts).to(dev)
            out = surface_distance(smpl_layer(smpl.float()).contiguous(), topo, points.contiguous(), counts)
            ok = out["status"] == 0
            hit, vhit = (out["face"] >= 0) & ok[:, None], (out["vpoint"] >= 0) & ok[:, None]
            f64 = lambda d, m: torch.where(m, d, torch.zeros_like(d)).to(torch.float64).sqrt().sum()
            n_ok = ok.sum().to(torch.float64)
            row = torch.stack([f64(out["d2"], hit), hit.sum().to(torch.float64), f64(out["vd2"], vhit),
                               vhit.sum().to(torch.float64), n_ok, n - n_ok])
            state = row if state is None else state + row
    finally:
        smpl_model.train(was_training)
    if state is None:
        raise ValueError("evaluate_scans: no batches")
    st = [float(x) for x in state.cpu()]
    nan = float("nan")
    return {"scan_to_mesh": st[0] / st[1] if st[1] else nan, "mesh_to_scan": st[2] / st[3] if st[3] else nan,
            "points": int(st[1]), "vertices": int(st[3]), "count": int(st[4]), "nonfinite": int(st[5])}


def evaluate_penetration(verts, topo, collide=None):
    """Self-penetration of meshes verts (B, V, 3) fp32 (metres), one `penetration.self_penetration` call: topo the meshes'
    `render.MeshTopology`, collide None (the default part-pair table) or a (P, P) table of 0 / 1.
    -> dict(inside (B,) int64 = vertices inside another part per mesh, max_depth (B,) float64 = the largest sqrt(d2) among
    them in metres (0 without one), total_inside, max_depth_overall, meshes_with_penetration, count = meshes counted,
    nonfinite = meshes left out because they held a NaN or Inf (their inside and max_depth are 0)).  The per-mesh tensors
    stay on verts' device; the totals are read back once at the end."""
    from .penetration import self_penetration
    with torch.no_grad():
        _, det = self_penetration(verts, topo, collide, return_details=True)
    ok = det["status"] == 0
    ins = det["inside"] & ok[:, None]
    count = ins.sum(1)
    depth = torch.where(ins, det["d2"].to(torch.float64), torch.zeros((), dtype=torch.float64, device=verts.device)).sqrt()
    depth = depth.amax(1) if depth.shape[1] else depth.sum(1)
    tot = torch.stack([count.sum().to(torch.float64), depth.max() if depth.numel() else depth.sum(),
                       (count > 0).sum().to(torch.float64), ok.sum().to(torch.float64)]).cpu()
    return {"inside": count, "max_depth": depth, "total_inside": int(tot[0]), "max_depth_overall": float(tot[1]),
            "meshes_with_penetration": int(tot[2]), "count": int(tot[3]), "nonfinite": int(verts.shape[0]) - int(tot[3])}


@torch.no_grad()
def evaluate_keypoints(proj_or_details, target, conf, thresholds=(0.05, 0.1, 0.2), scale=None):
    """2D joint errors in pixels from `keypoints.keypoint_energy`'s details (its d2 and status; stock torch, CPU tensors
    too) or from a plain proj (B, K, 2) tensor, against target (B, K, 2) and conf (B, K): a joint counts iff conf > 0 and
    its row is finite.  A row is left out whole when its status is NONFINITE or a counted joint's d2 is NaN / Inf.
    scale (B,) or None (ones): the per-row length that PCK's thresholds multiply (a torso or head size in pixels).
    -> dict(mean_error = the mean of sqrt(d2) over counted joints (NaN without one), per_joint (K,) float64 = that mean per
    joint (NaN where none counts), pck = {t: share of counted joints with sqrt(d2) <= t scale_b}, count = counted joints,
    per_joint_count (K,) int64, rows = rows counted, nonfinite = rows left out)."""
    if isinstance(proj_or_details, dict):
        d2 = proj_or_details["d2"].to(torch.float64)
        status = proj_or_details.get("status")
    else:
        r = proj_or_details.to(torch.float64) - target.to(torch.float64)
        d2, status = (r * r).sum(-1), None
    B, K = int(d2.shape[0]), int(d2.shape[1])
    if tuple(conf.shape) != (B, K):
        raise ValueError("conf must be (%d, %d), got %s" % (B, K, tuple(conf.shape)))
    counted = conf > 0
    bad = (counted & ~torch.isfinite(d2)).any(1)
    if status is not None:
        bad = bad | (status != 0)
    counted = counted & ~bad[:, None]
    zero = torch.zeros((), dtype=torch.float64, device=d2.device)
    dist = torch.where(counted, d2, zero).sqrt()
    s = torch.ones(B, dtype=torch.float64, device=d2.device) if scale is None else torch.as_tensor(scale).to(d2.device, torch.float64)
    if tuple(s.shape) != (B,):
        raise ValueError("scale must be (%d,), got %s" % (B, tuple(s.shape)))
    n_k = counted.sum(0)
    n = int(n_k.sum())
    nan = float("nan")
    pck = {float(t): (float((counted & (dist <= float(t) * s[:, None])).sum()) / n if n else nan) for t in thresholds}
    return {"mean_error": float(dist.sum()) / n if n else nan,
            "per_joint": torch.where(n_k > 0, dist.sum(0) / n_k.clamp(min=1), torch.full_like(zero, nan)),
            "pck": pck, "count": n, "per_joint_count": n_k, "rows": B - int(bad.sum()), "nonfinite": int(bad.sum())}


@torch.no_grad()
def evaluate_surface(details, targets, thresholds=(1.0, 2.0, 5.0)):
    """Residuals of dense surface correspondences, in the targets' unit (pixels with image targets, metres with 3D ones), from
    `surface.surface_energy`'s details (its d2 and status; stock torch, CPU tensors too) and the `SurfaceTargets` they were
    computed against: a correspondence counts iff it counts in the targets and its row is finite.  A row is left out whole
    when its status is NONFINITE or a counted d2 is NaN / Inf.  -> dict(mean_error, median_error = the mean and the median of
    sqrt(d2) over the counted correspondences (NaN without one), within = {t: the share of them with sqrt(d2) <= t}, count =
    counted correspondences, rows = rows counted, nonfinite = rows left out)."""
    d2 = details["d2"].to(torch.float64)
    counted = targets.counted().to(d2.device)
    if tuple(d2.shape) != tuple(counted.shape):
        raise ValueError("d2 is %s, the targets (%d, %d)" % (tuple(d2.shape), targets.B, targets.N))
    bad = (counted & ~torch.isfinite(d2)).any(1)
    if details.get("status") is not None:
        bad = bad | (details["status"] != 0)
    counted = counted & ~bad[:, None]
    dist = d2[counted].sqrt()
    n = int(dist.numel())
    nan = float("nan")
    return {"mean_error": float(dist.mean()) if n else nan, "median_error": float(dist.median()) if n else nan,
            "within": {float(t): (float((dist <= float(t)).sum()) / n if n else nan) for t in thresholds}, "count": n,
            "rows": int(d2.shape[0]) - int(bad.sum()), "nonfinite": int(bad.sum())}


@torch.no_grad()
def evaluate_label_distance(details, targets):
    """How far a mesh lies from its label map, from `labeldist.label_distance`'s details (stock torch, CPU tensors too) and
    the `LabelTargets` they were computed against (B images).  Per direction that the details hold - "m2i" from d2_v over
    the vertices that found a pixel of their class, "i2m" from d2_p over the labelled pixels that found a vertex - a dict of
    mean_px and median_px of sqrt(d2) (NaN without an entry), within_1px = the share with sqrt(d2) <= 1, count = the
    entries; a row whose status is NONFINITE is left out whole.  -> {"m2i": ..., "i2m": ..., "rows": rows counted,
    "nonfinite_rows": rows left out}."""
    status = details["status"]
    B = int(status.shape[0])
    if B != targets.B:
        raise ValueError("the details have %d rows, the targets %d images" % (B, targets.B))
    bad = status != 0
    out = {"rows": B - int(bad.sum()), "nonfinite_rows": int(bad.sum())}
    nan = float("nan")
    for name, key in (("m2i", "d2_v"), ("i2m", "d2_p")):
        d2 = details.get(key)
        if d2 is None:
            continue
        d2 = d2.to(torch.float64).reshape(B, -1)
        dist = d2[torch.isfinite(d2) & ~bad[:, None]].sqrt()
        n = int(dist.numel())
        out[name] = {"mean_px": float(dist.mean()) if n else nan, "median_px": float(np.median(dist.cpu().numpy())) if n else nan,
                     "within_1px": float((dist <= 1.0).sum()) / n if n else nan, "count": n}
    return out


@torch.no_grad()
def evaluate_registration(verts, topo, points, counts, spec, reg_verts=None):
    """How well registered meshes verts (B, V, 3) fp32 (metres) lie on scans points (B, N, 3) with counts (B,) or None, and
    what the surface paid for it: one `scan.surface_distance` call and one `meshreg.mesh_regularisers` call.  topo the
    meshes' `render.MeshTopology`, spec a `meshreg.MeshRegSpec`; reg_verts (B, V, 3) is the mesh the regulariser sees when
    that is not verts (`OffsetFitter` regularises v_template + D, not the posed surface).
    -> dict(scan_to_mesh (B,), mesh_to_scan (B,) float64 = the mean of sqrt(d2) over the row's counted points / of sqrt(vd2)
    over its vertices, in metres (NaN for a row without one or with a status), e_lap (B,), e_edge (B,) fp32, nonfinite =
    rows with a status).  Everything stays on verts' device but `nonfinite`."""
    from .meshreg import mesh_regularisers
    from .scan import surface_distance
    out = surface_distance(verts, topo, points, counts)
    ok = out["status"] == 0
    nan = torch.full((), float("nan"), dtype=torch.float64, device=verts.device)

    def mean_dist(d2, hit):
        hit = hit & ok[:, None]
        n = hit.sum(1)
        s = torch.where(hit, d2.to(torch.float64), torch.zeros((), dtype=torch.float64, device=verts.device)).sqrt().sum(1)
        return torch.where(n > 0, s / n.clamp(min=1), nan)
    terms = mesh_regularisers(verts if reg_verts is None else reg_verts, spec, return_terms=True)
    return {"scan_to_mesh": mean_dist(out["d2"], out["face"] >= 0), "mesh_to_scan": mean_dist(out["vd2"], out["vpoint"] >= 0),
            "e_lap": terms[:, 0], "e_edge": terms[:, 1], "nonfinite": int((~ok).sum())}
