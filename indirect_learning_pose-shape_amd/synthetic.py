"""Synthetic training batches on the device: sampled bodies -> proxy inputs.  Beyond the reference, which needs the UP-S31
files for every driver; after "Synthetic Training for Accurate 3D Human Pose and Shape Estimation" (same author), which
trains the regressor on rendered proxy representations instead of photographs.

    batches = SyntheticBatches(smpl_path, 128, 256, 48, spec=KeypointSpec.from_model(model), corruption={})
    trainer = SegTrainer(smpl_path, in_channels=batches.in_channels)
    fit(trainer, batches, trials, steps_per_trial)                      # no files beyond the SMPL model

One `next(batches)`: `BodySampler` draws pose, shape, heading and camera and decodes the vertices (`SMPLLayer`);
`render.render_mesh` draws the hard part map at the input size and, clean, at the label size; the 2D joints come from a
`keypoints.KeypointSpec`; `corruption_draws` draws part removal, an occluding box, a crop, joint noise, drops and left /
right swaps; `proxy_inputs` (csrc/proxy.hip, one launch) turns part map and joints into the encoder's (B, C, H, W) input.
Everything is drawn with torch from one generator on the device: no host traffic, no host synchronisation per batch.
`SyntheticBatches(seg="edges")` feeds the proxy of the later papers instead: the Canny edge map (`edges.py`) of the same
render's rgb in the place of the part map, then the same heat channels.

The definition of `proxy_inputs` (include/smplraster.h has the same text; tests/_synthetic_oracle.py is its NumPy form).
Per sample b and pixel (x, y), l = part[b, y, x]:
  l' = 0 if l > P, or bit l of remove[b] is set (bit 0 is ignored), or (x, y) lies in a box (x0, y0, x1, y1) of b
  (half-open; x1 <= x0 or y1 <= y0 is empty; coordinates outside the image clip); else l' = l.
  seg "index": one channel float(l') * rescale; "onehot": P + 1 channels (l' == c); "silhouette": one channel l' > 0;
  "none": no seg channel (needs joints).
  heat channel j, fp32 in this order, no FMA: dx = float(x) - jx, dy = float(y) - jy, d2 = dx*dx + dy*dy; the value is
  exp(-(d2 * inv2s2)) if keep[b, j], jx and jy are finite and d2 <= cut2, else 0; inv2s2 = fp32(1 / (2 sigma^2)),
  cut2 = fp32((cut sigma)^2), each formed in double and rounded once.  Integer coordinates are pixel centres.  Boxes and
  remove do not touch heat channels.  Rows are independent.
Device tensors run the kernel; CPU tensors run `proxy_inputs_torch`, the plain-torch restatement, which on device tensors is
the stock composition the kernel is timed against (tools/synthetic_time.py).
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr, stream

SEG_MODES = {"index": 0, "onehot": 1, "silhouette": 2, "none": 3}      # SMPLR_PROXY_SEG_* of include/smplraster.h
MAX_JOINTS, MAX_BOXES, MAX_PARTS, MAX_SIDE = 64, 4, 31, 4096
# `SyntheticBatches(seg="edges")`: the Canny keywords when none are given (the textbook 1 : 2 pair on the blurred L2 gradient: a
# choice, not a measurement of anything), and the keywords of `edge` that go to `render_mesh` instead
EDGE_DEFAULTS = {"low": 100, "high": 200}
EDGE_RENDER_KEYS = ("shading", "albedo", "lights", "background")


def seg_channels(seg, num_parts=31):
    """Seg channels of a mode: 1 ("index", "silhouette"), num_parts + 1 ("onehot"), 0 ("none")."""
    if seg not in SEG_MODES:
        raise ValueError("seg must be one of %s, got %r" % (", ".join(map(repr, SEG_MODES)), seg))
    return {"index": 1, "onehot": int(num_parts) + 1, "silhouette": 1, "none": 0}[seg]


def heat_constants(sigma, cut=6.0):
    """(inv2s2, cut2) = (1 / (2 sigma^2), (cut sigma)^2), formed in double and rounded once to fp32 (returned as the python
    floats of those fp32 numbers)."""
    s, c = float(sigma), float(cut)
    if not (math.isfinite(s) and s > 0 and math.isfinite(c) and c > 0):
        raise ValueError("sigma and cut must be finite and positive, got %r, %r" % (sigma, cut))
    with np.errstate(over="ignore"):
        inv2s2, cut2 = float(np.float32(1.0 / (2.0 * s * s))), float(np.float32((c * s) * (c * s)))
    if not (math.isfinite(inv2s2) and inv2s2 > 0 and math.isfinite(cut2) and cut2 > 0):
        raise ValueError("sigma = %r, cut = %r leave float32's range" % (sigma, cut))
    return inv2s2, cut2


def proxy_inputs_torch(part, joints=None, keep=None, remove=None, boxes=None, *, num_parts=31, seg="index", rescale=None,
                       sigma=4.0, cut=6.0):
    """The module's definition in plain torch, on any device: a dozen element-wise passes and a (B, J, H, W) broadcast.
    The CPU path of `proxy_inputs`, and on the HIP device the baseline it is timed against.  -> (B, C, H, W) fp32."""
    B, H, W = (int(s) for s in part.shape)
    P, cseg = int(num_parts), seg_channels(seg, num_parts)
    J = 0 if joints is None else int(joints.shape[1])
    rescale = 1.0 / P if rescale is None else float(rescale)
    dev = part.device
    lab = part.to(torch.int64)
    bad = lab > P
    if remove is not None:
        bad = bad | (((remove.to(torch.int64)[:, None, None] >> lab.clamp(max=31)) & 1) == 1) & (lab >= 1)
    ys = torch.arange(H, device=dev)[None, :, None]
    xs = torch.arange(W, device=dev)[None, None, :]
    if boxes is not None:
        for i in range(int(boxes.shape[1])):
            x0, y0, x1, y1 = (boxes[:, i, k].to(torch.int64)[:, None, None] for k in range(4))
            bad = bad | ((xs >= x0) & (xs < x1) & (ys >= y0) & (ys < y1))
    lab = torch.where(bad, torch.zeros_like(lab), lab)
    planes = []
    if seg == "index":
        planes.append((lab.to(torch.float32) * rescale)[:, None])
    elif seg == "onehot":
        planes.append((lab[:, None] == torch.arange(P + 1, device=dev)[None, :, None, None]).to(torch.float32))
    elif seg == "silhouette":
        planes.append((lab > 0).to(torch.float32)[:, None])
    if J:
        inv2s2, cut2 = heat_constants(sigma, cut)
        jx, jy = joints[..., 0, None, None].to(torch.float32), joints[..., 1, None, None].to(torch.float32)
        dx, dy = xs[None].to(torch.float32) - jx, ys[None].to(torch.float32) - jy
        d2 = dx * dx + dy * dy
        on = torch.isfinite(jx) & torch.isfinite(jy) & (d2 <= cut2)
        if keep is not None:
            on = on & (keep[..., None, None] != 0)
        planes.append(torch.where(on, torch.exp(-(d2 * inv2s2)), torch.zeros((), dtype=torch.float32, device=dev)))
    if not planes:
        raise ValueError("seg='none' needs joints")
    return torch.cat(planes, 1).contiguous() if len(planes) > 1 else planes[0].contiguous()


def _operand(t, name, shape, dtype, dev):
    if t is None:
        return None
    if not isinstance(t, torch.Tensor) or tuple(t.shape) != shape:
        raise ValueError("%s must be a %s tensor" % (name, shape))
    if t.dtype != dtype:
        raise RuntimeError("%s must be %s (got %s)" % (name, dtype, t.dtype))
    if t.device != dev:
        raise RuntimeError("%s lives on %s, part on %s" % (name, t.device, dev))
    return t.contiguous()


@_lib.on_device
def _launch(part, joints, keep, remove, boxes, out, J, NB, P, mode, rescale, inv2s2, cut2):
    B, H, W = (int(s) for s in part.shape)
    check(_lib.load().smplr_proxy_inputs(ptr(part), ptr(joints) if J else None, ptr(keep) if J else None, ptr(remove),
                                         ptr(boxes) if NB else None, B, H, W, J, NB, P, mode, rescale, inv2s2, cut2,
                                         ptr(out), stream()), "smplr_proxy_inputs")
    return out


def proxy_inputs(part, joints=None, keep=None, remove=None, boxes=None, *, num_parts=31, seg="index", rescale=None,
                 sigma=4.0, cut=6.0, out=None):
    """part (B, H, W) uint8 (`render_mesh(...)["part"]` at the input size), joints (B, J, 2) fp32 (x, y) in input pixels,
    keep (B, J) uint8, remove (B,) int32 bit masks, boxes (B, NB, 4) int32 -> (B, C, H, W) fp32, C = seg channels + J: see
    the module's definition.  rescale defaults to 1 / num_parts (the reference's 1 / (num_classes - 1)).  out: write into
    this contiguous tensor (a view may start at any 4-byte boundary).  On the HIP device one launch of csrc/proxy.hip and
    no host synchronisation; CPU tensors run `proxy_inputs_torch`."""
    if not isinstance(part, torch.Tensor) or part.dim() != 3 or part.dtype != torch.uint8:
        raise ValueError("part must be a (B, H, W) uint8 tensor")
    B, H, W = (int(s) for s in part.shape)
    P, cseg, mode = int(num_parts), seg_channels(seg, num_parts), SEG_MODES[seg]
    if not 1 <= P <= MAX_PARTS:
        raise ValueError("num_parts must lie in 1..%d, got %d" % (MAX_PARTS, P))
    if not (1 <= H <= MAX_SIDE and 1 <= W <= MAX_SIDE):
        raise ValueError("part maps must be 1..%d on a side" % MAX_SIDE)
    dev = part.device
    if joints is not None and (joints.dim() != 3 or joints.shape[2] != 2):
        raise ValueError("joints must be (B, J, 2)")
    J = 0 if joints is None else int(joints.shape[1])
    if J > MAX_JOINTS:
        raise ValueError("at most %d joints, got %d" % (MAX_JOINTS, J))
    if seg == "none" and J == 0:
        raise ValueError("seg='none' needs joints")
    if boxes is not None and (boxes.dim() != 3 or boxes.shape[2] != 4):
        raise ValueError("boxes must be (B, NB, 4)")
    NB = 0 if boxes is None else int(boxes.shape[1])
    if NB > MAX_BOXES:
        raise ValueError("at most %d boxes per sample, got %d" % (MAX_BOXES, NB))
    joints = _operand(joints, "joints", (B, J, 2), torch.float32, dev)
    keep = _operand(keep, "keep", (B, J), torch.uint8, dev)
    remove = _operand(remove, "remove", (B,), torch.int32, dev)
    boxes = _operand(boxes, "boxes", (B, NB, 4), torch.int32, dev)
    rescale = 1.0 / P if rescale is None else float(rescale)
    inv2s2, cut2 = heat_constants(sigma, cut)
    shape = (B, cseg + J, H, W)
    if out is not None:
        if not isinstance(out, torch.Tensor) or out.device != dev:
            raise RuntimeError("out must live on part's device")
        if out.dtype != torch.float32 or tuple(out.shape) != shape or not out.is_contiguous():
            raise ValueError("out must be a contiguous float32 tensor of shape %s" % (shape,))
    if not part.is_cuda:
        res = proxy_inputs_torch(part, joints if J else None, keep if J else None, remove, boxes if NB else None, num_parts=P,
                                 seg=seg, rescale=rescale, sigma=sigma, cut=cut)
        return res if out is None else out.copy_(res)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=dev)
    if B == 0:
        return out
    return _launch(part.contiguous(), joints, keep, remove, boxes, out, J, NB, P, mode, rescale, inv2s2, cut2)


# ---- corruption ------------------------------------------------------------------------------------------------------------
DRAW_KEYS = ("remove", "boxes", "keep", "joint_noise", "swap")


def corruption_draws(B, J, generator=None, *, img_wh, remove_parts=(), remove_prob=0.1, box_prob=0.5, box_frac=(0.1, 0.4),
                     crop_prob=0.1, crop_from=(0.4, 0.7), joint_noise_px=2.0, joint_drop_prob=0.1, swap_prob=0.1,
                     swap_pairs=(), device=None):
    """One set of corruption draws per sample, the counterpart of `augment.random_draws`: dict of device tensors
      remove       (B,) int32    bit p set for each class id p of `remove_parts`, independently with `remove_prob`
      boxes        (B, 2, 4) int32 (x0, y0, x1, y1), half-open: box 0 one occluder with probability `box_prob`, its sides
                   U(box_frac) of the image's, placed uniformly inside it; box 1 a crop with probability `crop_prob`: all
                   rows from y >= U(crop_from) H.  An absent box is (0, 0, 0, 0), which is empty
      keep         (B, J) uint8  0 with probability `joint_drop_prob`
      joint_noise  (B, J, 2) fp32 uniform in +-`joint_noise_px`, to be added to the joints
      swap         (B, len(swap_pairs)) bool: exchange the pair's two joints, each with probability `swap_prob`
    img_wh: W or (W, H) of the proxy input.  The numbers come from `generator` on its device (or `device`) as float64
    `torch.rand` calls in this fixed order, each made whatever the probabilities are: (B, len(remove_parts)) removal,
    (6, B) occluder [present, width, height, x, y] + crop [present], (B,) crop row, (B, J) drops, (B, J, 2) noise,
    (B, len(swap_pairs)) swaps.  No host sync.
    The defaults are choices in the spirit of the paper's augmentations, not measurements of anything."""
    W, H = (int(img_wh[0]), int(img_wh[1])) if isinstance(img_wh, (tuple, list)) else (int(img_wh), int(img_wh))
    B, J = int(B), int(J)
    dev = torch.device(device) if device is not None else (generator.device if generator is not None else torch.device("cpu"))
    parts = [int(p) for p in remove_parts]
    if any(not 1 <= p <= MAX_PARTS for p in parts):
        raise ValueError("remove_parts are class ids in 1..%d" % MAX_PARTS)
    pairs = [(int(a), int(b)) for a, b in swap_pairs]
    if any(not (0 <= a < J and 0 <= b < J) for a, b in pairs):
        raise ValueError("swap_pairs index joints in [0, %d)" % J)
    rand = lambda *shape: torch.rand(shape, dtype=torch.float64, device=dev, generator=generator)
    u_rem, u_box, u_crop, u_keep, u_noise, u_swap = rand(B, len(parts)), rand(6, B), rand(B), rand(B, J), rand(B, J, 2), \
        rand(B, len(pairs))
    bits = torch.tensor([1 << p for p in parts], dtype=torch.int64, device=dev)
    mask = ((u_rem < float(remove_prob)).to(torch.int64) * bits).sum(1)
    remove = torch.where(mask >= (1 << 31), mask - (1 << 32), mask).to(torch.int32)
    lo, hi = float(box_frac[0]), float(box_frac[1])
    bw, bh = (lo + u_box[1] * (hi - lo)) * W, (lo + u_box[2] * (hi - lo)) * H
    x0, y0 = u_box[3] * (W - bw).clamp(min=0), u_box[4] * (H - bh).clamp(min=0)
    box = torch.stack([x0.floor(), y0.floor(), (x0 + bw).ceil(), (y0 + bh).ceil()], -1)
    box = torch.where((u_box[0] < float(box_prob))[:, None], box, torch.zeros_like(box))
    clo, chi = float(crop_from[0]), float(crop_from[1])
    cy = ((clo + u_crop * (chi - clo)) * H).floor()
    crop = torch.stack([torch.zeros_like(cy), cy, torch.full_like(cy, W), torch.full_like(cy, H)], -1)
    crop = torch.where((u_box[5] < float(crop_prob))[:, None], crop, torch.zeros_like(crop))
    return {"remove": remove, "boxes": torch.stack([box, crop], 1).to(torch.int32),
            "keep": (u_keep >= float(joint_drop_prob)).to(torch.uint8),
            "joint_noise": ((2.0 * u_noise - 1.0) * float(joint_noise_px)).to(torch.float32),
            "swap": u_swap < float(swap_prob)}


def corrupt_joints(joints, draws, swap_pairs=()):
    """joints (B, J, 2) + draws["joint_noise"], then the joints of each pair (i, j) of `swap_pairs` exchanged where
    draws["swap"] says so.  Plain torch, no host sync; the kernel sees only the result."""
    out = joints + draws["joint_noise"].to(joints.dtype)
    pairs = [(int(a), int(b)) for a, b in swap_pairs]
    if not pairs:
        return out
    B, J = int(joints.shape[0]), int(joints.shape[1])
    idx = torch.arange(J, device=joints.device).expand(B, J).clone()
    for k, (i, j) in enumerate(pairs):
        s = draws["swap"][:, k]
        a, b = idx[:, i].clone(), idx[:, j].clone()
        idx[:, i], idx[:, j] = torch.where(s, b, a), torch.where(s, a, b)
    return out.gather(1, idx[..., None].expand(B, J, 2)).contiguous()


# ---- sampling --------------------------------------------------------------------------------------------------------------
def frame_cameras(verts, img_wh, fill, shift=None):
    """verts (B, V, 3) -> (B, 4) cameras (k_u, k_v, u0, v0) in `img_wh` units for u = u0 + k_u x, v = v0 + k_v y:
    k_u = k_v = fill W / max(x-extent, y-extent) of each mesh, and the bounding box's centre lands at W / 2 + shift W.
    fill: a number or (B,); shift: None, a number, (B,) or (B, 2) per axis.  No host sync."""
    W = float(img_wh)
    B = int(verts.shape[0])
    xy = verts[..., :2].to(torch.float64)
    lo, hi = xy.amin(1), xy.amax(1)                                         # (B, 2)
    fill = torch.as_tensor(fill, dtype=torch.float64, device=verts.device).expand(B)
    k = fill * W / (hi - lo).amax(1)
    sh = torch.zeros((B, 2), dtype=torch.float64, device=verts.device) if shift is None else \
        torch.as_tensor(shift, dtype=torch.float64, device=verts.device)
    if sh.dim() < 2:
        sh = sh.reshape(-1, 1).expand(B, 2)
    c0 = (W / 2.0 + sh * W) - k[:, None] * ((lo + hi) / 2.0)
    return torch.stack([k, k, c0[:, 0], c0[:, 1]], 1).to(torch.float32)


def _quat(aa):
    th = aa.norm(dim=-1, keepdim=True)
    half = th / 2.0
    # sin(th / 2) / th, with its limit 1 / 2 at 0
    k = torch.where(th > 1e-12, torch.sin(half) / th.clamp(min=1e-300), 0.5 - th * th / 48.0)
    return torch.cat([torch.cos(half), aa * k], -1)


def compose_axis_angle(a, b):
    """Axis-angle (.., 3) of R(a) R(b): the rotation b followed by a applied on its left.  Float64 torch through unit
    quaternions; the result's angle lies in [0, pi]."""
    qa, qb = _quat(a.to(torch.float64)), _quat(b.to(torch.float64))
    wa, va, wb, vb = qa[..., :1], qa[..., 1:], qb[..., :1], qb[..., 1:]
    w = wa * wb - (va * vb).sum(-1, keepdim=True)
    v = wa * vb + wb * va + torch.cross(va, vb, dim=-1)
    sgn = torch.where(w < 0, -torch.ones_like(w), torch.ones_like(w))
    w, v = w * sgn, v * sgn
    n = v.norm(dim=-1, keepdim=True)
    ang = 2.0 * torch.atan2(n, w)
    return torch.where(n > 1e-12, v * (ang / n.clamp(min=1e-300)), 2.0 * v)


class BodySampler:
    """Draws bodies: `sample(B, img_wh, generator)` -> dict(x (B, 86) fp32 = [camera | theta | beta], verts (B, V, 3),
    J_transformed (B, 24, 3) when the layer keeps it), on the generator's device, no host sync.

    poses None: theta[3:72] = the package's mean pose (`smpl_model.mean86`) + N(0, pose_std^2); poses (N, 69): a pool row
    drawn with replacement + N(0, pose_jitter^2).  beta = the mean shape + N(0, shape_std^2).  The global rotation is the
    mean's with a rotation by U(-yaw, yaw) about the image's vertical (y) axis applied on its left, composed in float64
    (`compose_axis_angle`).  The camera is `frame_cameras` of the decoded vertices with fill ~ U(fill) and a shift
    ~ U(-shift, shift) per axis.  `smpl_layer`: an `SMPLLayer`, or any callable x (B, 86) -> verts (B, V, 3).
    Draw order (float64, each made whatever the settings are): (B,) pool rows [only with poses], (B, 69) pose noise,
    (B, 10) shape noise, (4, B) uniform [yaw, fill, shift u, shift v].
    A `fitting.PosePrior` stores precision factors and is not a sampler."""

    def __init__(self, smpl_layer, poses=None, pose_std=0.2, pose_jitter=0.0, shape_std=1.0, yaw=math.pi, fill=(0.6, 0.9),
                 shift=0.05):
        self.smpl_layer = smpl_layer
        if poses is not None:
            poses = torch.as_tensor(poses)
            if poses.dim() != 2 or poses.shape[1] != 69 or poses.shape[0] < 1:
                raise ValueError("poses must be an (N, 69) pool")
        self.poses = poses
        self.pose_std, self.pose_jitter, self.shape_std = float(pose_std), float(pose_jitter), float(shape_std)
        self.yaw, self.shift = float(yaw), float(shift)
        self.fill = (float(fill[0]), float(fill[1])) if isinstance(fill, (tuple, list)) else (float(fill), float(fill))
        self._mean = {}

    def _mean_on(self, dev):
        m = self._mean.get(dev)
        if m is None:
            from .smpl_model import mean86
            m86 = torch.from_numpy(mean86(1.0)).to(dev)
            m = self._mean[dev] = (m86[4:76].clone(), m86[76:].clone(),
                                   None if self.poses is None else self.poses.to(dev, torch.float64))
        return m

    def sample(self, B, img_wh, generator=None, device=None):
        B = int(B)
        dev = torch.device(device) if device is not None else (generator.device if generator is not None
                                                              else torch.device("cpu"))
        pose_mean, shape_mean, pool = self._mean_on(dev)
        f64 = dict(dtype=torch.float64, device=dev)
        if pool is None:
            body = pose_mean[3:] + torch.randn((B, 69), generator=generator, **f64) * self.pose_std
        else:
            rows = (torch.rand((B,), generator=generator, **f64) * pool.shape[0]).long().clamp(max=pool.shape[0] - 1)
            body = pool[rows] + torch.randn((B, 69), generator=generator, **f64) * self.pose_jitter
        beta = shape_mean + torch.randn((B, 10), generator=generator, **f64) * self.shape_std
        u = torch.rand((4, B), generator=generator, **f64)
        yaw = torch.zeros((B, 3), **f64)
        yaw[:, 1] = (2.0 * u[0] - 1.0) * self.yaw
        root = compose_axis_angle(yaw, pose_mean[:3].expand(B, 3))
        x = torch.cat([torch.zeros((B, 4), **f64), root, body, beta], 1).to(torch.float32)
        with torch.no_grad():
            verts = self.smpl_layer(x)
        fill = self.fill[0] + u[1] * (self.fill[1] - self.fill[0])
        shift = (2.0 * u[2:4].t() - 1.0) * self.shift
        x[:, :4] = frame_cameras(verts, img_wh, fill, shift)
        out = {"x": x, "verts": verts}
        jt = getattr(self.smpl_layer, "J_transformed", None)
        if jt is not None:
            out["J_transformed"] = jt.detach()
        return out


def hull_topology(model):
    """A stand-in surface for a model that carries no faces (`synthetic_smpl_model`): the convex hull of each body part's
    template vertices, wound outward, as a `render.MeshTopology` with the model's part tables.  Needs scipy."""
    from scipy.spatial import ConvexHull
    from .render import MeshTopology
    from .smpl_model import load_part_tables
    V = int(model.num_verts)
    if V != 6890:
        raise ValueError("the part tables are SMPL's: 6890 vertices")
    ids, off = load_part_tables(1)
    vt = np.asarray(model.v_template, np.float64)
    faces = []
    for p in range(len(off) - 1):
        pid = np.asarray(ids[off[p]:off[p + 1]], np.int64)
        if len(pid) < 4:
            continue
        h = ConvexHull(vt[pid])
        f = pid[h.simplices]
        n = np.cross(vt[f[:, 1]] - vt[f[:, 0]], vt[f[:, 2]] - vt[f[:, 0]])
        flip = (n * h.equations[:, :3]).sum(1) < 0
        f[flip] = f[flip][:, ::-1]
        faces.append(f)
    return MeshTopology(np.concatenate(faces).astype(np.int32), V, part_tables=(ids, off))


class SyntheticBatches:
    """An endless iterator of (images, labels) or, with silh_wh, (images, labels, silh_labels) for `training.fit(trainer,
    batches, ...)` and `SegTrainer.step`: images (B, C, input_wh, input_wh) fp32 proxy inputs, labels (B, output_wh,
    output_wh) int32 the CLEAN part map in the decoder's layout, silh_labels = labels > 0 rendered at silh_wh.
    truth=True: (images, labels, silh_labels or None, truth) for `training.SupervisedTrainer.step`, truth = dict(x, verts,
    J_transformed, joints (the clean 2D joints, or None)) - the very tensors the sampler made (`last`'s), not copies; the
    generator's draws are the same either way.

    smpl_path_or_layer: an `SMPLLayer`, or what it is built from (a path, an `SMPLModelData`).  sampler: a `BodySampler`
    (default: `BodySampler(layer)`).  spec: a `keypoints.KeypointSpec` for the heatmaps, None for none.  seg, sigma:
    `proxy_inputs`' (sigma in input pixels), or seg="edges": one channel, the Canny edge map (`edges.canny_edges`) of the
    input-size render's rgb - the same render that gives the part map - with the batch's boxes applied, then the heat channels
    (`proxy_inputs(edges, ..., seg="silhouette", num_parts=1)`); edge: the dict of `canny_edges`' keywords (default
    `EDGE_DEFAULTS`) plus shading / albedo / lights / background for `render_mesh` (default: Lambert on white); part removal
    has no meaning on an edge map, so a non-empty remove_parts with seg="edges" is a ValueError.  corruption: the dict of
    `corruption_draws`' keywords ({}: its defaults), None for clean inputs.  topology: a `render.MeshTopology`; default: the model's faces with its part tables (a model without
    faces, as the synthetic one, needs it: `hull_topology`).  generator: a `torch.Generator` on the device (default: a new
    one on `device` seeded with `seed`).

    One `next()`: the sampler (in output_wh units: `last["x"]` is what the regressor should predict); the part map at
    input_wh with scale = input_wh / output_wh, as `render.render_predictions`; the part map at output_wh (and silh_wh);
    the 2D joints from `spec`'s dense form with the same camera and scale; `corruption_draws`; `proxy_inputs`.
    `last` keeps the batch's x, verts, J_transformed, joints (clean), keep and draws.  No host synchronisation per batch."""

    def __init__(self, smpl_path_or_layer, batch_size, input_wh, output_wh, *, sampler=None, spec=None, seg="index", sigma=4.0,
                 corruption=None, silh_wh=None, seed=1, generator=None, topology=None, device=None, num_parts=31, truth=False,
                 edge=None):
        from .keras_smpl.batch_smpl import SMPLLayer
        from .render import MeshTopology
        # (an SMPLLayer by what it offers, not by isinstance: the package is importable under two names)
        is_layer = callable(smpl_path_or_layer) and hasattr(smpl_path_or_layer, "_model")
        layer = smpl_path_or_layer if is_layer else SMPLLayer(smpl_path_or_layer)
        self.layer = layer
        model = layer._model
        if topology is None:
            if model.faces is None:
                raise ValueError("the SMPL model carries no faces: pass topology= (synthetic.hull_topology(model) for the "
                                 "synthetic model)")
            topology = MeshTopology(model.faces, model.num_verts)
        self.topo = topology
        self.batch_size, self.input_wh, self.output_wh = int(batch_size), int(input_wh), int(output_wh)
        self.silh_wh = None if silh_wh is None else int(silh_wh)
        self.sampler = sampler if sampler is not None else BodySampler(layer)
        self.spec, self.seg, self.sigma, self.num_parts = spec, seg, float(sigma), int(num_parts)
        self.corruption = None if corruption is None else dict(corruption)
        self.edge = self.edge_render = None
        if seg == "edges":
            if self.corruption is not None and len(tuple(self.corruption.get("remove_parts", ()))) > 0:
                raise ValueError("remove_parts has no meaning with seg='edges': an edge map has no parts to remove")
            edge = dict(EDGE_DEFAULTS if edge is None else edge)
            self.edge_render = {k: edge.pop(k) for k in EDGE_RENDER_KEYS if k in edge}
            if "value" in edge or "return_status" in edge or "out" in edge:
                raise ValueError("edge takes canny_edges' keywords except value, return_status and out")
            self.edge = edge
        elif edge is not None:
            raise ValueError("edge= belongs to seg='edges'")
        self.in_channels = (1 if seg == "edges" else seg_channels(seg, num_parts)) + (0 if spec is None else spec.K)
        if self.in_channels == 0:
            raise ValueError("seg='none' needs a spec")
        if generator is None:
            dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
            generator = torch.Generator(device=dev)
            generator.manual_seed(int(seed))
        self.generator = generator
        self.device = generator.device
        self.last = None
        self.truth = bool(truth)

    def __iter__(self):
        return self

    def _joints(self, s):
        """(B, K, 2) fp32 (x, y) in input pixels: p = (u0 + k_u J_x, v0 + k_v J_y), x = s p_u, y = H - 1 - s p_v."""
        d = self.spec.on(s["verts"].device)
        src = s["verts"]
        if self.spec.with_joints:
            src = torch.cat([src, s["J_transformed"]], 1)
        Jn = torch.einsum("ks,bsc->bkc", d["dense"], src.to(torch.float64))
        cam = s["x"][:, :4].to(torch.float64)
        sc = float(self.input_wh) / float(self.output_wh)
        px = sc * (cam[:, 2, None] + cam[:, 0, None] * Jn[..., 0])
        py = (self.input_wh - 1) - sc * (cam[:, 3, None] + cam[:, 1, None] * Jn[..., 1])
        return torch.stack([px, py], -1).to(torch.float32).contiguous()

    def _render(self, s, wh, key="part", **kw):
        from .render import render_mesh
        return render_mesh(s["verts"], self.topo, s["x"][:, :4], mode="ortho", img_wh=wh,
                           scale=float(wh) / float(self.output_wh), **kw)[key]

    def _batch(self, corrupt):
        B = self.batch_size
        s = self.sampler.sample(B, self.output_wh, self.generator)
        if self.seg == "edges":                                           # the one input-size render: its rgb, not its part
            rgb = self._render(s, self.input_wh, "rgb", **self.edge_render)
        else:
            part_in = self._render(s, self.input_wh)
        labels = self._render(s, self.output_wh).to(torch.int32)
        silh = None if self.silh_wh is None else (self._render(s, self.silh_wh) > 0).to(torch.int32)
        joints = keep = None
        K = 0
        if self.spec is not None:
            K = self.spec.K
            joints = self._joints(s)
            keep = torch.ones((B, K), dtype=torch.uint8, device=joints.device)
        last = {"x": s["x"], "verts": s["verts"], "J_transformed": s.get("J_transformed"), "joints": joints, "keep": keep,
                "draws": None}
        remove = boxes = None
        used = joints
        if corrupt and self.corruption is not None:
            draws = corruption_draws(B, K, self.generator, img_wh=self.input_wh, **self.corruption)
            remove, boxes = draws["remove"], draws["boxes"]
            if K:
                used = corrupt_joints(joints, draws, self.corruption.get("swap_pairs", ()))
                keep = draws["keep"]
            last.update(keep=keep, draws=draws)
        if self.seg == "edges":
            from .edges import canny_edges
            images = proxy_inputs(canny_edges(rgb, **self.edge), used, keep, None, boxes, num_parts=1, seg="silhouette",
                                  sigma=self.sigma)
        else:
            images = proxy_inputs(part_in, used, keep, remove, boxes, num_parts=self.num_parts, seg=self.seg, sigma=self.sigma)
        self.last = last
        return images, labels, silh

    def __next__(self):
        images, labels, silh = self._batch(True)
        if self.truth:
            return images, labels, silh, {k: self.last[k] for k in ("x", "verts", "J_transformed", "joints")}
        return (images, labels) if silh is None else (images, labels, silh)

    def truth_batches(self, n):
        """n pairs (images, (pose (B, 72), shape (B, 10))) with uncorrupted inputs, for `evaluate_3d` and (its first
        element) `evaluate_pose_param_mse`."""
        for _ in range(int(n)):
            images, _, _ = self._batch(False)
            x = self.last["x"]
            yield images, (x[:, 4:76].contiguous(), x[:, 76:].contiguous())

    def eval_batches(self, n):
        """n pairs (images, labels) with uncorrupted inputs, for `evaluate_iou_and_acc`."""
        for _ in range(int(n)):
            images, labels, _ = self._batch(False)
            yield images, labels
