"""Label-map distances, differentiable: how far a projected mesh is from an integer label map, in both directions and by
class - the silhouette term of "Unite the People", the data term that needs nothing but the labels and still pulls from
far away (the soft rasteriser's exp(-d) scores say nothing beyond a few pixels).  Beyond the reference.

    spec = LabelDistanceSpec.from_parts(load_part_tables(1), 6890)         # class = 1 + part; 32 classes, 0 the background
    targets = LabelTargets(labels, spec.num_classes)                       # (B, W, W) integer map: one prep launch
    e_m2i, e_i2m = label_distance(verts, x[:, :4], spec, targets, sigma=8.0)       # (B, V), (B, W, W) fp32

Definitions.
  Inputs    verts (B, V, 3) fp32; cam (B, 4) = (k_u, k_v, u0, v0); labels (B, W, W) integer, 1 <= W <= 160, in the stored
            frame of the seg head: stored pixel (r, c) sits at the point (c, W - 1 - r) of the projection frame
            (flip_rows=False: at (c, r)); its stored index is r W + c.  C classes, 2 <= C <= 32, class 0 the background; a
            label outside 0 .. C - 1 is "don't care", neither a target nor a query.  vclass (V,) int32, anything outside
            1 .. C - 1: the vertex takes no part.  vweight (B, V) fp32 or None (ones), a constant to autograd.
            A vertex is counted iff its class is in 1 .. C - 1 and vweight > 0 (a NaN does not count).
  Project   in fp64 on the fp32 inputs p_u = u0 + k_u X, p_v = v0 + k_v Y; Z is never read.
  m2i       per counted vertex i of class c, over the stored pixels q of image b labelled c: du = p_u - q_u, dv = p_v - q_v,
            d2 = du du + dv dv, every operation rounded to fp64 as written (no fused multiply-add).  near_pix[i] is the pixel
            of smallest d2, ties to the lower stored index, d2_v[i] that value.  Not counted, or no pixel of class c:
            near_pix = -1, d2_v = +Inf, e = 0, no gradient.
  i2m       per stored pixel q labelled c in 1 .. C - 1, over the counted vertices of class c, the same expression, ties to
            the lower vertex: near_vert, d2_p (B, W, W).  Background, don't care, or no counted vertex of class c: -1, +Inf, 0.
  Energy    s = max(d2 - slack, 0), slack >= 0 in px^2 (0.5: a point inside the union of its class's pixel squares costs
            nothing); rho = `fitting.robust_rho` (sigma=None: rho(s) = s); e_m2i = vweight rho(s), e_i2m = rho(s), each
            rounded to fp32 once.
  Gradient  with cotangents g_v (B, V), g_p (B, W, W), on the projection of vertex i
                dP_i = g_v w rho'(s) [d2 > slack] 2 (p_i - q_near)
                     + sum over the pixels q with near_vert(q) = i of g_p rho'(s_q) [d2_q > slack] 2 (p_i - q)
            the own term first, then the pixels in increasing stored index, in fp64; dverts = (dP_u k_u, dP_v k_v, 0) for every
            vertex (exact zeros where nothing applies); dcam = (sum dP_u X, sum dP_v Y, sum dP_u, sum dP_v) in fp64 in an
            order the launch geometry alone fixes; every output rounded once.  None for labels, vclass, vweight.
  Status    status (B,) int32 = NONFINITE (1) when a cam column of the row is not finite, or X or Y of a counted vertex is:
            the row's float outputs and gradients are NaN, its indices -1, other rows keep the bits they have alone.  A NaN in
            Z, or in a vertex that is not counted, does nothing.
Device tensors run csrc/labeldist.hip: `LabelTargets` one prep launch (a stable counting sort of the pixels by class),
`label_distance` one forward launch for both directions, one backward launch and one small one for dcam; no float atomics,
the same bits in every run and whatever else is in the batch.  CPU tensors run `label_distance_torch`, a float64 torch
restatement; on device tensors that function is the stock composition the kernels are timed against.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr, stream
from ._mesh_common import check_verts, nan_rows
from .keypoints import check_sigma

NONFINITE = 1          # SMPLR_LD_NONFINITE
MAX_CLASSES = 32
MAX_WH = 160
TILE = 256             # LD_T of csrc/labeldist.hip: lanes per workgroup
DIRECTIONS = ("m2i", "i2m")
KEYS = ("near_pix", "near_vert", "d2_v", "d2_p", "proj", "status")
CHUNK_ELEMS = 1 << 22  # entries of the largest (B, chunk, .) block of the torch restatement


class LabelDistanceSpec:
    """The class of every vertex: vclass (V,) integers, num_classes = C in 2 .. 32 (class 0 is the background; a vertex
    whose class lies outside 1 .. C - 1 takes no part).  Built once on the host.  Attributes: vclass (V,) int32,
    num_classes, num_verts; order (the kernels' slots: class-major, every class's run padded with -1 to a multiple of 256,
    then the vertices without a class), vrun (the classed vertices class-major, increasing within a class) and voff (C + 1)
    its runs - all int32 numpy."""

    def __init__(self, vclass, num_classes):
        from .penetration import part_major_order
        C = int(num_classes)
        if C < 2 or C > MAX_CLASSES:
            raise ValueError("2 <= num_classes <= %d, got %r" % (MAX_CLASSES, num_classes))
        if isinstance(vclass, torch.Tensor):
            vclass = vclass.detach().cpu().numpy()
        vc = np.asarray(vclass)
        if vc.ndim != 1 or vc.size < 1 or vc.size > (1 << 24) or not np.issubdtype(vc.dtype, np.integer):
            raise ValueError("vclass must be a (V,) integer array, 1 <= V <= 2^24")
        vc = np.clip(vc.astype(np.int64), -1, C).astype(np.int32)            # (anything outside 1 .. C - 1 takes no part)
        self.vclass, self.num_classes, self.num_verts = vc, C, int(vc.size)
        self.order = part_major_order(vc.astype(np.int64) - 1, C - 1, TILE).astype(np.int32)
        runs = [np.nonzero(vc == c)[0].astype(np.int32) for c in range(1, C)]
        self.vrun = np.concatenate(runs) if runs else np.zeros(0, np.int32)
        self.voff = np.concatenate([[0, 0], np.cumsum([len(r) for r in runs])]).astype(np.int32)
        self._dev = {}

    @classmethod
    def from_parts(cls, part_tables, num_verts):
        """Class = 1 + `render.vertex_parts` of the (ids, offsets) tables of `load_part_tables`: C = 1 + the number of parts
        (32 for the reference's 31), a vertex of no part class 0."""
        from .render import vertex_parts
        return cls(vertex_parts(part_tables, num_verts) + 1, len(part_tables[1]))

    @classmethod
    def silhouette(cls, num_verts):
        """Every vertex class 1, C = 2: the mesh against the foreground of `silhouette_labels`."""
        return cls(np.ones(int(num_verts), np.int32), 2)

    def on(self, device):
        """dict of vclass, order, vrun, voff as int32 tensors on `device`: uploaded once per device, so a later call copies
        nothing and can be captured into a graph."""
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        d = self._dev.get(device)
        if d is None:
            d = {n: torch.from_numpy(getattr(self, n)).to(device) for n in ("vclass", "order", "vrun", "voff")}
            self._dev[device] = d
        return d

    def to(self, device):
        self.on(device)
        return self


def silhouette_labels(labels, num_classes=MAX_CLASSES):
    """A part-label map of `num_classes` classes as a silhouette for C = 2: labels 1 .. num_classes - 1 -> 1, 0 stays, and a
    value out of range - don't care there - is kept: it is >= 2 or negative, so it is don't care here too."""
    return torch.where((labels > 0) & (labels < int(num_classes)), torch.ones_like(labels), labels)


def prep_torch(labels, num_classes):
    """The prep launch in stock torch: labels (B, W, W) integer -> off (B, C + 1), pix (B, W W) int32 - per image the
    stored pixel indices sorted by class, stably; -1 beyond off[C]; don't-care pixels nowhere."""
    B, C = int(labels.shape[0]), int(num_classes)
    lab = labels.reshape(B, -1).long()
    key = torch.where((lab >= 0) & (lab < C), lab, torch.full_like(lab, C))
    skey, order = torch.sort(key, dim=1, stable=True)
    pix = torch.where(skey < C, order, torch.full_like(order, -1)).to(torch.int32)
    counts = (key[:, :, None] == torch.arange(C, device=lab.device)).sum(1)
    off = torch.cat([torch.zeros((B, 1), dtype=torch.long, device=lab.device), counts.cumsum(1)], 1).to(torch.int32)
    return off, pix


class LabelTargets:
    """An integer label map (B, W, W), on whatever device it lives, ready for `label_distance`: labels as int32 plus, per
    image, the stored pixel indices sorted by class - off (B, C + 1), pix (B, W W) - from ONE launch of smplr_ld_prep (CPU
    tensors: `prep_torch`).  Built once per label batch, outside any iteration or captured graph."""

    def __init__(self, labels, num_classes, flip_rows=True):
        C = int(num_classes)
        if C < 2 or C > MAX_CLASSES:
            raise ValueError("2 <= num_classes <= %d, got %r" % (MAX_CLASSES, num_classes))
        if not isinstance(labels, torch.Tensor) or labels.is_floating_point() or labels.is_complex() or labels.dim() != 3 \
                or labels.shape[1] != labels.shape[2]:
            raise ValueError("labels must be a (B, W, W) integer tensor")
        B, W = int(labels.shape[0]), int(labels.shape[1])
        if W < 1 or W > MAX_WH:
            raise ValueError("1 <= W <= %d, got W = %d" % (MAX_WH, W))
        if B > 65535:
            raise ValueError("at most 65535 images, got %d" % B)
        big = torch.iinfo(torch.int32).max
        self.labels = labels.detach().clamp(-1, big).to(torch.int32).contiguous()     # (out of int32: out of range either way)
        self.B, self.W, self.num_classes, self.flip_rows = B, W, C, bool(flip_rows)
        self.off, self.pix = self._prep(self.labels)

    @_lib.on_device
    def _prep(self, labels):
        B, W, C = self.B, self.W, self.num_classes
        if not labels.is_cuda:
            return prep_torch(labels, C)
        off = torch.empty((B, C + 1), dtype=torch.int32, device=labels.device)
        pix = torch.empty((B, W * W), dtype=torch.int32, device=labels.device)
        check(_lib.load().smplr_ld_prep(ptr(labels), B, W, C, ptr(off), ptr(pix), stream()), "smplr_ld_prep")
        return off, pix

    @property
    def device(self):
        return self.labels.device

    def points(self, dtype=torch.float64):
        """(W W, 2): the point (u, v) of every stored pixel, by stored index."""
        W = self.W
        q = torch.arange(W * W, device=self.device)
        r, c = q // W, q % W
        return torch.stack([c, W - 1 - r if self.flip_rows else r], 1).to(dtype)


def check_slack(slack):
    s = float(slack)
    if not (s >= 0 and np.isfinite(np.float32(s))):
        raise ValueError("slack must be finite and >= 0 (px^2), got %r" % (slack,))
    return float(np.float32(s))


def check_directions(directions):
    """("m2i", "i2m"), or one of them (a string or a 1-tuple) -> a tuple in that order."""
    d = (directions,) if isinstance(directions, str) else tuple(directions)
    if not d or len(set(d)) != len(d) or any(x not in DIRECTIONS for x in d):
        raise ValueError("directions must be among %s, got %r" % (DIRECTIONS, directions))
    return tuple(x for x in DIRECTIONS if x in d)


def _rho(s, s2):
    return s if s2 == 0.0 else (s2 * s) / (s2 + s)


def _nearest(d2, ok, n):
    """d2 (B, a, n) float64, ok the candidates -> (min over the last axis, its lowest index or -1)."""
    inf = torch.full((), float("inf"), dtype=d2.dtype, device=d2.device)
    d2 = torch.where(ok, d2, inf)
    m = d2.min(2).values
    ar = torch.arange(n, device=d2.device)
    idx = torch.where(d2 == m[..., None], ar, torch.full_like(ar, n)).min(2).values
    has = (m < inf) & (idx < n)
    return torch.where(has, m, inf), torch.where(has, idx, torch.full_like(idx, -1))


def label_distance_torch(verts, cam, spec, targets, vweight=None, sigma=None, slack=0.5, directions=DIRECTIONS):
    """The definitions in float64 torch on any device (the CPU path, and the stock composition the kernels are timed
    against).  The winners are found without a gradient, in chunks, so that no (B, V, W^2) tensor exists; the energies are
    then formed from the winners alone and are differentiable in verts and cam by autograd (on rows whose status is 0).
    -> dict of e_m2i (B, V), e_i2m (B, W, W), d2_v, d2_p, proj (B, V, 2), all float64, near_pix (B, V), near_vert (B, W, W)
    and status (B,) int32; a direction that was not asked for is absent."""
    dirs = check_directions(directions)
    s2, sl = check_sigma(sigma) ** 2, check_slack(slack)
    f64, dev = torch.float64, verts.device
    B, V, W, C = int(verts.shape[0]), int(verts.shape[1]), targets.W, targets.num_classes
    N = W * W
    vclass = spec.on(dev)["vclass"].long()
    lab = targets.labels.reshape(B, N).long()
    pts = targets.points()
    qu, qv = pts[:, 0], pts[:, 1]
    c = cam.to(f64)
    X, Y = verts[..., 0].to(f64), verts[..., 1].to(f64)
    w = torch.ones((B, V), dtype=f64, device=dev) if vweight is None else vweight.detach().to(f64)
    counted = ((vclass >= 1) & (vclass < C))[None] & (w > 0)
    bad = ~torch.isfinite(c).all(1) | (counted & ~(torch.isfinite(X) & torch.isfinite(Y))).any(1)
    live = counted & ~bad[:, None]
    zero = torch.zeros((), dtype=f64, device=dev)
    inf = torch.full((), float("inf"), dtype=f64, device=dev)
    # (what the energies are made of: a vertex that is not live contributes neither a value nor a NaN to any gradient)
    pu = c[:, 2, None] + c[:, 0, None] * torch.where(live, X, zero)
    pv = c[:, 3, None] + c[:, 1, None] * torch.where(live, Y, zero)
    out = {"proj": nan_rows(bad, torch.stack([c[:, 2, None] + c[:, 0, None] * X, c[:, 3, None] + c[:, 1, None] * Y], -1)).detach(),
           "status": bad.to(torch.int32) * NONFINITE}

    def energy(d2, has, weight):
        s = torch.where(d2 > sl, d2 - sl, zero)
        e = _rho(s, s2) if weight is None else weight * _rho(s, s2)
        return nan_rows(bad, torch.where(has, e, zero))

    with torch.no_grad():
        pud, pvd = pu.detach(), pv.detach()
        if "m2i" in dirs:
            near = torch.empty((B, V), dtype=torch.long, device=dev)
            ch = max(1, CHUNK_ELEMS // max(1, B * N))
            for v0 in range(0, V, ch):
                v1 = min(V, v0 + ch)
                du, dv = pud[:, v0:v1, None] - qu, pvd[:, v0:v1, None] - qv
                ok = live[:, v0:v1, None] & (lab[:, None, :] == vclass[None, v0:v1, None])
                near[:, v0:v1] = _nearest(du * du + dv * dv, ok, N)[1]
        if "i2m" in dirs:
            nearv = torch.empty((B, N), dtype=torch.long, device=dev)
            ch = max(1, CHUNK_ELEMS // max(1, B * V))
            fg = (lab >= 1) & (lab < C)
            for q0 in range(0, N, ch):
                q1 = min(N, q0 + ch)
                du, dv = pud[:, None, :] - qu[q0:q1, None], pvd[:, None, :] - qv[q0:q1, None]          # (B, chunk, V)
                ok = live[:, None, :] & (vclass[None, None, :] == lab[:, q0:q1, None]) & fg[:, q0:q1, None]
                nearv[:, q0:q1] = _nearest(du * du + dv * dv, ok, V)[1]
    if "m2i" in dirs:
        has = near >= 0
        qi = near.clamp(min=0)
        du, dv = pu - qu[qi], pv - qv[qi]
        d2 = du * du + dv * dv
        out["e_m2i"] = energy(d2, has, torch.where(live, w, zero))
        out["d2_v"] = nan_rows(bad, torch.where(has, d2, inf)).detach()
        out["near_pix"] = near.to(torch.int32)
    if "i2m" in dirs:
        has = nearv >= 0
        vi = nearv.clamp(min=0)
        du, dv = torch.gather(pu, 1, vi) - qu, torch.gather(pv, 1, vi) - qv
        d2 = du * du + dv * dv
        out["e_i2m"] = energy(d2, has, None).reshape(B, W, W)
        out["d2_p"] = nan_rows(bad, torch.where(has, d2, inf)).detach().reshape(B, W, W)
        out["near_vert"] = nearv.to(torch.int32).reshape(B, W, W)
    return out


class _LabelDistFn(torch.autograd.Function):
    """verts, cam -> e_m2i, e_i2m, near_pix, near_vert, d2_v, d2_p, proj, status (a direction not asked for: None).  Device
    tensors: smplr_ld_fwd forward, smplr_ld_bwd backward; CPU tensors: the float64 torch path and its autograd."""

    @staticmethod
    def forward(ctx, verts, cam, spec, targets, vweight, sigma, slack, dirs):
        ctx.set_materialize_grads(False)
        dev = verts.device
        B, V, W, C = int(verts.shape[0]), int(verts.shape[1]), targets.W, targets.num_classes
        m2i, i2m = "m2i" in dirs, "i2m" in dirs
        if verts.is_cuda:
            d = spec.on(dev)
            f32, i32 = dict(dtype=torch.float32, device=dev), dict(dtype=torch.int32, device=dev)
            e_v, d2_v, near_pix = (torch.empty((B, V), **f32), torch.empty((B, V), **f32), torch.empty((B, V), **i32)) \
                if m2i else (None,) * 3
            e_p, d2_p, near_vert = (torch.empty((B, W, W), **f32), torch.empty((B, W, W), **f32),
                                    torch.empty((B, W, W), **i32)) if i2m else (None,) * 3
            proj, status = torch.empty((B, V, 2), **f32), torch.empty((B,), **i32)
            check(_lib.load().smplr_ld_fwd(ptr(verts), ptr(cam), ptr(targets.labels), ptr(targets.off), ptr(targets.pix),
                                           ptr(d["vclass"]), ptr(d["order"]), ptr(d["voff"]), ptr(d["vrun"]), ptr(vweight), B, V,
                                           W, C, len(spec.order), len(spec.vrun), int(targets.flip_rows), sigma, slack, ptr(e_v),
                                           ptr(e_p), ptr(near_pix), ptr(near_vert), ptr(d2_v), ptr(d2_p), ptr(proj), ptr(status),
                                           stream()), "smplr_ld_fwd")
        else:
            with torch.no_grad():
                o = label_distance_torch(verts, cam, spec, targets, vweight, sigma or None, slack, dirs)
            e_v, e_p, d2_v, d2_p, proj = (o[n].to(torch.float32) if n in o else None for n in ("e_m2i", "e_i2m", "d2_v", "d2_p", "proj"))
            near_pix, near_vert, status = o.get("near_pix"), o.get("near_vert"), o["status"]
        ctx.spec, ctx.targets, ctx.args, ctx.dims = spec, targets, (sigma, slack, dirs), (B, V, W, C)
        ctx.has_w = vweight is not None
        ctx.save_for_backward(*[t for t in (verts, cam, status, vweight, near_pix, near_vert) if t is not None])
        ctx.mark_non_differentiable(*[t for t in (near_pix, near_vert, d2_v, d2_p, proj, status) if t is not None])
        return e_v, e_p, near_pix, near_vert, d2_v, d2_p, proj, status

    @staticmethod
    def backward(ctx, g_v, g_p, *_):
        sigma, slack, dirs = ctx.args
        B, V, W, C = ctx.dims
        spec, targets = ctx.spec, ctx.targets
        saved = list(ctx.saved_tensors)
        verts, cam, status = saved[:3]
        rest = saved[3:]
        vweight = rest.pop(0) if ctx.has_w else None
        near_pix = rest.pop(0) if "m2i" in dirs else None
        near_vert = rest.pop(0) if "i2m" in dirs else None
        need_v, need_c = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if (g_v is None and g_p is None) or not (need_v or need_c):
            return (None,) * 8
        g_v = None if g_v is None else g_v.to(torch.float32).contiguous()
        g_p = None if g_p is None else g_p.to(torch.float32).contiguous()
        if not verts.is_cuda:
            with torch.enable_grad():
                v, c = verts.detach().requires_grad_(True), cam.detach().requires_grad_(True)
                o = label_distance_torch(v, c, spec, targets, vweight, sigma or None, slack, dirs)
                pairs = [(o[n], g.to(torch.float64)) for n, g in (("e_m2i", g_v), ("e_i2m", g_p)) if g is not None]
                dv, dc = torch.autograd.grad([e for e, _ in pairs], [v, c], [g for _, g in pairs], allow_unused=True)
            bad = status != 0
            dv = torch.zeros_like(v, dtype=torch.float64) if dv is None else dv
            dc = torch.zeros_like(c, dtype=torch.float64) if dc is None else dc
            dv, dc = nan_rows(bad, dv).to(torch.float32), nan_rows(bad, dc).to(torch.float32)
            return (dv if need_v else None, dc if need_c else None) + (None,) * 6
        dev = verts.device
        d = spec.on(dev)
        tiles = (len(spec.order) + TILE - 1) // TILE
        dverts = torch.empty((B, V, 3), dtype=torch.float32, device=dev)
        dcam = torch.empty((B, 4), dtype=torch.float32, device=dev) if need_c else None
        part = torch.empty((B, tiles, 4), dtype=torch.float64, device=dev) if need_c else None
        with torch.cuda.device(dev):
            check(_lib.load().smplr_ld_bwd(ptr(verts), ptr(cam), ptr(targets.off), ptr(targets.pix), ptr(d["vclass"]),
                                           ptr(d["order"]), ptr(vweight), ptr(near_pix), ptr(near_vert), ptr(status), ptr(g_v),
                                           ptr(g_p), B, V, W, C, len(spec.order), int(targets.flip_rows), sigma, slack,
                                           ptr(dverts), ptr(dcam), ptr(part), stream()), "smplr_ld_bwd")
        return (dverts if need_v else None, dcam) + (None,) * 6


@_lib.on_device
def _apply(verts, cam, spec, targets, vweight, sigma, slack, dirs):
    return _LabelDistFn.apply(verts, cam, spec, targets, vweight, sigma, slack, dirs)


def label_distance(verts, cam, spec, targets, vweight=None, sigma=None, slack=0.5, directions=DIRECTIONS, return_details=False):
    """verts (B, V, 3), cam (B, 4) fp32, spec a `LabelDistanceSpec`, targets a `LabelTargets` of B images on the same device,
    vweight (B, V) fp32 or None -> (e_m2i (B, V), e_i2m (B, W, W)) fp32, or the one direction asked for alone;
    differentiable in verts and cam.  With return_details=True also dict(near_pix, near_vert, d2_v, d2_p, proj (B, V, 2),
    status (B,)), constants to autograd (a direction not asked for: None)."""
    if not isinstance(spec, LabelDistanceSpec):
        raise TypeError("spec must be a LabelDistanceSpec")
    if not isinstance(targets, LabelTargets):
        raise TypeError("targets must be a LabelTargets")
    dirs = check_directions(directions)
    B, V = check_verts(verts, spec=spec)
    if spec.num_classes != targets.num_classes:
        raise ValueError("the spec has %d classes, the targets %d" % (spec.num_classes, targets.num_classes))
    if B != targets.B:
        raise ValueError("verts have %d rows, the targets %d images" % (B, targets.B))
    if targets.device != verts.device:
        raise RuntimeError("the targets live on %s, verts on %s" % (targets.device, verts.device))
    shapes = [("verts", verts, (B, V, 3)), ("cam", cam, (B, 4))] + ([("vweight", vweight, (B, V))] if vweight is not None else [])
    for name, t, shape in shapes:
        if not isinstance(t, torch.Tensor) or tuple(t.shape) != shape:
            raise ValueError("%s must be a %s tensor" % (name, shape))
        if t.dtype != torch.float32:
            raise RuntimeError("%s must be float32" % name)
        if t.device != verts.device:
            raise RuntimeError("%s lives on %s, verts on %s" % (name, t.device, verts.device))
    out = _apply(verts.contiguous(), cam.contiguous(), spec, targets, None if vweight is None else vweight.detach().contiguous(),
                 check_sigma(sigma), check_slack(slack), dirs)
    e = tuple(x for x, n in zip(out[:2], DIRECTIONS) if n in dirs)
    e = e if len(e) == 2 else e[0]
    return (e, dict(zip(KEYS, out[2:]))) if return_details else e
