"""Body measurements of a mesh, differentiable: signed volume, surface area, axis-aligned extents (height) and the girths
of plane cuts through chosen parts - what a tape measure or a known height can be compared with, and what a loss term can
hold fixed (under the orthographic camera the scale k_u and the body's size are otherwise confounded).  Beyond the
reference, which states shape as ten betas.

    topo = MeshTopology(faces, 6890)
    spec = MeasureSpec(topo, planes=[[0, 1, 0, 0.2]], part_mask=[torso_bits], names=["chest"])
    m = mesh_measures(verts, spec)                      # verts (B, V, 3); differentiable in verts (and planes)
    m["volume"], m["area"], m["extent"], m["girth"], m["status"], m["ext_idx"]

Definitions (per mesh; fp64 arithmetic on the fp32 inputs, one rounding to fp32 per output):
  volume = 1/6 sum_f v0 . (v1 x v2) (signed);  area = 1/2 sum_f |(v1 - v0) x (v2 - v0)|;
  extent[a] = max_i v_i[a] - min_i v_i[a], ext_idx = argmin x, y, z, argmax x, y, z (ties to the lowest index);
  girth[k]: plane k = [n_x, n_y, n_z, o] (n need not be unit), d_i = ((n_x x_i + n_y y_i) + n_z z_i) - o, vertex i is above
  iff d_i >= 0; a face whose part is in part_mask[k] and whose vertices are not all on one side has two edges from an above
  vertex i to a below vertex j, q = v_i + t (v_j - v_i) with t = d_i / (d_i - d_j), and adds |q - q'|.  A zero-length
  segment adds 0 and has zero gradient; a zero-area face has zero area gradient.
  status: NONFINITE (1) when a coordinate of the mesh or one of its planes is NaN / Inf - that mesh's outputs and its
  gradient rows are NaN, its ext_idx -1; the other meshes are untouched.
Device tensors run csrc/measure.hip (one forward launch, one backward launch, no atomics: the same bits in every run and
whatever else is in the batch); CPU tensors run the float64 torch restatement below, with autograd's gradient, so the API
works without a GPU.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr, stream
from ._mesh_common import check_topo, check_verts, neg_rows, nonfinite_rows

NONFINITE = 1          # SMPLR_MM_NONFINITE
MAX_PLANES = 16
ALL_PARTS = 0xFFFFFFFF


class MeasureSpec:
    """What to measure on meshes of one topology: K cutting planes (K, 4) = [n_x, n_y, n_z, o] rows (or None: the caller
    passes planes with every call), one 32-bit part mask per plane (bit p selects the faces with face_part == p; default
    every part) and optional names.  K <= 16; K = 0 (no planes, no masks) measures volume, area and extents only."""

    def __init__(self, topo, planes=None, part_mask=None, names=None):
        check_topo(topo, ("faces", "vf_off", "vf_face", "face_part", "on"))
        self.topo = topo
        if planes is not None:
            planes = torch.as_tensor(np.asarray(planes) if not isinstance(planes, torch.Tensor) else planes).detach()
            planes = planes.to(torch.float32).cpu()
            if planes.dim() != 2 or planes.shape[1] != 4:
                raise ValueError("planes must be (K, 4) rows [n_x, n_y, n_z, o], got %s" % (tuple(planes.shape),))
        if part_mask is not None:
            pm = np.asarray(part_mask.detach().cpu().numpy() if isinstance(part_mask, torch.Tensor) else part_mask)
            if pm.ndim != 1 or not (np.issubdtype(pm.dtype, np.integer) or pm.dtype == object or pm.size == 0):
                raise ValueError("part_mask must be (K,) integers")
            vals = [int(x) for x in pm.tolist()]
            if any(not 0 <= x <= ALL_PARTS for x in vals):
                raise ValueError("part masks must lie in 0 .. 2^32 - 1")
        ks = [n for n in (None if planes is None else int(planes.shape[0]), None if part_mask is None else len(vals),
                          None if names is None else len(names)) if n is not None]
        K = ks[0] if ks else 0
        if any(k != K for k in ks):
            raise ValueError("planes, part_mask and names disagree on the number of planes: %s" % ks)
        if K > MAX_PLANES:
            raise ValueError("at most %d planes (got %d)" % (MAX_PLANES, K))
        self.num_planes = K
        self.planes = planes
        self.part_mask = np.asarray(vals if part_mask is not None else [ALL_PARTS] * K, np.uint32).reshape(K)
        self.names = None if names is None else [str(n) for n in names]
        self._dev = {}

    def on(self, device):
        """The topology's device copies (`MeshTopology.on`) + part_mask (K,) int32 (the mask bits) and planes (K, 4) or None."""
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        d = self._dev.get(device)
        if d is None:
            d = dict(self.topo.on(device))
            d["part_mask"] = torch.from_numpy(self.part_mask.view(np.int32).copy()).to(device)
            d["planes"] = None if self.planes is None else self.planes.to(device)
            self._dev[device] = d
        return d


def planes_through(points, normals):
    """Planes through `points` (..., K, 3) with `normals` (..., K, 3) -> (..., K, 4) = [n, n . p]; differentiable."""
    points, normals = torch.as_tensor(points), torch.as_tensor(normals)
    if points.shape[-1:] != (3,) or normals.shape != points.shape:
        raise ValueError("points and normals must both be (..., K, 3), got %s and %s" % (tuple(points.shape), tuple(normals.shape)))
    return torch.cat([normals, (normals * points).sum(-1, keepdim=True)], -1)


def joint_planes(J_transformed, anchors, along):
    """Planes that move with the body: plane k passes through joint anchors[k] of J_transformed (B, J, 3) and its normal is
    the direction from joint along[k][0] to joint along[k][1] (e.g. anchors=[3], along=[(3, 6)]: through the lower spine,
    normal along the spine) -> (B, K, 4); differentiable."""
    J = J_transformed
    if J.dim() != 3 or J.shape[2] != 3:
        raise ValueError("J_transformed must be (B, J, 3)")
    anchors = [int(a) for a in anchors]
    along = [(int(a), int(b)) for a, b in along]
    if len(anchors) != len(along):
        raise ValueError("anchors and along must have one entry per plane")
    nj = J.shape[1]
    if any(not 0 <= j < nj for j in anchors) or any(not (0 <= a < nj and 0 <= b < nj) for a, b in along):
        raise ValueError("joint indices must lie in [0, %d)" % nj)
    if any(a == b for a, b in along):
        raise ValueError("a normal needs two different joints")
    idx = lambda l: torch.as_tensor(l, dtype=torch.long, device=J.device)
    return planes_through(J[:, idx(anchors)], J[:, idx([b for _, b in along])] - J[:, idx([a for a, _ in along])])


def _safe_norm(x):
    """|x| over the last axis with a zero (not NaN) gradient where x = 0."""
    s = (x * x).sum(-1)
    pos = s > 0
    return torch.where(pos, torch.sqrt(torch.where(pos, s, torch.ones_like(s))), torch.zeros_like(s))


def measures_torch(verts, faces, face_part, planes, part_mask):
    """The definitions in float64 torch on any device (the CPU path, and the stock composition the kernels are timed
    against): verts (B, V, 3), faces (F, 3) and face_part (F,) integer tensors, planes (B, K, 4), part_mask (K,) int64.
    -> volume, area, extent, girth (float32), ext_idx, status (int32); autograd supplies the gradient."""
    B, V = verts.shape[:2]
    K = planes.shape[1]
    dev = verts.device
    v_in, p_in = verts.to(torch.float64), planes.to(torch.float64)
    bad = nonfinite_rows(v_in) | nonfinite_rows(p_in)
    # a bad mesh is computed on zeros (nothing of it reaches its neighbours) and poisoned at the end: NaN outputs, NaN gradient rows
    v = torch.where(bad[:, None, None], torch.zeros_like(v_in), v_in)
    p = torch.where(bad[:, None, None], torch.zeros_like(p_in), p_in)
    nan = float("nan")
    # (masked on both sides: the outer where keeps the NaN out of the good meshes' values, the inner ones out of their gradients)
    only_bad = lambda x: torch.where(bad[:, None, None], x, torch.zeros_like(x))
    poison = torch.where(bad, (only_bad(v_in) * nan).reshape(B, -1).sum(1) + (only_bad(p_in) * nan).reshape(B, -1).sum(1),
                         torch.zeros(B, dtype=torch.float64, device=dev))
    faces = faces.long()
    t = v[:, faces]                                                     # (B, F, 3, 3)
    v0, v1, v2 = t[:, :, 0], t[:, :, 1], t[:, :, 2]
    volume = (v0 * torch.linalg.cross(v1, v2)).sum(-1).sum(1) / 6.0
    area = _safe_norm(torch.linalg.cross(v1 - v0, v2 - v0)).sum(1) * 0.5
    ar = torch.arange(V, device=dev)[None, :, None]
    lo, hi = v.detach().amin(1, keepdim=True), v.detach().amax(1, keepdim=True)
    imin = torch.where(v.detach() == lo, ar, V).amin(1)                  # (B, 3): ties to the lowest index
    imax = torch.where(v.detach() == hi, ar, V).amin(1)
    extent = v.gather(1, imax[:, None])[:, 0] - v.gather(1, imin[:, None])[:, 0]
    ext_idx = torch.cat([imin, imax], 1)
    ext_idx = neg_rows(bad, ext_idx).to(torch.int32)
    if K > 0:
        n, o = p[:, :, :3], p[:, :, 3]
        d = ((n[:, :, None, 0] * v[:, None, :, 0] + n[:, :, None, 1] * v[:, None, :, 1]) + n[:, :, None, 2] * v[:, None, :, 2]) \
            - o[:, :, None]                                             # (B, K, V)
        df = d[:, :, faces]                                             # (B, K, F, 3)
        above = df >= 0
        na = above.sum(-1)
        sel = ((part_mask.to(dev).long()[:, None] >> face_part.to(dev).long()[None, :]) & 1).bool()      # (K, F)
        hit = ((na == 1) | (na == 2)) & sel[None]
        up = na == 1
        lone = torch.where(above[..., 0] == up, 0, torch.where(above[..., 1] == up, 1, 2))               # (B, K, F)
        order = (lone[..., None] + torch.arange(3, device=dev)) % 3                                      # lone, next, next
        dd = df.gather(-1, order)
        tt = t[:, None].expand(B, K, -1, 3, 3).gather(3, order[..., None].expand(-1, -1, -1, -1, 3))
        A, Bv, C = tt[..., 0, :], tt[..., 1, :], tt[..., 2, :]
        dA, dB, dC = dd[..., 0], dd[..., 1], dd[..., 2]
        u3 = up[..., None]

        def cut(Pi, Pj, di, dj):
            D = torch.where(hit, di - dj, torch.ones_like(di))
            return Pi + (di / D)[..., None] * (Pj - Pi)
        q1 = cut(torch.where(u3, A, Bv), torch.where(u3, Bv, A), torch.where(up, dA, dB), torch.where(up, dB, dA))
        q2 = cut(torch.where(u3, A, C), torch.where(u3, C, A), torch.where(up, dA, dC), torch.where(up, dC, dA))
        seg = _safe_norm(q1 - q2)
        girth = torch.where(hit, seg, torch.zeros_like(seg)).sum(-1)
    else:
        girth = torch.zeros((B, 0), dtype=torch.float64, device=dev)
    f32 = lambda x: (x + poison.reshape((B,) + (1,) * (x.dim() - 1))).to(torch.float32)
    return f32(volume), f32(area), f32(extent), f32(girth), ext_idx, bad.to(torch.int32) * NONFINITE


class _MeshMeasuresFn(torch.autograd.Function):
    """verts (B, V, 3), planes (K, 4) / (B, K, 4) / None -> volume, area, extent, girth, ext_idx, status through
    smplr_mesh_measures; backward through smplr_mesh_measures_bwd, the planes' gradient = g_girth[..., None] * dgirth_dplane."""

    @staticmethod
    def forward(ctx, verts, planes, spec):
        ctx.set_materialize_grads(False)
        dev = verts.device
        B, V = int(verts.shape[0]), int(verts.shape[1])
        t = spec.on(dev)
        F = spec.topo.num_faces
        K = 0 if planes is None else int(planes.shape[-2])
        bstride = K * 4 if (planes is not None and planes.dim() == 3) else 0
        f = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)
        volume, area, extent, girth = f(B), f(B), f(B, 3), f(B, K)
        ext_idx = torch.empty((B, 6), dtype=torch.int32, device=dev)
        status = torch.empty((B,), dtype=torch.int32, device=dev)
        want_p = K > 0 and ctx.needs_input_grad[1]
        dgdp = f(B, K, 4) if want_p else None
        check(_lib.load().smplr_mesh_measures(ptr(verts), ptr(t["faces"]) if F else None, ptr(t["face_part"]) if K else None,
                                              ptr(planes) if K else None, bstride, ptr(t["part_mask"]) if K else None, B, V, F, K,
                                              ptr(volume), ptr(area), ptr(extent), ptr(ext_idx), ptr(girth) if K else None,
                                              ptr(dgdp), ptr(status), stream()), "smplr_mesh_measures")
        ctx.spec, ctx.dims = spec, (B, V, F, K, bstride)
        ctx.save_for_backward(verts, planes, ext_idx, status, dgdp)
        ctx.mark_non_differentiable(ext_idx, status)
        return volume, area, extent, girth, ext_idx, status

    @staticmethod
    def backward(ctx, g_volume, g_area, g_extent, g_girth, _g_idx, _g_status):
        verts, planes, ext_idx, status, dgdp = ctx.saved_tensors
        B, V, F, K, bstride = ctx.dims
        dverts = dplanes = None
        cont = lambda g: None if g is None else g.to(torch.float32).contiguous()
        g_volume, g_area, g_extent, g_girth = cont(g_volume), cont(g_area), cont(g_extent), cont(g_girth)
        if ctx.needs_input_grad[0]:
            t = ctx.spec.on(verts.device)
            dverts = torch.empty_like(verts)
            with torch.cuda.device(verts.device):
                check(_lib.load().smplr_mesh_measures_bwd(
                    ptr(verts), ptr(t["faces"]) if F else None, ptr(t["vf_off"]), ptr(t["vf_face"]) if F else None,
                    int(t["vf_face"].numel()), ptr(t["face_part"]) if K else None, ptr(planes) if K else None, bstride,
                    ptr(t["part_mask"]) if K else None, ptr(ext_idx), ptr(status), ptr(g_volume), ptr(g_area), ptr(g_extent),
                    ptr(g_girth) if K else None, B, V, F, K, ptr(dverts), stream()), "smplr_mesh_measures_bwd")
        if planes is not None and ctx.needs_input_grad[1]:
            if g_girth is None or dgdp is None:
                dplanes = torch.zeros_like(planes)
            else:
                dplanes = g_girth[..., None] * dgdp
                if planes.dim() == 2:
                    dplanes = dplanes.sum(0)
        return dverts, dplanes, None


@_lib.on_device
def _mesh_measures_hip(verts, planes, spec):
    if verts.dtype != torch.float32 or (planes is not None and planes.dtype != torch.float32):
        raise RuntimeError("verts and planes must be float32 on the HIP path")
    if planes is not None and not planes.is_cuda:
        raise RuntimeError("planes live on %s, verts on %s" % (planes.device, verts.device))
    return _MeshMeasuresFn.apply(verts.contiguous(), None if planes is None else planes.contiguous(), spec)


def mesh_measures(verts, spec, planes=None):
    """verts (B, V, 3) -> dict(volume (B,), area (B,), extent (B, 3), girth (B, K) fp32; status (B,), ext_idx (B, 6) int32).
    planes: (K, 4) or (B, K, 4), overriding the spec's (planes that move with the body: `joint_planes`); K must be the
    spec's.  Differentiable in verts and planes."""
    B, V = check_verts(verts)
    if not isinstance(spec, MeasureSpec):
        raise TypeError("spec must be a MeasureSpec")
    if V != spec.topo.num_verts:
        raise ValueError("verts have %d vertices, the topology %d" % (V, spec.topo.num_verts))
    K = spec.num_planes
    if planes is None:
        planes = spec.on(verts.device)["planes"] if K else None
        if K and planes is None:
            raise ValueError("the spec holds no planes: pass planes=")
    else:
        planes = torch.as_tensor(planes)
        if planes.device != verts.device:
            raise RuntimeError("planes live on %s, verts on %s" % (planes.device, verts.device))
    if planes is not None and not ((planes.dim() == 2 and tuple(planes.shape) == (K, 4)) or
                                   (planes.dim() == 3 and tuple(planes.shape) == (B, K, 4))):
        raise ValueError("planes must be (%d, 4) or (%d, %d, 4), got %s" % (K, B, K, tuple(planes.shape)))
    if verts.is_cuda:
        out = _mesh_measures_hip(verts, planes if K else None, spec)
    else:
        t = spec.on(verts.device)
        pl = torch.zeros((B, 0, 4), dtype=torch.float64) if not K else \
            (planes if planes.dim() == 3 else planes[None].expand(B, K, 4))
        out = measures_torch(verts, t["faces"], t["face_part"], pl, torch.from_numpy(spec.part_mask.astype(np.int64)))
    return dict(zip(("volume", "area", "extent", "girth", "ext_idx", "status"), out))
