"""Scan distances, differentiable: a point cloud (a depth frame, a laser scan, another model's mesh) against a decoded
mesh without correspondences - what a fit to a scan minimises and what an evaluation against one reports.  Beyond the
reference, which compares label maps only.

    topo = MeshTopology(faces, 6890)
    out = surface_distance(verts, topo, points, counts=None, directions=("p2m", "m2p"))
    out["d2"], out["face"], out["bary"], out["resid"]        # per point: to the nearest face's closest point q
    out["vd2"], out["vpoint"]                                 # per vertex: to the nearest used, finite point
    out["status"]

Definitions (verts (B, V, 3), points (B, N, 3) fp32; counts (B,) int32: mesh b uses its points 0 .. counts[b] - 1):
  p2m: d2(p, f) = min over w >= 0, sum w = 1 of |p - sum_k w_k v_{f,k}|^2 - the closest point q of the closed triangle (a
  zero-area face is a segment or a point); per point d2, face (ties to the lower index), bary = w, resid = p - q.
  m2p: vd2 = min over the mesh's used, finite points of |v - p|^2, vpoint (ties to the lower index).
  status: NONFINITE (1) when a coordinate of the mesh is NaN / Inf - every float output and gradient row of that mesh is
  NaN, every index -1; the other meshes are untouched.  A non-finite point has d2, bary, resid NaN and face -1, adds
  nothing to any gradient and is no candidate for m2p.  Points at or beyond counts[b]: d2 0, face -1, bary = resid = 0, no
  gradient.  No usable point: vd2 +Inf, vpoint -1.  No face: d2 +Inf, face -1.
  Gradient, defined on the op's own outputs (the envelope theorem for the minimum over w):
    dverts[b, i]  = sum over (n, k) with faces[face[b, n], k] = i of -2 g_d2[b, n] bary[b, n, k] resid[b, n]
                    + 2 g_vd2[b, i] (v_i - points[b, vpoint[b, i]])
    dpoints[b, n] = 2 g_d2[b, n] resid[b, n] - sum over i with vpoint[b, i] = n of 2 g_vd2[b, i] (v_i - p_n)
Device tensors run csrc/scan.hip: an fp32 search with an fp64 finish per direction (one launch each, only the directions
asked for) and one backward launch without atomics - the same bits in every run and whatever else is in the batch (the
second term of dpoints is a torch index_add_ and is outside that claim).  CPU tensors run the float64 torch restatement
`surface_distance_torch`, chunked over the points, with the same gradient - the API works without a GPU, and on device
tensors that function is the stock composition the kernels are timed against.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr, stream
from ._mesh_common import check_verts, dot3, nan_rows, neg_rows, nonfinite_rows

NONFINITE = 1          # SMPLR_SCAN_NONFINITE
DIRECTIONS = ("p2m", "m2p")
KEYS = ("d2", "face", "bary", "resid", "vd2", "vpoint", "status")


def _seg_weight(A, Bv):
    E = Bv - A
    ee = dot3(E, E)
    pos = ee > 0
    t = -dot3(A, E) / torch.where(pos, ee, torch.ones_like(ee))
    return torch.where(pos, t.clamp(0.0, 1.0), torch.zeros_like(t))


def closest_point(A, Bv, C):
    """The closest point to the origin of the triangles A Bv C (..., 3) (corners relative to the query point) -> d2 (...),
    weights (..., 3), q (..., 3): the minimum over the edges 01, 12, 20 as clamped segments, then the interior (a later
    candidate wins only when strictly closer), as csrc/scan.hip's `closest_point`."""
    t01, t12, t20 = _seg_weight(A, Bv), _seg_weight(Bv, C), _seg_weight(C, A)
    mix = lambda t, X, Y: (1.0 - t)[..., None] * X + t[..., None] * Y
    q01, q12, q20 = mix(t01, A, Bv), mix(t12, Bv, C), mix(t20, C, A)
    d01, d12, d20 = dot3(q01, q01), dot3(q12, q12), dot3(q20, q20)
    zero, one = torch.zeros_like(t01), torch.ones_like(t01)
    d2, q = d01, q01
    w = torch.stack([one - t01, t01, zero], -1)
    for d, qq, ww in ((d12, q12, torch.stack([zero, one - t12, t12], -1)), (d20, q20, torch.stack([t20, zero, one - t20], -1))):
        m = d < d2
        d2, q, w = torch.where(m, d, d2), torch.where(m[..., None], qq, q), torch.where(m[..., None], ww, w)
    E0, E1 = Bv - A, C - A
    a00, a01, a11, b0, b1 = dot3(E0, E0), dot3(E0, E1), dot3(E1, E1), -dot3(E0, A), -dot3(E1, A)
    det = a00 * a11 - a01 * a01
    ok = det > 0
    sd = torch.where(ok, det, torch.ones_like(det))
    v = (a11 * b0 - a01 * b1) / sd
    ww = (a00 * b1 - a01 * b0) / sd
    u = (1.0 - v) - ww
    qi = (u[..., None] * A + v[..., None] * Bv) + ww[..., None] * C
    di = dot3(qi, qi)
    m = ok & (v >= 0) & (ww >= 0) & (u >= 0) & (di < d2)
    d2, q, w = torch.where(m, di, d2), torch.where(m[..., None], qi, q), torch.where(m[..., None], torch.stack([u, v, ww], -1), w)
    return d2, w, q


def surface_distance_torch(verts, faces, points, counts=None, directions=DIRECTIONS, pairs_per_chunk=1 << 21):
    """The definitions in float64 torch on any device (the CPU path, and the stock composition the kernels are timed
    against): verts (B, V, 3), faces (F, 3) integer tensor, points (B, N, 3), counts (B,) or None.  The points go through in
    chunks of pairs_per_chunk / F (pairs_per_chunk / V for m2p), so (B, N, F) never exists at once.
    -> dict of d2, bary, resid, vd2 (float32), face, vpoint, status (int32); no autograd (`surface_distance` adds it)."""
    B, V = int(verts.shape[0]), int(verts.shape[1])
    N, F = int(points.shape[1]), int(faces.shape[0])
    dev = verts.device
    v, p = verts.detach().to(torch.float64), points.detach().to(torch.float64)
    bad = nonfinite_rows(v)
    v = torch.where(bad[:, None, None], torch.zeros_like(v), v)
    cnt = torch.full((B,), N, dtype=torch.long, device=dev) if counts is None else counts.to(dev).long().clamp(0, N)
    used = torch.arange(N, device=dev)[None, :] < cnt[:, None]                        # (B, N)
    fin = torch.isfinite(p).reshape(B, N, 3).all(2)
    live = used & fin
    p0 = torch.where(live[..., None], p, torch.zeros_like(p))
    nan, inf = float("nan"), float("inf")
    out = {"status": bad.to(torch.int32) * NONFINITE}
    if "p2m" in directions:
        d2 = torch.full((B, N), inf, dtype=torch.float64, device=dev)
        face = torch.full((B, N), -1, dtype=torch.long, device=dev)
        bary = torch.zeros((B, N, 3), dtype=torch.float64, device=dev)
        resid = torch.zeros((B, N, 3), dtype=torch.float64, device=dev)
        fl = faces.long()
        fok = ((fl >= 0) & (fl < V)).all(1) if F else torch.zeros(0, dtype=torch.bool, device=dev)
        if F and bool(fok.any()) and N:
            tri = v[:, torch.where(fok[:, None], fl, torch.zeros_like(fl))]             # (B, F, 3, 3)
            step = max(1, pairs_per_chunk // max(1, B * F))
            for s in range(0, N, step):
                q = p0[:, s:s + step, None, :]                                          # (B, C, 1, 3)
                dd, _, _ = closest_point(tri[:, None, :, 0] - q, tri[:, None, :, 1] - q, tri[:, None, :, 2] - q)
                dd = torch.where(fok[None, None, :], dd, torch.full_like(dd, inf))
                f = dd.argmin(2)                                                        # (ties: the first, i.e. lowest face)
                # torch.argmin names the first minimum on CPU only by convention: make it explicit
                mn = dd.gather(2, f[..., None])
                f = torch.where(dd == mn, torch.arange(F, device=dev)[None, None, :], F).amin(2)
                t = tri.gather(1, f[:, :, None, None].expand(-1, -1, 3, 3))             # (B, C, 3, 3)
                pc = p0[:, s:s + step]
                dw, ww, qq = closest_point(t[:, :, 0] - pc, t[:, :, 1] - pc, t[:, :, 2] - pc)
                d2[:, s:s + step], face[:, s:s + step], bary[:, s:s + step], resid[:, s:s + step] = dw, f, ww, -qq
        l1, l3 = live, live[..., None]
        d2 = torch.where(l1, d2, torch.where(used, torch.full_like(d2, nan), torch.zeros_like(d2)))
        fill3 = torch.where(used[..., None], torch.full_like(bary, nan), torch.zeros_like(bary))
        bary, resid = torch.where(l3, bary, fill3), torch.where(l3, resid, fill3)
        face = torch.where(l1, face, torch.full_like(face, -1))
        out["d2"], out["bary"] = nan_rows(bad, d2).to(torch.float32), nan_rows(bad, bary).to(torch.float32)
        out["resid"], out["face"] = nan_rows(bad, resid).to(torch.float32), neg_rows(bad, face).to(torch.int32)
    if "m2p" in directions:
        vd2 = torch.full((B, V), inf, dtype=torch.float64, device=dev)
        vpoint = torch.full((B, V), -1, dtype=torch.long, device=dev)
        step = max(1, pairs_per_chunk // max(1, B * V))
        for s in range(0, N, step):
            e = v[:, :, None, :] - p0[:, None, s:s + step, :]                           # (B, V, C, 3)
            dd = torch.where(live[:, None, s:s + step], dot3(e, e), torch.full((), inf, dtype=torch.float64, device=dev))
            mn = dd.amin(2)
            j = torch.where(dd == mn[..., None], torch.arange(s, s + dd.shape[2], device=dev)[None, None, :], N).amin(2)
            better = mn < vd2                                                           # (strict: ties stay with the lower point)
            vd2, vpoint = torch.where(better, mn, vd2), torch.where(better, j, vpoint)
        out["vd2"], out["vpoint"] = nan_rows(bad, vd2).to(torch.float32), neg_rows(bad, vpoint).to(torch.int32)
    return out


def _backward_torch(verts, faces, points, face, bary, resid, vpoint, status, g_d2, g_vd2, want_v, want_p):
    """The gradient definition in float64 torch (index_add_), rounded to float32 once -> dverts, dpoints (or None)."""
    B, V = verts.shape[:2]
    N = points.shape[1]
    dev = verts.device
    dv = torch.zeros((B * V, 3), dtype=torch.float64, device=dev) if want_v else None
    dp = torch.zeros((B * N, 3), dtype=torch.float64, device=dev) if want_p else None
    if g_d2 is not None and face is not None and faces.shape[0]:
        hit = face >= 0
        g = torch.where(hit, g_d2.to(torch.float64), torch.zeros((), dtype=torch.float64, device=dev))
        r = torch.where(hit[..., None], resid.to(torch.float64), torch.zeros((), dtype=torch.float64, device=dev))
        if want_p:
            dp += (2.0 * g[..., None] * r).reshape(-1, 3)
        if want_v:
            w = torch.where(hit[..., None], bary.to(torch.float64), torch.zeros((), dtype=torch.float64, device=dev))
            ids = faces.long()[face.long().clamp(min=0)]                                # (B, N, 3)
            ids = ids + (torch.arange(B, device=dev) * V)[:, None, None]
            for k in range(3):
                dv.index_add_(0, ids[..., k].reshape(-1), (((-2.0 * g) * w[..., k])[..., None] * r).reshape(-1, 3))
    if g_vd2 is not None and vpoint is not None and N:
        hit = vpoint >= 0
        j = vpoint.long().clamp(min=0)
        pj = points.to(torch.float64).gather(1, j[..., None].expand(-1, -1, 3))
        term = 2.0 * torch.where(hit, g_vd2.to(torch.float64), torch.zeros((), dtype=torch.float64, device=dev))[..., None] \
            * (verts.to(torch.float64) - pj)
        term = torch.where(hit[..., None], term, torch.zeros_like(term))
        if want_v:
            dv += term.reshape(-1, 3)
        if want_p:
            dp.index_add_(0, (j + (torch.arange(B, device=dev) * N)[:, None]).reshape(-1), -term.reshape(-1, 3))
    fin = lambda t, n: None if t is None else nan_rows(status != 0, t.reshape(B, n, 3)).to(torch.float32)
    return fin(dv, V), fin(dp, N)


class _SurfaceDistanceFn(torch.autograd.Function):
    """verts (B, V, 3), points (B, N, 3) -> d2, face, bary, resid, vd2, vpoint, status (None for a direction not asked for).
    Device tensors: smplr_scan_p2m / smplr_scan_m2p forward, smplr_scan_bwd backward; CPU tensors: the float64 torch path."""

    @staticmethod
    def forward(ctx, verts, points, counts, topo, directions):
        ctx.set_materialize_grads(False)
        dev = verts.device
        B, V, N, F = int(verts.shape[0]), int(verts.shape[1]), int(points.shape[1]), topo.num_faces
        faces = topo.on(dev)["faces"]
        p2m, m2p = "p2m" in directions, "m2p" in directions
        d2 = face = bary = resid = vd2 = vpoint = None
        if verts.is_cuda:
            lib = _lib.load()
            f = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)
            i = lambda *s: torch.empty(s, dtype=torch.int32, device=dev)
            status = i(B)
            if p2m:
                d2, face, bary, resid = f(B, N), i(B, N), f(B, N, 3), f(B, N, 3)
                check(lib.smplr_scan_p2m(ptr(verts), ptr(faces) if F else None, ptr(points) if N else None, ptr(counts), B, V,
                                         F, N, ptr(d2), ptr(face), ptr(bary), ptr(resid), ptr(status), stream()),
                      "smplr_scan_p2m")
            if m2p:
                vd2, vpoint = f(B, V), i(B, V)
                check(lib.smplr_scan_m2p(ptr(verts), ptr(points) if N else None, ptr(counts), B, V, N, ptr(vd2), ptr(vpoint),
                                         ptr(status), stream()), "smplr_scan_m2p")
        else:
            o = surface_distance_torch(verts, faces, points, counts, directions)
            d2, face, bary, resid, vd2, vpoint, status = (o.get(k) for k in KEYS)
        ctx.topo, ctx.dims = topo, (B, V, F, N)
        ctx.save_for_backward(verts, points, face, bary, resid, vpoint, status)
        ctx.mark_non_differentiable(*[t for t in (face, bary, resid, vpoint, status) if t is not None])
        return d2, face, bary, resid, vd2, vpoint, status

    @staticmethod
    def backward(ctx, g_d2, _gf, _gb, _gr, g_vd2, _gp, _gs):
        verts, points, face, bary, resid, vpoint, status = ctx.saved_tensors
        B, V, F, N = ctx.dims
        want_v, want_p = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        faces = ctx.topo.on(verts.device)["faces"]
        cont = lambda g: None if g is None else g.to(torch.float32).contiguous()
        g_d2, g_vd2 = cont(g_d2) if face is not None else None, cont(g_vd2) if vpoint is not None else None
        if not verts.is_cuda:
            dv, dp = _backward_torch(verts, faces, points, face, bary, resid, vpoint, status, g_d2, g_vd2, want_v, want_p)
            return dv, dp, None, None, None
        dverts = dpoints = None
        if want_v:
            dverts = torch.empty_like(verts)
            with torch.cuda.device(verts.device):
                check(_lib.load().smplr_scan_bwd(ptr(verts), ptr(faces) if F else None, ptr(points) if N else None, ptr(face),
                                                 ptr(bary), ptr(resid), ptr(vpoint), ptr(status), ptr(g_d2), ptr(g_vd2), B, V,
                                                 F, N, ptr(dverts), stream()), "smplr_scan_bwd")
        if want_p:
            _, dpoints = _backward_torch(verts, faces, points, face, bary, resid, vpoint, status, g_d2, g_vd2, False, True)
        return dverts, dpoints, None, None, None


@_lib.on_device
def _apply(verts, points, counts, topo, directions):
    return _SurfaceDistanceFn.apply(verts, points, counts, topo, directions)


def surface_distance(verts, topo, points, counts=None, directions=DIRECTIONS):
    """verts (B, V, 3), points (B, N, 3) fp32, counts (B,) integers or None -> dict(d2 (B, N), face (B, N) int32, bary
    (B, N, 3), resid (B, N, 3) for "p2m"; vd2 (B, V), vpoint (B, V) int32 for "m2p"; status (B,) int32).  Differentiable in
    verts and points through d2 and vd2; bary, resid and the indices are constants of the gradient."""
    B, V = check_verts(verts, topo, ("faces", "num_faces", "num_verts", "on"))
    if not isinstance(points, torch.Tensor) or points.dim() != 3 or points.shape[0] != B or points.shape[2] != 3:
        raise ValueError("points must be a (%d, N, 3) tensor" % B)
    if points.device != verts.device:
        raise RuntimeError("points live on %s, verts on %s" % (points.device, verts.device))
    directions = (directions,) if isinstance(directions, str) else tuple(directions)
    if not directions or any(d not in DIRECTIONS for d in directions):
        raise ValueError("directions must name \"p2m\" and / or \"m2p\", got %r" % (directions,))
    N = int(points.shape[1])
    if N > (1 << 24):
        raise ValueError("at most 2^24 points per mesh (got %d)" % N)
    if verts.dtype != torch.float32 or points.dtype != torch.float32:
        raise RuntimeError("verts and points must be float32")
    if counts is not None:
        if not isinstance(counts, torch.Tensor):
            c = np.asarray(counts)
            if c.shape != (B,) or not np.issubdtype(c.dtype, np.integer):
                raise ValueError("counts must be (%d,) integers" % B)
            if c.size and (int(c.min()) < 0 or int(c.max()) > N):
                raise ValueError("counts must lie in 0 .. %d" % N)
            counts = torch.from_numpy(c.astype(np.int32)).to(verts.device)
        else:
            if tuple(counts.shape) != (B,) or counts.dtype not in (torch.int32, torch.int64):
                raise ValueError("counts must be (%d,) int32 or int64" % B)
            if not counts.is_cuda and counts.numel() and (int(counts.min()) < 0 or int(counts.max()) > N):
                raise ValueError("counts must lie in 0 .. %d" % N)
            # (a device tensor is not read back: the kernels clamp it to 0 .. N)
            counts = counts.to(device=verts.device, dtype=torch.int32).contiguous()
    out = _apply(verts.contiguous(), points.contiguous(), counts, topo, directions)
    return {k: t for k, t in zip(KEYS, out) if t is not None}


def sample_surface(verts, topo, n, generator=None):
    """n area-weighted samples of each mesh's surface: a face drawn in proportion to its area, then uniform barycentric
    weights (1 - sqrt(r1), sqrt(r1) (1 - r2), sqrt(r1) r2).  verts (B, V, 3) -> points (B, n, 3) in verts' dtype, face (B, n)
    int64 and bary (B, n, 3); in torch, on verts' device, the draws from `generator` (on that device)."""
    if verts.dim() != 3 or verts.shape[2] != 3 or verts.shape[1] != topo.num_verts:
        raise ValueError("verts must be (B, %d, 3)" % topo.num_verts)
    if topo.num_faces == 0:
        raise ValueError("the topology has no faces to sample")
    B, dev = int(verts.shape[0]), verts.device
    faces = topo.on(dev)["faces"].long()
    v = verts.detach().to(torch.float64)
    tri = v[:, faces]                                                                   # (B, F, 3, 3)
    area = torch.linalg.cross(tri[:, :, 1] - tri[:, :, 0], tri[:, :, 2] - tri[:, :, 0]).norm(dim=-1)
    if not bool((area.sum(1) > 0).all()) or not bool(torch.isfinite(area).all()):
        raise ValueError("every mesh needs a finite, positive surface area")
    f = torch.multinomial(area, int(n), replacement=True, generator=generator)          # (B, n)
    r = torch.rand((B, int(n), 2), dtype=torch.float64, device=dev, generator=generator)
    s = r[..., 0].sqrt()
    bary = torch.stack([1.0 - s, s * (1.0 - r[..., 1]), s * r[..., 1]], -1)
    t = tri.gather(1, f[:, :, None, None].expand(-1, -1, 3, 3))
    pts = (bary[..., None] * t).sum(2)
    return pts.to(verts.dtype), f, bary
