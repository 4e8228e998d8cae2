"""Self-penetration, differentiable: a penalty on a body mesh passing through itself - SMPLify's fourth regulariser, the
one that needs the mesh.  Beyond the reference, which compares label maps only.

    topo = MeshTopology(faces, 6890)                              # faces, vertex -> face CSR, a part per vertex
    e = self_penetration(verts, topo)                             # (B, V) fp32, differentiable in verts
    e, det = self_penetration(verts, topo, collide, return_details=True)   # det: d2, near, inside, status

Definitions (verts (B, V, 3) fp32; part = topo.vertex_part in -1 .. P - 1, P <= 31; collide (P, P) of 0 / 1, row = the
query's part, column = the candidate's, not necessarily symmetric, its diagonal ignored):
  candidates of vertex i: every j != i with part[i] >= 0, part[j] >= 0, part[i] != part[j], collide[part[i], part[j]] = 1; a
          part outside -1 .. P - 1 counts as -1.
  near[i] the candidate with the smallest |v_i - v_j|^2, ties to the lower j; d2[i] that squared distance.  Without a
          candidate near = -1 and d2 = +Inf.
  n_j     sum over the faces incident to j, in increasing face id, of cross(v_b - v_a, v_c - v_a) with (a, b, c) the face's
          corners as listed: area-weighted, not normalised; float64 on the fp32 coordinates, for the winner only.
  inside[i] = s_i < 0, s_i = ((d_x n_x + d_y n_y) + d_z n_z), d = v_i - v_near(i), float64.  s = 0 (a vertex in the tangent
          plane, a zero normal) is not inside.
  e[i]    inside[i] ? d2[i] : 0, rounded to fp32 once.  Contact from outside costs nothing.
  status  NONFINITE (1) when a coordinate of the mesh is NaN / Inf: its e, d2 and gradient rows are NaN, near -1, inside
          False; the other meshes are untouched.
  Gradient (the choice and the sign are piecewise constant), with cotangent g on e:
    dverts[k] = 2 g_k inside_k (v_k - v_near(k)) - sum over i with near(i) = k and inside_i of 2 g_i (v_i - v_k)
  the own term first, then the others in increasing i; float64, rounded once.
Device tensors run csrc/penetration.hip: one forward launch (an fp32 search over the mesh's own vertices in part-major
order with tile pruning, an fp64 finish) and one backward launch without atomics - the same bits in every run and whatever
else is in the batch.  CPU tensors run the float64 torch restatement `self_penetration_torch`, chunked over the queries so
that no (B, V, V) tensor exists; on device tensors that function is the stock composition the kernels are timed against.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr, stream
from ._mesh_common import check_verts, dot3, nan_rows, neg_rows, nonfinite_rows

NONFINITE = 1          # SMPLR_PEN_NONFINITE
MAX_PARTS = 31
KEYS = ("d2", "near", "inside", "status")


def _num_parts(topo):
    vp = np.asarray(topo.vertex_part)
    return int(vp.max()) + 1 if vp.size and int(vp.max()) >= 0 else 0


def part_collision_table(topo, hops=1):
    """The default part-pair table, a host function run once: (P, P) uint8 numpy array, P = 1 + the largest part of
    topo.vertex_part.  Two parts are adjacent when some face has vertices of both; two parts collide (1) unless they are the
    same part or within `hops` steps of each other in that graph.  hops = 0: every pair of distinct parts collides."""
    hops = int(hops)
    if hops < 0:
        raise ValueError("hops must be >= 0, got %r" % (hops,))
    P = _num_parts(topo)
    if P > MAX_PARTS:
        raise ValueError("at most %d parts (got %d)" % (MAX_PARTS, P))
    vp = np.asarray(topo.vertex_part, np.int64)
    adj = np.zeros((P, P), bool)
    if topo.num_faces and P:
        fp = vp[np.asarray(topo.faces, np.int64)]                               # (F, 3)
        for a, b in ((0, 1), (1, 2), (2, 0)):
            m = (fp[:, a] >= 0) & (fp[:, b] >= 0) & (fp[:, a] != fp[:, b])
            adj[fp[m, a], fp[m, b]] = True
            adj[fp[m, b], fp[m, a]] = True
    reach = np.eye(P, dtype=bool)
    for _ in range(hops):
        reach = reach | ((reach.astype(np.int64) @ adj.astype(np.int64)) > 0)
    return (~reach).astype(np.uint8)


def part_major_order(vertex_part, P, tile=256):
    """int32 slots of the pruned walk of csrc/penetration.hip, queries and candidates alike: the vertices by part (0 .. P - 1,
    each in increasing index, each part's run padded with -1 to a multiple of `tile` slots, so that a tile of the walk holds
    one part and its bounding sphere is that part's), then those without a part.  Every vertex appears exactly once."""
    vp = np.asarray(vertex_part, np.int64)
    key = np.where((vp >= 0) & (vp < P), vp, P)
    runs = []
    for p in range(P + 1):
        ids = np.nonzero(key == p)[0].astype(np.int32)
        pad = (-len(ids)) % tile if p < P else 0
        runs += [ids, np.full(pad, -1, np.int32)]
    return np.concatenate(runs) if runs else np.zeros(0, np.int32)


def check_collide(collide, topo):
    """None (the default table, cached on the topology) or a (P, P) array of 0 / 1 with P <= 31 -> (P, P) uint8 numpy."""
    if collide is None:
        c = getattr(topo, "_pen_default", None)
        if c is None:
            c = part_collision_table(topo, 1)
            topo._pen_default = c
        return c
    c = np.asarray(collide.detach().cpu() if isinstance(collide, torch.Tensor) else collide)
    if c.ndim != 2 or c.shape[0] != c.shape[1]:
        raise ValueError("collide must be a (P, P) table, got shape %s" % (c.shape,))
    if c.shape[0] > MAX_PARTS:
        raise ValueError("at most %d parts (collide is %d x %d)" % (MAX_PARTS, c.shape[0], c.shape[0]))
    if not (c.dtype == np.bool_ or np.issubdtype(c.dtype, np.integer)) or not np.isin(c, (0, 1)).all():
        raise ValueError("collide must hold 0 / 1")
    return np.ascontiguousarray(c, np.uint8)


def _device_operands(topo, collide, device):
    """faces, vf_off, vf_face, part (int32), perm (int32), collide (uint8) on `device`: uploaded once per device and table
    (no copy in later calls, so a call can be captured into a graph)."""
    d = topo.on(device)
    P = int(collide.shape[0])
    key = ("pen", P, collide.tobytes())
    ops = d.get(key)
    if ops is None:
        dev = d["faces"].device
        ops = (torch.from_numpy(np.asarray(topo.vertex_part).astype(np.int32)).to(dev),
               torch.from_numpy(part_major_order(topo.vertex_part, P)).to(dev), torch.from_numpy(collide.copy()).to(dev))
        d[key] = ops
    return (d["faces"], d["vf_off"], d["vf_face"]) + ops


def vertex_normals_torch(v, faces, vf_off, vf_face):
    """v (B, V, 3) float64 -> (B, V, 3): per vertex the sum, in the CSR's order, of cross(v_b - v_a, v_c - v_a) over its
    faces - one addition per vertex and round of the loop, so the order of the sum is the definition's."""
    B, V = v.shape[:2]
    n = torch.zeros_like(v)
    F = int(faces.shape[0])
    if F == 0:
        return n
    fl = faces.long()
    a, b, c = v[:, fl[:, 0]], v[:, fl[:, 1]], v[:, fl[:, 2]]
    u, w = b - a, c - a
    cr = torch.stack([u[..., 1] * w[..., 2] - u[..., 2] * w[..., 1], u[..., 2] * w[..., 0] - u[..., 0] * w[..., 2],
                      u[..., 0] * w[..., 1] - u[..., 1] * w[..., 0]], -1)          # (B, F, 3)
    off = vf_off.long()
    deg = off[1:] - off[:-1]
    for k in range(int(deg.max()) if V else 0):
        has = deg > k
        f = vf_face.long()[(off[:-1] + k).clamp(max=vf_face.shape[0] - 1)]
        n = n + torch.where(has[None, :, None], cr[:, f], torch.zeros((), dtype=v.dtype, device=v.device))
    return n


def self_penetration_torch(verts, topo, collide=None, pairs_per_chunk=1 << 21):
    """The definitions in float64 torch on any device (the CPU path, and the stock composition the kernels are timed
    against).  The queries go through in chunks of pairs_per_chunk / (B V), so (B, V, V) never exists at once.
    -> dict of e, d2 (float32), near, status (int32), inside (bool); no autograd (`self_penetration` adds it)."""
    collide = check_collide(collide, topo)
    B, V = int(verts.shape[0]), int(verts.shape[1])
    dev = verts.device
    d = topo.on(dev)
    P = int(collide.shape[0])
    v = verts.detach().to(torch.float64)
    bad = nonfinite_rows(v)
    v = torch.where(bad[:, None, None], torch.zeros_like(v), v)
    part = d["vertex_part"].long()
    part = torch.where((part >= 0) & (part < P), part, torch.full_like(part, -1))
    table = torch.from_numpy(collide).to(dev).bool() & ~torch.eye(P, dtype=torch.bool, device=dev)
    inf = float("inf")
    d2 = torch.full((B, V), inf, dtype=torch.float64, device=dev)
    near = torch.full((B, V), -1, dtype=torch.long, device=dev)
    if P and B:
        ids = torch.arange(V, device=dev)
        pc = part.clamp(min=0)
        step = max(1, pairs_per_chunk // max(1, B * V))
        for s in range(0, V, step):
            q = slice(s, s + step)
            ok = (part[q, None] >= 0) & (part[None, :] >= 0) & (part[q, None] != part[None, :]) & table[pc[q]][:, pc]   # (C, V)
            e = v[:, None, :, :] - v[:, q, None, :]                                   # (B, C, V, 3)
            dd = torch.where(ok[None], dot3(e, e), torch.full((), inf, dtype=torch.float64, device=dev))
            mn = dd.amin(2)
            j = torch.where((dd == mn[..., None]) & ok[None], ids[None, None, :], V).amin(2)   # ties: the lowest index
            hit = j < V
            d2[:, q] = torch.where(hit, mn, torch.full_like(mn, inf))
            near[:, q] = torch.where(hit, j, torch.full_like(j, -1))
    hit = near >= 0
    nj = near.clamp(min=0)[..., None].expand(-1, -1, 3)
    n = vertex_normals_torch(v, d["faces"], d["vf_off"], d["vf_face"]).gather(1, nj)
    dv = v - v.gather(1, nj)
    inside = hit & (dot3(dv, n) < 0)
    e = torch.where(inside, d2, torch.zeros_like(d2))
    return {"e": nan_rows(bad, e).to(torch.float32), "d2": nan_rows(bad, d2).to(torch.float32),
            "near": neg_rows(bad, near).to(torch.int32), "inside": inside & ~bad[:, None], "status": bad.to(torch.int32) * NONFINITE}


def _backward_torch(verts, near, inside, status, g):
    """The gradient definition in float64 torch, rounded to float32 once: the own term, then index_add_ of the others (on the
    CPU in increasing i)."""
    B, V = verts.shape[:2]
    dev = verts.device
    v = verts.detach().to(torch.float64)
    live = inside & (near >= 0)
    c = 2.0 * torch.where(live, g.to(torch.float64), torch.zeros((), dtype=torch.float64, device=dev))     # (B, V)
    nj = near.long().clamp(min=0)
    diff = torch.where(live[..., None], v - v.gather(1, nj[..., None].expand(-1, -1, 3)), torch.zeros_like(v))
    term = c[..., None] * diff
    dv = term.reshape(B * V, 3).clone()
    sel = live.reshape(-1).nonzero()[:, 0]                                           # (increasing (b, i))
    tgt = (nj + (torch.arange(B, device=dev) * V)[:, None]).reshape(-1)
    dv.index_add_(0, tgt[sel], -term.reshape(B * V, 3)[sel])
    return nan_rows(status != 0, dv.reshape(B, V, 3)).to(torch.float32)


class _SelfPenetrationFn(torch.autograd.Function):
    """verts (B, V, 3) -> e, d2, near, inside, status.  Device tensors: smplr_pen_fwd forward, smplr_pen_bwd backward; CPU
    tensors: the float64 torch path."""

    @staticmethod
    def forward(ctx, verts, topo, collide):
        ctx.set_materialize_grads(False)
        dev = verts.device
        B, V = int(verts.shape[0]), int(verts.shape[1])
        if verts.is_cuda:
            faces, vf_off, vf_face, part, perm, table = _device_operands(topo, collide, dev)
            F, P = topo.num_faces, int(collide.shape[0])
            e = torch.empty((B, V), dtype=torch.float32, device=dev)
            d2 = torch.empty((B, V), dtype=torch.float32, device=dev)
            near = torch.empty((B, V), dtype=torch.int32, device=dev)
            inside8 = torch.empty((B, V), dtype=torch.uint8, device=dev)
            status = torch.empty((B,), dtype=torch.int32, device=dev)
            check(_lib.load().smplr_pen_fwd(ptr(verts), ptr(faces) if F else None, ptr(vf_off), ptr(vf_face) if F else None,
                                            ptr(part), ptr(table) if P else None, ptr(perm), int(perm.shape[0]), B, V, F, P, ptr(e), ptr(d2),
                                            ptr(near), ptr(inside8), ptr(status), stream()), "smplr_pen_fwd")
            inside = inside8.view(torch.bool)
        else:
            o = self_penetration_torch(verts, topo, collide)
            e, d2, near, inside, status = o["e"], o["d2"], o["near"], o["inside"], o["status"]
        ctx.dims = (B, V)
        ctx.save_for_backward(verts, near, inside, status)
        ctx.mark_non_differentiable(d2, near, inside, status)
        return e, d2, near, inside, status

    @staticmethod
    def backward(ctx, g, *_):
        verts, near, inside, status = ctx.saved_tensors
        B, V = ctx.dims
        if g is None or not ctx.needs_input_grad[0]:
            return None, None, None
        g = g.to(torch.float32).contiguous()
        if not verts.is_cuda:
            return _backward_torch(verts, near, inside, status, g), None, None
        dverts = torch.empty_like(verts)
        with torch.cuda.device(verts.device):
            check(_lib.load().smplr_pen_bwd(ptr(verts), ptr(near), ptr(inside.view(torch.uint8)), ptr(status), ptr(g), B, V,
                                            ptr(dverts), stream()), "smplr_pen_bwd")
        return dverts, None, None


@_lib.on_device
def _apply(verts, topo, collide):
    return _SelfPenetrationFn.apply(verts, topo, collide)


def self_penetration(verts, topo, collide=None, return_details=False):
    """verts (B, V, 3) fp32, topo a `render.MeshTopology`, collide None (`part_collision_table(topo, 1)`) or a (P, P) table of
    0 / 1 -> e (B, V) fp32, differentiable in verts; with return_details=True also dict(d2 (B, V) fp32, near (B, V) int32,
    inside (B, V) bool, status (B,) int32), constants of the gradient."""
    check_verts(verts, topo, ("faces", "vf_off", "vf_face", "vertex_part", "num_faces", "num_verts", "on"))
    if verts.dtype != torch.float32:
        raise RuntimeError("verts must be float32")
    collide = check_collide(collide, topo)
    e, d2, near, inside, status = _apply(verts.contiguous(), topo, collide)
    return (e, dict(zip(KEYS, (d2, near, inside, status)))) if return_details else e
