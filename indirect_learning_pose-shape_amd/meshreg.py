"""Mesh regularisers for SMPL+D registration, differentiable: a Laplacian term against a reference mesh and a relative
edge-length term.  Free per-vertex offsets (`SMPLLayer(x, offsets=D)`, `fitting.OffsetFitter`) reach a clothed scan; these
two terms keep the surface a mesh of SMPL's shape while they do.  Beyond the reference, which moves 86 parameters only.

    topo = MeshTopology(faces, 6890)
    spec = MeshRegSpec(topo, v_template, weights="cotangent")      # built once on the host, in float64
    terms = mesh_regularisers(verts, spec, return_terms=True)      # (B, 2) = (E_lap, E_edge); differentiable in verts
    e = mesh_regularisers(verts, spec, lap_weight=10.0, edge_weight=1.0)       # (B,) = the weighted sum

Definitions (per mesh; fp64 arithmetic on the fp32 inputs, one rounding to fp32 per output):
  L(v)_i = v_i - sum_k w_ik v_k over the one-ring of i (the vertices sharing a face with i); 0 for a vertex of degree 0;
  E_lap  = 1/V sum_i vweight_i |L(v)_i - lap_ref_i|^2, lap_ref = L(ref) (the mesh keeps the reference's local shape) or
           zeros with smooth=True (plain smoothing);
  E_edge = 1/E sum over the E unique edges of (|v_i - v_j|^2 / l_e^2 - 1)^2, l_e the edge's length in ref: smooth at zero
           length and dimensionless.  An edge of zero reference length is left out (and not counted in E); E = 0 gives 0.
Weights: "uniform" = 1 / deg; "cotangent" = max(sum of the cotangents of the angles opposite the edge, 0) measured on ref,
each row divided by its sum (a row whose clamped weights sum to 0 falls back to uniform); or an array (nnz,) in the order
of the spec's CSR (rows by vertex, neighbours increasing), taken as it is.  The stored fp32 arrays are the definition: the
weights are rounded to fp32 first and lap_ref = L(ref) is formed with the rounded weights.
Device tensors run csrc/meshreg.hip (one forward call, one backward launch, no atomics: the same bits in every run and
whatever else is in the batch); CPU tensors run the float64 torch restatement `mesh_reg_torch`, with autograd's gradient.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr, stream
from ._mesh_common import check_topo, check_verts


def one_ring(faces, V):
    """The symmetric one-ring of a face list as a CSR: (off (V + 1,), idx (nnz,)) int64, rows by vertex, neighbours
    increasing, no (i, i), every pair once however many faces share the edge."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    a = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    a = np.concatenate([a, a[:, ::-1]])
    a = a[a[:, 0] != a[:, 1]]
    key = np.unique(a[:, 0] * V + a[:, 1])
    row, idx = key // V, key % V
    off = np.concatenate([[0], np.cumsum(np.bincount(row, minlength=V))]).astype(np.int64)
    return off, idx


def cotangent_raw(faces, ref, off, idx):
    """Per CSR entry (i, k): the sum over the faces holding the edge of the cotangent of the angle opposite it, measured on
    ref (float64); a face of zero area adds nothing."""
    V = len(off) - 1
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    r = np.asarray(ref, np.float64)
    key = np.repeat(np.arange(V), np.diff(off)) * V + idx
    raw = np.zeros(len(idx))
    for c in range(3):
        i, j, k = f[:, (c + 1) % 3], f[:, (c + 2) % 3], f[:, c]            # edge (i, j), opposite corner k
        u, w = r[i] - r[k], r[j] - r[k]
        cr = np.linalg.norm(np.cross(u, w), axis=1)
        ok = (cr > 0) & (i != j)
        cot = np.where(ok, (u * w).sum(1) / np.where(ok, cr, 1.0), 0.0)
        for a, b in ((i, j), (j, i)):
            pos = np.searchsorted(key, a[ok] * V + b[ok])
            np.add.at(raw, pos, cot[ok])
    return raw


class MeshRegSpec:
    """The regularisers' constants for meshes of one topology, built once on the host in float64: topo a
    render.MeshTopology, ref (V, 3) the reference mesh (normally the model's v_template), weights "uniform" | "cotangent" |
    an (nnz,) array, vweight (V,) >= 0 or None (ones), smooth=True for lap_ref = 0.

    Holds nb_off (V + 1) int32, nb_idx (nnz) int32, nb_w (nnz, 3) fp32 = [w_ik, w_ki, 1 / l_ik^2] per entry, lap_ref (V, 3)
    fp32 or None, vweight (V,) fp32 or None, num_edges = E."""

    def __init__(self, topo, ref, weights="uniform", vweight=None, smooth=False):
        check_topo(topo, ("faces", "num_verts", "on"))
        V = int(topo.num_verts)
        r = ref.detach().cpu().numpy() if isinstance(ref, torch.Tensor) else np.asarray(ref)
        if r.shape != (V, 3):
            raise ValueError("ref must be (%d, 3), got %s" % (V, r.shape))
        r = r.astype(np.float64)
        if not np.isfinite(r).all():
            raise ValueError("ref holds a value that is not finite")
        off, idx = one_ring(topo.faces, V)
        deg = np.diff(off)
        nnz = int(idx.size)
        row = np.repeat(np.arange(V), deg)
        uniform = 1.0 / np.maximum(deg, 1)[row].astype(np.float64)
        if isinstance(weights, str):
            if weights == "uniform":
                w = uniform
            elif weights == "cotangent":
                raw = np.maximum(cotangent_raw(topo.faces, r, off, idx), 0.0)
                rs = np.bincount(row, raw, minlength=V)
                good = (rs > 0) & np.isfinite(rs)
                w = np.where(good[row], raw / np.where(good, rs, 1.0)[row], uniform)
            else:
                raise ValueError("weights must be \"uniform\", \"cotangent\" or an (nnz,) array, got %r" % (weights,))
        else:
            w = np.asarray(weights.detach().cpu().numpy() if isinstance(weights, torch.Tensor) else weights, np.float64)
            if w.shape != (nnz,) or not np.isfinite(w).all():
                raise ValueError("a weight array must be (%d,) finite values in the CSR's order" % nnz)
        w32 = w.astype(np.float32)
        back = np.searchsorted(row * V + idx, idx * V + row)                  # the entry (k, i) of the entry (i, k)
        d = r[row] - r[idx]
        l2 = (d * d).sum(1)
        il2 = np.where(l2 > 0, 1.0 / np.where(l2 > 0, l2, 1.0), 0.0).astype(np.float32)
        il2 = np.where(np.isfinite(il2), il2, 0.0).astype(np.float32)         # (1 / l^2 beyond fp32: left out as well)
        self.topo = topo
        self.num_verts, self.nnz = V, nnz
        self.num_edges = int(((idx > row) & (il2 != 0)).sum())
        self.weights = weights if isinstance(weights, str) else "array"
        self.nb_off = off.astype(np.int32)
        self.nb_idx = idx.astype(np.int32)
        self.nb_w = np.ascontiguousarray(np.stack([w32, w32[back], il2], 1), np.float32).reshape(nnz, 3)
        if smooth:
            self.lap_ref = None
        else:
            s = np.zeros((V, 3))
            np.add.at(s, row, w32.astype(np.float64)[:, None] * r[idx])
            self.lap_ref = np.where((deg > 0)[:, None], r - s, 0.0).astype(np.float32)
        if vweight is None:
            self.vweight = None
        else:
            vw = np.asarray(vweight.detach().cpu().numpy() if isinstance(vweight, torch.Tensor) else vweight, np.float64)
            if vw.shape != (V,):
                raise ValueError("vweight must be (%d,), got %s" % (V, vw.shape))
            if not np.isfinite(vw).all() or (vw < 0).any():
                raise ValueError("vweight must be finite and >= 0")
            self.vweight = vw.astype(np.float32)
        self._dev = {}

    def on(self, device):
        """The device copies (uploaded once per device): nb_off, nb_idx, nb_w, lap_ref or None, vweight or None."""
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        d = self._dev.get(device)
        if d is None:
            up = lambda a: None if a is None else torch.from_numpy(a).to(device)
            d = {k: up(getattr(self, k)) for k in ("nb_off", "nb_idx", "nb_w", "lap_ref", "vweight")}
            self._dev[device] = d
        return d


def mesh_reg_torch(verts, nb_off, nb_idx, nb_w, lap_ref=None, vweight=None, num_edges=None):
    """The definitions in float64 torch on any device (the CPU path, and the stock composition the kernels are timed
    against): verts (B, V, 3), the spec's arrays as tensors on verts' device -> terms (B, 2) in verts' dtype; autograd
    supplies the gradient.  num_edges None: counted here (a host read)."""
    B, V = verts.shape[:2]
    dev = verts.device
    v = verts.to(torch.float64)
    idx = nb_idx.long()
    deg = (nb_off[1:] - nb_off[:-1]).long()
    row = torch.repeat_interleave(torch.arange(V, device=dev), deg)
    w = nb_w.to(torch.float64)
    s = torch.zeros((B, V, 3), dtype=torch.float64, device=dev).index_add(1, row, w[None, :, 0, None] * v[:, idx])
    has = (deg > 0)[None, :, None]
    d = torch.where(has, v - s, torch.zeros_like(v))
    if lap_ref is not None:
        d = d - lap_ref.to(torch.float64)[None]
    sq = (d * d).sum(-1)
    if vweight is not None:
        sq = sq * vweight.to(torch.float64)[None]
    e_lap = sq.sum(1) / V
    m = (idx > row) & (w[:, 2] != 0)
    E = int(m.sum()) if num_edges is None else int(num_edges)
    if E > 0:
        dd = v[:, row[m]] - v[:, idx[m]]
        q = (dd * dd).sum(-1) * w[m, 2][None] - 1.0
        e_edge = (q * q).sum(1) / E
    else:
        e_edge = torch.zeros(B, dtype=torch.float64, device=dev) + 0.0 * v.reshape(B, -1)[:, :0].sum(1)
    return torch.stack([e_lap, e_edge], 1).to(verts.dtype)


class _MeshRegFn(torch.autograd.Function):
    """verts (B, V, 3) -> terms (B, 2) through smplr_mesh_reg_fwd; backward through smplr_mesh_reg_bwd."""

    @staticmethod
    def forward(ctx, verts, spec):
        dev = verts.device
        B, V = int(verts.shape[0]), int(verts.shape[1])
        t = spec.on(dev)
        lib = _lib.load()
        terms = torch.empty((B, 2), dtype=torch.float32, device=dev)
        ws = torch.empty(max(int(lib.smplr_mesh_reg_workspace(B, V)) // 8, 1), dtype=torch.float64, device=dev)
        check(lib.smplr_mesh_reg_fwd(ptr(verts), ptr(t["nb_off"]), ptr(t["nb_idx"]) if spec.nnz else None,
                                     ptr(t["nb_w"]) if spec.nnz else None, spec.nnz, ptr(t["lap_ref"]), ptr(t["vweight"]),
                                     spec.num_edges, B, V, ptr(terms), ptr(ws), stream()), "smplr_mesh_reg_fwd")
        ctx.spec = spec
        ctx.save_for_backward(verts)
        return terms

    @staticmethod
    def backward(ctx, g):
        (verts,) = ctx.saved_tensors
        spec = ctx.spec
        B, V = int(verts.shape[0]), int(verts.shape[1])
        t = spec.on(verts.device)
        g = g.to(torch.float32).contiguous()
        dverts = torch.empty_like(verts)
        with torch.cuda.device(verts.device):
            check(_lib.load().smplr_mesh_reg_bwd(ptr(verts), ptr(t["nb_off"]), ptr(t["nb_idx"]) if spec.nnz else None,
                                                 ptr(t["nb_w"]) if spec.nnz else None, spec.nnz, ptr(t["lap_ref"]),
                                                 ptr(t["vweight"]), spec.num_edges, ptr(g), B, V, ptr(dverts), stream()),
                  "smplr_mesh_reg_bwd")
        return dverts, None


@_lib.on_device
def _mesh_reg_hip(verts, spec):
    if verts.dtype != torch.float32:
        raise RuntimeError("verts must be float32 on the HIP path")
    return _MeshRegFn.apply(verts.contiguous(), spec)


def mesh_regularisers(verts, spec, return_terms=False, lap_weight=1.0, edge_weight=1.0):
    """verts (B, V, 3) -> terms (B, 2) = (E_lap, E_edge) with return_terms, else lap_weight E_lap + edge_weight E_edge (B,).
    Differentiable in verts."""
    check_verts(verts)
    if not isinstance(spec, MeshRegSpec):
        raise TypeError("spec must be a MeshRegSpec")
    if int(verts.shape[1]) != spec.num_verts:
        raise ValueError("verts have %d vertices, the spec %d" % (int(verts.shape[1]), spec.num_verts))
    if verts.is_cuda:
        terms = _mesh_reg_hip(verts, spec)
    else:
        t = spec.on(verts.device)
        terms = mesh_reg_torch(verts, t["nb_off"], t["nb_idx"], t["nb_w"], t["lap_ref"], t["vweight"], spec.num_edges)
    if return_terms:
        return terms
    return float(lap_weight) * terms[:, 0] + float(edge_weight) * terms[:, 1]
