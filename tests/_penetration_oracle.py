"""The self-penetration term's definition in NumPy float64 by brute force over every pair (INTEGRATION.md 4o,
csrc/penetration.hip): candidates, choice, normal, inside test, energy, gradient - operation for operation, so that the
fp64 finish of the kernel and this file give the same bits for the same chosen vertex.

verts (V, 3), faces (F, 3), part (V,) in -1 .. P - 1 (anything else counts as -1), collide (P, P) of 0 / 1 (row = the query's
part, column = the candidate's; the diagonal is ignored)."""
import numpy as np


def dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def clean_part(part, P):
    p = np.asarray(part, np.int64)
    return np.where((p >= 0) & (p < P), p, -1)


def allowed(part, collide):
    """(V, V) bool: allowed[i, j] = j is a candidate of i."""
    c = np.asarray(collide).astype(bool)
    P = c.shape[0]
    p = clean_part(part, P)
    if P == 0:
        return np.zeros((len(p), len(p)), bool)
    c = c & ~np.eye(P, dtype=bool)
    has = p >= 0
    pc = np.where(has, p, 0)
    return has[:, None] & has[None, :] & (p[:, None] != p[None, :]) & c[pc][:, pc]


def pair_d2(verts, part, collide, rows=None):
    """(rows, V) float64 squared distances, +Inf where j is no candidate of i."""
    v = np.asarray(verts, np.float64)
    ok = allowed(part, collide)
    sl = slice(None) if rows is None else rows
    e = v[None, :, :] - v[sl, None, :]
    return np.where(ok[sl], dot3(e, e), np.inf)


def csr(faces, V):
    """The vertex -> face CSR, faces in increasing id per vertex (render.MeshTopology builds the same)."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    flat = f.reshape(-1)
    fid = np.repeat(np.arange(len(f)), 3)
    order = np.argsort(flat, kind="stable")
    return np.concatenate([[0], np.cumsum(np.bincount(flat, minlength=V))]), fid[order]


def normal(verts, faces, j, vf=None):
    """n_j = sum over the faces incident to j, in increasing face id, of cross(v_b - v_a, v_c - v_a), one face at a time."""
    v = np.asarray(verts, np.float64)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    off, vf_face = csr(f, len(v)) if vf is None else vf
    n = np.zeros(3)
    for k in range(off[j], off[j + 1]):
        a, b, c = v[f[vf_face[k], 0]], v[f[vf_face[k], 1]], v[f[vf_face[k], 2]]
        u, w = b - a, c - a
        n = n + np.array([u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0]])
    return n


def at(verts, faces, near, vf=None):
    """The finish for GIVEN winners near (V,) (-1: none) -> d2 (V,) float64, s (V,), inside (V,) bool, e (V,) float64."""
    v = np.asarray(verts, np.float64)
    V = len(v)
    vf = csr(faces, V) if vf is None else vf
    d2, s = np.full(V, np.inf), np.zeros(V)
    cache = {}
    for i in range(V):
        j = int(near[i])
        if j < 0:
            continue
        d = v[i] - v[j]
        d2[i] = dot3(d, d)
        if j not in cache:
            cache[j] = normal(v, faces, j, vf)
        s[i] = dot3(d, cache[j])
    inside = (np.asarray(near) >= 0) & (s < 0)
    return d2, s, inside, np.where(inside, d2, 0.0)


def self_penetration(verts, faces, part, collide, chunk=1024):
    """-> dict(near (V,) int64, d2, e (V,) float64, inside (V,) bool, s (V,)), every pair evaluated (in row chunks)."""
    v = np.asarray(verts, np.float64)
    V = len(v)
    near = np.full(V, -1, np.int64)
    for r in range(0, V, chunk):
        M = pair_d2(v, part, collide, slice(r, r + chunk))
        j = M.argmin(1)                                   # (np.argmin: the first minimum = the lowest index)
        near[r:r + chunk] = np.where(np.isfinite(M[np.arange(len(j)), j]), j, -1)
    d2, s, inside, e = at(v, faces, near)
    return {"near": near, "d2": d2, "e": e, "inside": inside, "s": s}


def grads(verts, near, inside, g):
    """The closed form, teacher-forced on near / inside: dverts (V, 3) float64 and T (V, 3) = the sum of |terms|.
    dverts[k] = 2 g_k inside_k (v_k - v_near(k)) - sum_{i: near(i) = k, inside_i} 2 g_i (v_i - v_k), own term first, then
    increasing i."""
    v = np.asarray(verts, np.float64)
    g = np.asarray(g, np.float64)
    V = len(v)
    dv, T = np.zeros((V, 3)), np.zeros((V, 3))
    live = np.asarray(inside, bool) & (np.asarray(near) >= 0)
    for k in range(V):
        if live[k]:
            t = (2.0 * g[k]) * (v[k] - v[near[k]])
            dv[k] = t
            T[k] = np.abs(t)
    for i in range(V):
        if live[i]:
            k = near[i]
            t = (2.0 * g[i]) * (v[i] - v[k])
            dv[k] = dv[k] - t
            T[k] += np.abs(t)
    return dv, T
