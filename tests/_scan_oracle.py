"""Scan distances in float64 NumPy, brute force over every (point, face) and every (vertex, point) pair: the definitions
of `ilps_amd.scan` restated.

p2m: for point p and face f, d2(p, f) = min over w >= 0, sum w = 1 of |p - sum_k w_k v_{f,k}|^2, the closest point q of the
closed triangle (a zero-area face is a segment or a point).  `closest` evaluates it in coordinates relative to p as the
minimum over the three edges as clamped segments, in the order 01, 12, 20, then the interior (the normal equations of the
plane through corner 0, accepted when the determinant is positive and all three weights are non-negative); a later
candidate wins only when strictly closer.  The operations and their order are those of csrc/scan.hip's fp64 finish, so on
the same fp32 inputs and the same face both give the same float64 numbers.
m2p: per vertex the squared distance to the nearest used, finite point.
Gradient (defined on the op's own outputs): `grads`."""
import numpy as np


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _seg_weight(A, B):
    E = B - A
    ee = _dot(E, E)
    pos = ee > 0
    with np.errstate(divide="ignore", invalid="ignore"):
        t = -_dot(A, E) / np.where(pos, ee, 1.0)
    return np.where(pos, np.clip(t, 0.0, 1.0), 0.0)


def _mix2(wa, A, wb, B):
    return wa[..., None] * A + wb[..., None] * B


def closest(A, B, C):
    """The closest point to the origin of the triangles A B C (..., 3), float64 -> dict(d2, w (..., 3), q (..., 3),
    which: 0, 1, 2 = edge 01, 12, 20, 3 = interior)."""
    A, B, C = (np.asarray(x, np.float64) for x in (A, B, C))
    A, B, C = np.broadcast_arrays(A, B, C)
    one = np.ones(A.shape[:-1])
    t01, t12, t20 = _seg_weight(A, B), _seg_weight(B, C), _seg_weight(C, A)
    q01, q12, q20 = _mix2(one - t01, A, t01, B), _mix2(one - t12, B, t12, C), _mix2(one - t20, C, t20, A)
    d01, d12, d20 = _dot(q01, q01), _dot(q12, q12), _dot(q20, q20)
    d2, which = d01.copy(), np.zeros(d01.shape, np.int64)
    m = d12 < d2
    d2, which = np.where(m, d12, d2), np.where(m, 1, which)
    m = d20 < d2
    d2, which = np.where(m, d20, d2), np.where(m, 2, which)
    E0, E1 = B - A, C - A
    a00, a01, a11, b0, b1 = _dot(E0, E0), _dot(E0, E1), _dot(E1, E1), -_dot(E0, A), -_dot(E1, A)
    det = a00 * a11 - a01 * a01
    ok = det > 0
    sd = np.where(ok, det, 1.0)
    v = (a11 * b0 - a01 * b1) / sd
    w = (a00 * b1 - a01 * b0) / sd
    u = (1.0 - v) - w
    ok = ok & (v >= 0) & (w >= 0) & (u >= 0)
    qi = (u[..., None] * A + v[..., None] * B) + w[..., None] * C
    di = _dot(qi, qi)
    m = ok & (di < d2)
    d2, which = np.where(m, di, d2), np.where(m, 3, which)
    zero = np.zeros_like(one)
    sel = lambda c0, c1, c2, c3: np.where(which == 0, c0, np.where(which == 1, c1, np.where(which == 2, c2, c3)))
    wts = np.stack([sel(one - t01, zero, t20, u), sel(t01, one - t12, zero, v), sel(zero, t12, one - t20, w)], -1)
    wh = which[..., None]
    q = np.where(wh == 0, q01, np.where(wh == 1, q12, np.where(wh == 2, q20, qi)))
    return {"d2": d2, "w": wts, "q": q, "which": which}


def point_face(p, tri):
    """One point against one triangle (3, 3): d2, w (3,), q (3,) absolute, which."""
    p, tri = np.asarray(p, np.float64), np.asarray(tri, np.float64)
    r = closest(tri[0] - p, tri[1] - p, tri[2] - p)
    return {"d2": float(r["d2"]), "w": r["w"], "q": p + r["q"], "which": int(r["which"])}


def _valid_faces(faces, V):
    faces = np.asarray(faces).reshape(-1, 3)
    return ((faces >= 0) & (faces < V)).all(1) if len(faces) else np.zeros(0, bool)


def pair_d2(verts, faces, points, chunk=64):
    """(N, F) float64: d2 of every (point, face) pair of ONE mesh; +Inf for a face naming a vertex outside the mesh."""
    verts, points = np.asarray(verts, np.float64), np.asarray(points, np.float64)
    faces = np.asarray(faces).reshape(-1, 3)
    ok = _valid_faces(faces, len(verts))
    tri = verts[np.where(ok[:, None], faces, 0)]                        # (F, 3, 3)
    out = np.empty((len(points), len(faces)))
    for s in range(0, len(points), chunk):
        p = points[s:s + chunk, None, :]
        out[s:s + chunk] = closest(tri[None, :, 0] - p, tri[None, :, 1] - p, tri[None, :, 2] - p)["d2"]
    out[:, ~ok] = np.inf
    return out


def at_faces(verts, faces, points, face):
    """The closest-point evaluation of points (N, 3) on the faces named by `face` (N,) (all valid): d2 (N,), w (N, 3),
    resid (N, 3) = p - q, q (N, 3) absolute."""
    verts, points = np.asarray(verts, np.float64), np.asarray(points, np.float64)
    tri = verts[np.asarray(faces).reshape(-1, 3)[np.asarray(face)]]
    r = closest(tri[:, 0] - points, tri[:, 1] - points, tri[:, 2] - points)
    return {"d2": r["d2"], "w": r["w"], "resid": -r["q"], "q": points + r["q"]}


def pair_vd2(verts, points, count=None):
    """(V, N) float64 of ONE mesh: |v - p|^2, +Inf for points at or beyond `count` and for non-finite points."""
    verts, points = np.asarray(verts, np.float64), np.asarray(points, np.float64)
    use = np.isfinite(points).all(1)
    if count is not None:
        use &= np.arange(len(points)) < count
    e = verts[:, None, :] - np.where(use[:, None], points, 0.0)[None]
    d = _dot(e, e)
    d[:, ~use] = np.inf
    return d


def surface_distance(verts, faces, points, count=None):
    """ONE mesh, by brute force: the op's outputs in float64 (ties to the lower index)."""
    verts, points = np.asarray(verts, np.float64), np.asarray(points, np.float64)
    V, N = len(verts), len(points)
    count = N if count is None else int(count)
    faces = np.asarray(faces).reshape(-1, 3)
    out = {"d2": np.zeros(N), "face": np.full(N, -1), "bary": np.zeros((N, 3)), "resid": np.zeros((N, 3)),
           "vd2": np.full(V, np.inf), "vpoint": np.full(V, -1), "status": 0}
    if not np.isfinite(verts).all():
        out.update(d2=np.full(N, np.nan), bary=np.full((N, 3), np.nan), resid=np.full((N, 3), np.nan),
                   vd2=np.full(V, np.nan), status=1)
        return out
    used = np.arange(N) < count
    fin = np.isfinite(points).all(1)
    out["d2"][used & ~fin] = np.nan
    out["bary"][used & ~fin] = np.nan
    out["resid"][used & ~fin] = np.nan
    s = np.flatnonzero(used & fin)
    if len(s):
        if _valid_faces(faces, V).any():
            M = pair_d2(verts, faces, points[s])
            f = M.argmin(1)
            r = at_faces(verts, faces, points[s], f)
            out["d2"][s], out["face"][s], out["bary"][s], out["resid"][s] = r["d2"], f, r["w"], r["resid"]
        else:
            out["d2"][s] = np.inf
        D = pair_vd2(verts, points, count)
        out["vpoint"] = D.argmin(1)
        out["vd2"] = D[np.arange(V), out["vpoint"]]
    return out


def grads(verts, faces, points, face, bary, resid, vpoint, g_d2=None, g_vd2=None):
    """The gradient of ONE mesh, defined on the op's own outputs, in float64:
      dverts[i]  = sum over (n, k) with faces[face[n], k] = i of -2 g_d2[n] bary[n, k] resid[n] + 2 g_vd2[i] (v_i - p_vpoint[i])
      dpoints[n] = 2 g_d2[n] resid[n] - sum over i with vpoint[i] = n of 2 g_vd2[i] (v_i - p_n)
    -> dverts, dpoints and T (V, 3), the sum of the absolute values of dverts' terms."""
    verts, points = np.asarray(verts, np.float64), np.asarray(points, np.float64)
    faces = np.asarray(faces).reshape(-1, 3)
    face, vpoint = np.asarray(face), np.asarray(vpoint)
    bary, resid = np.asarray(bary, np.float64), np.asarray(resid, np.float64)
    dv, T, dp = np.zeros_like(verts), np.zeros_like(verts), np.zeros_like(points)
    if g_d2 is not None:
        g = np.asarray(g_d2, np.float64)
        for n in np.flatnonzero(face >= 0):
            dp[n] += 2.0 * g[n] * resid[n]
            for k in range(3):
                term = (-2.0 * g[n]) * bary[n, k] * resid[n]
                dv[faces[face[n], k]] += term
                T[faces[face[n], k]] += np.abs(term)
    if g_vd2 is not None:
        g = np.asarray(g_vd2, np.float64)
        for i in np.flatnonzero(vpoint >= 0):
            term = 2.0 * g[i] * (verts[i] - points[vpoint[i]])
            dv[i] += term
            T[i] += np.abs(term)
            dp[vpoint[i]] -= term
    return dv, dp, T
