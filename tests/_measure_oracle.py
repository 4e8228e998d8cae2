"""Oracle for the mesh measurements (csrc/measure.hip, ilps_amd.measure): the definitions in NumPy float64, one mesh at a
time, and their gradients from a separate torch-float64 restatement under autograd (not the package's CPU path: hit faces
are picked out with boolean indexing and every face corner is its own leaf, so the per-face contributions - and with them
T = sum |terms|, what the rounding bars are stated in - come out of autograd too).

    d_i = ((n_x x_i + n_y y_i) + n_z z_i) - o, above iff d_i >= 0; a selected face that is not on one side has two edges from
    an above vertex i to a below vertex j, q = v_i + t (v_j - v_i), t = d_i / (d_i - d_j), and adds |q - q'|.
"""
import numpy as np
import torch

EDGES = ((0, 1), (1, 2), (2, 0))


def plane_dist(v, plane):
    n, o = plane[:3], plane[3]
    return ((n[0] * v[..., 0] + n[1] * v[..., 1]) + n[2] * v[..., 2]) - o


def _selected(face_part, mask, F):
    part = np.zeros(F, np.int64) if face_part is None else np.asarray(face_part, np.int64)     # (no parts: every face is part 0)
    return ((int(mask) >> part) & 1).astype(bool)


def cut(verts, faces, plane, sel):
    """One plane on one mesh -> (segment lengths of the counted faces, their face ids, conditioning number)."""
    v = np.asarray(verts, np.float64)
    p = np.asarray(plane, np.float64)
    d = plane_dist(v, p)
    f = np.asarray(faces, np.int64)
    df = d[f]
    ab = df >= 0
    na = ab.sum(1)
    hit = np.nonzero(((na == 1) | (na == 2)) & sel)[0]
    if hit.size == 0:
        return np.zeros(0), hit, 0.0
    fh, dh, ah = f[hit], df[hit], ab[hit]
    qs, cross, cond = [], [], []
    for a, b in EDGES:
        cr = ah[:, a] != ah[:, b]
        i = np.where(ah[:, a], a, b)                       # the above corner of the edge
        j = np.where(ah[:, a], b, a)
        r = np.arange(len(hit))
        vi, vj, di, dj = v[fh[r, i]], v[fh[r, j]], dh[r, i], dh[r, j]
        D = np.where(cr, di - dj, 1.0)
        qs.append(vi + (di / D)[:, None] * (vj - vi))
        cross.append(cr)
        c = (np.linalg.norm(p[:3]) * np.maximum(np.linalg.norm(vi, axis=1), np.linalg.norm(vj, axis=1)) + abs(p[3])) / np.abs(D)
        cond.append(np.where(cr, c, 0.0))
    qs, cross = np.stack(qs, 1), np.stack(cross, 1)          # (n, 3, 3), (n, 3)
    assert (cross.sum(1) == 2).all()
    q = qs[cross].reshape(len(hit), 2, 3)
    return np.linalg.norm(q[:, 0] - q[:, 1], axis=1), hit, float(np.max(cond))


def measures(verts, faces, face_part=None, planes=None, part_mask=None):
    """verts (V, 3), faces (F, 3), planes (K, 4), part_mask (K,) -> dict: volume, area, extent (3), ext_idx (6), girth (K),
    each sum with its T = sum |terms| (volume_T, area_T, girth_T), counted (K) faces, zero_len (K) of them, cond (K)."""
    v = np.asarray(verts, np.float64)
    f = np.asarray(faces, np.int64)
    v0, v1, v2 = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    det = (v0 * np.cross(v1, v2)).sum(1)
    ar = np.linalg.norm(np.cross(v1 - v0, v2 - v0), axis=1)
    out = {"volume": det.sum() / 6.0, "volume_T": np.abs(det).sum() / 6.0, "area": ar.sum() / 2.0, "area_T": ar.sum() / 2.0}
    imin = np.array([int(np.flatnonzero(v[:, a] == v[:, a].min())[0]) for a in range(3)])
    imax = np.array([int(np.flatnonzero(v[:, a] == v[:, a].max())[0]) for a in range(3)])
    out["ext_idx"] = np.concatenate([imin, imax]).astype(np.int32)
    out["extent"] = v[imax, np.arange(3)] - v[imin, np.arange(3)]
    planes = np.zeros((0, 4)) if planes is None else np.asarray(planes, np.float64).reshape(-1, 4)
    K = len(planes)
    part_mask = [0xFFFFFFFF] * K if part_mask is None else list(part_mask)
    g, cnt, zl, cond = np.zeros(K), np.zeros(K, int), np.zeros(K, int), np.zeros(K)
    for k in range(K):
        L, hit, c = cut(v, f, planes[k], _selected(face_part, part_mask[k], len(f)))
        g[k], cnt[k], zl[k], cond[k] = L.sum(), len(hit), int((L == 0).sum()), c
    out.update(girth=g, girth_T=g.copy(), counted=cnt, zero_len=zl, cond=cond)
    return out


# ---- gradients: torch float64 under autograd, every face corner a leaf -------------------------------------------------

def _norm0(x):
    """|x| with zero gradient at x = 0 (a zero-length segment, a zero-area face)."""
    s = (x * x).sum(-1)
    nz = s > 0
    out = torch.zeros_like(s)
    out[nz] = torch.sqrt(s[nz])
    return out


def _girth_corners(t, plane, sel):
    """t (F, 3, 3) corner copies, plane (4,) (or (F, 4) per-face copies) -> the girth, through the counted faces only."""
    pl = plane if plane.dim() == 2 else plane[None].expand(t.shape[0], 4)
    d = ((pl[:, None, 0] * t[..., 0] + pl[:, None, 1] * t[..., 1]) + pl[:, None, 2] * t[..., 2]) - pl[:, None, 3]
    ab = d.detach() >= 0
    na = ab.sum(1)
    hit = ((na == 1) | (na == 2)) & torch.from_numpy(sel)
    idx = torch.nonzero(hit)[:, 0]
    if idx.numel() == 0:
        return (t.sum() + pl.sum()) * 0.0
    th, dh, ah = t[idx], d[idx], ab[idx]
    r = torch.arange(idx.numel())
    qs, crs = [], []
    for a, b in EDGES:
        cr = ah[:, a] != ah[:, b]
        i = torch.where(ah[:, a], a, b)
        j = torch.where(ah[:, a], b, a)
        vi, vj, di, dj = th[r, i], th[r, j], dh[r, i], dh[r, j]
        D = torch.where(cr, di - dj, torch.ones_like(di))
        qs.append(vi + (di / D)[:, None] * (vj - vi))
        crs.append(cr)
    qs, crs = torch.stack(qs, 1), torch.stack(crs, 1)
    q = qs[crs].reshape(idx.numel(), 2, 3)
    return _norm0(q[:, 0] - q[:, 1]).sum()


def grads(verts, faces, face_part=None, planes=None, part_mask=None, g_volume=None, g_area=None, g_extent=None, g_girth=None):
    """The gradient of g_volume volume + g_area area + g_extent . extent + g_girth . girth of ONE mesh -> dverts (V, 3),
    dverts_T (V, 3) = sum of |per-face, per-term contributions| at each vertex component, dgirth_dplane (K, 4) (unweighted)
    and its T (K, 4).  Absent cotangents are zero."""
    v = np.asarray(verts, np.float64)
    f = np.asarray(faces, np.int64)
    V, F = len(v), len(f)
    planes = np.zeros((0, 4)) if planes is None else np.asarray(planes, np.float64).reshape(-1, 4)
    K = len(planes)
    part_mask = [0xFFFFFFFF] * K if part_mask is None else list(part_mask)
    dv, dvT = np.zeros((V, 3)), np.zeros((V, 3))

    def add(fn, weight):
        t = torch.from_numpy(v[f]).clone().requires_grad_(True)            # (F, 3, 3)
        fn(t).backward()
        c = t.grad.numpy() * weight
        np.add.at(dv, f.reshape(-1), c.reshape(-1, 3))
        np.add.at(dvT, f.reshape(-1), np.abs(c).reshape(-1, 3))

    if g_volume is not None:
        add(lambda t: (t[:, 0] * torch.linalg.cross(t[:, 1], t[:, 2])).sum() / 6.0, float(g_volume))
    if g_area is not None:
        add(lambda t: _norm0(torch.linalg.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])).sum() / 2.0, float(g_area))
    dp, dpT = np.zeros((K, 4)), np.zeros((K, 4))
    for k in range(K):
        sel = _selected(face_part, part_mask[k], F)
        pk = torch.from_numpy(planes[k])
        if g_girth is not None:
            add(lambda t: _girth_corners(t, pk, sel), float(np.asarray(g_girth, np.float64)[k]))
        pf = pk[None].expand(F, 4).clone().requires_grad_(True)           # a copy of the plane per face
        _girth_corners(torch.from_numpy(v[f]), pf, sel).backward()
        dp[k], dpT[k] = pf.grad.numpy().sum(0), np.abs(pf.grad.numpy()).sum(0)
    if g_extent is not None:
        ge = np.asarray(g_extent, np.float64)
        ei = measures(v, f)["ext_idx"]
        for a in range(3):
            dv[ei[a], a] -= ge[a]
            dv[ei[3 + a], a] += ge[a]
            dvT[ei[a], a] += abs(ge[a])
            dvT[ei[3 + a], a] += abs(ge[a])
    return {"dverts": dv, "dverts_T": dvT, "dgirth_dplane": dp, "dgirth_dplane_T": dpT}


def within(got, ref, T, rel=2.0 ** -24, absT=2.0 ** -28):
    """The rounding bar |got - ref| <= 2^-24 |ref| + 2^-28 T, elementwise -> (ok, worst ratio of error to bar)."""
    got, ref, T = (np.asarray(a, np.float64) for a in (got, ref, T))
    bar = rel * np.abs(ref) + absT * T
    err = np.abs(got - ref)
    ratio = np.where(err == 0, 0.0, err / np.where(bar > 0, bar, np.finfo(np.float64).tiny))
    return bool((err <= bar).all()), float(ratio.max()) if ratio.size else 0.0
