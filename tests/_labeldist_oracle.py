"""Float64 NumPy restatement of the label-map distance term (ilps_amd/labeldist.py, csrc/labeldist.hip), one row at a time
and one class at a time, from the label map itself - it shares nothing with the sorted pixel lists or the slot order under
test: projection, both searches, energies, status and the closed-form gradients, and beside every float output the number T
that its rounding bar is made of (`_keypoint_oracle.within`: |got - want| <= 2^-24 |want| + 2^-28 T).

The winners are defined in fp64 on the fp32 inputs, operation for operation: p_u = u0 + k_u X (the product of two fp32
numbers is exact in fp64: one rounding), du = p_u - q_u, d2 = du du + dv dv (three roundings, no fused multiply-add),
smallest d2, ties to the lower index - np.argmin's first occurrence over candidates in increasing index.  So the indices must
be equal, not close.  T, first order, as in _keypoint_oracle:
      p      T_p  = |u0| + |k_u X|
      du     T_du = T_p + |q_u|
      d2     T_d2 = 2 (|du| T_du + |dv| T_dv) + d2
      s      T_s  = T_d2 + slack                                  (s = d2 - slack where d2 > slack, else 0 with T 0)
      e      T_e  = w (rho'(s) T_s + rho(s))
      term   T_t  = |g| w (2 rho'(s) T_du + 2 |du| |rho''(s)| T_s) + |term|     (a gradient term g w rho'(s) 2 du)
      dP     T    = the sum of its terms' T
      dverts T    = |k| T_dP;   dcam: sum (T_dP |X| + |dP| |X|) for the first two columns, sum T_dP for the last two.
The constants are the model's; nothing here was tuned to the kernels.
"""
import numpy as np

from _keypoint_oracle import ddrho, drho, rho, within  # noqa: F401  (the robust function and the bar are the keypoint term's)

NONFINITE = 1
BLOCK = 1 << 22        # entries of the largest (vertices, pixels) block


def points(W, flip_rows=True):
    """(W W, 2) float64: the point of every stored pixel by stored index r W + c: (c, W - 1 - r), or (c, r)."""
    q = np.arange(W * W)
    r, c = q // W, q % W
    return np.stack([c, W - 1 - r if flip_rows else r], 1).astype(np.float64)


def prep(labels, C):
    """One image: off (C + 1), pix (W W): the stored indices sorted by class, stably; -1 beyond off[C]."""
    lab = np.asarray(labels).reshape(-1).astype(np.int64)
    key = np.where((lab >= 0) & (lab < C), lab, C)
    order = np.argsort(key, kind="stable")
    n = int((key < C).sum())
    pix = np.where(np.arange(len(lab)) < n, order, -1).astype(np.int32)
    off = np.concatenate([[0], np.cumsum(np.bincount(key, minlength=C + 1)[:C])]).astype(np.int32)
    return off, pix


def forward(verts, cam, labels, vclass, C, vweight=None, sigma=None, slack=0.5, flip_rows=True):
    """One row: verts (V, 3), cam (4,), labels (W, W) integers, vclass (V,), vweight (V,) or None -> dict of near_pix, d2_v,
    e_m2i (V,), near_vert, d2_p, e_i2m (W W,), proj (V, 2), status, the T of each float, `ties` (how many winners had an
    equal runner-up, per direction) and `margin` (the smallest gap between a winner and its runner-up)."""
    verts, cam = np.asarray(verts, np.float64), np.asarray(cam, np.float64)
    V, lab = len(verts), np.asarray(labels).reshape(-1).astype(np.int64)
    W = int(round(np.sqrt(len(lab))))
    N, sl = W * W, float(np.float32(slack))
    vclass = np.asarray(vclass).astype(np.int64)
    w = np.ones(V) if vweight is None else np.asarray(vweight, np.float64)
    pts = points(W, flip_rows)
    with np.errstate(all="ignore"):
        counted = (vclass >= 1) & (vclass < C) & (w > 0)
        X, Y = verts[:, 0], verts[:, 1]
        p = np.stack([cam[2] + cam[0] * X, cam[3] + cam[1] * Y], 1)
        Tp = np.stack([abs(cam[2]) + np.abs(cam[0] * X), abs(cam[3]) + np.abs(cam[1] * Y)], 1)
        bad = (not np.isfinite(cam).all()) or bool((counted & ~(np.isfinite(X) & np.isfinite(Y))).any())
    out = dict(near_pix=np.full(V, -1, np.int32), near_vert=np.full(N, -1, np.int32), d2_v=np.full(V, np.inf),
               d2_p=np.full(N, np.inf), e_m2i=np.zeros(V), e_i2m=np.zeros(N), T_e_m2i=np.zeros(V), T_e_i2m=np.zeros(N),
               T_d2_v=np.zeros(V), T_d2_p=np.zeros(N), proj=p, T_proj=Tp, status=NONFINITE if bad else 0, counted=counted,
               w=w, ties=[0, 0], margin=np.inf, W=W, flip_rows=flip_rows, slack=sl, sigma=sigma)
    if bad:
        for n in ("d2_v", "d2_p", "e_m2i", "e_i2m", "proj"):
            out[n] = np.full_like(out[n], np.nan)
        return out

    def runner_up(d2, axis):
        if d2.shape[axis] < 2:
            return
        two = np.partition(d2, 1, axis=axis)
        gap = np.take(two, 1, axis=axis) - np.take(two, 0, axis=axis)
        out["margin"] = min(out["margin"], float(gap.min()))
        return int((gap == 0).sum())

    for c in range(1, C):
        vi, qi = np.nonzero(counted & (vclass == c))[0], np.nonzero(lab == c)[0]
        if not len(vi) or not len(qi):
            continue
        step = max(1, BLOCK // len(qi))
        best_q = np.full(len(qi), np.inf)
        for v0 in range(0, len(vi), step):
            vv = vi[v0:v0 + step]
            du, dv = p[vv, 0, None] - pts[qi, 0][None], p[vv, 1, None] - pts[qi, 1][None]
            d2 = du * du + dv * dv
            j = d2.argmin(1)                                            # (the first of equal minima: the lower stored index)
            out["near_pix"][vv], out["d2_v"][vv] = qi[j], d2[np.arange(len(vv)), j]
            out["ties"][0] += runner_up(d2, 1) or 0
            k = d2.argmin(0)                                            # (vertices in increasing index, chunk after chunk)
            m = d2[k, np.arange(len(qi))]
            better = m < best_q
            out["near_vert"][qi[better]], best_q[better] = vv[k[better]], m[better]
        out["d2_p"][qi] = best_q
        if len(vi) <= step:
            out["ties"][1] += runner_up(d2, 0) or 0
    _energies(out, p, Tp, pts)
    return out


def _residual(out, p, Tp, pts, side):
    """du (n, 2), its T, d2, T_d2, s, T_s and the mask of entries with a winner, for "v" (vertices) or "p" (pixels)."""
    if side == "v":
        has = out["near_pix"] >= 0
        q = pts[np.maximum(out["near_pix"], 0)]
        du, Tdu = p - q, Tp + np.abs(q)
    else:
        has = out["near_vert"] >= 0
        i = np.maximum(out["near_vert"], 0)
        du, Tdu = p[i] - pts, Tp[i] + np.abs(pts)
    d2 = (du * du).sum(1)
    Td2 = 2.0 * (np.abs(du) * Tdu).sum(1) + d2
    far = has & (d2 > out["slack"])
    s, Ts = np.where(far, d2 - out["slack"], 0.0), np.where(far, Td2 + out["slack"], 0.0)
    return du, Tdu, d2, Td2, s, Ts, has, far


def _energies(out, p, Tp, pts):
    sg = out["sigma"]
    for side, e, w in (("v", "e_m2i", out["w"]), ("p", "e_i2m", 1.0)):
        du, Tdu, d2, Td2, s, Ts, has, far = _residual(out, p, Tp, pts, side)
        assert np.array_equal(np.where(has, d2, np.inf), out["d2_" + side])
        out["T_d2_" + side] = np.where(has, Td2, 0.0)
        out[e] = np.where(has, w * rho(s, sg), 0.0)
        out["T_" + e] = np.where(has, w * (drho(s, sg) * Ts + rho(s, sg)), 0.0)


def grads(fwd, verts, cam, g_v=None, g_p=None):
    """The closed-form gradient of sum g_v e_m2i + sum g_p e_i2m for one row whose status is 0, from `forward`'s dict ->
    dict of dverts (V, 3), dcam (4,) and their T."""
    verts, cam = np.asarray(verts, np.float64), np.asarray(cam, np.float64)
    V, sg = len(verts), fwd["sigma"]
    pts = points(fwd["W"], fwd["flip_rows"])
    with np.errstate(all="ignore"):
        p = np.stack([cam[2] + cam[0] * verts[:, 0], cam[3] + cam[1] * verts[:, 1]], 1)
        Tp = np.stack([abs(cam[2]) + np.abs(cam[0] * verts[:, 0]), abs(cam[3]) + np.abs(cam[1] * verts[:, 1])], 1)
    p, Tp = np.where(fwd["counted"][:, None], p, 0.0), np.where(fwd["counted"][:, None], Tp, 0.0)
    dP, TdP = np.zeros((V, 2)), np.zeros((V, 2))

    def terms(side, g, w):
        du, Tdu, d2, Td2, s, Ts, has, far = _residual(fwd, p, Tp, pts, side)
        cf = np.where(far, g * w * drho(s, sg), 0.0)
        t = cf[:, None] * (2.0 * du)
        Tt = np.where(far[:, None], (np.abs(g) * w)[:, None] * (2.0 * drho(s, sg)[:, None] * Tdu
                                                              + 2.0 * np.abs(du) * (np.abs(ddrho(s, sg)) * Ts)[:, None]) + np.abs(t), 0.0)
        return t, Tt, far
    if g_v is not None:                                                 # the own term first ...
        t, Tt, _ = terms("v", np.asarray(g_v, np.float64).reshape(-1), fwd["w"])
        dP, TdP = dP + t, TdP + Tt
    if g_p is not None:                                                 # ... then the pixels in increasing stored index
        t, Tt, far = terms("p", np.asarray(g_p, np.float64).reshape(-1), np.ones(len(pts)))
        i = fwd["near_vert"][far]
        np.add.at(dP, i, t[far])
        np.add.at(TdP, i, Tt[far])
    k = cam[None, :2]
    XY = np.where(fwd["counted"][:, None], verts[:, :2], 0.0)
    zeros = np.zeros((V, 1))
    return dict(dverts=np.concatenate([dP * k, zeros], 1), T_dverts=np.concatenate([TdP * np.abs(k) + np.abs(dP * k), zeros], 1),
                dcam=np.concatenate([(dP * XY).sum(0), dP.sum(0)]),
                T_dcam=np.concatenate([(TdP * np.abs(XY) + np.abs(dP * XY)).sum(0), (TdP + np.abs(dP)).sum(0)]), dP=dP)
