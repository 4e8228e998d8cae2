"""Float64 NumPy restatement of the supervised 3D terms (ilps_amd/supervised.py, csrc/supervised.hip), one row at a time, from
the DENSE joint regressor R (K, S) - so it shares nothing with the CSR packing or the kernels' contraction of the Rodrigues
derivative: the five terms, the status and hand-written gradients (the derivative of R as an explicit 3 x 3 x 3 tensor), and
beside every output the number T that its rounding bar is made of.

The bar (tests/_keypoint_oracle.within, the package's bar for fp64-inside kernels):  |got - want| <= 2^-24 |want| + 2^-28 T.
T is the sum of the absolute values of the terms an output adds; for an output computed from such sums, the first-order
propagation of their T through the formula plus the output's own magnitude:
      d = a - b        T_d  = |a| + |b|
      d^2              T    = 2 |d| T_d + d^2
      d_k (joints)     T_dk = sum |w| (|source| + |source*|);  r_k = d_k - d_root: T_r = T_dk + T_droot
      R(theta)         f(|c|, |s|, |1 - c|) + a f(|s|, |c|, |s|), f the sum of the absolute values of the entry's three
                       summands: the second part carries a rounding of the angle a through cos and sin (derivatives swapped in)
      dR / dtheta      likewise over the summands of the derivative's formula
      dtheta_m         sum_ab |G_ab| T_dR_abm + T_G_ab |dR_abm|,  G = c_2 D, T_G = |c_2| T_D
      dverts           |c_0| (|v| + |v*|) + sum_k |w_ki| T_ddk;  dd_k = c_1 r_k: T = |c_1| T_r + |dd_k|, the root's the sum
The constants are the model's; nothing here was tuned to the kernels."""
import numpy as np

from _keypoint_oracle import within  # noqa: F401  (the bar)

NONFINITE = 1
EPS = 1e-8


def skew(v):
    return np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])


def _parts(theta):
    t = np.asarray(theta, np.float64)
    e = t + EPS
    a = np.sqrt((e * e).sum())
    return t, a, t / a, e / a


def rodrigues(theta):
    """theta (3,) -> R (3, 3), T_R (3, 3): oracle/np_oracle.batch_rodrigues for one joint."""
    t, a, r, u = _parts(theta)
    c, s = np.cos(a), np.sin(a)
    R = c * np.eye(3) + (1 - c) * np.outer(r, r) + s * skew(r)
    f = lambda cc, ss, mm: cc * np.eye(3) + mm * np.abs(np.outer(r, r)) + ss * np.abs(skew(r))
    return R, f(abs(c), abs(s), abs(1 - c)) + a * f(abs(s), abs(c), abs(s))


def rodrigues_jac(theta):
    """theta (3,) -> dR[a, b, m] = dR_ab / dtheta_m and its T, by the product rule on the formula: a' = u = (theta + eps) / a,
    r' = (I - r u^T) / a."""
    t, a, r, u = _parts(theta)
    c, s = np.cos(a), np.sin(a)
    dr = (np.eye(3) - np.outer(r, u)) / a                         # dr[i, m]
    Tdr = (np.eye(3) + np.abs(np.outer(r, u))) / a
    dR, TdR = np.zeros((3, 3, 3)), np.zeros((3, 3, 3))
    I, rr, K = np.eye(3), np.outer(r, r), skew(r)
    for m in range(3):
        dK, TdK = skew(dr[:, m]), np.abs(skew(Tdr[:, m]))
        drr = np.outer(dr[:, m], r) + np.outer(r, dr[:, m])
        Tdrr = np.outer(Tdr[:, m], np.abs(r)) + np.outer(np.abs(r), Tdr[:, m])
        dR[:, :, m] = -s * u[m] * I + s * u[m] * rr + (1 - c) * drr + c * u[m] * K + s * dK
        f = lambda cc, ss, mm: (ss * abs(u[m]) * (I + np.abs(rr)) + mm * Tdrr + cc * abs(u[m]) * np.abs(K) + ss * TdK)
        TdR[:, :, m] = f(abs(c), abs(s), abs(1 - c)) + a * f(abs(s), abs(c), abs(s))
    return dR, TdR


def _weights(row_w, K, num_cam):
    w = np.ones(5) if row_w is None else np.asarray(row_w, np.float64)
    with np.errstate(invalid="ignore"):
        on = w > 0
    wt = np.where(on, w, 0.0)
    wbad = bool((on & ~np.isfinite(w)).any())
    on = on.copy()
    if K == 0:
        on[1] = False
    if num_cam == 0:
        on[4] = False
    return wt, on, wbad


def forward(R, x, x_t, verts, verts_t, jtr=None, jtr_t=None, root=-1, row_w=None, cam_scale=None, num_cam=4):
    """One row: R (K, S) dense joint weights or None, x, x_t (>= num_cam + 82,), verts, verts_t (V, 3), jtr, jtr_t (24, 3) or
    None -> dict of terms (5,), T_terms, status and what `grads` needs."""
    f64 = lambda a: None if a is None else np.asarray(a, np.float64)
    x, x_t, verts, verts_t, jtr, jtr_t = (f64(a) for a in (x, x_t, verts, verts_t, jtr, jtr_t))
    V, nc = len(verts), int(num_cam)
    K = 0 if R is None else int(np.asarray(R).shape[0])
    wt, on, bad = _weights(row_w, K, nc)
    cs = np.ones(nc) if cam_scale is None else f64(cam_scale)
    terms, T = np.zeros(5), np.zeros(5)
    out = dict(on=on, wt=wt, V=V, K=K, nc=nc, root=int(root), cs=cs, x=x, x_t=x_t, verts=verts, verts_t=verts_t)
    with np.errstate(all="ignore"):
        if on[0]:
            d, Td = verts - verts_t, np.abs(verts) + np.abs(verts_t)
            bad |= not (np.isfinite(verts).all() and np.isfinite(verts_t).all())
            terms[0], T[0] = wt[0] * (d * d).sum() / V, wt[0] * (2 * np.abs(d) * Td + d * d).sum() / V
        if on[1]:
            src = verts if jtr is None else np.concatenate([verts, jtr])
            src_t = verts_t if jtr_t is None else np.concatenate([verts_t, jtr_t])
            Rd = np.asarray(R, np.float64)[:, :len(src)]
            dk, Tdk = np.zeros((K, 3)), np.zeros((K, 3))
            for k in range(K):
                nz = np.nonzero(Rd[k])[0]
                bad |= not (np.isfinite(src[nz]).all() and np.isfinite(src_t[nz]).all())
                dk[k] = (Rd[k, nz, None] * (src[nz] - src_t[nz])).sum(0)
                Tdk[k] = (np.abs(Rd[k, nz, None]) * (np.abs(src[nz]) + np.abs(src_t[nz]))).sum(0)
            r, Tr = (dk - dk[root], Tdk + Tdk[root]) if root >= 0 else (dk, Tdk)
            if root >= 0:
                r[root], Tr[root] = 0.0, 0.0
            terms[1], T[1] = wt[1] * (r * r).sum() / K, wt[1] * (2 * np.abs(r) * Tr + r * r).sum() / K
            out.update(r=r, T_r=Tr, Rd=Rd)
        if on[2]:
            th, th_t = x[nc:nc + 72].reshape(24, 3), x_t[nc:nc + 72].reshape(24, 3)
            bad |= not (np.isfinite(th).all() and np.isfinite(th_t).all())
            D, TD = np.zeros((24, 3, 3)), np.zeros((24, 3, 3))
            for j in range(24):
                (Rp, Tp), (Rt, Tt) = rodrigues(th[j]), rodrigues(th_t[j])
                D[j], TD[j] = Rp - Rt, Tp + Tt
            terms[2], T[2] = wt[2] * (D * D).sum() / 24, wt[2] * (2 * np.abs(D) * TD + D * D).sum() / 24
            out.update(D=D, T_D=TD)
        if on[3]:
            p, t = x[nc + 72:nc + 82], x_t[nc + 72:nc + 82]
            bad |= not (np.isfinite(p).all() and np.isfinite(t).all())
            d, Td = p - t, np.abs(p) + np.abs(t)
            terms[3], T[3] = wt[3] * (d * d).sum() / 10, wt[3] * (2 * np.abs(d) * Td + d * d).sum() / 10
        if on[4]:
            p, t = x[:nc], x_t[:nc]
            bad |= not (np.isfinite(p).all() and np.isfinite(t).all() and np.isfinite(cs).all())
            d, Td = cs * (p - t), np.abs(cs) * (np.abs(p) + np.abs(t))
            terms[4], T[4] = wt[4] * (d * d).sum() / nc, wt[4] * (2 * np.abs(d) * Td + d * d).sum() / nc
    if bad:
        terms = np.full(5, np.nan)
    out.update(terms=terms, T_terms=T, status=NONFINITE if bad else 0)
    return out


def grads(fwd, g, with_jtr=False):
    """The gradient of sum_t g_t terms_t for one row whose status is 0 -> dict of dverts (V, 3), djtr (24, 3) (with_jtr), dx
    (len(x),) and their T."""
    g = np.asarray(g, np.float64)
    on, wt, V, K, nc, root = (fwd[n] for n in ("on", "wt", "V", "K", "nc", "root"))
    x, x_t = fwd["x"], fwd["x_t"]
    S = V + (24 if with_jtr else 0)
    dsrc, Tsrc = np.zeros((S, 3)), np.zeros((S, 3))
    dx, Tdx = np.zeros(len(x)), np.zeros(len(x))
    if on[0]:
        c0 = g[0] * wt[0] * 2.0 / V
        dsrc[:V] += c0 * (fwd["verts"] - fwd["verts_t"])
        Tsrc[:V] += abs(c0) * (np.abs(fwd["verts"]) + np.abs(fwd["verts_t"]))
    if on[1]:
        c1 = g[1] * wt[1] * 2.0 / K
        dd = c1 * fwd["r"]
        Tdd = abs(c1) * fwd["T_r"] + np.abs(dd)
        if root >= 0:
            dd[root], Tdd[root] = -np.delete(dd, root, 0).sum(0), np.delete(Tdd, root, 0).sum(0)
        Rd = fwd["Rd"][:, :S]
        dsrc += Rd.T @ dd
        Tsrc += np.abs(Rd).T @ Tdd
    if on[2]:
        c2 = g[2] * wt[2] * 2.0 / 24
        th = x[nc:nc + 72].reshape(24, 3)
        for j in range(24):
            dR, TdR = rodrigues_jac(th[j])
            G, TG = c2 * fwd["D"][j], abs(c2) * fwd["T_D"][j]
            dx[nc + 3 * j:nc + 3 * j + 3] = np.einsum("ab,abm->m", G, dR)
            Tdx[nc + 3 * j:nc + 3 * j + 3] = np.einsum("ab,abm->m", np.abs(G), TdR) + np.einsum("ab,abm->m", TG, np.abs(dR))
    if on[3]:
        c3 = g[3] * wt[3] * 2.0 / 10
        p, t = x[nc + 72:nc + 82], x_t[nc + 72:nc + 82]
        dx[nc + 72:nc + 82], Tdx[nc + 72:nc + 82] = c3 * (p - t), abs(c3) * (np.abs(p) + np.abs(t))
    if on[4]:
        c4, cs = g[4] * wt[4] * 2.0 / nc, fwd["cs"]
        dx[:nc], Tdx[:nc] = c4 * cs * cs * (x[:nc] - x_t[:nc]), abs(c4) * cs * cs * (np.abs(x[:nc]) + np.abs(x_t[:nc]))
    out = dict(dverts=dsrc[:V], T_dverts=Tsrc[:V], dx=dx, T_dx=Tdx)
    if with_jtr:
        out.update(djtr=dsrc[V:], T_djtr=Tsrc[V:])
    return out
