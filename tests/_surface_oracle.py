"""Float64 NumPy restatement of the dense surface-correspondence term (ilps_amd/surface.py, csrc/surface.hip), one row at a
time and in the CALLER's order, from a DENSE (N, V) weight matrix assembled from `faces` and `bary` - so it shares nothing with
the sorting, the row CSRs or the vertex -> (face, corner) lists under test: points, residuals, energy, status and the
closed-form gradients, and beside every output the number T that its rounding bar is made of.

The bar is the one of tests/_keypoint_oracle.py (`within` is that file's):  |got - want| <= 2^-24 |want| + 2^-28 T.
  * 2^-24 |want|: every output is rounded to fp32 once, half an ulp, at most 2^-24 relative.
  * 2^-28 T: the kernel's fp64 arithmetic before that rounding.  A sum of n products carries at most (n + 1) 2^-53 times the
    sum of the |terms| whatever the order (n <= 3 * 65 536 terms per vertex: far below 2^-28); T is that sum of |terms| for a
    plain sum and, for an output computed from such sums, the first-order propagation of their T through the formula plus the
    output's own magnitude (each later operation adds 2^-53 of its operands), exactly as that file's docstring does:
      P      T_P  = sum_c |bary_c| |x_c|                         (per coordinate; A |x| with A the matrix of |bary|)
      p      T_p  = |u0| + |k_u| T_Px  (and v likewise; D = 2)   r      T_r  = T_p + |t|   (D = 3: T_P + |t|)
      d2     T_d2 = 2 sum |r| T_r + d2
      e      T_e  = conf (rho'(d2) T_d2 + rho(d2))               (0 for a correspondence that does not count)
      q      T_q  = |g| conf (2 rho'(d2) T_r + 2 |r| |rho''(d2)| T_d2) + |q|
      dP     T_dP = |k| T_q (D = 2), T_q (D = 3)
      dverts T    = sum over (n, c) on the vertex of |bary| T_dP  (A^T T_dP)
      dcam   T    = sum_n (T_q |P| + |q| T_P)  for the first two columns,  sum_n T_q  for the last two.
The constants are the model's; nothing here was tuned to the kernels.
A correspondence counts iff 0 <= face < F and conf > 0; one that does not count has e = d2 = point = 0 (T = 0) and no gradient.
status = NONFINITE when a counted correspondence has a non-finite coordinate among its face's three vertices, a non-finite
weight or target, or (D = 2) a cam column is non-finite; then e, d2 and point are NaN.
"""
import numpy as np

from _keypoint_oracle import ddrho, drho, rho, within  # noqa: F401  (`within`: the bar, reused)

NONFINITE = 1


def weights(faces, face, bary, counted, V):
    """-> (Wm, A) dense (N, V): Wm[n, i] = the sum of bary[n, c] over the corners c of face[n] that are vertex i, A the same
    sum of |bary|; rows that do not count are zero."""
    N = len(face)
    Wm, A = np.zeros((N, V)), np.zeros((N, V))
    rows = np.nonzero(counted)[0]
    for c in range(3):
        cols = faces[face[rows], c]
        np.add.at(Wm, (rows, cols), bary[rows, c])
        np.add.at(A, (rows, cols), np.abs(bary[rows, c]))
    return Wm, A


def forward(faces, verts, cam, face, bary, target, conf, sigma=None):
    """One row: faces (F, 3) ints, verts (V, 3), cam (4,) or None (D = 3), face (N,), bary (N, 3), target (N, D), conf (N,)
    (float32 or float64 arrays; the arithmetic is float64) -> dict of point, r, d2, e, counted, status, the matrices and the
    T of each."""
    faces, face = np.asarray(faces, np.int64), np.asarray(face, np.int64)
    verts, bary, target, conf = (np.asarray(a, np.float64) for a in (verts, bary, target, conf))
    F, V, D = len(faces), len(verts), target.shape[1]
    counted = (face >= 0) & (face < F) & (conf > 0)
    rows = np.nonzero(counted)[0]
    bad = False
    if D == 2:
        cam = np.asarray(cam, np.float64)
        bad = not np.isfinite(cam).all()
    if len(rows):
        bad = bad or not (np.isfinite(verts[faces[face[rows]]]).all() and np.isfinite(bary[rows]).all() and np.isfinite(target[rows]).all())
    with np.errstate(all="ignore"):
        Wm, A = weights(faces, face, np.where(counted[:, None], bary, 0.0), counted, V)
        vz = np.where(np.isfinite(verts), verts, 0.0)             # (a NaN no counted correspondence touches does not matter)
        P, TP = Wm @ vz, A @ np.abs(vz)
        t = np.where(counted[:, None], target, 0.0)
        if D == 2:
            r = np.stack([cam[2] + cam[0] * P[:, 0], cam[3] + cam[1] * P[:, 1]], 1) - t
            Tr = np.stack([abs(cam[2]) + abs(cam[0]) * TP[:, 0], abs(cam[3]) + abs(cam[1]) * TP[:, 1]], 1) + np.abs(t)
        else:
            r, Tr = P - t, TP + np.abs(t)
        d2 = (r * r).sum(1)
        Td2 = 2.0 * (np.abs(r) * Tr).sum(1) + d2
        e = np.where(counted, conf * rho(d2, sigma), 0.0)
        Te = np.where(counted, conf * (drho(d2, sigma) * Td2 + rho(d2, sigma)), 0.0)
        d2, Td2 = np.where(counted, d2, 0.0), np.where(counted, Td2, 0.0)
        P, TP = np.where(counted[:, None], P, 0.0), np.where(counted[:, None], TP, 0.0)
    out = dict(point=P, T_point=TP, r=r, T_r=Tr, d2=d2, T_d2=Td2, e=e, T_e=Te, counted=counted, W=Wm, A=A,
               status=NONFINITE if bad else 0)
    if bad:
        for n in ("point", "d2", "e"):
            out[n] = np.full_like(out[n], np.nan)
    return out


def grads(fwd, cam, conf, g, sigma=None):
    """The closed-form gradient of sum_n g_n e_n for one row whose status is 0, from `forward`'s dict -> dict of dverts
    (V, 3), dcam (4,) or None (D = 3) and their T."""
    conf, g = np.asarray(conf, np.float64), np.asarray(g, np.float64)
    counted, r, d2, D = fwd["counted"], fwd["r"], fwd["d2"], fwd["r"].shape[1]
    with np.errstate(all="ignore"):
        c = g * conf * drho(d2, sigma)
        q = np.where(counted[:, None], c[:, None] * 2.0 * r, 0.0)
        Tq = np.where(counted[:, None], (np.abs(g) * conf)[:, None] * (2.0 * drho(d2, sigma)[:, None] * fwd["T_r"]
                                                                      + 2.0 * np.abs(r) * (np.abs(ddrho(d2, sigma)) * fwd["T_d2"])[:, None])
                      + np.abs(q), 0.0)
    if D == 2:
        k = np.asarray(cam, np.float64)[None, :2]
        dP = np.concatenate([q * k, np.zeros((len(q), 1))], 1)
        TdP = np.concatenate([Tq * np.abs(k), np.zeros((len(q), 1))], 1)
        P, TP = fwd["point"][:, :2], fwd["T_point"][:, :2]
        dcam = np.concatenate([(q * P).sum(0), q.sum(0)])
        Tdcam = np.concatenate([(Tq * np.abs(P) + np.abs(q) * TP).sum(0), Tq.sum(0)])
    else:
        dP, TdP, dcam, Tdcam = q, Tq, None, None
    return dict(dverts=fwd["W"].T @ dP, T_dverts=fwd["A"].T @ TdP, dcam=dcam, T_dcam=Tdcam, q=q)
