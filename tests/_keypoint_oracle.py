"""Float64 NumPy restatement of the 2D keypoint term (ilps_amd/keypoints.py, csrc/keypoints.hip), one row at a time, from the
DENSE regressor R (K, S) - so it shares nothing with the CSR packing under test: joints, projection, energy, status and the
closed-form gradients, and beside every output the number T that its rounding bar is made of.

The bar (the rounding model of tests/test_gpu_measure.py, `check_bar`):  |got - want| <= 2^-24 |want| + 2^-28 T.
  * 2^-24 |want|: every output is rounded to fp32 once, half an ulp, at most 2^-24 relative.
  * 2^-28 T: the kernel's fp64 arithmetic before that rounding.  A sum of n products carries at most (n + 1) 2^-53 times the
    sum of the |terms| whatever the order (n <= 2^24 sources: below 2^-28); T is that sum of |terms| for a plain sum and, for
    an output computed from such sums, the first-order propagation of their T through the formula plus the output's own
    magnitude (each later operation adds 2^-53 of its operands):
      J      T_J  = sum |w| |x|                                  (per coordinate)
      p      T_p  = |u0| + |k_u| T_Jx                            (and v likewise)
      r      T_r  = T_p + |t|
      d2     T_d2 = 2 (|r_u| T_ru + |r_v| T_rv) + d2
      e      T_e  = conf (rho'(d2) T_d2 + rho(d2))               (0 for a joint that does not count)
      q      T_q  = |g| conf (2 rho'(d2) T_r + 2 |r| |rho''(d2)| T_d2) + |q|,   rho''(s) = -2 sigma^4 / (sigma^2 + s)^3 (or 0)
      dJ     T_dJ = |k| T_q
      dsrc   T    = sum_k |w_ki| T_dJk
      dcam   T    = sum_k (T_q |J| + |q| T_J)  for the first two columns,  sum_k T_q  for the last two.
    Every later operation's own 2^-53 is far inside the factor 2^25 between 2^-53 and 2^-28.
The constants are the model's; nothing here was tuned to the kernels.
"""
import numpy as np

NONFINITE = 1


def within(got, ref, T, rel=2.0 ** -24, absT=2.0 ** -28):
    """The bar, elementwise -> (ok, worst ratio of error to bar)."""
    got, ref, T = (np.asarray(a, np.float64) for a in (got, ref, T))
    bar = rel * np.abs(ref) + absT * T
    err = np.abs(got - ref)
    ratio = np.where(err == 0, 0.0, err / np.where(bar > 0, bar, np.finfo(np.float64).tiny))
    return bool((err <= bar).all()), float(ratio.max()) if ratio.size else 0.0


def rho(s, sigma):
    if sigma is None:
        return s
    s2 = float(np.float32(sigma)) ** 2
    return s2 * s / (s2 + s)


def drho(s, sigma):
    if sigma is None:
        return np.ones_like(s)
    s2 = float(np.float32(sigma)) ** 2
    return s2 * s2 / (s2 + s) ** 2


def ddrho(s, sigma):
    if sigma is None:
        return np.zeros_like(s)
    s2 = float(np.float32(sigma)) ** 2
    return -2.0 * s2 * s2 / (s2 + s) ** 3


def forward(R, verts, cam, target, conf, sigma=None, jtr=None):
    """One row: R (K, S) weights, verts (V, 3), cam (4,), target (K, 2), conf (K,), jtr (24, 3) or None (all as float32 or
    float64 arrays; the arithmetic is float64) -> dict of J, proj, r, d2, e, counted, status and the T of each."""
    src = np.asarray(verts, np.float64) if jtr is None else np.concatenate([np.asarray(verts, np.float64), np.asarray(jtr, np.float64)])
    R = np.asarray(R, np.float64)[:, :len(src)]
    cam, target, conf = (np.asarray(a, np.float64) for a in (cam, target, conf))
    K = R.shape[0]
    J, TJ, jbad = np.zeros((K, 3)), np.zeros((K, 3)), np.zeros(K, bool)
    with np.errstate(all="ignore"):
        for k in range(K):
            nz = np.nonzero(R[k])[0]
            terms = R[k, nz, None] * src[nz]
            jbad[k] = not np.isfinite(src[nz]).all()
            J[k], TJ[k] = terms.sum(0), np.abs(terms).sum(0)
        counted = conf > 0
        p = np.stack([cam[2] + cam[0] * J[:, 0], cam[3] + cam[1] * J[:, 1]], 1)
        Tp = np.stack([abs(cam[2]) + abs(cam[0]) * TJ[:, 0], abs(cam[3]) + abs(cam[1]) * TJ[:, 1]], 1)
        r = p - target
        Tr = Tp + np.abs(target)
        d2 = (r * r).sum(1)
        Td2 = 2.0 * (np.abs(r) * Tr).sum(1) + d2
        e = np.where(counted, conf * rho(d2, sigma), 0.0)
        Te = np.where(counted, conf * (drho(d2, sigma) * Td2 + rho(d2, sigma)), 0.0)
    bad = (not np.isfinite(cam).all()) or bool((counted & (jbad | ~np.isfinite(target).all(1))).any())
    out = dict(J=J, T_J=TJ, proj=p, T_proj=Tp, r=r, T_r=Tr, d2=d2, T_d2=Td2, e=e, T_e=Te, counted=counted,
               status=NONFINITE if bad else 0)
    if bad:
        for n in ("J", "proj", "d2", "e"):
            out[n] = np.full_like(out[n], np.nan)
    return out


def grads(R, fwd, cam, conf, g, sigma=None):
    """The closed-form gradient of sum_k g_k e_k for one row whose status is 0, from `forward`'s dict -> dict of dsrc (S, 3),
    dcam (4,) and their T."""
    R = np.asarray(R, np.float64)
    cam, conf, g = (np.asarray(a, np.float64) for a in (cam, conf, g))
    counted, r, d2 = fwd["counted"], fwd["r"], fwd["d2"]
    J = fwd["J"] if fwd["status"] == 0 else np.zeros_like(fwd["T_J"])
    with np.errstate(all="ignore"):
        c = g * conf * drho(d2, sigma)
        q = np.where(counted[:, None], c[:, None] * 2.0 * r, 0.0)
        Tq = np.where(counted[:, None], (np.abs(g) * conf)[:, None] * (2.0 * drho(d2, sigma)[:, None] * fwd["T_r"]
                                                                      + 2.0 * np.abs(r) * (np.abs(ddrho(d2, sigma)) * fwd["T_d2"])[:, None])
                      + np.abs(q), 0.0)
    k = cam[None, :2]
    dJ = np.concatenate([q * k, np.zeros((len(q), 1))], 1)
    TdJ = np.concatenate([Tq * np.abs(k), np.zeros((len(q), 1))], 1)
    Jc = np.where(counted[:, None], J[:, :2], 0.0)
    TJc = np.where(counted[:, None], fwd["T_J"][:, :2], 0.0)
    dcam = np.concatenate([(q * Jc).sum(0), q.sum(0)])
    Tdcam = np.concatenate([(Tq * np.abs(Jc) + np.abs(q) * TJc).sum(0), Tq.sum(0)])
    return dict(dsrc=R.T @ dJ, T_dsrc=np.abs(R).T @ TdJ, dcam=dcam, T_dcam=Tdcam, q=q)
