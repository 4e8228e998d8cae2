"""Float64 NumPy restatement of the four alignment modes of `ilps_amd.eval3d` (np.linalg.svd), mesh by mesh, and the
recipe the parity tests draw their point sets from.

    none         |p - g|
    translation  centroids removed (or each set's point `root`)
    scale        centroids removed, s = sum pc.gc / sum |pc|^2
    similarity   M = sum gc pc^T = U S V^T, d = sign(det U det V), R = U diag(1, 1, d) V^T, s = (S1 + S2 + d S3) / sum |pc|^2,
                 t = mean g - s R mean p
`gap` = (S2 + d S3) / S1 measures how well R is determined: the rotation about the first singular direction is fixed by
the second and third pairs only, and a perturbation E of M turns R by about |E| / (S1 gap)."""
import numpy as np

MODES = ("none", "translation", "scale", "similarity")


def align_one(p, g, root=None):
    """p, g (N, 3) -> dict(per_point (4, N), mean (4,), s2, s, R (3, 3), t (3,), gap, degenerate)."""
    p = np.asarray(p, np.float64)
    g = np.asarray(g, np.float64)
    N = p.shape[0]
    mp, mg = p.mean(0), g.mean(0)
    pc, gc = p - mp, g - mg
    spp = float((pc * pc).sum())
    M = gc.T @ pc
    U, S, Vt = np.linalg.svd(M)
    d = -1.0 if np.linalg.det(U) * np.linalg.det(Vt) < 0 else 1.0
    degenerate = spp == 0.0 or N == 1
    if degenerate:
        s2, s, R = 1.0, 1.0, np.eye(3)
    else:
        R = U @ np.diag([1.0, 1.0, d]) @ Vt
        s2 = np.trace(M) / spp
        s = (S[0] + S[1] + d * S[2]) / spp
    t = mg - s * R @ mp
    if root is None or root < 0:
        e1 = pc - gc
    else:
        e1 = (p - p[root]) - (g - g[root])
    per = np.stack([np.linalg.norm(p - g, axis=1), np.linalg.norm(e1, axis=1), np.linalg.norm(s2 * pc - gc, axis=1),
                    np.linalg.norm(s * pc @ R.T - gc, axis=1)])
    gap = (S[1] + d * S[2]) / S[0] if S[0] > 0 else 0.0
    return {"per_point": per, "mean": per.mean(1), "s2": s2, "s": s, "R": R, "t": t, "gap": gap, "degenerate": degenerate,
            "sing": S, "d": d}


def align(pred, gt, root=None):
    """pred, gt (B, N, 3) -> dict of stacked results: per_point (B, 4, N), mean (B, 4), s (B,), R (B, 3, 3), t (B, 3), gap (B,)."""
    rs = [align_one(p, g, root) for p, g in zip(pred, gt)]
    return {k: np.stack([np.asarray(r[k]) for r in rs]) for k in ("per_point", "mean", "s2", "s", "R", "t", "gap", "d")}


def random_rotation(rng):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def make_case(B, N, seed):
    """The parity recipe: gt a body-sized cloud whose covariance is exactly diag(0.3, 0.6, 0.15 m)^2 in a random frame (a
    whitened Gaussian sample, so that a 14-point set is as well conditioned as a 6 890-point one: gap ~0.31, mirrored
    ~0.19), pred a random similarity transform of it (scale 0.5-2, any rotation) plus Gaussian noise (1-3 cm) and a
    translation.  Every third mesh (index % 3 == 1) is
    mirrored first, so its cross-covariance has a negative determinant (the reflection branch); every third (index % 3 == 2)
    sits 5-10 m down the optical axis.  -> pred, gt (B, N, 3) float32."""
    rng = np.random.default_rng(seed)
    pred = np.empty((B, N, 3), np.float32)
    gt = np.empty((B, N, 3), np.float32)
    for b in range(B):
        q, _ = np.linalg.qr(rng.normal(size=(N, 3)) - rng.normal(size=(N, 3)).mean(0))
        q = (q - q.mean(0)) * np.sqrt(N)
        q, _ = np.linalg.qr(q)
        g = (q * np.sqrt(N) * np.array([0.3, 0.6, 0.15])) @ random_rotation(rng).T + rng.normal(size=3) * 0.3
        src = g.copy()
        if b % 3 == 1:
            src[:, 0] = -src[:, 0]
        s = rng.uniform(0.5, 2.0)
        R = random_rotation(rng)
        p = s * src @ R.T + rng.normal(size=(N, 3)) * rng.uniform(0.01, 0.03) + rng.normal(size=3) * 0.5
        if b % 3 == 2:
            depth = np.array([0.0, 0.0, rng.uniform(5.0, 10.0)])
            g = g + depth
            p = p + depth
        pred[b], gt[b] = p, g
    return pred, gt
