"""NumPy float64 restatement of the pose and shape priors (csrc/prior_device.h; the semantics block of ilps_amd/fitting.py).

Inputs are what the kernel gets - fp32 arrays - cast up; every operation after that is float64.  Nothing here is shared with
the code under test.  Beside every value the cancellation-free magnitude the tests' bars are relative to is returned: the sum
of the absolute values of the terms the value is made of."""
import numpy as np

D = 69


def up(a):
    return np.asarray(a, np.float32).astype(np.float64)


def make_prior(K, A, seed, mean_pose, repeat=True, dense=False):
    """The seeded recipe of the GPU tests: mean = mean_pose[3:] + N(0, 0.3^2); A_k upper-triangular with diagonal U[2, 6] and
    off-diagonal N(0, 0.3^2); c ~ U[0, 3]; A angle terms on distinct theta indices in 3..71 (the last one repeats the first
    when repeat and A >= 2) with scales U[-2, 2]; shape_mean ~ N(0, 0.5^2); dense: N(0, 0.3^2) below the diagonal as well (the
    kernel treats A_k as dense).  -> dict of fp32 / int32 arrays."""
    rng = np.random.default_rng(seed)
    mean = np.asarray(mean_pose, np.float64)[None, 3:] + rng.normal(0.0, 0.3, (K, D))
    factor = np.triu(rng.normal(0.0, 0.3, (K, D, D)), 1)
    for k in range(K):
        factor[k][np.diag_indices(D)] = rng.uniform(2.0, 6.0, D)
    if dense:
        factor += np.tril(np.random.default_rng(seed + 500).normal(0.0, 0.3, (K, D, D)), -1)
    idx = rng.choice(np.arange(3, 72), A, replace=False) if A else np.zeros(0, np.int64)
    if repeat and A >= 2:
        idx[-1] = idx[0]
    return dict(mean=mean.astype(np.float32), factor=factor.astype(np.float32), offset=rng.uniform(0.0, 3.0, K).astype(np.float32),
                angle_idx=idx.astype(np.int32), angle_scale=rng.uniform(-2.0, 2.0, A).astype(np.float32),
                shape_mean=rng.normal(0.0, 0.5, 10).astype(np.float32))


def make_rows(prior, B, num_cam, seed):
    """x (B, num_cam + 82) fp32: theta' = mean[random k] + N(0, 0.1^2), the rest N(0, 1) (camera columns N(24, 5^2))."""
    rng = np.random.default_rng(seed + 1000)
    K = prior["mean"].shape[0]
    x = rng.normal(0.0, 1.0, (B, num_cam + 82))
    x[:, :num_cam] = rng.normal(24.0, 5.0, (B, num_cam))
    x[:, num_cam:num_cam + 3] = rng.normal(0.0, 1.0, (B, 3))
    ks = rng.integers(0, K, B)
    x[:, num_cam + 3:num_cam + 72] = prior["mean"][ks].astype(np.float64) + rng.normal(0.0, 0.1, (B, D))
    return x.astype(np.float32)


def prior(x, num_cam, p, weights):
    """-> dict(E_pose, E_angle, E_shape, E (B,), comp (B,) int, grad (B, P), gap (B,): the relative gap between the lowest
    and the second-lowest component energy (inf for K = 1), and *_mag: the magnitudes of E_pose, E_angle, E_shape, E, grad)."""
    x = up(x)
    B, P = x.shape
    assert P == num_cam + 82
    mean, fac, off = up(p["mean"]), up(p["factor"]), up(p["offset"])
    idx, sc, smean = np.asarray(p["angle_idx"], np.int64), up(p["angle_scale"]), up(p["shape_mean"])
    wp, wa, ws = (float(w) for w in up(weights))
    K = mean.shape[0]
    out = {k: np.zeros(B) for k in ("E_pose", "E_angle", "E_shape", "E", "E_pose_mag", "E_angle_mag", "E_shape_mag", "E_mag")}
    out["comp"] = np.zeros(B, np.int64)
    out["gap"] = np.full(B, np.inf)
    out["grad"] = np.zeros((B, P))
    out["grad_mag"] = np.zeros((B, P))
    with np.errstate(all="ignore"):
        for b in range(B):
            th, beta = x[b, num_cam:num_cam + 72], x[b, num_cam + 72:]
            g, gm = np.zeros(P), np.zeros(P)
            if wp != 0.0:
                d = th[None, 3:] - mean                                        # (K, 69)
                y = np.einsum("kij,kj->ki", fac, d)
                ymag = np.einsum("kij,kj->ki", np.abs(fac), np.abs(d))
                Ek = 0.5 * (y * y).sum(1) + off
                ks = 0
                for k in range(1, K):
                    if Ek[k] < Ek[ks]:
                        ks = k
                if K > 1 and np.all(np.isfinite(Ek)):
                    two = np.sort(Ek)[:2]
                    out["gap"][b] = (two[1] - two[0]) / max(abs(two[0]), 1e-300)
                out["comp"][b] = ks
                out["E_pose"][b] = Ek[ks]
                out["E_pose_mag"][b] = 0.5 * (ymag[ks] * ymag[ks]).sum() + off[ks]
                g[num_cam + 3:num_cam + 72] += wp * (fac[ks].T @ y[ks])
                gm[num_cam + 3:num_cam + 72] += wp * (np.abs(fac[ks]).T @ ymag[ks])
                out["E"][b] += wp * out["E_pose"][b]
                out["E_mag"][b] += wp * out["E_pose_mag"][b]
            if wa != 0.0:
                Ea = 0.0
                for a in range(idx.size):
                    if not 0 <= idx[a] < 72:
                        continue
                    e = np.exp(sc[a] * th[idx[a]])
                    Ea += e
                    g[num_cam + idx[a]] += wa * sc[a] * e
                    gm[num_cam + idx[a]] += wa * abs(sc[a]) * e
                out["E_angle"][b] = out["E_angle_mag"][b] = Ea
                out["E"][b] += wa * Ea
                out["E_mag"][b] += wa * Ea
            if ws != 0.0:
                r = beta - smean
                out["E_shape"][b] = out["E_shape_mag"][b] = (r * r).sum()
                rm = np.abs(beta) + np.abs(smean)
                g[num_cam + 72:] += ws * 2.0 * r
                gm[num_cam + 72:] += ws * 2.0 * rm
                out["E"][b] += ws * out["E_shape"][b]
                out["E_mag"][b] += ws * out["E_shape"][b]
            out["grad"][b], out["grad_mag"][b] = g, gm
    return out
