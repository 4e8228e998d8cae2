"""Float64 NumPy statements of the probabilistic head (ilps_amd/prob.py, csrc/prob.hip), written from the definitions: the
samples and the likelihood with their backward passes, the fusion of a group's Gaussians and the statistics of sampled
points.  Every function also returns the magnitude sums a test's bar is relative to: the sum of the absolute values of what
the definition adds up for that output."""
import numpy as np

NONFINITE = 1


def drawn_mask(S, D, stochastic=None, mean_first=False):
    """(S, D) bool: which entries of a row are drawn."""
    m = np.ones((S, D), bool) if stochastic is None else np.broadcast_to(np.asarray(stochastic).astype(bool), (S, D)).copy()
    if mean_first:
        m[0] = False
    return m


def samples(mu, s, eps, stochastic=None, mean_first=False):
    """-> x (B, S, D) float64 (unrounded), status (B,), mag (B, S, D) = |mu| + |sigma eps| (|mu| where not drawn)."""
    mu, s, eps = (np.asarray(a, np.float64) for a in (mu, s, eps))
    B, S, D = eps.shape
    m = drawn_mask(S, D, stochastic, mean_first)
    with np.errstate(all="ignore"):
        sig = np.exp(0.5 * s)
        e = np.where(m, eps, 0.0)
        x = np.where(m, mu[:, None] + sig[:, None] * e, mu[:, None] + 0 * e)
        mag = np.abs(mu)[:, None] + np.abs(sig[:, None] * e)
        bad = ~np.isfinite(mu).all(1) | ~np.isfinite(s).all(1) | ~np.isfinite(e).all((1, 2)) | \
            ~np.isfinite(x.astype(np.float32)).all((1, 2))
    x[bad] = np.nan
    return x, bad.astype(np.int32) * NONFINITE, mag


def samples_backward(s, eps, g, stochastic=None, mean_first=False, status=None):
    """-> dmu, ds (B, D) float64, mag_mu = sum_i |g|, mag_s = sigma / 2 sum_{drawn} |g eps|."""
    s, eps, g = (np.asarray(a, np.float64) for a in (s, eps, g))
    B, S, D = eps.shape
    m = drawn_mask(S, D, stochastic, mean_first)
    e = np.where(m, eps, 0.0)
    sig = np.exp(0.5 * s)
    dmu, ds = g.sum(1), 0.5 * sig * (g * e).sum(1)
    mag_mu, mag_s = np.abs(g).sum(1), 0.5 * sig * np.abs(g * e).sum(1)
    if status is not None:
        dmu[np.asarray(status) != 0] = np.nan
        ds[np.asarray(status) != 0] = np.nan
    return dmu, ds, mag_mu, mag_s


def _groups(groups, G):
    groups = np.asarray(groups, np.int64)
    assert groups.min() >= -1 and groups.max() < G
    return groups, np.array([(groups == k).sum() for k in range(G)])


def nll(mu, s, target, groups, G, row_w=None):
    """-> nll (B, G) float64, status (B,), mag (B, G) = w / (2 n) sum (|s| + r^2 exp(-s))."""
    mu, s, t = (np.asarray(a, np.float64) for a in (mu, s, target))
    B, D = mu.shape
    groups, n = _groups(groups, G)
    w = np.ones((B, G)) if row_w is None else np.asarray(row_w, np.float64)
    on = w > 0
    out, mag, bad = np.zeros((B, G)), np.zeros((B, G)), np.zeros(B, bool)
    with np.errstate(all="ignore"):
        for b in range(B):
            for k in range(G):
                c = groups == k
                if not on[b, k]:
                    continue
                if not (np.isfinite(mu[b, c]).all() and np.isfinite(s[b, c]).all() and np.isfinite(t[b, c]).all()
                        and np.isfinite(w[b, k])):
                    bad[b] = True
                    continue
                if n[k] == 0:
                    continue
                r2e = (t[b, c] - mu[b, c]) ** 2 * np.exp(-s[b, c])
                out[b, k] = w[b, k] * 0.5 / n[k] * (s[b, c] + r2e).sum()
                mag[b, k] = w[b, k] * 0.5 / n[k] * (np.abs(s[b, c]) + r2e).sum()
                bad[b] |= not np.isfinite(np.float32(out[b, k]))
    out[bad] = np.nan
    return out, bad.astype(np.int32) * NONFINITE, mag


def nll_backward(mu, s, target, groups, G, g, row_w=None, status=None):
    """-> dmu, ds (B, D) float64 and their magnitudes (ds adds two terms: |c| (1 + r^2 exp(-s)))."""
    mu, s, t, g = (np.asarray(a, np.float64) for a in (mu, s, target, g))
    B, D = mu.shape
    groups, n = _groups(groups, G)
    w = np.ones((B, G)) if row_w is None else np.asarray(row_w, np.float64)
    dmu, ds, mag_mu, mag_s = (np.zeros((B, D)) for _ in range(4))
    with np.errstate(all="ignore"):
        for d in range(D):
            k = groups[d]
            if k < 0:
                continue
            on = w[:, k] > 0
            c = np.where(on, g[:, k] * np.where(on, w[:, k], 0.0) / n[k], 0.0)
            e = np.exp(-np.where(on, s[:, d], 0.0))
            r = np.where(on, t[:, d] - mu[:, d], 0.0)
            dmu[:, d] = c * (-r) * e
            ds[:, d] = 0.5 * c * (1.0 - r * r * e)
            mag_mu[:, d] = np.abs(dmu[:, d])
            mag_s[:, d] = 0.5 * np.abs(c) * (1.0 + r * r * e)
    if status is not None:
        dmu[np.asarray(status) != 0] = np.nan
        ds[np.asarray(status) != 0] = np.nan
    return dmu, ds, mag_mu, mag_s


def fuse(mu, s, G):
    """-> mu_f, s_f (B / G, D) float64, status (B / G,), mag_mu = sum |mu_i| p_i / sum p_i, mag_s = |m| + |log sum p_i|."""
    mu, s = np.asarray(mu, np.float64), np.asarray(s, np.float64)
    B, D = mu.shape
    assert B % G == 0
    m3, s3 = mu.reshape(B // G, G, D), s.reshape(B // G, G, D)
    with np.errstate(all="ignore"):
        fin = np.isfinite(m3).all(1) & np.isfinite(s3).all(1)
        m = np.where(fin, s3.min(1), 0.0)
        p = np.exp(-(np.where(fin[:, None], s3, 0.0) - m[:, None]))
        den = p.sum(1)
        mu_f = (np.where(fin[:, None], m3, 0.0) * p).sum(1) / den
        s_f = m - np.log(den)
        mag_mu = (np.abs(np.where(fin[:, None], m3, 0.0)) * p).sum(1) / den
        mag_s = np.abs(m) + np.abs(np.log(den))
    mu_f[~fin] = np.nan
    s_f[~fin] = np.nan
    return mu_f, s_f, (~fin).any(1).astype(np.int32) * NONFINITE, mag_mu, mag_s


def spread(points, S):
    """-> mean (B, N, 3), rms (B, N) float64, status (B,), mag_mean = 1 / S sum |p|.  Two passes in float64 on the data shifted
    by sample 0 (exact in float64 for fp32 inputs): the definition, not the one-pass form the kernel uses."""
    p = np.asarray(points, np.float64)
    N = p.shape[1]
    p = p.reshape(-1, S, N, 3)
    with np.errstate(all="ignore"):
        fin = np.isfinite(p).all((1, 3))                                       # (B, N)
        q = np.where(fin[:, None, :, None], p, 0.0)
        d = q - q[:, :1]
        md = d.mean(1)
        mean = q[:, 0] + md
        rms = np.sqrt(np.maximum(((d - md[:, None]) ** 2).sum(-1).mean(1), 0.0))
        mag = np.abs(q).mean(1)
    if S == 1:
        mean, rms = q[:, 0].copy(), np.zeros_like(rms)
    mean[~fin] = np.nan
    rms[~fin] = np.nan
    return mean, rms, (~fin).any(1).astype(np.int32) * NONFINITE, mag
