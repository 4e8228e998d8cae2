"""NumPy float64 restatement of one smplr_fit_step_group call (csrc/fit.hip fit_group_kernel; the semantics a - h of
ilps_amd/fitting.py): rows in groups of G consecutive rows, tied columns, a first-difference penalty between the rows of a group.

Inputs are what the kernel gets - fp32 arrays and fp32 scalars - cast up; every operation after that is float64, so the
result is the exact value the kernel approximates.  With a prior the caller passes the per-row energies E (B,) and gradients
dE (B, P) as fp32 values (the kernel's own, from the separately tested smplr_prior_energy).  With G = 1, no smoothing and no
prior the statements are those of tests/_fitting_oracle.py `fit_step`, in the same order: the two agree exactly.  Nothing here
is shared with the code under test."""
import numpy as np

FLOAT_KEYS = ("x", "m", "v", "best_x", "best_loss")
INT_KEYS = ("t", "calls", "stall", "bad", "best_step", "active")


def f32(a):
    return np.float64(np.float32(a))


def up(a):
    return np.asarray(a, np.float32).astype(np.float64)


def row_loss(loss, silh_loss=None, silh_weight=1.0):
    L = up(loss).mean(axis=1)
    if silh_loss is not None:
        L = L + f32(silh_weight) * up(silh_loss).mean(axis=1)
    return L


def smoothness(x, G, smooth, tie=None):
    """x (B, P) float64, smooth (P,) -> (E_s (B / G,), s (B, P), E_s_mag (B / G,), s_mag (B, P)): the energy per group and its
    gradient per row; the magnitudes are the sums of the absolute values of the terms with |x_r| + |x_r-1| in place of every
    difference (what the fp64 work's 2^-50 is relative to).  Columns with tie set or a zero weight get nothing."""
    B, P = x.shape
    w = up(smooth).copy()
    if tie is not None:
        w[np.asarray(tie) != 0] = 0.0
    xg = x.reshape(B // G, G, P)
    d = np.zeros_like(xg)
    dm = np.zeros_like(xg)
    d[:, 1:] = xg[:, 1:] - xg[:, :-1]                                  # d[r] = x_r - x_{r-1}, 0 at r = 0
    dm[:, 1:] = np.abs(xg[:, 1:]) + np.abs(xg[:, :-1])
    nxt = np.zeros_like(xg)
    nm = np.zeros_like(xg)
    nxt[:, :-1] = d[:, 1:]                                             # x_{r+1} - x_r, 0 at r = G - 1
    nm[:, :-1] = dm[:, 1:]
    on = w != 0.0
    with np.errstate(invalid="ignore", over="ignore"):
        E = np.where(on, w * (d * d).sum(axis=1), 0.0).sum(axis=1)
        s = np.where(on, 2.0 * w * (d - nxt), 0.0)
        Em = np.where(on, w * (dm * dm).sum(axis=1), 0.0).sum(axis=1)
        sm = np.where(on, 2.0 * w * (dm + nm), 0.0)
    return E, s.reshape(B, P), Em, sm.reshape(B, P)


def fit_step_group(state, g, loss, silh_loss=None, silh_weight=1.0, col_scale=None, history=None, G=1, tie=None, smooth=None,
                   E=None, dE=None, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-7, gscale=1.0, mode="keras", patience=0):
    """One call on a copy of `state` -> (new state, info).  info: L_rows (B,) every row's own loss and L_rows_mag = L_data + |E|;
    L (B / G,) the groups';
    L_mag (B / G,) the sum of the magnitudes of L's terms; E_s, E_s_mag (B / G,); s, s_mag (B, P); g_upd (B, P) the gradient
    each entry was updated with (a tied column: the group's sum, repeated); A (B, P) its cancellation-free magnitude
    |g_r| + |dE_r| + |s_r| (a tied column: summed over the group); n_add (B, P) the fp32 roundings between the inputs and
    g_upd (prior 1, smoothing 2, tied 1); m_mag, v_mag, dx_mag (B, P): |b1 m| + (1 - b1) gscale A, b2 v + (1 - b2) (gscale A)^2
    and the step with m_mag in place of m; updated (B,) bool: rows that took step h."""
    assert mode in ("keras", "torch")
    s = {k: np.array(a, copy=True) for k, a in state.items()}
    g = up(g)
    B, P = s["x"].shape
    assert 1 <= G <= 16 and B % G == 0
    tied = np.zeros(P, bool) if tie is None else np.asarray(tie) != 0
    cs = np.ones(P) if col_scale is None else up(col_scale)
    lr, b1, b2, eps, gscale = f32(lr), f32(beta1), f32(beta2), f32(eps), f32(gscale)
    # a. per-row loss
    L_rows = row_loss(loss, silh_loss, silh_weight)
    L_rows_mag = np.abs(L_rows)
    if E is not None:
        L_rows_mag = L_rows_mag + np.abs(up(E))
        L_rows = L_rows + up(E)
    # b. per-row gradient
    A = np.abs(g)
    n_add = np.zeros((B, P))
    if dE is not None:
        A = A + np.abs(up(dE))
        g = g + up(dE)
        n_add += 1
    # c. smoothness
    Es, Esm = np.zeros(B // G), np.zeros(B // G)
    sr, srm = np.zeros((B, P)), np.zeros((B, P))
    if smooth is not None:
        Es, sr, Esm, srm = smoothness(s["x"], G, smooth, tied)
        on = (up(smooth) != 0.0) & ~tied
        with np.errstate(invalid="ignore"):
            g = np.where(on, g + sr, g)
            A = np.where(on, A + np.abs(sr), A)
        n_add += 2 * on
    info = dict(L_rows=L_rows, L_rows_mag=L_rows_mag, L=np.zeros(B // G), L_mag=np.zeros(B // G), E_s=Es, E_s_mag=Esm, s=sr, s_mag=srm, g_upd=g.copy(), A=A.copy(),
                n_add=n_add, m_mag=np.zeros((B, P)), v_mag=np.zeros((B, P)), dx_mag=np.zeros((B, P)), updated=np.zeros(B, bool))
    for k in range(B // G):
        rows = list(range(k * G, k * G + G))
        b0 = rows[0]
        # d. group loss, rows in order
        L = 0.0
        for b in rows:
            L = L + L_rows[b]
        L = L + Es[k]
        info["L"][k] = L
        info["L_mag"][k] = L_rows_mag[rows].sum() + Es[k]
        # e. trace
        for b in rows:
            c = int(s["calls"][b])
            if history is not None and 0 <= c < history.shape[0]:
                history[c, b] = L_rows[b]
            s["calls"][b] = c + 1
        # f. bad call
        if not (np.isfinite(L) and np.all(np.isfinite(g[rows]))):
            for b in rows:
                s["bad"][b] += 1
            continue
        # g. best iterate and stop, from the first row's scalars
        if not s["active"][b0]:
            continue
        t0, stall0 = int(s["t"][b0]), int(s["stall"][b0])
        better = L < s["best_loss"][b0]
        stall1 = 0 if better else stall0 + 1
        for b in rows:
            if better:
                s["best_loss"][b] = L
                s["best_x"][b] = s["x"][b]
                s["best_step"][b] = t0
            s["stall"][b] = stall1
        if patience > 0 and stall1 >= patience:
            for b in rows:
                s["active"][b] = 0
            continue
        # h. update
        t = float(t0 + 1)
        c1, c2 = 1.0 - b1 ** t, 1.0 - b2 ** t
        g_sum = g[b0].copy()
        A_sum = A[b0].copy()
        for b in rows[1:]:
            g_sum = g_sum + g[b]
            A_sum = A_sum + A[b]
        m0, v0, x0 = s["m"][b0].copy(), s["v"][b0].copy(), s["x"][b0].copy()
        for b in rows:
            s["t"][b] = t0 + 1
            info["updated"][b] = True
            gb = np.where(tied, g_sum, g[b])
            Ab = np.where(tied, A_sum, A[b])
            mb, vb, xb = np.where(tied, m0, s["m"][b]), np.where(tied, v0, s["v"][b]), np.where(tied, x0, s["x"][b])
            gh = gscale * gb
            Ah = gscale * Ab
            m_mag = np.abs(b1 * mb) + np.abs((1.0 - b1) * Ah)
            m = b1 * mb + (1.0 - b1) * gh
            v = b2 * vb + (1.0 - b2) * gh * gh
            v_mag = b2 * vb + (1.0 - b2) * Ah * Ah
            with np.errstate(divide="ignore", invalid="ignore"):
                if mode == "keras":
                    unit = lr * cs * np.sqrt(c2) / c1 / (np.sqrt(v) + eps)
                else:
                    unit = lr * cs / c1 / (np.sqrt(v) / np.sqrt(c2) + eps)
                move = (cs != 0.0) & (m != 0.0)
                s["x"][b] = np.where(move, xb - np.where(move, unit * m, 0.0), s["x"][b])
                info["dx_mag"][b] = np.where(cs != 0.0, np.where(m_mag != 0.0, unit * m_mag, 0.0), 0.0)
            s["m"][b], s["v"][b] = m, v
            info["m_mag"][b], info["v_mag"][b] = m_mag, v_mag
            info["g_upd"][b], info["A"][b] = gb, Ab
            info["n_add"][b] = n_add[b] + tied * (G > 1)
    return s, info
