"""NumPy float64 restatement of one smplr_fit_step call (csrc/fit.hip; the semantics block of ilps_amd/fitting.py).

Inputs are what the kernel gets - fp32 arrays and fp32 scalars - cast up; every operation after that is float64, so the
result is the exact value the kernel approximates.  Nothing here is shared with the code under test."""
import numpy as np

FLOAT_KEYS = ("x", "m", "v", "best_x", "best_loss")
INT_KEYS = ("t", "calls", "stall", "bad", "best_step", "active")


def new_state(x0):
    x = np.asarray(x0, np.float32).astype(np.float64)
    B = x.shape[0]
    z = lambda: np.zeros(B, np.int64)
    return dict(x=x.copy(), m=np.zeros_like(x), v=np.zeros_like(x), best_x=x.copy(), t=z(), calls=z(), stall=z(), bad=z(),
                best_step=z(), active=np.ones(B, np.int64), best_loss=np.full(B, np.inf))


def from_tensors(state):
    """A `fitting.FitState` (any device) -> the oracle's dict: fp32 cast up to float64, integers to int64."""
    out = {}
    for k in FLOAT_KEYS:
        out[k] = getattr(state, k).detach().cpu().numpy().astype(np.float64)
    for k in INT_KEYS:
        out[k] = getattr(state, k).detach().cpu().numpy().astype(np.int64)
    return out


def f32(a):
    return np.float64(np.float32(a))


def row_loss(loss, silh_loss=None, silh_weight=1.0):
    """Step 1: (B,) float64."""
    L = np.asarray(loss, np.float32).astype(np.float64).mean(axis=1)
    if silh_loss is not None:
        L = L + f32(silh_weight) * np.asarray(silh_loss, np.float32).astype(np.float64).mean(axis=1)
    return L


def fit_step(state, g, loss, silh_loss=None, silh_weight=1.0, col_scale=None, history=None, lr=1e-3, beta1=0.9, beta2=0.999,
             eps=1e-7, gscale=1.0, mode="keras", patience=0):
    """One call on a copy of `state` -> (new state, L (B,), terms): `history` (H, B) float64 is written in place when
    given; terms = dict(m_mag, v_mag, dx_mag) are the cancellation-free magnitudes the error bars of
    tests/test_gpu_fitting.py are relative to: |b1 m| + |(1 - b1) g^|, b2 v + (1 - b2) g^ g^, and the step computed from
    m_mag in place of m."""
    assert mode in ("keras", "torch")
    s = {k: np.array(a, copy=True) for k, a in state.items()}
    g = np.asarray(g, np.float32).astype(np.float64)
    B, P = s["x"].shape
    cs = np.ones(P) if col_scale is None else np.asarray(col_scale, np.float32).astype(np.float64)
    lr, b1, b2, eps, gscale = f32(lr), f32(beta1), f32(beta2), f32(eps), f32(gscale)
    L = row_loss(loss, silh_loss, silh_weight)
    terms = dict(m_mag=np.zeros((B, P)), v_mag=np.zeros((B, P)), dx_mag=np.zeros((B, P)))
    for b in range(B):
        c = int(s["calls"][b])
        if history is not None and 0 <= c < history.shape[0]:
            history[c, b] = L[b]
        s["calls"][b] = c + 1
        if not (np.isfinite(L[b]) and np.all(np.isfinite(g[b]))):
            s["bad"][b] += 1
            continue
        if not s["active"][b]:
            continue
        if L[b] < s["best_loss"][b]:
            s["best_loss"][b] = L[b]
            s["best_x"][b] = s["x"][b]
            s["best_step"][b] = s["t"][b]
            s["stall"][b] = 0
        else:
            s["stall"][b] += 1
        if patience > 0 and s["stall"][b] >= patience:
            s["active"][b] = 0
            continue
        s["t"][b] += 1
        t = float(s["t"][b])
        gh = gscale * g[b]
        m_mag = np.abs(b1 * s["m"][b]) + np.abs((1.0 - b1) * gh)
        m = b1 * s["m"][b] + (1.0 - b1) * gh
        v = b2 * s["v"][b] + (1.0 - b2) * gh * gh
        c1, c2 = 1.0 - b1 ** t, 1.0 - b2 ** t
        with np.errstate(divide="ignore", invalid="ignore"):
            if mode == "keras":
                unit = lr * cs * np.sqrt(c2) / c1 / (np.sqrt(v) + eps)
            else:
                unit = lr * cs / c1 / (np.sqrt(v) / np.sqrt(c2) + eps)
            move = (cs != 0.0) & (m != 0.0)
            s["x"][b] = np.where(move, s["x"][b] - np.where(move, unit * m, 0.0), s["x"][b])
            terms["dx_mag"][b] = np.where(cs != 0.0, np.where(m_mag != 0.0, unit * m_mag, 0.0), 0.0)
        s["m"][b], s["v"][b] = m, v
        terms["m_mag"][b], terms["v_mag"][b] = m_mag, v
    return s, L, terms
