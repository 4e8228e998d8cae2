"""NumPy restatement of one smplr_lbfgs_step call (csrc/lbfgs.hip; the semantics block of ilps_amd/fitting.py, rules 1 - 9).

State and inputs are the fp32 values the kernel gets, held in float64 arrays.  Every dot product is float64 on those values,
combined by the kernel's own fixed tree (`tree_sum`: the xor butterfly of a 64-lane wave, then the waves (0 + 1) + (2 + 3)), so
the decisions taken from them are the kernel's; every operation a rule names as fp32 is done in np.float32, every stored
value is rounded to fp32 once.  Nothing here is shared with the code under test.

`lbfgs_step` also reports, per row, the branches of the state machine the call went through (`BRANCHES`)."""
import numpy as np

FLOAT_KEYS = ("x", "best_x", "best_loss", "x0", "g0", "f0", "d", "gd", "alpha", "S", "Y")
INT_KEYS = ("t", "calls", "stall", "bad", "best_step", "active", "ls", "pairs", "phase")
BRANCHES = ("accept", "shrink", "ring_wrap", "curvature_skip", "nondescent_reset", "max_ls_reset", "ls_failure", "tol_grad_stop",
            "patience_stop", "bad_phase0", "bad_phase1", "start", "inactive")
THREADS, WAVE = 256, 64
CURV = 1e-10


def new_state(x0, memory=8):
    x = np.asarray(x0, np.float32).astype(np.float64)
    B, P = x.shape
    z = lambda: np.zeros(B, np.int64)
    zf = lambda: np.zeros(B)
    return dict(x=x.copy(), best_x=x.copy(), t=z(), calls=z(), stall=z(), bad=z(), best_step=z(), active=np.ones(B, np.int64),
                best_loss=np.full(B, np.inf), x0=x.copy(), g0=np.zeros_like(x), f0=zf(), d=np.zeros_like(x), gd=zf(), alpha=zf(),
                ls=z(), pairs=z(), phase=z(), S=np.zeros((B, memory, P)), Y=np.zeros((B, memory, P)))


def from_tensors(state):
    """A `fitting.LbfgsState` (any device) -> the oracle's dict: fp32 cast up to float64, integers to int64."""
    out = {}
    for k in FLOAT_KEYS:
        out[k] = getattr(state, k).detach().cpu().numpy().astype(np.float64)
    for k in INT_KEYS:
        out[k] = getattr(state, k).detach().cpu().numpy().astype(np.int64)
    return out


def f32(a):
    return np.float32(a).astype(np.float64)


def tree_sum(v):
    """Sum of v (n <= 256,) float64 as the workgroup forms it: thread j holds v[j] (+0 beyond n), a wave's 64 values go through
    the xor butterfly 32, 16, .. 1, the four waves' sums are added (0 + 1) + (2 + 3)."""
    w = np.zeros(THREADS)
    w[:len(v)] = v
    w = w.reshape(THREADS // WAVE, WAVE)
    lane = np.arange(WAVE)
    for o in (32, 16, 8, 4, 2, 1):
        w = w + w[:, lane ^ o]
    return (w[0, 0] + w[1, 0]) + (w[2, 0] + w[3, 0])


def dot(a, b):
    return tree_sum(np.asarray(a, np.float64) * np.asarray(b, np.float64))


def _strided(p):
    """Thread i's fp32 serial sum p[i] + p[i + 256] + ... -> (256,) float64."""
    p = np.asarray(p, np.float32)
    s = np.zeros(THREADS, np.float32)
    for k in range(0, len(p), THREADS):
        part = p[k:k + THREADS]
        s[:len(part)] = s[:len(part)] + part
    return s.astype(np.float64)


def row_loss(loss, silh_loss=None, silh_weight=1.0, energy=None):
    """Step 1 with the kernel's own tree: (B,) float64 holding the fp32 value L; energy (B,): a prior's fp32 E, added in fp64
    before the one rounding."""
    loss = np.asarray(loss, np.float32)
    out = np.empty(loss.shape[0])
    for b in range(loss.shape[0]):
        Ld = tree_sum(_strided(loss[b])) / float(loss.shape[1])
        if silh_loss is not None:
            q = np.asarray(silh_loss, np.float32)[b]
            Ld = Ld + np.float64(np.float32(silh_weight)) * (tree_sum(_strided(q)) / float(len(q)))
        if energy is not None:
            Ld = Ld + np.float64(np.float32(energy[b]))
        with np.errstate(over="ignore"):
            out[b] = f32(Ld)
    return out


def first_alpha(lr, n1):
    with np.errstate(divide="ignore"):
        return f32(lr * min(1.0, 1.0 / n1))


def direction(gh, S, Y, pairs):
    """7.4: the two-loop recursion over the k = min(pairs, M) newest pairs -> (d fp32 values, gd fp32 value, k)."""
    M = S.shape[0]
    k = min(int(pairs), M)
    q = gh.copy()
    a, rho = np.zeros(k), np.zeros(k)
    ys_new = yy_new = 0.0
    for i in range(k):                                     # newest first
        s, y = S[(pairs - 1 - i) % M], Y[(pairs - 1 - i) % M]
        ys = dot(y, s)
        rho[i] = 1.0 / ys
        a[i] = rho[i] * dot(s, q)
        if i == 0:
            ys_new, yy_new = ys, dot(y, y)
        q = q - a[i] * y
    if k > 0:
        q = (ys_new / yy_new) * q
    for i in range(k - 1, -1, -1):                         # oldest first
        s, y = S[(pairs - 1 - i) % M], Y[(pairs - 1 - i) % M]
        bi = rho[i] * dot(y, q)
        q = q + (a[i] - bi) * s
    d = f32(-q)
    return d, f32(dot(gh, d)), k


def lbfgs_step(state, g, L, col_scale=None, history=None, lr=1.0, c1=1e-4, max_ls=10, tol_grad=0.0, gscale=1.0, patience=0):
    """One call on a copy of `state` -> (new state, events): g (B, P) the gradient (with a prior: g + dE already added in fp32),
    L (B,) the fp32 loss values of `row_loss`; `history` (H, B) float64 is written in place when given; events[b] = the set of
    `BRANCHES` row b went through."""
    s = {k: np.array(a, copy=True) for k, a in state.items()}
    g32 = np.asarray(g, np.float32)
    B, P = s["x"].shape
    M = s["S"].shape[1]
    cs32 = np.ones(P, np.float32) if col_scale is None else np.asarray(col_scale, np.float32)
    cs = cs32.astype(np.float64)
    lr, c1, tol_grad = float(np.float32(lr)), float(np.float32(c1)), float(np.float32(tol_grad))
    L = np.asarray(L, np.float64)
    events = [set() for _ in range(B)]
    for b in range(B):
        ev = events[b]
        c = int(s["calls"][b])
        if history is not None and 0 <= c < history.shape[0]:
            history[c, b] = L[b]
        s["calls"][b] = c + 1
        with np.errstate(over="ignore", invalid="ignore"):
            gh32 = cs32 * (np.float32(gscale) * g32[b])                       # 3. two fp32 products
        gh = gh32.astype(np.float64)
        trial = bool(s["phase"][b])
        bad = not (np.isfinite(L[b]) and np.all(np.isfinite(g32[b])))
        if bad:                                                               # 4.
            s["bad"][b] += 1
            ev.add("bad_phase1" if trial else "bad_phase0")
            if not trial:
                continue
        if not s["active"][b]:                                                # 5.
            ev.add("inactive")
            continue
        x = s["x"][b].copy()
        if not bad:                                                           # 6.
            if L[b] < s["best_loss"][b]:
                s["best_loss"][b], s["best_x"][b], s["best_step"][b], s["stall"][b] = L[b], x, s["t"][b], 0
            else:
                s["stall"][b] += 1
            if patience > 0 and s["stall"][b] >= patience:
                s["active"][b] = 0
                ev.add("patience_stop")
                continue
        alpha0 = s["alpha"][b]
        accept = not bad and (not trial or L[b] <= s["f0"][b] + (c1 * alpha0) * s["gd"][b])
        if accept:                                                            # 7.
            ev.add("accept" if trial else "start")
            pairs = int(s["pairs"][b])
            if trial:                                                         # 7.1
                sv = (np.float32(alpha0) * s["d"][b].astype(np.float32)).astype(np.float64)
                yv = (gh32 - s["g0"][b].astype(np.float32)).astype(np.float64)
                if dot(yv, sv) > CURV:
                    s["S"][b, pairs % M], s["Y"][b, pairs % M] = sv, yv
                    pairs += 1
                    if pairs > M:
                        ev.add("ring_wrap")
                else:
                    ev.add("curvature_skip")
                s["t"][b] += 1
            s["x0"][b], s["f0"][b], s["g0"][b] = x, L[b], gh                  # 7.2
            s["pairs"][b] = pairs
            if np.all(np.abs(gh) <= tol_grad):                                # 7.3
                s["active"][b] = 0
                ev.add("tol_grad_stop")
                continue
            d, gd, k = direction(gh, s["S"][b], s["Y"][b], pairs)             # 7.4
            if k > 0 and not gd < 0.0:                                        # 7.5
                pairs = 0
                ev.add("nondescent_reset")
            if k == 0 or pairs == 0:                                          # 7.6
                d, gd, alpha = -gh, f32(-dot(gh, gh)), first_alpha(lr, tree_sum(np.abs(gh)))
            else:
                alpha = lr
            s["d"][b], s["gd"][b], s["alpha"][b], s["pairs"][b] = d, gd, alpha, pairs
            s["ls"][b], s["phase"][b] = 0, 1                                  # 7.7
            x0 = x
        else:                                                                 # 8.
            s["ls"][b] += 1
            x0 = s["x0"][b]
            if s["ls"][b] > max_ls:
                if s["pairs"][b] == 0:
                    s["active"][b] = 0
                    ev.add("ls_failure")
                    continue
                g0 = s["g0"][b]
                s["pairs"][b], s["d"][b], s["gd"][b] = 0, -g0, f32(-dot(g0, g0))
                s["alpha"][b], s["ls"][b] = first_alpha(lr, tree_sum(np.abs(g0))), 0
                ev.add("max_ls_reset")
            else:
                s["alpha"][b] = f32(alpha0 * 0.5)
                ev.add("shrink")
        # 9. three fp32 operations
        step = np.float32(s["alpha"][b]) * cs32
        with np.errstate(over="ignore", invalid="ignore"):
            xn = (x0.astype(np.float32) + step * s["d"][b].astype(np.float32)).astype(np.float64)
        s["x"][b] = np.where(cs32 != 0, xn, s["x"][b])
    return s, events


def restart(state):
    s = {k: np.array(a, copy=True) for k, a in state.items()}
    s["x"] = np.where((s["phase"] != 0)[:, None], s["x0"], s["x"])
    s["pairs"][:], s["ls"][:], s["phase"][:] = 0, 0, 0
    return s


def minimise(fun, x_start, evaluations, memory=8, col_scale=None, **kw):
    """The loop a fitter runs, on one row: fun(x (P,) float64 holding fp32 values) -> (f, g) float64; L = fp32(f), g fp32.
    -> (state, trace of per-call event sets)."""
    st = new_state(np.asarray(x_start, np.float64)[None], memory)
    trace = []
    for _ in range(evaluations):
        f, g = fun(st["x"][0])
        with np.errstate(over="ignore"):
            st, ev = lbfgs_step(st, np.float32(g)[None], f32(np.array([f])), col_scale, **kw)
        trace.append(ev[0])
        if not st["active"][0]:
            break
    return st, trace
