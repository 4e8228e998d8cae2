"""Seeded inputs for the L-BFGS step's tests: test problems with float64 values and gradients, and a scripted six-row
trajectory of the oracle (tests/_lbfgs_oracle.py) that reaches every branch of the state machine.  The CPU test checks the
branches on it; the GPU test replays it call by call against the kernel (teacher forcing)."""
import numpy as np

import _lbfgs_oracle as o

N_LOSS = 300                   # loss values per row: thread i < 44 of a row's 256 takes a second trip of its strided sum


def quadratic(P, cond, seed):
    """f(x) = 1/2 (x - m)^T Q^T diag(a) Q (x - m), a log-spaced over 1 .. cond, Q a seeded rotation: strictly convex.
    -> (fun(x) -> (f, g) float64, x_start)."""
    rng = np.random.default_rng(seed)
    a = np.logspace(0.0, np.log10(cond), P) if P > 1 else np.array([float(cond)])
    Q = np.linalg.qr(rng.normal(size=(P, P)))[0]
    A = Q.T @ (a[:, None] * Q)
    m = rng.normal(size=P)

    def fun(x):
        r = np.asarray(x, np.float64) - m
        return 0.5 * r @ A @ r, A @ r
    return fun, m + rng.normal(size=P)


def rosenbrock(x):
    x = np.asarray(x, np.float64)
    f = np.sum(100.0 * (x[1:] - x[:-1] ** 2) ** 2 + (1.0 - x[:-1]) ** 2)
    g = np.zeros_like(x)
    g[:-1] = -400.0 * x[:-1] * (x[1:] - x[:-1] ** 2) - 2.0 * (1.0 - x[:-1])
    g[1:] += 200.0 * (x[1:] - x[:-1] ** 2)
    return f, g


def cosines(x):
    """sum_j cos(x_j): concave around 0, so a step accepted there has y . s < 0 (the curvature rule skips the pair)."""
    x = np.asarray(x, np.float64)
    return np.sum(np.cos(x)), -np.sin(x)


def loss_rows(values, rng):
    """(B,) wanted losses -> (B, N_LOSS) fp32 per-pixel losses whose mean is the wanted value up to fp32 rounding: seeded
    positive weights of mean 1 times the value (a NaN or an infinity fills its row)."""
    w = rng.uniform(0.5, 1.5, (len(values), N_LOSS))
    w /= w.mean(1, keepdims=True)
    with np.errstate(over="ignore", invalid="ignore"):
        return (w * np.asarray(values, np.float64)[:, None]).astype(np.float32)


WALL = 1e3                     # added to the accepted loss by a row that rejects every trial


def script(P, M, seed=0, calls=46):
    """A trajectory of B = 6 rows over `calls` launches -> dict(col_scale (P,) fp32, steps = [dict(before, g, loss, L, params,
    after, events)], branches = the union of the events).  max_ls = 2 keeps line searches short.  The rows:
      0  a quadratic of condition 1e2: accepts, shrinks, and - past M stored pairs - the ring wraps;
      1  sum cos(x_j) from 0.3: steps accepted with negative curvature (the pair is skipped);
      2  a quadratic that, from call 8 on, reports f0 + WALL at every trial: shrinks, the reset at max_ls, then the failure,
         then an inactive row;
      3  a quadratic with a NaN loss at call 0 (phase 0) and an infinite gradient entry at call 5 (phase 1), and at call 9 a
         state set to phase 0 with a memory of one pair of negative curvature (s, -s): the direction points uphill, the
         non-descent reset;
      4  a quadratic that reports f0 + WALL from call 30 on, where the launches run with patience = 2: the patience stop;
      5  a constant: the gradient is 0, the row stops at tol_grad = 0 in its first call.
    With P > 1 the odd columns below P // 2 are frozen (col_scale 0), the others scaled 0.5 .. 2."""
    rng = np.random.default_rng(1000 * P + 10 * M + seed)
    B = 6
    cs = rng.uniform(0.5, 2.0, P).astype(np.float32)
    if P > 1:
        cs[1:P // 2:2] = 0.0
    quads = {b: quadratic(P, 1e2, 7 * P + b + seed) for b in (0, 2, 3, 4)}
    x_start = np.zeros((B, P))
    for b, (_, xs) in quads.items():
        x_start[b] = xs
    x_start[1] = 0.3 + 0.05 * rng.normal(size=P)
    x_start[5] = rng.normal(size=P)
    st = o.new_state(x_start, M)
    steps, branches = [], set()
    for k in range(calls):
        params = dict(lr=1.0, c1=1e-4, max_ls=2, tol_grad=0.0, gscale=0.5, patience=2 if k >= 30 else 0)
        if k == 9:                                         # row 3: one stored pair of negative curvature
            e = rng.normal(size=P).astype(np.float32).astype(np.float64)
            st["pairs"][3], st["phase"][3] = 1, 0          # (phase 0: this call stores no pair of its own over it)
            st["S"][3, 0], st["Y"][3, 0] = e, -e
        f = np.zeros(B)
        g = np.zeros((B, P))
        for b in range(B):
            x = st["x"][b]
            if b in quads:
                f[b], g[b] = quads[b][0](x)
            elif b == 1:
                f[b], g[b] = cosines(x)
            else:
                f[b] = 2.5
        if k >= 8 and st["phase"][2]:
            f[2] = st["f0"][2] + WALL
        if k >= 30 and st["phase"][4]:
            f[4] = st["f0"][4] + WALL
        if k == 0:
            f[3] = np.nan
        if k == 5:
            g[3, P // 2] = np.inf
        loss = loss_rows(f, rng)
        g32 = (g / params["gscale"]).astype(np.float32)   # (the launch multiplies by gscale again)
        L = o.row_loss(loss)
        before = {key: a.copy() for key, a in st.items()}
        st, ev = o.lbfgs_step(st, g32, L, cs, **params)
        steps.append(dict(before=before, g=g32, loss=loss, L=L, params=params, after={key: a.copy() for key, a in st.items()},
                          events=ev))
        for e in ev:
            branches |= e
    return dict(col_scale=cs, steps=steps, branches=branches, B=B)
