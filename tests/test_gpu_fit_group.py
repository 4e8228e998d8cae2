"""smplr_fit_step_group (csrc/fit.hip fit_group_kernel) and `ParamFitter.fit(group_size=...)` on the GPU, against
tests/_fit_group_oracle.py (NumPy float64).

Error bars of the step-parity test, from the kernel's operation count (u = 2^-24, the relative error of one fp32 rounding to
nearest; none is taken from the kernel's output).  The plain step's bars (tests/test_gpu_fitting.py) are the base: with the
exact gradient m is held to 4 u of |b1 m| + |(1 - b1) g^|, v to 4 u of v, the step to 16 u of its magnitude D plus u |x|.
  L_r  the row's loss: the plain bar `loss_bar` on the data term, plus one rounding of the total with a prior (E_r is the
       kernel's own fp32 value, handed to the oracle): (loss_bar + u) of L_data + |E_r|.
  E_s  fp64 on the fp32 operands, rounded once: u of its value plus 2^-50 of the sum of smooth_j (|x_r| + |x_r-1|)^2;
  s_r  likewise u of its value plus 2^-50 of 2 smooth_j times the sum of the |x| that enter (test_smoothness_alone sees both
       directly: with g = 0, loss = 0, beta1 = 0 and gscale = 1 the kernel leaves fp32(E_s) in best_loss and fp32(s_r) in m).
  L    fp32(sum_r L_r + E_s), every term non-negative: each L_r's own bar, one rounding for E_s, one for the total:
       (loss_bar + 2 u) of the sum of the terms' magnitudes.
  g    the gradient an entry is updated with differs from the exact one by n roundings relative to its cancellation-free
       magnitude A (untied: |g_r| + |dE_r| + |s_r|; tied: that summed over the group): the addition of dE_r 1, s_r's own rounding
       and its addition 2, the tied sum (fp64, rounded once) 1 - so n = 0 .. 4 per entry, and 0 leaves the plain bars.  This is
       the count of the code as written; the issue's estimate (2) did not count s_r's own rounding nor the prior's addition.
  m    (4 + n) u of |b1 m| + (1 - b1) gscale A  (+ 2^-50 (1 - b1) gscale s_mag for the fp64 work behind s_r).
  v    (4 + 2 n) u of b2 v + (1 - b2) (gscale A)^2: the gradient enters squared.
  x    (16 + n + n kappa) u of D (the step with the magnitude of m in place of m) plus u |x|: n u through m, and 2 n u of v's
       magnitude through sqrt(v), which halves it but divides by the exact v: kappa = v's magnitude / v >= 1, and 1 unless
       the terms of g cancel.
The observed maxima are printed (pytest -s) and recorded in DESIGN.md section 18."""
import importlib
import importlib.util
import math
import os

import numpy as np
import pytest
import torch

import _fit_group_oracle as go
import _fitting_oracle as fo
import _prior_oracle as po
from _inputs import make_x

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
SLACK = 1.0 + 2.0 ** -10                                               # second-order terms of the first-order counts above
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = fo.FLOAT_KEYS + fo.INT_KEYS


def fitting_module():
    return importlib.import_module("ilps_amd.fitting")


def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def t(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(dev())


def same_bits(a, b):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    if a.dtype == torch.float32:
        a, b = a.view(torch.int32), b.view(torch.int32)
    return torch.equal(a, b)


def loss_bar(N, Ns=0):
    return (math.ceil(max(N, Ns) / fitting_module().THREADS) + math.ceil(math.log2(fitting_module().THREADS))) * U


def log_uniform_grads(rng, B, P):
    g = 10.0 ** rng.uniform(-8.0, 2.0, (B, P)) * rng.choice([-1.0, 1.0], (B, P))
    return g.astype(np.float32)


def mean_pose():
    from ilps_amd.smpl_model import load_mean_params
    return load_mean_params()[0]


def state_from(s):
    fitting = fitting_module()
    f = lambda a: t(np.asarray(a, np.float32))
    i = lambda a: t(np.asarray(a, np.int32), torch.int32)
    return fitting.FitState(x=f(s["x"]), m=f(s["m"]), v=f(s["v"]), best_x=f(s["best_x"]), t=i(s["t"]), calls=i(s["calls"]),
                            stall=i(s["stall"]), bad=i(s["bad"]), best_step=i(s["best_step"]),
                            active=t(np.asarray(s["active"], np.uint8), torch.uint8), best_loss=f(s["best_loss"]))


def op_group_step(st, g, loss, silh, sw, cs, hist, tie, smooth, prior, w, G, lr, eps, gscale, mode, patience, num_cam=4):
    """The torch op, so that the at::Tensor layer runs on the device too."""
    from ilps_amd import torch_ops
    fitting = fitting_module()
    pr = [None] * 7 if prior is None else [prior.mean, prior.factor, prior.offset, prior.angle_idx, prior.angle_scale,
                                           prior.shape_mean, w]
    torch_ops.load().fit_step_group(st.x, g, st.m, st.v, st.t, st.calls, st.stall, st.bad, st.best_step, st.active, st.best_loss,
                                    st.best_x, loss, silh, cs, hist, tie, smooth, *pr, G, lr, 0.9, 0.999, eps, gscale, sw,
                                    fitting.MODES.index(mode), patience, num_cam)


@pytest.fixture(scope="module")
def prior86():
    fitting = fitting_module()
    p = po.make_prior(8, 4, seed=21, mean_pose=mean_pose())
    return p, fitting.PosePrior(**p).to(dev())


# ---- 1. a group of one is the plain step, bit for bit ------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["keras", "torch"])
@pytest.mark.parametrize("with_prior", [False, True])
@pytest.mark.parametrize("with_silh", [False, True])
@pytest.mark.parametrize("N", [144, 2305])
def test_group_of_one_has_the_plain_steps_bits(N, with_silh, with_prior, mode, prior86):
    fitting = fitting_module()
    B, P, Ns, calls = 5, 86, 64 * 64, 6
    p, prior = prior86
    rng = np.random.default_rng(N + 7 * with_silh + 3 * with_prior + (mode == "torch"))
    x0 = t(po.make_rows(p, B, 4, seed=5))
    plain, by_op, by_py = fitting.FitState.new(x0), fitting.FitState.new(x0), fitting.FitState.new(x0)
    hists = [torch.full((calls, B), float("nan"), device=dev()) for _ in range(3)]
    cs = rng.uniform(0.5, 30.0, P).astype(np.float32)
    cs[[2, 40, 80]] = 0.0
    cs = t(cs)
    tie = fitting.tie_mask(shape=True, pose=(N == 144)).to(dev())
    zeros = torch.zeros(P, device=dev())
    w = t(np.array([0.02, 0.01, 0.05], np.float32)) if with_prior else None
    kw = dict(lr=2e-3, eps=1e-7 if mode == "keras" else 1e-8, mode=mode, patience=2, grad_scale=0.3)
    pkw = dict(prior=prior, prior_weights=w) if with_prior else {}
    for k in range(calls):
        g = log_uniform_grads(rng, B, P)
        g[rng.random((B, P)) < 0.05] = 0.0
        g[3] = 0.0
        if k == 2:
            g[1, 9] = np.nan
        g = t(g)
        loss = t(rng.exponential(0.05, (B, N)) * (1.0 - 0.1 * k * (np.arange(B)[:, None] % 2)))
        silh = t(rng.exponential(0.3, (B, Ns))) if with_silh else None
        fitting.fit_step(plain, g, loss, silh, 0.7, cs, hists[0], **kw, **pkw)
        op_group_step(by_op, g, loss, silh, 0.7, cs, hists[1], tie, None, prior if with_prior else None, w, 1, kw["lr"], kw["eps"],
                      0.3, mode, 2)
        fitting.fit_step(by_py, g, loss, silh, 0.7, cs, hists[2], group_size=1, tie=tie, smooth=zeros, **kw, **pkw)
        torch.cuda.synchronize()
        for name in NAMES:
            assert same_bits(getattr(by_op, name), getattr(plain, name)), (name, k, "op, smooth = NULL")
            assert same_bits(getattr(by_py, name), getattr(plain, name)), (name, k, "fit_step, smooth = 0")
    assert same_bits(hists[1], hists[0]) and same_bits(hists[2], hists[0])
    assert int(plain.t.max()) > 0 and int(plain.bad.sum()) == 1 and not same_bits(plain.x, x0)


# ---- 2. step parity against the oracle, teacher-forced -----------------------------------------------------------------
def parity_case(G, B, P, N, tie_names, with_smooth, with_prior, mode, with_silh, seen):
    fitting = fitting_module()
    num_cam, Ns, calls, sw = P - 82, 17 * 17, 4, 0.7
    rng = np.random.default_rng(1000 * G + 10 * B + P + N + 3 * with_smooth + 5 * with_prior + len(tie_names))
    tie = fitting.tie_mask(**{n: True for n in tie_names}, num_cam=num_cam).numpy()
    smooth = fitting.smooth_weights(cam=0.05, global_rot=0.5, pose=0.3, num_cam=num_cam).numpy() if with_smooth else None
    prior = p = None
    if with_prior:
        p = po.make_prior(4, 4, seed=G + P, mean_pose=mean_pose())
        prior = fitting.PosePrior(**p).to(dev())
        x0 = po.make_rows(p, B, num_cam, seed=G)
    else:
        x0 = rng.normal(0.0, 1.0, (B, P)).astype(np.float32)
    x0 = np.where(tie != 0, np.repeat(x0[::G], G, axis=0), x0)         # tied columns enter equal within a group
    state = fitting.FitState.new(t(x0))
    cs = rng.uniform(0.5, 30.0, P).astype(np.float32)
    frozen = [1, num_cam + 40, P - 2]
    cs[frozen] = 0.0
    zero_cols = rng.choice(P, 5, replace=False)
    hist = torch.full((calls, B), float("nan"), device=dev())
    w = np.array([0.02, 0.01, 0.05], np.float32)
    kw = dict(lr=2e-3, beta1=0.9, beta2=0.999, eps=1e-7 if mode == "keras" else 1e-8, mode=mode, patience=0)
    lb = loss_bar(N, Ns if with_silh else 0)
    tie_d, smooth_d, cs_d, w_d = t(tie, torch.uint8), t(smooth) if with_smooth else None, t(cs), t(w)
    x_start = state.x.clone()
    for k in range(calls):
        g = log_uniform_grads(rng, B, P)
        g[rng.random((B, P)) < 0.05] = 0.0
        g[:, zero_cols] = 0.0
        loss = rng.exponential(0.05, (B, N)).astype(np.float32)
        silh = rng.exponential(0.3, (B, Ns)).astype(np.float32) if with_silh else None
        before = fo.from_tensors(state)                               # the oracle restarts from what the kernel left
        E = dE = None
        if with_prior:
            terms = fitting.prior_terms(state.x, prior, w_d, num_cam=num_cam)
            E, dE = terms["energy"][:, 3].cpu().numpy(), terms["grad"].cpu().numpy()
        fitting.fit_step(state, t(g), t(loss), t(silh) if with_silh else None, sw, cs_d, hist, grad_scale=0.3, group_size=G,
                         tie=tie_d, smooth=smooth_d, num_cam=num_cam, **(dict(prior=prior, prior_weights=w_d) if with_prior else {}),
                         **kw)
        torch.cuda.synchronize()
        after = fo.from_tensors(state)
        want, info = go.fit_step_group(before, g, loss, silh, sw, cs, None, G=G, tie=tie, smooth=smooth, E=E, dE=dE, gscale=0.3, **kw)
        for key in fo.INT_KEYS:
            assert np.array_equal(after[key], want[key]), (key, k, after[key], want[key])
        got_rows = hist[k].cpu().numpy().astype(np.float64)
        e_rows = np.abs(got_rows - info["L_rows"]) / info["L_rows_mag"]
        assert np.all(e_rows <= lb + U), (k, e_rows.max() / U)
        Lg, Lmag = np.repeat(info["L"], G), np.repeat(info["L_mag"], G)
        e_L = np.abs(after["best_loss"] - want["best_loss"]) / Lmag
        assert np.all(e_L <= lb + 2 * U), (k, e_L.max() / U)
        if k == 0:
            assert np.all(np.abs(after["best_loss"] - Lg) <= (lb + 2 * U) * Lmag)   # (the first call is a new best: L itself)
        assert np.array_equal(after["best_x"], want["best_x"])        # a copy of the kernel's own x: exact
        n = info["n_add"]
        safe = lambda a: np.where(a > 0, a, 1.0)
        mag_m = info["m_mag"] + 2.0 ** -50 / U * (1.0 - 0.9) * 0.3 * np.where(n >= 2, info["s_mag"], 0.0)
        em = np.abs(after["m"] - want["m"]) / safe(mag_m) / U
        ev = np.abs(after["v"] - want["v"]) / safe(info["v_mag"]) / U
        assert np.all(em <= (4 + n) * SLACK), (k, (em - n).max())
        assert np.all(ev <= (4 + 2 * n) * SLACK), (k, (ev - 2 * n).max())
        with np.errstate(divide="ignore", invalid="ignore"):
            kappa = np.where(want["v"] > 0, info["v_mag"] / want["v"], np.where(info["v_mag"] > 0, np.inf, 1.0))
            bar_x = (16 + n + np.where(n > 0, n * kappa, 0.0)) * SLACK
        ex = np.abs(after["x"] - want["x"])
        assert np.all(ex <= bar_x * U * info["dx_mag"] + U * np.maximum(np.abs(want["x"]), np.abs(after["x"]))), k
        moved = info["dx_mag"] > 0
        edx = np.maximum(ex - U * np.abs(after["x"]), 0.0)[moved] / info["dx_mag"][moved] / U
        seen.update(L_row=max(seen["L_row"], e_rows.max() / U), L=max(seen["L"], e_L.max() / U), lb=lb / U,
                    m=max(seen["m"], (em - n).max()), v=max(seen["v"], (ev - 2 * n).max()),
                    dx=max(seen["dx"], (edx - (n + np.where(n > 0, n * kappa, 0.0))[moved]).max()),
                    kappa=max(seen["kappa"], float(kappa[np.isfinite(kappa)].max())))
        # tied columns and the scalars are identical across a group; frozen and zero entries keep their bits
        xg = state.x.reshape(B // G, G, P)
        for name in ("x", "m", "v", "best_x"):
            a = getattr(state, name).reshape(B // G, G, P)[:, :, tie != 0]
            assert same_bits(a, a[:, :1].expand(-1, G, -1)), (name, k)
        for name in fo.INT_KEYS + ("best_loss",):
            a = getattr(state, name).reshape(B // G, G)
            assert same_bits(a, a[:, :1].expand(-1, G)), (name, k)
        assert same_bits(state.x[:, frozen], x_start[:, frozen])
        if not with_prior and not with_smooth:
            assert same_bits(state.x[:, zero_cols], x_start[:, zero_cols]) and not state.v[:, zero_cols].any()
    assert not same_bits(state.x, x_start) and int(state.t.min()) == calls and xg.shape[1] == G


@pytest.mark.parametrize("with_prior", [False, True])
@pytest.mark.parametrize("with_smooth", [False, True])
@pytest.mark.parametrize("tie_names", [("shape",), ("shape", "pose")])
@pytest.mark.parametrize("N", [144, 2305])
@pytest.mark.parametrize("P", [86, 256])
@pytest.mark.parametrize("G", [2, 3, 16])
def test_step_parity_teacher_forced(G, P, N, tie_names, with_smooth, with_prior):
    seen = dict(L_row=0.0, L=0.0, m=-9.0, v=-9.0, dx=-99.0, kappa=1.0, lb=0.0)
    case = G + (P == 256) + (N == 144) + len(tie_names) + with_smooth + with_prior
    mode, with_silh = ("keras", "torch")[case % 2], (case // 2) % 2 == 1
    for B in (G, 3 * G):
        parity_case(G, B, P, N, tie_names, with_smooth, with_prior, mode, with_silh, seen)
    print("fit_step_group parity G=%d P=%d N=%d tie=%s smooth=%d prior=%d %s silh=%d: max error in units of 2^-24: L_r %.2f (bar %.0f + 1), "
          "L %.2f (bar %.0f + 2), m %.2f over n (bar 4), v %.2f over 2 n (bar 4), step %.2f over n + n kappa (bar 16), kappa <= %.3g"
          % (G, P, N, "+".join(tie_names), with_smooth, with_prior, mode, with_silh, seen["L_row"], seen["lb"], seen["L"], seen["lb"],
             seen["m"], seen["v"], seen["dx"], seen["kappa"]))


def test_smoothness_alone():
    """g = 0, loss = 0, beta1 = 0, gscale = 1: best_loss = fp32(E_s) and m = fp32(s_r), seen directly.  Frames that differ by
    1e-3 of their values: the differences are taken in fp64."""
    fitting = fitting_module()
    G, K, P = 5, 3, 86
    B = G * K
    rng = np.random.default_rng(8)
    base = np.repeat(rng.normal(0.0, 1.0, (K, 1, P)), G, axis=1)
    x0 = (base * (1.0 + 1e-3 * rng.normal(0.0, 1.0, (K, G, P)))).reshape(B, P).astype(np.float32)
    tie = fitting.tie_mask().numpy()
    smooth = fitting.smooth_weights(cam=0.05, global_rot=0.5, pose=0.3, shape=9.0).numpy()      # (shape is tied: ignored)
    smooth[10] = 0.0
    state = fitting.FitState.new(t(x0))
    before = fo.from_tensors(state)
    z = np.zeros((B, P), np.float32)
    fitting.fit_step(state, t(z), t(np.zeros((B, 7), np.float32)), beta1=0.0, group_size=G, tie=t(tie, torch.uint8), smooth=t(smooth))
    torch.cuda.synchronize()
    want, info = go.fit_step_group(before, z, np.zeros((B, 7), np.float32), G=G, tie=tie, smooth=smooth, beta1=0.0)
    got_E = state.best_loss.cpu().numpy().astype(np.float64).reshape(K, G)
    assert np.all(got_E == got_E[:, :1]) and np.all(info["E_s"] > 0)
    eE = np.abs(got_E[:, 0] - info["E_s"])
    assert np.all(eE <= U * info["E_s"] + 2.0 ** -50 * info["E_s_mag"]), eE / info["E_s"] / U
    got_s = state.m.cpu().numpy().astype(np.float64)
    es = np.abs(got_s - info["s"])
    assert np.all(es <= U * np.abs(info["s"]) + 2.0 ** -50 * info["s_mag"])
    off = (tie != 0) | (smooth == 0)
    assert not got_s[:, off].any() and got_s[:, ~off].all() and same_bits(state.x[:, off], t(x0)[:, off])
    assert int(state.t.min()) == 1 and not same_bits(state.x, t(x0))
    print("smoothness alone: max error in units of 2^-24: E_s %.3f, s_r %.3f (bar 1)"
          % ((eE / info["E_s"]).max() / U, (es[:, ~off] / np.abs(info["s"][:, ~off])).max() / U))


# ---- 3. bookkeeping, exact ---------------------------------------------------------------------------------------------
def test_group_bookkeeping_exact():
    fitting = fitting_module()
    G, K, P, N, calls = 3, 3, 86, 144, 6
    B = G * K
    rng = np.random.default_rng(5)
    # constant rows of values with few mantissa bits: every sum and mean is exact in fp32 and in float64
    script = np.array([[6.0, 5.0, 4.0, 3.0, 2.0, 1.0], [1.0, 1.5, 1.0, 1.0, 1.0, 1.0], [2.0, 2.0, 2.0, 1.0, 1.0, 0.5],    # group 0 falls
                       [3.0, 2.0, 2.5, 2.75, 3.0, 3.25], [1.0, 1.0, 1.0, 1.0, 1.0, 1.0], [0.5, 0.5, 0.5, 0.5, 0.5, 0.5],  # group 1 rises from call 2
                       [5.0, 4.0, 3.0, 2.0, 2.0, 1.0], [1.0, 1.0, 1.0, np.inf, 0.5, 0.5], [1.0, 1.0, 1.0, 1.0, 0.5, 0.5]])  # group 2: bad calls
    x0 = make_x(B, 48, seed=9)
    tie = fitting.tie_mask(pose=True).numpy()
    x0 = np.where(tie != 0, np.repeat(x0[::G], G, axis=0), x0).astype(np.float32)
    state = fitting.FitState.new(t(x0))
    hist = torch.full((calls, B), float("nan"), device=dev())
    hist_want = np.full((calls, B), np.nan)
    snaps = []
    for k in range(calls):
        g = log_uniform_grads(rng, B, P)
        if k == 1:
            g[8, 17] = np.nan                                         # the last row of group 2
        loss = np.repeat(script[:, k:k + 1], N, axis=1).astype(np.float32)
        if k == 3:
            loss[7, 1:] = 1.0                                          # one inf among finite values
        before = fo.from_tensors(state)
        fitting.fit_step(state, t(g), t(loss), None, 1.0, None, hist, patience=2, group_size=G, tie=t(tie, torch.uint8))
        torch.cuda.synchronize()
        after = fo.from_tensors(state)
        want, _ = go.fit_step_group(before, g, loss, history=hist_want, patience=2, G=G, tie=tie)
        for key in fo.INT_KEYS + ("best_loss", "best_x"):
            assert np.array_equal(after[key], want[key]), (key, k, after[key], want[key])
        for key in fo.INT_KEYS:
            a = after[key].reshape(K, G)
            assert np.array_equal(a, np.repeat(a[:, :1], G, 1)), (key, k)
        a = state.x.reshape(K, G, P)[:, :, tie != 0]
        assert same_bits(a, a[:, :1].expand(-1, G, -1)), k
        snaps.append((after, state.x.clone(), state.m.clone(), state.v.clone()))
    assert np.array_equal(hist.cpu().numpy().astype(np.float64), hist_want, equal_nan=True)
    end = snaps[-1][0]
    assert end["t"].tolist() == [6] * 3 + [3] * 3 + [4] * 3 and end["calls"].tolist() == [6] * B
    assert end["bad"].tolist() == [0] * 6 + [2] * 3 and end["active"].tolist() == [1] * 3 + [0] * 3 + [1] * 3
    assert end["best_loss"].tolist() == [2.5] * 3 + [3.5] * 3 + [2.0] * 3 and end["best_step"].tolist() == [5] * 3 + [1] * 3 + [3] * 3
    assert [s[0]["active"][3] for s in snaps] == [1, 1, 1, 0, 0, 0]
    # the bad calls of group 2 change nothing of the group but `bad` and `calls`; the other groups moved in those calls
    for k in (1, 3):
        for j in (1, 2, 3):
            assert same_bits(snaps[k][j][6:], snaps[k - 1][j][6:])
            assert not same_bits(snaps[k][j][:3], snaps[k - 1][j][:3])
    assert not same_bits(snaps[1][1][3:6], snaps[0][1][3:6])
    for j in (1, 2, 3):
        assert bool(torch.isfinite(snaps[-1][j]).all())
        assert same_bits(snaps[2][j][3:6], snaps[5][j][3:6])            # a stopped group stays as it is


# ---- 4. groups are independent, launches repeat ------------------------------------------------------------------------
def test_groups_are_independent_and_launches_repeat(prior86):
    fitting = fitting_module()
    p, prior = prior86
    G, K, P, N, Ns = 4, 3, 86, 2305, 4096
    B = G * K
    rng = np.random.default_rng(11)
    tie = fitting.tie_mask().numpy()
    x0 = po.make_rows(p, B, 4, seed=4)
    s0 = fo.new_state(np.where(tie != 0, np.repeat(x0[::G], G, axis=0), x0))
    s0["m"] = np.where(tie != 0, np.repeat(rng.normal(0, 1e-2, (K, P)), G, axis=0), rng.normal(0, 1e-2, (B, P)))
    s0["v"] = np.where(tie != 0, np.repeat(rng.uniform(0, 1e-3, (K, P)), G, axis=0), rng.uniform(0, 1e-3, (B, P)))
    s0["t"][:] = np.repeat(rng.integers(0, 50, K), G)
    s0["best_loss"][:] = np.repeat(rng.uniform(0.0, 50.0, K), G)
    s0["active"][G:2 * G] = 0
    g, loss, silh = log_uniform_grads(rng, B, P), rng.exponential(0.05, (B, N)), rng.exponential(0.3, (B, Ns))
    g[2 * G + 1, 3] = np.inf
    cs, w = t(rng.uniform(0.0, 5.0, P)), t(np.array([0.02, 0.01, 0.05], np.float32))
    g, loss, silh = t(g), t(loss), t(silh)
    tie_d, smooth_d = t(tie, torch.uint8), fitting.smooth_weights(cam=0.05, global_rot=0.5, pose=0.3).to(dev())

    def run(lo, hi):
        st = state_from({k: a[lo:hi] for k, a in s0.items()})
        hist = torch.full((2, hi - lo), float("nan"), device=dev())
        fitting.fit_step(st, g[lo:hi].contiguous(), loss[lo:hi].contiguous(), silh[lo:hi].contiguous(), 0.5, cs, hist, mode="torch",
                         patience=3, prior=prior, prior_weights=w, group_size=G, tie=tie_d, smooth=smooth_d)
        torch.cuda.synchronize()
        return st, hist
    whole, hw = run(0, B)
    again, ha = run(0, B)
    for k in NAMES:
        assert same_bits(getattr(whole, k), getattr(again, k)), k
    assert same_bits(hw[0], ha[0])
    for q in range(K):
        one, h1 = run(q * G, q * G + G)
        for k in NAMES:
            assert same_bits(getattr(one, k), getattr(whole, k)[q * G:q * G + G]), (k, q)
        assert same_bits(h1[0], hw[0, q * G:q * G + G])
    assert whole.bad.tolist() == [0] * 8 + [1] * 4 and whole.t[G:2 * G].tolist() == s0["t"][G:2 * G].tolist()
    assert int(whole.t[0]) == int(s0["t"][0]) + 1


# ---- 5. the whole fit --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fit_time():
    spec = importlib.util.spec_from_file_location("fit_time", os.path.join(ROOT, "tools", "fit_time.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def fitter(smpl_model):
    return fitting_module().ParamFitter(smpl_model, img_wh=48, deterministic=True)


@pytest.fixture(scope="module")
def views(fitter, fit_time):
    """Two bodies, three views each: labels (6, 48, 48) = arg-max part maps of x* with one beta and one body pose per group
    under three global rotations and cameras (tools/fit_time.py `group_problem`); xs (6, 86) = x*."""
    labels, xs = fit_time.group_problem(fitter, 2, 3, 48, seed=0)
    return labels, xs


def stages():
    from ilps_amd.fitting import column_scale
    return [(20, column_scale(cam=100.0, pose=3.0, shape=0.0)), (20, column_scale(cam=20.0, pose=3.0, shape=3.0))]


def test_end_to_end_three_views(fitter, views):
    fitting = fitting_module()
    labels, xs = views
    G, K, B = 3, 2, 6
    tie = fitting.tie_mask(pose=True).to(dev()).bool()
    assert same_bits(xs[:, tie].reshape(K, G, -1), xs[::G][:, tie][:, None].expand(-1, G, -1)) and not same_bits(xs[0, :7], xs[1, :7])
    kw = dict(group_size=G, tie=("shape", "pose"), stages=stages(), history=True)
    r = fitter.fit(labels, **kw)
    hist = r.history.cpu().numpy().astype(np.float64)
    assert r.steps == 40 and hist.shape == (40, B) and np.isfinite(hist).all() and r.group_size == G
    start = hist[0].reshape(K, G).sum(1)
    best = r.loss.cpu().numpy().astype(np.float64).reshape(K, G)
    assert np.all(best == best[:, :1]) and np.all(best[:, 0] < start * (1.0 - 1e-6)), (best[:, 0], start)
    assert np.all(np.abs(best[:, 0] - hist.reshape(40, K, G).sum(2).min(0)) <= 4 * U * best[:, 0])
    for a in (r.x, r.final_x, r.state.m, r.state.v):
        a = a[:, tie].reshape(K, G, -1)
        assert same_bits(a, a[:, :1].expand(-1, G, -1))
    assert not same_bits(r.final_x[0, :7], r.final_x[1, :7])            # the views' own cameras and global rotations moved apart
    step = r.step.reshape(K, G)
    assert same_bits(step, step[:, :1].expand(-1, G)) and r.state.t.tolist() == [40] * B and int(r.nonfinite.sum()) == 0
    graph = fitter.fit(labels, graph=True, graph_steps=4, **kw)
    assert graph.steps == 40
    for k in ("x", "loss", "step", "final_x", "history"):
        assert same_bits(getattr(graph, k), getattr(r, k)), k
    for k in ("t", "m", "v", "calls", "best_x", "best_loss"):
        assert same_bits(getattr(graph.state, k), getattr(r.state, k)), k
    # beside three independent fits per body (recorded, not asserted: nobody has measured either)
    single = fitter.fit(labels, stages=stages())
    beta = lambda x: (x[:, 76:] - xs[:, 76:]).norm(dim=1).reshape(K, G).cpu().numpy()
    mean0 = fitter.initial(B, None, None, dev())
    print("three views, 40 iterations from the mean: |beta - beta*| start %s, tied fit %s, independent fits %s; group loss start %s best %s"
          % (beta(mean0)[:, 0].round(3).tolist(), beta(r.x)[:, 0].round(3).tolist(), beta(single.x).round(3).tolist(),
             start.round(5).tolist(), best[:, 0].round(5).tolist()))


def test_smoothed_clip_and_start_at_the_group_mean(fitter, views):
    fitting = fitting_module()
    labels, xs = views
    G, K, B = 3, 2, 6
    init = xs + 0.02 * torch.randn(xs.shape, generator=torch.Generator().manual_seed(1)).to(dev())
    sm = fitting.smooth_weights(cam=0.01, global_rot=0.1, pose=0.1)
    r = fitter.fit(labels, init=init, steps=6, group_size=G, tie=("shape",), smooth=sm, history=True, lr=2e-3)
    plain = fitter.fit(labels, init=init, steps=6, group_size=G, tie=("shape",), history=True, lr=2e-3)
    assert r.steps == 6 and bool(torch.isfinite(r.history).all()) and int(r.nonfinite.sum()) == 0
    # call 0: the rows' own losses do not see the penalty, the group's loss does; from call 1 on the iterates differ
    assert same_bits(r.history[0], plain.history[0]) and not same_bits(r.final_x, plain.final_x)
    # the start's tied columns are the group's mean, the others the caller's
    r0 = fitter.fit(labels, init=init, steps=0, group_size=G, tie=("shape",))
    mean = init[:, 76:].reshape(K, G, 10).mean(1, keepdim=True).expand(-1, G, -1).reshape(B, 10)
    beta0 = r0.final_x[:, 76:].reshape(K, G, 10)
    assert torch.allclose(r0.final_x[:, 76:], mean, rtol=0, atol=1e-6) and same_bits(beta0, beta0[:, :1].expand(-1, G, -1))
    assert same_bits(r0.final_x[:, :76], init[:, :76]) and r0.steps == 0
    with pytest.raises(ValueError):
        fitter.fit(labels[:5], steps=1, group_size=G)


def test_refine_predictions_in_groups(smpl_model, views):
    from ilps_amd.fitting import ParamFitter
    from ilps_amd.inference import refine_predictions
    from ilps_amd.keras_smpl.set_cam_params import load_mean_set_cam_params
    labels = views[0]

    class TinyEncoder(torch.nn.Module):                                # images -> (N, 86), as `model.SMPLRegressor` ends
        def __init__(self):
            super().__init__()
            self.fc = torch.nn.Linear(3 * 8 * 8, 86)

        def forward(self, images):
            return load_mean_set_cam_params(self.fc(images.flatten(1)) * 0.005, 48)
    torch.manual_seed(0)
    enc = TinyEncoder().to(dev())
    images = torch.rand(6, 3, 8, 8, device=dev())
    out = refine_predictions(enc, ParamFitter(smpl_model, img_wh=48), images, labels, steps=5, history=True, group_size=3)
    res = out["result"]
    assert res.group_size == 3 and res.steps == 5 and tuple(out["refined"].shape) == (6, 86) and tuple(res.history.shape) == (5, 6)
    beta = out["refined"][:, 76:].reshape(2, 3, 10)
    assert same_bits(beta, beta[:, :1].expand(-1, 3, -1)) and not same_bits(out["smpl"][0, 76:], out["smpl"][1, 76:])
    assert same_bits(out["loss"].reshape(2, 3), out["loss"].reshape(2, 3)[:, :1].expand(-1, 3))
    start = res.history[0].double().reshape(2, 3).sum(1)
    assert bool((out["loss"].reshape(2, 3)[:, 0].double() <= start * (1 + 4 * U)).all())
