"""smplr_fit_step (csrc/fit.hip) and `fitting.ParamFitter` on the GPU, against tests/_fitting_oracle.py (NumPy float64).

Error bars of the step-parity test, derived from the kernel's operation count (u = 2^-24, the relative error of one fp32
rounding to nearest; none is taken from the kernel's output):
  L   a sum of non-negative fp32 terms: every rounding adds at most u relative to the running sum, the issue's bar is
      (ceil(N / THREADS) + ceil(log2 THREADS)) u - the serial share of a thread plus a binary tree over the threads.  The
      kernel stays inside it: ceil(N / THREADS) - 1 fp32 additions per thread, the tree in fp64, one rounding to fp32.  With a
      silhouette term L is a sum of two such means, and a non-negative sum is as accurate as its worse term: N is the larger
      of N and Ns.
  m   4 u relative to |b1 m| + |(1 - b1) g^| (the terms' magnitudes: m itself may cancel): g^ = gscale g, (1 - b1) g^ and the
      fused multiply-add are three roundings.
  v   4 u relative to v (no cancellation): g^, (1 - b2) g^, b2 v, and the fused multiply-add.
  x   16 u relative to the step's magnitude D (the step with |b1 m| + |(1 - b1) g^| in place of m) - at most 13 roundings
      reach the step: m 3, sqrt(v) 2 + 1, [torch: the fp32 sqrt(1 - b2^t) 1 and the division 1,] + eps 1, the division 1, the
      fp32 step factor 1, its product with col_scale 1, the last product 1 - plus u |x| for the subtraction that stores x.
The observed maxima are printed (pytest -s) and recorded in DESIGN.md section 14."""
import importlib.util
import math
import os

import numpy as np
import pytest
import torch

import _fitting_oracle as fo
from _inputs import make_x

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def t(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(dev())


def bits(a):
    a = a.detach().cpu().contiguous()
    return a.view(torch.int32) if a.dtype == torch.float32 else a


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def loss_bar(N, Ns=0):
    from ilps_amd.fitting import THREADS
    return (math.ceil(max(N, Ns) / THREADS) + math.ceil(math.log2(THREADS))) * U


def log_uniform_grads(rng, B, P):
    g = 10.0 ** rng.uniform(-8.0, 2.0, (B, P)) * rng.choice([-1.0, 1.0], (B, P))
    return g.astype(np.float32)


def state_from(fitting, s, device):
    """The oracle's dict -> a FitState on the device."""
    f = lambda a: torch.as_tensor(np.asarray(a, np.float32)).to(device)
    i = lambda a: torch.as_tensor(np.asarray(a, np.int32)).to(device)
    return fitting.FitState(x=f(s["x"]), m=f(s["m"]), v=f(s["v"]), best_x=f(s["best_x"]), t=i(s["t"]), calls=i(s["calls"]),
                            stall=i(s["stall"]), bad=i(s["bad"]), best_step=i(s["best_step"]),
                            active=torch.as_tensor(np.asarray(s["active"], np.uint8)).to(device), best_loss=f(s["best_loss"]))


# ---- 1. step parity, teacher-forced ------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["keras", "torch"])
@pytest.mark.parametrize("with_silh", [False, True])
@pytest.mark.parametrize("N", [144, 2304, 2305])
def test_step_parity_teacher_forced(N, with_silh, mode):
    from ilps_amd import fitting
    B, P, Ns, calls = 5, 86, 64 * 64, 6
    rng = np.random.default_rng(N + 7 * with_silh + (mode == "torch"))
    state = fitting.FitState.new(t(make_x(B, 48, seed=3)))
    cs = rng.uniform(0.5, 30.0, P).astype(np.float32)
    frozen = [2, 40]
    cs[frozen] = 0.0
    zero_row = 3
    zero_cols = rng.choice(P, 6, replace=False)                      # entries whose g is 0 in every call: m = v = 0 throughout
    hist = torch.full((calls, B), float("nan"), device=dev())
    kw = dict(lr=2e-3, beta1=0.9, beta2=0.999, eps=1e-7 if mode == "keras" else 1e-8, mode=mode, patience=0)
    sw = 0.7
    seen = dict(L=0.0, m=0.0, v=0.0, dx=0.0)
    x_start = state.x.clone()
    for k in range(calls):
        g = log_uniform_grads(rng, B, P)
        g[rng.random((B, P)) < 0.05] = 0.0
        g[:, zero_cols] = 0.0
        g[zero_row] = 0.0
        loss = rng.exponential(0.05, (B, N)).astype(np.float32)
        silh = rng.exponential(0.3, (B, Ns)).astype(np.float32) if with_silh else None
        before = fo.from_tensors(state)                               # the oracle restarts from what the kernel left
        fitting.fit_step(state, t(g), t(loss), t(silh) if with_silh else None, sw, t(cs), hist, grad_scale=0.3, **kw)
        torch.cuda.synchronize()
        after = fo.from_tensors(state)
        want, L, terms = fo.fit_step(before, g, loss, silh, sw, cs, None, gscale=0.3, **kw)
        for key in fo.INT_KEYS:
            assert np.array_equal(after[key], want[key]), (key, k)
        got_L = hist[k].cpu().numpy().astype(np.float64)
        eL = np.abs(got_L - L) / L
        assert np.all(eL <= loss_bar(N, Ns if with_silh else 0)), (k, eL.max())
        assert np.all(np.abs(after["best_loss"] - want["best_loss"]) <= loss_bar(N, Ns if with_silh else 0) * want["best_loss"])
        assert np.array_equal(after["best_x"], want["best_x"])        # a copy of the kernel's own x: exact
        em = np.abs(after["m"] - want["m"]) / np.where(terms["m_mag"] > 0, terms["m_mag"], 1.0)
        ev = np.abs(after["v"] - want["v"]) / np.where(terms["v_mag"] > 0, terms["v_mag"], 1.0)
        assert np.all(em <= 4 * U) and np.all(ev <= 4 * U), (k, em.max() / U, ev.max() / U)
        ex = np.abs(after["x"] - want["x"])
        assert np.all(ex <= 16 * U * terms["dx_mag"] + U * np.maximum(np.abs(want["x"]), np.abs(after["x"]))), k
        moved = terms["dx_mag"] > 0
        edx = np.max(np.maximum(ex - U * np.abs(after["x"]), 0.0)[moved] / terms["dx_mag"][moved])
        seen = dict(L=max(seen["L"], eL.max()), m=max(seen["m"], em.max()), v=max(seen["v"], ev.max()), dx=max(seen["dx"], edx))
        # frozen columns, the zero row and the zero entries keep their bits
        assert same_bits(state.x[:, frozen], x_start[:, frozen])
        assert same_bits(state.x[zero_row], x_start[zero_row]) and same_bits(state.x[:, zero_cols], x_start[:, zero_cols])
        assert not state.m[zero_row].any() and not state.v[:, zero_cols].any()
    assert not same_bits(state.x, x_start) and int(state.t.min()) == calls
    print("fit_step parity N=%d silh=%d %s: max error in units of 2^-24: L %.2f (bar %.0f), m %.2f (4), v %.2f (4), step %.2f (16)"
          % (N, with_silh, mode, seen["L"] / U, loss_bar(N, Ns if with_silh else 0) / U, seen["m"] / U, seen["v"] / U, seen["dx"] / U))


# ---- 2. row bookkeeping, exact -----------------------------------------------------------------------------------------
def test_row_bookkeeping_exact():
    from ilps_amd import fitting
    B, P, N, calls = 4, 86, 144, 6
    rng = np.random.default_rng(5)
    # constant rows of values with few mantissa bits: every sum and mean is exact in fp32 and in float64
    script = np.array([[6.0, 5.0, 4.0, 3.0, 2.0, 1.0],               # strictly decreasing
                       [3.0, 2.0, 2.5, 2.75, 3.0, 3.25],             # rises from call 2 on
                       [5.0, 4.0, 3.0, np.inf, 2.0, 1.0],            # + NaN in g at call 1, inf in loss at call 3
                       [2.0, 2.0, 2.0, 2.0, 2.0, 2.0]])              # equal losses
    state = fitting.FitState.new(t(make_x(B, 48, seed=9)))
    hist = torch.full((calls, B), float("nan"), device=dev())
    hist_want = np.full((calls, B), np.nan)
    xs, snaps = [], []
    for k in range(calls):
        g = log_uniform_grads(rng, B, P)
        if k == 1:
            g[2, 17] = np.nan
        loss = np.repeat(script[:, k:k + 1], N, axis=1).astype(np.float32)
        if k == 3:
            loss[2, 1:] = 1.0                                          # one inf among finite values
        before = fo.from_tensors(state)
        xs.append(state.x.clone())
        fitting.fit_step(state, t(g), t(loss), None, 1.0, None, hist, patience=2)
        torch.cuda.synchronize()
        after = fo.from_tensors(state)
        want, L, _ = fo.fit_step(before, g, loss, history=hist_want, patience=2)
        for key in fo.INT_KEYS + ("best_loss", "best_x"):
            assert np.array_equal(after[key], want[key]), (key, k, after[key], want[key])
        snaps.append((after, state.x.clone(), state.m.clone(), state.v.clone()))
    assert np.array_equal(hist.cpu().numpy().astype(np.float64), hist_want, equal_nan=True)
    end = snaps[-1][0]
    # row 0
    assert end["t"][0] == 6 and end["best_step"][0] == 5 and end["best_loss"][0] == 1.0 and end["active"][0] == 1
    assert same_bits(state.best_x[0], xs[5][0])
    # row 1: best at call 1, two stalls, stopped at call 3, frozen afterwards
    assert end["active"][1] == 0 and end["t"][1] == 3 and end["best_step"][1] == 1 and end["best_loss"][1] == 2.0
    assert same_bits(state.best_x[1], xs[1][1])
    assert [s[0]["active"][1] for s in snaps] == [1, 1, 1, 0, 0, 0]
    assert same_bits(snaps[2][1][1], snaps[5][1][1]) and same_bits(snaps[2][2][1], snaps[5][2][1])
    assert not same_bits(snaps[1][1][1], snaps[2][1][1])              # (the first stall still updates)
    # row 2: two bad calls change nothing but `bad` and `calls`
    assert end["bad"][2] == 2 and end["t"][2] == 4 and end["calls"][2] == 6 and end["active"][2] == 1
    for k in (1, 3):
        for j in (1, 2, 3):
            assert same_bits(snaps[k][j][2], snaps[k - 1][j][2])
    assert torch.isfinite(state.x[2]).all() and torch.isfinite(state.m[2]).all() and torch.isfinite(state.v[2]).all()
    assert end["best_loss"][2] == 1.0 and end["best_step"][2] == 3
    # row 3: strict <
    assert end["best_step"][3] == 0 and end["best_loss"][3] == 2.0 and end["active"][3] == 0
    assert same_bits(state.best_x[3], xs[0][3])
    assert np.array_equal(end["bad"], [0, 0, 2, 0])


# ---- 3. rows are independent -------------------------------------------------------------------------------------------
def test_rows_are_independent_and_launches_repeat():
    from ilps_amd import fitting
    B, P, N, Ns = 7, 86, 2305, 4096
    rng = np.random.default_rng(11)
    s0 = fo.new_state(make_x(B, 48, seed=4))
    s0["m"] = rng.normal(0, 1e-2, (B, P))
    s0["v"] = rng.uniform(0, 1e-3, (B, P))
    s0["t"][:] = rng.integers(0, 50, B)
    s0["best_loss"][:] = rng.uniform(0.0, 0.2, B)
    s0["active"][5] = 0
    g, loss, silh = log_uniform_grads(rng, B, P), rng.exponential(0.05, (B, N)), rng.exponential(0.3, (B, Ns))
    g[6, 3] = np.inf
    cs = t(rng.uniform(0.0, 5.0, P))
    g, loss, silh = t(g), t(loss), t(silh)

    def run(lo, hi):
        st = state_from(fitting, {k: a[lo:hi] for k, a in s0.items()}, dev())
        hist = torch.full((2, hi - lo), float("nan"), device=dev())
        fitting.fit_step(st, g[lo:hi].contiguous(), loss[lo:hi].contiguous(), silh[lo:hi].contiguous(), 0.5, cs, hist,
                         mode="torch", patience=3)
        torch.cuda.synchronize()
        return st, hist
    whole, hw = run(0, B)
    again, ha = run(0, B)
    names = fo.FLOAT_KEYS + fo.INT_KEYS
    for k in names:
        assert same_bits(getattr(whole, k), getattr(again, k)), k
    assert same_bits(hw[0], ha[0])
    for b in range(B):
        one, h1 = run(b, b + 1)
        for k in names:
            assert same_bits(getattr(one, k)[0], getattr(whole, k)[b]), (k, b)
        assert same_bits(h1[0], hw[0, b:b + 1])
    assert int(whole.bad[6]) == 1 and int(whole.t[5]) == int(s0["t"][5])


# ---- 4 - 6: the loop ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fit_time():
    spec = importlib.util.spec_from_file_location("fit_time", os.path.join(ROOT, "tools", "fit_time.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def fitter(smpl_model):
    from ilps_amd.fitting import ParamFitter
    return ParamFitter(smpl_model, img_wh=48, deterministic=True)


@pytest.fixture(scope="module")
def problem(fitter, fit_time):
    """labels (3, 48, 48) = arg-max of the decoder's scores at x* = make_x(3, 48); init = x* with pose noise and a camera
    shift (tools/fit_time.py `problem`, the stock loop's inputs as well)."""
    labels, x0, xs = fit_time.problem(fitter, 3, 48, seed=0, pose_sigma=0.05, cam_shift=1.5)
    return labels, x0, xs


def stages():
    from ilps_amd.fitting import column_scale
    return [(20, column_scale(cam=100.0, pose=0.0, shape=0.0)), (20, column_scale(cam=0.0, pose=3.0, shape=0.0))]


@pytest.fixture(scope="module")
def fitted(fitter, problem):
    labels, x0, _ = problem
    return fitter.fit(labels, init=x0, stages=stages(), history=True)


def test_end_to_end_two_stages(fitter, problem, fitted, fit_time):
    labels, x0, _ = problem
    r = fitted
    B = 3
    hist = r.history.cpu().numpy()
    assert hist.shape == (40, B) and r.steps == 40 and np.isfinite(hist).all()
    # history[0] is the loss of init, computed separately: by the loop's own reduction bit for bit, and in float64
    L0 = fitter.losses(x0, labels)
    assert same_bits(r.history[0], L0)
    with torch.no_grad():
        per_pixel = fitter.decoder(x0, labels)["seg_loss"]
    L64 = fo.row_loss(per_pixel.cpu().numpy())
    assert np.all(np.abs(hist[0] - L64) <= loss_bar(48 * 48) * L64)
    best = r.loss.cpu().numpy()
    print("fit: start", hist[0], "best", best, "at", r.step.cpu().numpy())
    assert np.all(best < hist[0])
    assert np.array_equal(best, hist.min(axis=0)) and np.array_equal(r.step.cpu().numpy(), hist.argmin(axis=0))
    assert same_bits(fitter.losses(r.x, labels), r.loss)              # the best iterate reproduces its loss
    assert same_bits(r.x[:, 76:], x0[:, 76:]) and same_bits(r.final_x[:, 76:], x0[:, 76:])
    assert not same_bits(r.final_x[:, :4], x0[:, :4]) and not same_bits(r.final_x[:, 4:76], x0[:, 4:76])
    assert int(r.nonfinite.sum()) == 0 and bool(r.active.all()) and np.array_equal(r.state.t.cpu().numpy(), [40] * B)
    # the stock loop improves every row on the same inputs: the problem is not a hard one
    _, sbest, _, shist = fit_time.stock_fit(fitter.decoder, labels, x0, 40, lr=1e-2, history=True)
    print("stock: start", shist[0].cpu().numpy(), "best", sbest.cpu().numpy())
    assert bool((sbest < shist[0]).all())


def test_first_stage_moves_the_camera_only(fitter, problem):
    labels, x0, _ = problem
    r = fitter.fit(labels, init=x0, stages=stages()[:1], history=True)
    assert same_bits(r.final_x[:, 4:], x0[:, 4:]) and not same_bits(r.final_x[:, :4], x0[:, :4])


def test_nan_row_is_counted_and_isolated(fitter, problem, fitted):
    labels, x0, _ = problem
    bad = x0[:1].clone()
    bad[0, 4:76] = float("nan")
    x4 = torch.cat([x0, bad])
    lab4 = torch.cat([labels, labels[:1]])
    r = fitter.fit(lab4, init=x4, stages=stages(), history=True)
    assert int(r.nonfinite[3]) == 40 == r.steps and r.nonfinite[:3].tolist() == [0, 0, 0]
    assert same_bits(r.final_x[3], x4[3]) and same_bits(r.x[3], x4[3]) and int(r.state.t[3]) == 0
    assert math.isinf(float(r.loss[3]))
    for got, want in ((r.x[:3], fitted.x), (r.final_x[:3], fitted.final_x), (r.loss[:3], fitted.loss), (r.step[:3], fitted.step),
                      (r.history[:, :3], fitted.history)):
        assert same_bits(got, want)


def test_graph_replay_equals_eager(fitter, problem):
    labels, x0, _ = problem
    kw = dict(init=x0, steps=12, history=True, lr=2e-3)
    eager = fitter.fit(labels, **kw)
    graph = fitter.fit(labels, graph=True, graph_steps=4, **kw)
    assert graph.steps == eager.steps == 12
    for k in ("x", "loss", "step", "final_x", "history"):
        assert same_bits(getattr(graph, k), getattr(eager, k)), k
    for k in ("t", "m", "v", "calls", "best_x", "best_loss"):
        assert same_bits(getattr(graph.state, k), getattr(eager.state, k)), k
    assert graph.state.t.tolist() == [12, 12, 12]
    # a step count that is no multiple of G: two replays and two eager iterations
    odd = fitter.fit(labels, graph=True, graph_steps=4, init=x0, steps=10, history=True, lr=2e-3)
    assert same_bits(odd.history, eager.history[:10]) and odd.state.t.tolist() == [10, 10, 10]


def test_patience_and_check_every_stop_early(fitter, problem):
    labels, x0, _ = problem
    r = fitter.fit(labels, init=x0, steps=30, lr=0.0, patience=2, check_every=3, history=True)
    # lr = 0: the loss never improves after call 0, every row stalls twice and stops at call 2; the check at 3 sees it
    assert r.steps == 3 and not bool(r.active.any()) and r.state.t.tolist() == [2, 2, 2] and r.step.tolist() == [0, 0, 0]
    assert same_bits(r.final_x, x0) and r.history.shape == (3, 3)


def test_refine_predictions_and_fit_debug_model(smpl_model, problem):
    from ilps_amd.fitting import ParamFitter
    from ilps_amd.inference import refine_predictions
    from ilps_amd.keras_smpl.set_cam_params import load_mean_set_cam_params
    from ilps_amd.model import EmbeddedSMPLParams, fit_debug_model
    labels = problem[0][:2]

    class TinyEncoder(torch.nn.Module):                                # images -> (N, 86), as `model.SMPLRegressor` ends
        def __init__(self):
            super().__init__()
            self.fc = torch.nn.Linear(3 * 8 * 8, 86)

        def forward(self, images):
            return load_mean_set_cam_params(self.fc(images.flatten(1)) * 0.005, 48)
    torch.manual_seed(0)
    enc = TinyEncoder().to(dev())
    images = torch.rand(2, 3, 8, 8, device=dev())
    fitter = ParamFitter(smpl_model, img_wh=48)
    out = refine_predictions(enc, fitter, images, labels, steps=5, history=True)
    assert tuple(out["smpl"].shape) == tuple(out["refined"].shape) == (2, 86) and tuple(out["loss"].shape) == (2,)
    assert out["result"].steps == 5 and tuple(out["result"].history.shape) == (5, 2)
    assert torch.allclose(out["smpl"], enc(images).detach(), rtol=1e-6, atol=1e-6)
    assert bool((out["loss"] <= fitter.losses(out["smpl"], labels)).all())
    table = EmbeddedSMPLParams(48)
    idx = torch.tensor([3, 7])
    with torch.no_grad():
        start = table(idx).to(dev())
    model, res = fit_debug_model(labels, smpl_model, 48, 32, indices=idx, steps=5, smpl_model=table, history=True)
    assert model is table and tuple(res.x.shape) == (2, 86) and res.steps == 5
    assert same_bits(res.history[0], fitter.losses(start, labels)) and bool((res.loss <= res.history[0]).all())
    with torch.no_grad():
        assert torch.allclose(table(idx), res.x.cpu(), atol=1e-5)
