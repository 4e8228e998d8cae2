"""smplr_lbfgs_step (csrc/lbfgs.hip) and the fitters' mode="lbfgs" on the GPU, against tests/_lbfgs_oracle.py.

Error bars of the teacher-forced test, in ulps of fp32, derived from the rounding count of each field's definition (none is
taken from the kernel's output).  Before every launch the oracle's state, loss values and gradient are loaded to the device, so
both sides start a call from the same fp32 values:
  integers, phase, active   exact.
  x0, g0, S, Y, best_x      0: copies of loaded values, or ONE fp32 operation on loaded values (g^ = c (gscale g): two products,
                            each correctly rounded from the same operands; s = alpha d; y = g^ - g0).
  history, f0, best_loss    1: L is rounded once from the fp64 tree sum (the fp32 strided sums below it are exact restatements).
  d, gd, alpha              1: rounded once from fp64 (the two-loop recursion's q, the dot product, lr min(1, 1 / |g|_1)); a halved
                            alpha is exact.
  x                         1 + 3: rule 9's three fp32 operations on an alpha and a d of 1 ulp each.
The oracle forms every fp64 sum by the kernel's own tree, so the observed maxima (printed, pytest -s) are expected to be 0.
Entries a call does not touch - where the oracle's state after the call equals the one before it - keep their bits."""
import importlib
import importlib.util
import os

import numpy as np
import pytest
import torch

import _lbfgs_cases as cases
import _lbfgs_oracle as o
import _prior_oracle as po
from test_gpu_fitting import dev, same_bits, t

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ULPS = dict(x=4, d=1, gd=1, alpha=1, f0=1, best_loss=1, x0=0, g0=0, S=0, Y=0, best_x=0)


@pytest.fixture(scope="module")
def fitting():
    return importlib.import_module("ilps_amd.fitting")


def ordered(a):
    """fp32 values -> int64 that count representable numbers in order (-0 = +0 = 0)."""
    i = np.asarray(a, np.float32).view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7FFFFFFF), i)


def ulps(got, want):
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    both_nan = np.isnan(got) & np.isnan(want)
    return np.where(both_nan, 0, np.abs(ordered(got) - ordered(want)))


def state_from(fitting, s, device=None):
    """The oracle's dict -> an LbfgsState on the device."""
    device = device or dev()
    f = lambda a: torch.as_tensor(np.ascontiguousarray(a, np.float32)).to(device)
    i = lambda a: torch.as_tensor(np.ascontiguousarray(a, np.int32)).to(device)
    u = lambda a: torch.as_tensor(np.ascontiguousarray(a, np.uint8)).to(device)
    return fitting.LbfgsState(**{k: f(s[k]) for k in o.FLOAT_KEYS},
                              **{k: (u if k in ("active", "phase") else i)(s[k]) for k in o.INT_KEYS})


def params_kw(p):
    return dict(lr=p["lr"], c1=p["c1"], max_ls=p["max_ls"], tol_grad=p["tol_grad"], grad_scale=p["gscale"], patience=p["patience"])


# ---- 1. teacher-forced trajectories ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 3, 16])
@pytest.mark.parametrize("P", [1, 65, 86, 256])
def test_step_parity_teacher_forced(fitting, P, M):
    r = cases.script(P, M)
    assert set(o.BRANCHES) - r["branches"] <= ({"ring_wrap"} if (P, M) == (1, 16) else set())
    cs = t(r["col_scale"])
    calls = len(r["steps"])
    seen = {k: 0 for k in ULPS}
    seen["history"] = 0
    for k, s in enumerate(r["steps"]):
        state = state_from(fitting, s["before"])
        hist = torch.full((calls, r["B"]), float("nan"), device=dev())
        fitting.lbfgs_step(state, t(s["g"]), t(s["loss"]), None, 1.0, cs, hist, **params_kw(s["params"]))
        torch.cuda.synchronize()
        got, want, before = o.from_tensors(state), s["after"], s["before"]
        for key in o.INT_KEYS:
            assert np.array_equal(got[key], want[key]), (key, k, got[key], want[key])
        for key, bar in ULPS.items():
            e = ulps(got[key], want[key])
            seen[key] = max(seen[key], int(e.max()))
            assert e.max() <= bar, (key, k, int(e.max()), np.argwhere(e > bar)[:4].tolist())
            still = np.float32(want[key]).view(np.int32) == np.float32(before[key]).view(np.int32)
            assert np.array_equal(np.float32(got[key])[still].view(np.int32), np.float32(before[key])[still].view(np.int32)), (key, k)
        h = hist.cpu().numpy()
        row = s["before"]["calls"]                                  # (every row has made k calls)
        assert np.all(row == k)
        e = ulps(h[k], s["L"])
        seen["history"] = max(seen["history"], int(e.max()))
        assert e.max() <= 1 and np.isnan(np.delete(h, k, axis=0)).all()
    print("lbfgs step parity P=%d M=%d: max ulps %s" % (P, M, seen))


# ---- 2. a row's outputs are the same bits alone and inside a batch ---------------------------------------------------------
def test_batch_independence(fitting):
    r = cases.script(86, 3)
    cs = t(r["col_scale"])
    for k in (0, 9, 12, 31):
        s = r["steps"][k]
        whole = state_from(fitting, s["before"])
        hw = torch.full((1, r["B"]), float("nan"), device=dev())
        whole.calls.zero_()
        fitting.lbfgs_step(whole, t(s["g"]), t(s["loss"]), None, 1.0, cs, hw, **params_kw(s["params"]))
        for b in range(r["B"]):
            one = state_from(fitting, {key: a[b:b + 1] for key, a in s["before"].items()})
            one.calls.zero_()
            h1 = torch.full((1, 1), float("nan"), device=dev())
            fitting.lbfgs_step(one, t(s["g"][b:b + 1]), t(s["loss"][b:b + 1]), None, 1.0, cs, h1, **params_kw(s["params"]))
            for key in o.FLOAT_KEYS + o.INT_KEYS:
                assert same_bits(getattr(one, key)[0], getattr(whole, key)[b]), (key, b, k)
            assert same_bits(h1[0], hw[0, b:b + 1])


# ---- 3. the prior form = the plain form fed the prior's E and gradient by hand --------------------------------------------
@pytest.fixture(scope="module")
def prior86(fitting):
    from ilps_amd.smpl_model import load_mean_params
    p = po.make_prior(2, 2, seed=33, mean_pose=load_mean_params()[0])
    return p, fitting.PosePrior(**p).to(dev())


def test_prior_form_equals_the_plain_form_fed_by_hand(fitting, prior86):
    p, prior = prior86
    B, P, M = 4, 86, 3
    rng = np.random.default_rng(5)
    w = t(np.array([0.7, 0.2, 1.5], np.float32))
    cs = t(rng.uniform(0.5, 2.0, P).astype(np.float32))
    a = fitting.LbfgsState.new(t(po.make_rows(p, B, 4, seed=6)), M)
    b = a.clone()
    ha, hb = (torch.full((8, B), float("nan"), device=dev()) for _ in range(2))
    kw = dict(lr=0.5, c1=1e-4, max_ls=3, tol_grad=0.0, grad_scale=0.7, patience=0)
    target = t(po.make_rows(p, B, 4, seed=7))
    for k in range(8):
        assert same_bits(a.x, b.x)
        x = a.x.clone()
        g = (x - target) * 0.3                                       # a data term 0.15 |x - target|^2: N = 1 loss value per row
        loss = (0.15 * (x - target).double().square().sum(1)).float()[:, None].contiguous()
        terms = fitting.prior_terms(x, prior, w, 4)
        fitting.lbfgs_step(a, g, loss, None, 1.0, cs, ha, prior=prior, prior_weights=w, num_cam=4, **kw)
        # by hand: L = fp32((double)l + (double)E) - N = 1, so the plain form's mean is the value itself - and g + dE in fp32
        loss_b = (loss[:, 0].double() + terms["energy"][:, 3].double()).float()[:, None].contiguous()
        fitting.lbfgs_step(b, g + terms["grad"], loss_b, None, 1.0, cs, hb, **kw)
        for key in o.FLOAT_KEYS + o.INT_KEYS:
            assert same_bits(getattr(a, key), getattr(b, key)), (key, k)
    assert same_bits(ha, hb) and int(a.t.max()) >= 1 and int(a.phase.max()) == 1


# ---- 4. both bindings ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_prior", [False, True])
def test_op_and_ctypes_leave_the_same_bits(fitting, prior86, with_prior):
    from ilps_amd import torch_ops
    ns = torch_ops.load()
    p, prior = prior86
    r = cases.script(86, 3, calls=14)
    cs = t(r["col_scale"])
    w = t(np.array([0.7, 0.2, 1.5], np.float32))
    pr = (prior.mean, prior.factor, prior.offset, prior.angle_idx, prior.angle_scale, prior.shape_mean, w)
    rng = np.random.default_rng(2)
    for k in (0, 6, 9, 13):
        s = r["steps"][k]
        a, b = state_from(fitting, s["before"]), state_from(fitting, s["before"])
        for st in (a, b):
            st.calls.zero_()
        g, loss, silh = t(s["g"]), t(s["loss"]), t(rng.exponential(0.3, (r["B"], 70)).astype(np.float32))
        ha, hb = (torch.full((2, r["B"]), float("nan"), device=dev()) for _ in range(2))
        scal = dict(lr=0.8, c1=2e-4, max_ls=2, tol_grad=1e-9, grad_scale=0.5, patience=5)
        fitting.lbfgs_step(a, g, loss, silh, 0.7, cs, ha, **(dict(prior=prior, prior_weights=w, num_cam=4) if with_prior else {}), **scal)
        tensors = (b.x, g, b.x0, b.g0, b.d, b.S, b.Y, b.f0, b.gd, b.alpha, b.ls, b.pairs, b.phase, b.t, b.calls, b.stall, b.bad,
                   b.best_step, b.active, b.best_loss, b.best_x, loss, silh, cs, hb)
        scalars = (scal["lr"], scal["c1"], scal["max_ls"], scal["tol_grad"], scal["grad_scale"], 0.7, scal["patience"])
        if with_prior:
            ns.lbfgs_step_prior(*tensors, *pr, *scalars, 4)
        else:
            ns.lbfgs_step(*tensors, *scalars)
        for key in o.FLOAT_KEYS + o.INT_KEYS:
            assert same_bits(getattr(a, key), getattr(b, key)), (key, k)
        assert same_bits(ha, hb) and not torch.isnan(ha[0, :3]).any()         # (row 3's loss is a NaN at call 0, by the script)


def test_launchers_refuse_bad_arguments(fitting):
    st = fitting.LbfgsState.new(torch.zeros((2, 5), device=dev()), 2)
    g, loss = torch.zeros((2, 5), device=dev()), torch.zeros((2, 7), device=dev())
    for bad in (dict(lr=0.0), dict(c1=1.0), dict(c1=0.0), dict(max_ls=-1), dict(tol_grad=-1.0), dict(patience=-1)):
        with pytest.raises(RuntimeError, match="smplr_lbfgs_step"):
            fitting.lbfgs_step(st, g, loss, **bad)
    assert int(st.calls.sum()) == 0


# ---- 5. the free-running quadratic -----------------------------------------------------------------------------------------
def test_free_running_quadratic_and_graph_replay(fitting):
    """P = 8, condition 1e2, M = 16, 40 launches, value and gradient evaluated by torch on the device (fp64, rounded to fp32):
    the CPU test's bar, |g|_inf <= 1e-5 |g(x_start)|_inf; and 10 replays of 4 captured iterations leave the eager loop's bits."""
    P, M, B = 8, 16, 3
    funs = [cases.quadratic(P, 1e2, 200 + b) for b in range(B)]
    # the quadratics as device tensors: f_b(x) = 1/2 (x - m_b)^T A_b (x - m_b); A and m recovered from the seeded functions
    ms, As = [], []
    for f, _ in funs:
        g0 = f(np.zeros(P))[1]                                       # = -A m
        Amat = np.stack([f(np.eye(P)[i])[1] - g0 for i in range(P)], 1)
        As.append(Amat)
        ms.append(np.linalg.solve(Amat, -g0))
    A, m = t(np.stack(As), torch.float64), t(np.stack(ms), torch.float64)
    x_start = t(np.stack([xs for _, xs in funs]))

    def evaluate(x):
        r = x.double() - m
        Ar = torch.einsum("bij,bj->bi", A, r)
        return (0.5 * (r * Ar).sum(1)).float()[:, None].contiguous(), Ar.float().contiguous()

    def body(state, hist):
        loss, g = evaluate(state.x)
        fitting.lbfgs_step(state, g, loss, None, 1.0, None, hist)

    eager = fitting.LbfgsState.new(x_start, M)
    he = torch.full((40, B), float("nan"), device=dev())
    for _ in range(40):
        body(eager, he)
    torch.cuda.synchronize()
    g_start, g_end = evaluate(x_start)[1].abs().amax(1), evaluate(eager.x0)[1].abs().amax(1)
    print("free-running quadratic: |g|_inf %s -> %s" % (g_start.tolist(), g_end.tolist()))
    assert bool((g_end <= 1e-5 * g_start).all())
    assert bool((eager.best_loss <= he[0]).all()) and int(eager.bad.sum()) == 0
    graph = fitting.LbfgsState.new(x_start, M)
    hg = torch.full((40, B), float("nan"), device=dev())
    replay = fitting._capture(body, (graph.clone(), None), (graph, hg), 4, dev())
    for _ in range(10):
        replay()
    torch.cuda.synchronize()
    for key in o.FLOAT_KEYS + o.INT_KEYS:
        assert same_bits(getattr(eager, key), getattr(graph, key)), key
    assert same_bits(he, hg)


# ---- 6. the fitters --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fit_time():
    spec = importlib.util.spec_from_file_location("fit_time", os.path.join(ROOT, "tools", "fit_time.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def two_stages(fitting, n):
    cs = fitting.column_scale
    return [(n, cs(cam=10.0, pose=0.0, shape=0.0)), (n, cs(cam=10.0, pose=1.0, shape=0.0))]


def check_fitter(fitting, monkeypatch, fit, first_loss, x0, n):
    """fit(**kw) -> FitResult with two stages of n evaluations, the shape block frozen in both (the pose block in the first)."""
    trace = []
    real = fitting.lbfgs_step

    def recording(state, *a, **kw):
        out = real(state, *a, **kw)
        trace.append({k: getattr(state, k).clone() for k in ("f0", "t", "pairs", "phase", "active")})
        return out
    monkeypatch.setattr(fitting, "lbfgs_step", recording)
    kw = dict(init=x0, stages=two_stages(fitting, n), mode=fitting.Lbfgs(memory=3, max_ls=4), history=True)
    r = fit(**kw)
    monkeypatch.setattr(fitting, "lbfgs_step", real)
    B = x0.shape[0]
    assert r.optimizer == "lbfgs" and isinstance(r.state, fitting.LbfgsState) and r.steps == 2 * n == len(trace)
    assert r.history.shape == (2 * n, B) and same_bits(r.history[0], first_loss) and bool(torch.isfinite(r.history).all())
    # the losses of accepted iterates never increase within a stage
    accepted = 0
    for k in range(1, 2 * n):
        if k == n:
            continue                                                  # (a new objective: f0 starts over)
        a, b_ = trace[k - 1], trace[k]
        assert bool((b_["f0"] <= a["f0"]).all()), k
        moved = b_["t"] > a["t"]
        assert bool((b_["f0"][moved] < a["f0"][moved]).all()) and same_bits(b_["f0"][~moved], a["f0"][~moved])
        accepted += int(moved.sum())
    assert accepted >= 1
    # best_loss <= the start's loss; frozen columns keep the start's bits
    assert bool((r.loss <= r.history[0]).all()) and bool((r.loss < r.history[0]).any())
    for x in (r.x, r.final_x, r.state.x, r.state.x0):
        assert same_bits(x[:, 76:], x0[:, 76:])
    assert same_bits(r.final_x, r.state.x0) and not same_bits(r.final_x[:, :4], x0[:, :4])
    # restart() at the boundary: the first call of the second stage starts a search with an empty memory
    assert int(trace[n - 1]["pairs"].max()) > 0 and int(trace[n]["pairs"].abs().sum()) == 0
    assert bool((trace[n]["phase"][trace[n]["active"] != 0] == 1).all())
    # the graph run equals the eager run bit for bit
    g = fit(graph=True, graph_steps=3, **kw)
    assert g.steps == r.steps
    for key in ("x", "loss", "step", "final_x", "history", "nonfinite"):
        assert same_bits(getattr(r, key), getattr(g, key)), key
    for key in o.FLOAT_KEYS + o.INT_KEYS:
        assert same_bits(getattr(r.state, key), getattr(g.state, key)), key
    return r


def test_keypoint_fitter_with_lbfgs(fitting, monkeypatch, smpl_model):
    fitter = fitting.KeypointFitter(smpl_model, sigma=6.0, img_wh=48)
    B, K = 2, fitter.spec.K
    rng = np.random.default_rng(12)
    x0 = fitter.initial(B, device=dev())
    d = np.zeros((B, 86), np.float32)
    d[:, 2:4] = rng.normal(0, 1.5, (B, 2))
    d[:, 4:76] = rng.normal(0, 0.15, (B, 72))
    with torch.no_grad():
        _, det, _ = fitter.terms(x0 + t(d), torch.zeros((B, K, 2), device=dev()), torch.ones((B, K), device=dev()))
    target, conf = det["proj"].clone(), t(rng.uniform(0.3, 1.0, (B, K)))
    r = check_fitter(fitting, monkeypatch, lambda **kw: fitter.fit(target, conf, **kw), fitter.losses(x0, target, conf), x0, 12)
    print("KeypointFitter lbfgs: loss %s -> %s" % (r.history[0].tolist(), r.loss.tolist()))


def test_param_fitter_with_lbfgs(fitting, monkeypatch, smpl_model, fit_time):
    fitter = fitting.ParamFitter(smpl_model, img_wh=48, deterministic=True)
    labels, x0, _ = fit_time.problem(fitter, 2, 48, seed=0, pose_sigma=0.05, cam_shift=1.5)
    r = check_fitter(fitting, monkeypatch, lambda **kw: fitter.fit(labels, **kw), fitter.losses(x0, labels), x0, 12)
    print("ParamFitter lbfgs: loss %s -> %s" % (r.history[0].tolist(), r.loss.tolist()))


def test_lbfgs_refuses_groups_on_the_device(fitting, smpl_model):
    fitter = fitting.KeypointFitter(smpl_model, img_wh=48)
    K = fitter.spec.K
    target, conf = torch.zeros((4, K, 2), device=dev()), torch.ones((4, K), device=dev())
    for kw in (dict(group_size=2), dict(smooth=fitting.smooth_weights(pose=1.0))):
        with pytest.raises(ValueError, match="lbfgs"):
            fitter.fit(target, conf, steps=2, mode="lbfgs", **kw)


# ---- 7. Adam is what it was ------------------------------------------------------------------------------------------------
def test_adam_is_unchanged_beside_lbfgs(fitting, smpl_model):
    """A fit that names Adam's mode gives the bits of one that leaves it out, on a `FitState`, through smplr_fit_step alone."""
    fitter = fitting.KeypointFitter(smpl_model, sigma=6.0, img_wh=48)
    B, K = 2, fitter.spec.K
    rng = np.random.default_rng(3)
    target, conf = t(rng.uniform(10.0, 38.0, (B, K, 2))), t(rng.uniform(0.3, 1.0, (B, K)))
    calls = []
    real = fitting.lbfgs_step
    fitting.lbfgs_step = lambda *a, **kw: calls.append(1) or real(*a, **kw)
    try:
        a = fitter.fit(target, conf, steps=6, history=True)
        b = fitter.fit(target, conf, steps=6, history=True, mode="torch")
    finally:
        fitting.lbfgs_step = real
    assert not calls and a.optimizer == b.optimizer == "adam" and type(a.state) is fitting.FitState
    for key in ("x", "loss", "final_x", "history"):
        assert same_bits(getattr(a, key), getattr(b, key)), key
    assert same_bits(a.state.m, b.state.m) and same_bits(a.state.v, b.state.v) and same_bits(a.final_x, a.state.x)
