"""The pose and shape priors on the GPU (csrc/prior_device.h: smplr_prior_energy, smplr_fit_step_prior, `fitting.PosePrior`)
against tests/_prior_oracle.py (NumPy float64).

Error bars, from the rounding counts in the header of csrc/prior_device.h (u = 2^-24, the relative error of one fp32 rounding
to nearest; none is taken from the kernel's output): the routine works in fp64 on the fp32 operands and rounds each output
to fp32 ONCE, so E_pose, E_angle, E_shape, E and every gradient entry are held to 1 u of their cancellation-free magnitude
(the sum of the absolute values of their terms, which the oracle returns), times (1 + 2^-16) for the fp64 work: fewer than
300 operations of 2^-53 each, under 2^-40 of the magnitude.  The winning component must be the oracle's on every row: the
seeded recipe's gap between the two lowest energies is asserted to be above 5 times the lowest (5.4 at the least over the
cases here), and the kernel's energies are good to 2^-24 of theirs.
The fused step's L = fp32(L_data + E): fit_step's own bar (tests/test_gpu_fitting.py `loss_bar`) on the total plus E's one
rounding.  The observed maxima are printed (pytest -s) and recorded in DESIGN.md section 16."""
import importlib.util
import math
import os

import numpy as np
import pytest
import torch

import _fitting_oracle as fo
import _prior_oracle as po

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
BAR = (1.0 + 2.0 ** -16) * U
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WEIGHTS = [(0.7, 1.3, 2.1), (1.5, 0.0, 0.0), (0.0, 0.8, 0.0), (0.0, 0.0, 3.0), (0.0, 0.0, 0.0)]


def fitting_module():
    """`ilps_amd.fitting` by the name the suite's other imports (`ilps_amd.smpl_model`, ...) use: one copy of every class."""
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


def loss_bar(N):
    """fit_step's bar on L (tests/test_gpu_fitting.py): a thread's serial share plus a binary tree over the threads."""
    fitting = fitting_module()
    return (math.ceil(N / fitting.THREADS) + math.ceil(math.log2(fitting.THREADS))) * U


def log_uniform_grads(rng, B, P):
    g = 10.0 ** rng.uniform(-8.0, 2.0, (B, P)) * rng.choice([-1.0, 1.0], (B, P))
    return g.astype(np.float32)


def mean_pose():
    from ilps_amd.smpl_model import load_mean_params
    return load_mean_params()[0]


def device_prior(p):
    fitting = fitting_module()
    return fitting.PosePrior(**p).to(dev())


def terms(x, prior, w, num_cam=4):
    """One stand-alone launch -> NumPy float64 (energy (B, 4), comp, grad)."""
    fitting = fitting_module()
    out = fitting.prior_terms(t(x), prior, w, num_cam=num_cam)
    torch.cuda.synchronize()
    return out["energy"].cpu().numpy().astype(np.float64), out["comp"].cpu().numpy(), out["grad"].cpu().numpy().astype(np.float64)


def rel(got, want, mag):
    """|got - want| in units of u of the magnitude; 0 where both are exactly 0."""
    err = np.abs(got - want)
    return np.where(mag > 0, err / np.where(mag > 0, mag, 1.0), np.where(err > 0, np.inf, 0.0)) / U


# ---- 1. parity, stand-alone --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,A,dense", [(K, A, False) for K in (1, 2, 8, 16) for A in (0, 4, 16)] + [(2, 4, True), (8, 4, True)])
def test_parity_stand_alone(K, A, dense):
    """dense: entries below the diagonal as well - rows 64..68 of A_k in full, the lanes of a wave's last row, the clamped
    column of lanes >= 5 (the recipe's upper-triangular factors hold zeros there)."""
    p = po.make_prior(K, A, seed=10 * K + A + 77 * dense, mean_pose=mean_pose(), dense=dense)
    assert bool(np.tril(p["factor"], -1).any()) == dense
    if A >= 2:
        assert p["angle_idx"][-1] == p["angle_idx"][0]                # a repeated index
    prior = device_prior(p)
    seen = dict(E_pose=0.0, E_angle=0.0, E_shape=0.0, E=0.0, grad=0.0)
    for B in (1, 5):
        for num_cam in (0, 3, 4):
            x = po.make_rows(p, B, num_cam, seed=K + A + B + num_cam)
            for w in WEIGHTS:
                want = po.prior(x, num_cam, p, w)
                energy, comp, grad = terms(x, prior, w, num_cam)
                assert np.all(want["gap"] > 5.0), want["gap"]
                assert np.array_equal(comp, want["comp"]), (B, num_cam, w, comp, want["comp"])
                for col, key in enumerate(("E_pose", "E_angle", "E_shape", "E")):
                    e = rel(energy[:, col], want[key], want[key + "_mag"])
                    assert np.all(e <= BAR / U), (key, B, num_cam, w, e.max())
                    seen[key] = max(seen[key], e.max())
                e = rel(grad, want["grad"], want["grad_mag"])
                assert np.all(e <= BAR / U), (B, num_cam, w, e.max())
                seen["grad"] = max(seen["grad"], e.max())
                # exact zeros: the camera and global-rotation columns (no angle index of the recipe names 0..2), the terms
                # whose weight is 0, and everything when all three are
                zero = want["grad_mag"] == 0
                assert zero[:, :num_cam + 3].all() and not grad[zero].any() and not np.signbit(grad[zero]).any()
                if w[0] == 0.0:
                    assert not energy[:, 0].any() and not comp.any()
                if w[1] == 0.0 or A == 0:
                    assert not energy[:, 1].any()
                if w[2] == 0.0:
                    assert not energy[:, 2].any() and not grad[:, num_cam + 72:].any()
                if w == (0.0, 0.0, 0.0):
                    assert not energy.any() and not grad.any()
    print("prior parity K=%d A=%d dense=%d: max error in units of 2^-24 (bar %.5f): E_pose %.3f, E_angle %.3f, E_shape %.3f, E %.3f, grad %.3f"
          % (K, A, dense, BAR / U, seen["E_pose"], seen["E_angle"], seen["E_shape"], seen["E"], seen["grad"]))


# ---- 2. rows are independent, launches repeat --------------------------------------------------------------------------
def test_rows_are_independent_and_launches_repeat():
    fitting = fitting_module()
    p = po.make_prior(16, 16, seed=3, mean_pose=mean_pose())
    prior = device_prior(p)
    B = 7
    x = t(po.make_rows(p, B, 4, seed=3))
    w = t(np.array([0.7, 1.3, 2.1], np.float32))
    whole = fitting.prior_terms(x, prior, w)
    again = fitting.prior_terms(x, prior, w)
    for k in ("energy", "comp", "grad"):
        assert same_bits(whole[k], again[k]), k
    for b in range(B):
        one = fitting.prior_terms(x[b:b + 1].contiguous(), prior, w)
        for k in ("energy", "comp", "grad"):
            assert same_bits(one[k][0], whole[k][b]), (k, b)
    assert len(set(whole["comp"].tolist())) > 1


# ---- 3. hostile rows ---------------------------------------------------------------------------------------------------
def hostile(p):
    """Row 0 plain; row 1 a theta entry inf; row 2 a theta entry NaN; row 3 angle_scale theta = 200 in the first angle term."""
    x = po.make_rows(p, 4, 4, seed=6)
    x[1, 4 + 20] = np.inf
    x[2, 4 + 41] = np.nan
    p["angle_scale"][0] = 2.0
    x[3, 4 + int(p["angle_idx"][0])] = 100.0
    return x


def test_hostile_rows_stand_alone():
    p = po.make_prior(4, 4, seed=6, mean_pose=mean_pose(), repeat=False)
    x = hostile(p)
    prior = device_prior(p)
    for w in ((1.0, 1.0, 1.0), (1.0, 0.0, 1.0)):
        want = po.prior(x, 4, p, w)
        energy, comp, grad = terms(x, prior, w)
        with np.errstate(over="ignore", invalid="ignore"):
            E32, g32 = want["E"].astype(np.float32), want["grad"].astype(np.float32)
        assert np.array_equal(np.isnan(energy[:, 3]), np.isnan(E32)) and np.array_equal(np.isinf(energy[:, 3]), np.isinf(E32))
        assert np.array_equal(np.isfinite(grad), np.isfinite(g32))
        assert np.array_equal(comp, want["comp"]) and comp.min() >= 0 and comp.max() < 4
        assert np.isfinite(energy[0]).all() and np.isfinite(grad[0]).all()
        assert not np.isfinite(energy[1, 3]) and not np.isfinite(energy[2, 3])
        # row 3: exp(200) = 7e86 is an fp64 number and an fp32 infinity; with w_angle = 0 the term is not evaluated
        assert np.isfinite(energy[3, 3]) == (w[1] == 0.0) and np.isfinite(grad[3]).all() == (w[1] == 0.0)
        if w[1] == 0.0:
            assert not energy[:, 1].any()
            e = rel(grad[3], want["grad"][3], want["grad_mag"][3])
            assert np.all(e <= BAR / U) and rel(energy[3, 3], want["E"][3], want["E_mag"][3]) <= BAR / U


def test_hostile_rows_are_bad_calls_in_the_fused_step():
    fitting = fitting_module()
    p = po.make_prior(4, 4, seed=6, mean_pose=mean_pose(), repeat=False)
    x = hostile(p)
    prior = device_prior(p)
    rng = np.random.default_rng(2)
    g, loss = t(log_uniform_grads(rng, 4, 86)), t(rng.exponential(0.05, (4, 144)))
    for w, bad_rows in (((1.0, 1.0, 1.0), [1, 2, 3]), ((1.0, 0.0, 1.0), [1, 2])):
        state = fitting.FitState.new(t(x))
        before = state.clone()
        hist = torch.full((2, 4), float("nan"), device=dev())
        for _ in range(2):
            fitting.fit_step(state, g, loss, history=hist, prior=prior, prior_weights=w)
        torch.cuda.synchronize()
        assert state.calls.tolist() == [2] * 4
        assert state.bad.tolist() == [2 if b in bad_rows else 0 for b in range(4)]
        for b in range(4):
            changed = [k for k in fo.FLOAT_KEYS + ("t", "stall", "best_step", "active")
                       if not same_bits(getattr(state, k)[b], getattr(before, k)[b])]
            if b in bad_rows:
                assert changed == [], (b, changed)                    # nothing but `bad` and `calls`
                assert not bool(torch.isfinite(hist[:, b]).any())
            else:
                assert {"x", "m", "v", "t", "best_loss"} <= set(changed) and int(state.t[b]) == 2, (b, changed)
                assert bool(torch.isfinite(hist[:, b]).all())


# ---- 4. fused = composed -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["keras", "torch"])
def test_fused_step_equals_prior_energy_then_plain_step(mode):
    fitting = fitting_module()
    B, P, N, calls = 5, 86, 144, 6
    p = po.make_prior(8, 4, seed=21, mean_pose=mean_pose())
    prior = device_prior(p)
    w = (0.02, 0.01, 0.05)
    wd = t(np.array(w, np.float32))
    rng = np.random.default_rng(17 + (mode == "torch"))
    x0 = t(po.make_rows(p, B, 4, seed=21))
    fused, composed = fitting.FitState.new(x0), fitting.FitState.new(x0)
    ints = fo.from_tensors(fused)
    hist = torch.full((calls, B), float("nan"), device=dev())
    cs = t(rng.uniform(0.5, 30.0, P))
    kw = dict(lr=2e-3, eps=1e-7 if mode == "keras" else 1e-8, mode=mode, patience=0, grad_scale=0.3)
    worst = 0.0
    for k in range(calls):
        g = log_uniform_grads(rng, B, P)
        loss = rng.exponential(0.05, (B, N)).astype(np.float32)
        xk = fused.x.cpu().numpy()
        want = po.prior(xk, 4, p, w)
        sep = fitting.prior_terms(composed.x, prior, wd)
        fitting.fit_step(fused, t(g), t(loss), None, 1.0, cs, hist, prior=prior, prior_weights=wd, **kw)
        fitting.fit_step(composed, t(g) + sep["grad"], t(loss), None, 1.0, cs, None, **kw)
        torch.cuda.synchronize()
        for key in ("x", "m", "v", "t"):
            assert same_bits(getattr(fused, key), getattr(composed, key)), (key, k)
        Ld = fo.row_loss(loss)
        L = Ld + want["E"]
        got = hist[k].cpu().numpy().astype(np.float64)
        bar = loss_bar(N) * (Ld + np.abs(want["E"])) + BAR * want["E_mag"]
        assert np.all(np.abs(got - L) <= bar), (k, np.abs(got - L) / bar)
        worst = max(worst, float(np.max(np.abs(got - L) / (U * (Ld + want["E_mag"])))))
        # the integer state: the fitting oracle on the totals
        g_tot = (t(g) + sep["grad"]).cpu().numpy()
        ints, _, _ = fo.fit_step(ints, g_tot, L[:, None].astype(np.float32), None, 1.0, cs.cpu().numpy(), None, lr=kw["lr"],
                                 eps=kw["eps"], gscale=0.3, mode=mode, patience=0)
        after = fo.from_tensors(fused)
        for key in fo.INT_KEYS:
            assert np.array_equal(after[key], ints[key]), (key, k, after[key], ints[key])
    assert int(fused.t.min()) == calls and not same_bits(fused.x, x0)
    print("fused step %s: L = L_data + E, max error %.2f in units of 2^-24 of L_data + |E| terms (bar %.0f + 1)"
          % (mode, worst, loss_bar(N) / U))


def test_without_a_prior_the_call_is_the_plain_one():
    fitting = fitting_module()
    rng = np.random.default_rng(4)
    x0 = t(rng.normal(0.0, 1.0, (3, 86)))
    g, loss = t(log_uniform_grads(rng, 3, 86)), t(rng.exponential(0.05, (3, 2305)))
    a, b = fitting.FitState.new(x0), fitting.FitState.new(x0)
    ha, hb = torch.zeros((3, 3), device=dev()), torch.zeros((3, 3), device=dev())
    for _ in range(3):
        fitting.fit_step(a, g, loss, history=ha, mode="torch")
        fitting.fit_step(b, g, loss, history=hb, mode="torch", prior=None, prior_weights=None, num_cam=4)
    torch.cuda.synchronize()
    for k in fo.FLOAT_KEYS + fo.INT_KEYS:
        assert same_bits(getattr(a, k), getattr(b, k)), k
    assert same_bits(ha, hb) and int(a.t.min()) == 3
    with pytest.raises(ValueError):
        fitting.fit_step(a, g, loss, prior_weights=(1.0, 1.0, 1.0))


# ---- 5. autograd -------------------------------------------------------------------------------------------------------
def test_prior_energy_is_differentiable():
    fitting = fitting_module()
    p = po.make_prior(8, 4, seed=31, mean_pose=mean_pose())
    prior = device_prior(p)
    w = (0.7, 1.3, 2.1)
    xn = po.make_rows(p, 3, 4, seed=31)
    want = po.prior(xn, 4, p, w)
    x = t(xn).requires_grad_(True)
    E = fitting.prior_energy(x, prior, w)
    assert tuple(E.shape) == (3,) and E.requires_grad
    E.sum().backward()
    g1 = x.grad.clone()
    assert np.all(rel(E.detach().cpu().numpy().astype(np.float64), want["E"], want["E_mag"]) <= BAR / U)
    assert np.all(rel(g1.cpu().numpy().astype(np.float64), want["grad"], want["grad_mag"]) <= BAR / U)
    x.grad = None
    up = torch.tensor([2.0, 0.0, -1.0], device=dev())
    (fitting.prior_energy(x, prior, w) * up).sum().backward()
    assert same_bits(x.grad, up[:, None] * g1) and not x.grad[1].any() and bool(x.grad[0].any())
    E2, out = fitting.prior_energy(x, prior, w, return_terms=True)     # the breakdown of the differentiable launch itself
    assert E2.requires_grad and not out["energy"].requires_grad and not out["grad"].requires_grad
    x.grad = None
    E2.sum().backward()
    assert same_bits(x.grad, g1) and same_bits(out["energy"][:, 3], E2)
    assert same_bits(E2, E) and same_bits(out["grad"], g1) and np.array_equal(out["comp"].cpu().numpy(), want["comp"])
    assert np.all(rel(out["energy"][:, 0].cpu().numpy().astype(np.float64), want["E_pose"], want["E_pose_mag"]) <= BAR / U)


def test_a_prior_of_the_wrong_layout_is_refused_before_the_launch():
    """Fields put on a device prior behind the constructor's back: the launchers get raw pointers, so the Python entry
    points refuse a wrong shape, dtype or stride and nothing is launched."""
    fitting = fitting_module()
    p = po.make_prior(2, 2, seed=1, mean_pose=mean_pose())
    good = device_prior(p)
    x = t(po.make_rows(p, 2, 4, seed=1))
    state = fitting.FitState.new(x)
    before = state.clone()
    g, loss = torch.zeros_like(x), torch.ones((2, 16), device=dev())
    broken = dict(factor=good.factor[:, :68].contiguous(), mean=good.mean[:, :68].contiguous(), offset=good.offset[:1].contiguous(),
                  angle_scale=good.angle_scale[:1].contiguous(), shape_mean=good.shape_mean[:9].contiguous(), angle_idx=None)
    broken["factor_t"] = good.factor.transpose(1, 2)                     # the right shape, not contiguous
    broken["idx64"] = good.angle_idx.long()
    for name, value in broken.items():
        bad = good.to(dev())
        setattr(bad, {"factor_t": "factor", "idx64": "angle_idx"}.get(name, name), value)
        with pytest.raises(RuntimeError):
            fitting.prior_terms(x, bad)
        with pytest.raises(RuntimeError):
            fitting.prior_energy(x, bad)
        with pytest.raises(RuntimeError):
            fitting.fit_step(state, g, loss, prior=bad)
    torch.cuda.synchronize()
    for k in fo.FLOAT_KEYS + fo.INT_KEYS:
        assert same_bits(getattr(state, k), getattr(before, k)), k
    # the constructor validates tensors that live on the device too, and hands back a CPU prior
    with pytest.raises(ValueError):
        fitting.PosePrior(mean=good.mean, factor=good.factor[:, :68], offset=good.offset)
    again = fitting.PosePrior(mean=good.mean, factor=good.factor, offset=good.offset)
    assert not again.mean.is_cuda and again.A == 0 and torch.equal(again.factor, good.factor.cpu())


# ---- 6. the whole fit --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fit_time():
    spec = importlib.util.spec_from_file_location("fit_time", os.path.join(ROOT, "tools", "fit_time.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def fitter(smpl_model):
    fitting = fitting_module()
    return fitting.ParamFitter(smpl_model, img_wh=48, deterministic=True)


@pytest.fixture(scope="module")
def problem(fitter, fit_time):
    labels, x0, _ = fit_time.problem(fitter, 2, 48, seed=0, pose_sigma=0.05, cam_shift=1.5)
    return labels, x0


def test_fit_with_annealed_prior_graph_equals_eager(fitter, problem):
    fitting = fitting_module()
    PosePrior, column_scale = fitting.PosePrior, fitting.column_scale
    labels, x0 = problem
    prior = PosePrior.mean_pose(0.5).with_angles()
    stages = [(6, column_scale(cam=20.0, pose=1.0, shape=0.0)), (6, column_scale(cam=0.0, pose=3.0, shape=1.0))]
    weights = [(0.05, 0.02, 0.0), (0.01, 0.005, 0.02)]
    kw = dict(init=x0, stages=stages, history=True, lr=2e-3, prior=prior, prior_weights=weights)
    eager = fitter.fit(labels, **kw)
    graph = fitter.fit(labels, graph=True, graph_steps=3, **kw)
    assert eager.steps == graph.steps == 12 and eager.state.t.tolist() == [12, 12] and int(eager.nonfinite.sum()) == 0
    for k in ("x", "loss", "step", "final_x", "history"):
        assert same_bits(getattr(graph, k), getattr(eager, k)), k
    for k in ("t", "m", "v", "calls", "best_x", "best_loss"):
        assert same_bits(getattr(graph.state, k), getattr(eager.state, k)), k
    # the trace holds L_data + E with the stage's weights: call 0 by `losses`, bit for bit; and the prior changed the fit
    assert same_bits(eager.history[0], fitter.losses(x0, labels, prior=prior, prior_weights=weights[0]))
    plain = fitter.fit(labels, init=x0, stages=stages, history=True, lr=2e-3)
    assert bool((eager.history[0] > plain.history[0]).all()) and not same_bits(eager.final_x, plain.final_x)
    one = fitter.fit(labels, **dict(kw, prior_weights=weights[0]))      # one triple for every stage: differs from stage 2 on
    assert same_bits(one.history[:6], eager.history[:6]) and not same_bits(one.history[6], eager.history[6])
    with pytest.raises(ValueError):
        fitter.fit(labels, **dict(kw, prior_weights=weights + weights))


def test_shape_prior_pulls_the_shape_to_its_mean(fitter, problem):
    fitting = fitting_module()
    labels, x0 = problem
    rng = np.random.default_rng(5)
    beta0 = x0[:, 76:].cpu().numpy().astype(np.float64)
    shape_mean = (beta0.max(0) + rng.uniform(0.5, 1.0, 10)).astype(np.float32)      # every row starts 0.5 or more below it
    prior = fitting.PosePrior.mean_pose(0.5).with_shape_mean(shape_mean)
    # the data term's gradient at the start, as the loop computes it
    x = x0.detach().clone().requires_grad_(True)
    seg_loss = fitter.decoder(x, labels)["seg_loss"]
    (g_data,) = torch.autograd.grad([seg_loss], [x], grad_outputs=[torch.full_like(seg_loss, 1.0 / seg_loss.shape[1])])
    g_data = g_data[:, 76:].abs().cpu().numpy().astype(np.float64)
    g_shape = fitting.prior_terms(x0, prior.to(dev()), (0.0, 0.0, 1.0))["grad"][:, 76:].abs().cpu().numpy().astype(np.float64)
    assert g_shape.min() >= 0.99
    w_shape = max(1.0, 101.0 * float((g_data / g_shape).max()))
    assert np.all(w_shape * g_shape >= 100.0 * g_data)
    stages = [(6, fitting.column_scale(cam=0.0, pose=0.0, shape=1.0)), (6, fitting.column_scale(cam=0.0, pose=0.0, shape=1.0))]
    r = fitter.fit(labels, init=x0, stages=stages, lr=1e-2, prior=prior, prior_weights=[(0.0, 0.0, w_shape), (0.0, 0.0, 2.0 * w_shape)])
    assert r.state.t.tolist() == [12, 12] and same_bits(r.final_x[:, :76], x0[:, :76])
    start = np.abs(beta0 - shape_mean.astype(np.float64))
    end = np.abs(r.final_x[:, 76:].cpu().numpy().astype(np.float64) - shape_mean.astype(np.float64))
    print("shape prior: w_shape %.3g, |beta - mean| from %s to %s" % (w_shape, start.round(3).tolist(), end.round(3).tolist()))
    assert np.all(end < start)
