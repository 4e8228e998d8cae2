"""The at::Tensor layer of the fit step on the device: torch.ops.smplraster.fit_step, fit_step_prior, fit_step_group and
prior_energy (csrc/torch_ops.cpp) beside the ctypes binding (`fitting.fit_step`, `fitting.prior_terms`).

Both bindings hand the same operands to the same launcher, so everything they leave behind agrees bit for bit: the eleven
fields of `FitState` and the history.  Each binding spells the list of operands out on its own; an operand that is swapped,
dropped or cast differently in one of them shows here as a difference.  The scalars are all distinct and none is a default."""
import numpy as np
import pytest
import torch

import _fitting_oracle as fo
import _prior_oracle as po
from test_gpu_fitting import dev, log_uniform_grads, same_bits, state_from, t

pytestmark = pytest.mark.gpu

NAMES = fo.FLOAT_KEYS + fo.INT_KEYS
B, P, N, NS, H, CALLS, K, A = 6, 86, 300, 70, 2, 3, 2, 2           # N > 256: a thread's strided sum takes a second trip
SCALARS = dict(lr=2e-3, beta1=0.85, beta2=0.995, eps=3e-7, grad_scale=0.3, patience=2)
SILH_WEIGHT = 0.7
CASES = {"plain": dict(G=1, prior=False, smooth=False, silh=False, mode="keras"),
         "prior": dict(G=1, prior=True, smooth=False, silh=True, mode="torch"),
         "group": dict(G=2, prior=False, smooth=False, silh=False, mode="torch"),
         "group_prior_smooth": dict(G=2, prior=True, smooth=True, silh=True, mode="keras")}


@pytest.fixture(scope="module")
def prior86():
    from ilps_amd import fitting
    from ilps_amd.smpl_model import load_mean_params
    p = po.make_prior(K, A, seed=33, mean_pose=load_mean_params()[0])
    return p, fitting.PosePrior(**p).to(dev())


def seeded_state(p, G, tie):
    """A state in mid-fit; with groups, the tied columns and the scalars of a group's rows are equal, as `fit` keeps them.
    The last group can never improve on its best loss, so patience = 2 stops it on the second call."""
    rng = np.random.default_rng(17 + G)
    per_group = lambda a: np.repeat(a[::G], G, axis=0)
    x0 = po.make_rows(p, B, 4, seed=6)
    s = fo.new_state(np.where(tie != 0, per_group(x0), x0))
    m, v = rng.normal(0, 1e-2, (B, P)), rng.uniform(0, 1e-3, (B, P))
    s["m"], s["v"] = np.where(tie != 0, per_group(m), m), np.where(tie != 0, per_group(v), v)
    s["t"][:] = per_group(rng.integers(0, 50, B))
    s["best_loss"][:] = per_group(rng.uniform(5.0, 50.0, B))
    s["best_loss"][B - G:] = 0.0
    return s


def op_step(ns, case, st, g, loss, silh, cs, hist, tie, smooth, pr, mode):
    from ilps_amd import fitting
    state = (st.x, g, st.m, st.v, st.t, st.calls, st.stall, st.bad, st.best_step, st.active, st.best_loss, st.best_x, loss, silh, cs,
             hist)
    k = SCALARS
    scalars = (k["lr"], k["beta1"], k["beta2"], k["eps"], k["grad_scale"], SILH_WEIGHT, fitting.MODES.index(mode), k["patience"])
    if case["G"] > 1:
        ns.fit_step_group(*state, tie, smooth, *(pr if case["prior"] else [None] * 7), case["G"], *scalars, 4)
    elif case["prior"]:
        ns.fit_step_prior(*state, *pr, *scalars, 4)
    else:
        ns.fit_step(*state, *scalars)


@pytest.mark.parametrize("name", list(CASES))
def test_op_and_ctypes_leave_the_same_bits(name, prior86):
    from ilps_amd import fitting, torch_ops
    ns = torch_ops.load()
    case = CASES[name]
    p, prior = prior86
    G, mode = case["G"], case["mode"]
    rng = np.random.default_rng(sorted(CASES).index(name))
    tie = fitting.tie_mask(shape=True, pose=True).numpy() if G > 1 else np.zeros(P, np.uint8)
    s0 = seeded_state(p, G, tie)
    by_py, by_op = state_from(fitting, s0, dev()), state_from(fitting, s0, dev())
    hists = [torch.full((H, B), float("nan"), device=dev()) for _ in range(2)]
    cs = rng.uniform(0.5, 30.0, P).astype(np.float32)
    cs[[2, 40, 80]] = 0.0
    cs = t(cs)
    tie_d = t(tie, torch.uint8) if G > 1 else None
    smooth_d = fitting.smooth_weights(cam=0.05, global_rot=0.5, pose=0.3).to(dev()) if case["smooth"] else None
    w = t(np.array([0.02, 0.01, 0.05], np.float32))
    pr = [prior.mean, prior.factor, prior.offset, prior.angle_idx, prior.angle_scale, prior.shape_mean, w]
    pkw = dict(prior=prior, prior_weights=w) if case["prior"] else {}
    gkw = dict(group_size=G, tie=tie_d, smooth=smooth_d) if G > 1 else {}
    x_start = by_py.x.clone()
    for k in range(CALLS):
        g = log_uniform_grads(rng, B, P)
        if k == 1:
            g[1, 9] = np.nan
        g = t(g)
        loss = t(rng.exponential(0.05, (B, N)))
        silh = t(rng.exponential(0.3, (B, NS))) if case["silh"] else None
        fitting.fit_step(by_py, g, loss, silh, SILH_WEIGHT, cs, hists[0], mode=mode, **SCALARS, **pkw, **gkw)
        op_step(ns, case, by_op, g, loss, silh, cs, hists[1], tie_d, smooth_d, pr, mode)
        torch.cuda.synchronize()
        for field in NAMES:
            assert same_bits(getattr(by_op, field), getattr(by_py, field)), (field, k)
    assert same_bits(hists[1], hists[0]) and bool(torch.isfinite(hists[0]).all())
    # the calls did what they were set up to do: the history bound was crossed, one bad call, one stop, the rest moved
    assert by_py.calls.tolist() == [CALLS] * B and by_py.bad.tolist() == ([1, 1, 0, 0, 0, 0] if G > 1 else [0, 1, 0, 0, 0, 0])
    assert by_py.active[B - G:].tolist() == [0] * G and by_py.stall[B - G:].tolist() == [2] * G
    assert bool((by_py.t[:B - G].cpu() > torch.as_tensor(s0["t"][:B - G])).all()) and by_py.t[B - G:].tolist() == (s0["t"][B - G:] + 1).tolist()
    assert not same_bits(by_py.x[:B - G], x_start[:B - G]) and same_bits(by_py.x[:, [2, 40, 80]], x_start[:, [2, 40, 80]])


@pytest.mark.parametrize("with_grad", [True, False])
def test_prior_energy_op_and_ctypes_leave_the_same_bits(with_grad, prior86):
    from ilps_amd import fitting, torch_ops
    ns = torch_ops.load()
    p, prior = prior86
    x = t(po.make_rows(p, B, 4, seed=8))
    w = t(np.array([0.7, 0.2, 1.5], np.float32))
    want = fitting.prior_terms(x, prior, w, 4, with_grad)
    energy, comp, grad = ns.prior_energy(x, prior.mean, prior.factor, prior.offset, prior.angle_idx, prior.angle_scale,
                                         prior.shape_mean, w, 4, with_grad)
    torch.cuda.synchronize()
    assert tuple(energy.shape) == (B, 4) and same_bits(energy, want["energy"]) and bool(torch.isfinite(energy).all())
    assert comp.dtype == torch.int32 and same_bits(comp, want["comp"])
    if with_grad:
        assert tuple(grad.shape) == (B, P) and same_bits(grad, want["grad"]) and bool(grad.any())
    else:
        assert tuple(grad.shape) == (0, P) and want["grad"] is None
