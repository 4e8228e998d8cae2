"""Per-row L-BFGS, without a GPU: the oracle's own checks (tests/_lbfgs_oracle.py restates smplr_lbfgs_step's rules 1 - 9) -
every branch of the state machine on seeded inputs, convergence on quadratics and Rosenbrock's function - and the host side of
`fitting`: the `Lbfgs` record, `LbfgsState`, `restart()`, argument errors."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _lbfgs_cases as cases  # noqa: E402
import _lbfgs_oracle as o  # noqa: E402

import importlib  # noqa: E402

fitting = importlib.import_module("ilps_amd.fitting")   # (the name the suite's fixtures import the package under)

MACHINE = set(o.BRANCHES)


@pytest.fixture(scope="module")
def scripts():
    return {(P, M): cases.script(P, M) for P in (1, 86) for M in (1, 3, 16)}


@pytest.mark.parametrize("P, M", [(1, 1), (1, 3), (1, 16), (86, 1), (86, 3), (86, 16)])
def test_the_script_reaches_every_branch(scripts, P, M):
    """accept, shrink, ring wrap (pairs > M), curvature skip, non-descent reset, max_ls reset, line-search failure, tol_grad
    stop, patience stop, a bad call in each phase, a start and an inactive row: each reached, and asserted.  A single column
    cannot fill 16 pairs (a 1-D quadratic is solved by its first pair): there the ring wraps at M = 1 and 3 only."""
    r = scripts[(P, M)]
    want = MACHINE - ({"ring_wrap"} if (P, M) == (1, 16) else set())
    assert want - r["branches"] == set(), sorted(want - r["branches"])
    rows = lambda name: {b for s in r["steps"] for b, ev in enumerate(s["events"]) if name in ev}
    assert 0 in rows("accept") and rows("shrink")
    assert rows("curvature_skip") >= {1} and 2 in rows("max_ls_reset") and 2 in rows("ls_failure")
    assert 3 in rows("bad_phase0") and 3 in rows("bad_phase1") and 3 in rows("nondescent_reset")
    assert rows("patience_stop") and 5 in rows("tol_grad_stop")
    if P > 1:                                              # (a single column has converged and stopped before its wall comes)
        assert 4 in rows("patience_stop")
    if (P, M) != (1, 16):
        assert int(max(s["after"]["pairs"].max() for s in r["steps"])) > M


def test_what_each_branch_leaves_behind(scripts):
    r = scripts[(86, 3)]
    for s in r["steps"]:
        a, b_, pr = s["after"], s["before"], s["params"]
        for b, ev in enumerate(s["events"]):
            assert a["calls"][b] == b_["calls"][b] + 1
            if "bad_phase0" in ev or "inactive" in ev:
                for k in a:
                    if k not in ("calls", "bad"):
                        assert np.array_equal(a[k][b], b_[k][b], equal_nan=True), k
                assert a["bad"][b] == b_["bad"][b] + ("bad_phase0" in ev)
            if "bad_phase1" in ev:
                assert a["bad"][b] == b_["bad"][b] + 1 and a["stall"][b] == b_["stall"][b]
                assert ev & {"shrink", "max_ls_reset", "ls_failure"}
            if "shrink" in ev:
                assert a["alpha"][b] == 0.5 * b_["alpha"][b] and a["ls"][b] == b_["ls"][b] + 1
                assert np.array_equal(a["x0"][b], b_["x0"][b]) and a["t"][b] == b_["t"][b]
            if "accept" in ev:
                assert a["t"][b] == b_["t"][b] + 1 and np.array_equal(a["x0"][b], b_["x"][b]) and a["f0"][b] == s["L"][b]
                assert s["L"][b] <= b_["f0"][b] + np.float32(pr["c1"]) * b_["alpha"][b] * b_["gd"][b]
                if a["active"][b]:
                    assert a["ls"][b] == 0 and a["phase"][b] == 1 and a["gd"][b] < 0
            if "curvature_skip" in ev:
                assert a["pairs"][b] in (b_["pairs"][b], 0)
            if "max_ls_reset" in ev:
                assert b_["pairs"][b] > 0 and a["pairs"][b] == 0 and a["ls"][b] == 0 and a["active"][b] == 1
                assert np.array_equal(a["d"][b], -b_["g0"][b])
            if "ls_failure" in ev:
                assert b_["pairs"][b] == 0 and a["active"][b] == 0 and np.array_equal(a["x"][b], b_["x"][b])
            if "nondescent_reset" in ev:
                assert a["pairs"][b] == 0 and np.array_equal(a["d"][b], -a["g0"][b])
            if ev & {"tol_grad_stop", "patience_stop"}:
                assert a["active"][b] == 0 and np.array_equal(a["x"][b], b_["x"][b])


@pytest.mark.parametrize("P, M", [(86, 3), (256, 16)])
def test_frozen_columns_keep_their_bits(P, M):
    r = cases.script(P, M, calls=20)
    frozen = r["col_scale"] == 0
    assert frozen.any() and not frozen.all()
    start = r["steps"][0]["before"]["x"]
    moved = False
    for s in r["steps"]:
        for k in ("x", "x0", "best_x"):
            assert np.array_equal(s["after"][k][:, frozen], start[:, frozen]), k
        assert np.all(s["after"]["d"][:, frozen] == 0) and np.all(s["after"]["g0"][:, frozen] == 0)
        moved |= bool((s["after"]["x"][:, ~frozen] != start[:, ~frozen]).any())
    assert moved


def test_tree_sum_is_the_butterfly():
    rng = np.random.default_rng(3)
    v = rng.normal(size=200) * 10.0 ** rng.uniform(-8, 8, 200)
    w = np.zeros(256)
    w[:200] = v
    waves = []
    for k in range(4):                                     # the butterfly of a wave, spelled as the tree it is
        a = w[64 * k:64 * k + 64]
        for o_ in (32, 16, 8, 4, 2, 1):
            a = a[:o_] + a[o_:2 * o_]
        waves.append(a[0])
    assert o.tree_sum(v) == (waves[0] + waves[1]) + (waves[2] + waves[3])
    assert abs(o.tree_sum(v) - np.sum(v)) <= 1e-13 * np.abs(v).sum()
    assert o.row_loss(np.full((1, 300), 0.25, np.float32))[0] == 0.25


# ---- convergence: the prototype's results with a margin of 30 x or more, on differently seeded instances ----------------
def test_quadratic_p8_condition_1e2():
    fun, xs = cases.quadratic(8, 1e2, 123)
    g_start = np.abs(fun(o.f32(xs))[1]).max()
    st, _ = o.minimise(fun, xs, 40, memory=16)
    assert np.abs(fun(st["x0"][0])[1]).max() <= 1e-5 * g_start


def test_quadratic_p86_condition_1e4():
    fun, xs = cases.quadratic(86, 1e4, 123)
    f_start = fun(o.f32(xs))[0]
    st, _ = o.minimise(fun, xs, 320, memory=8)
    assert fun(st["x0"][0])[0] <= 1e-6 * f_start


def test_rosenbrock_p10_stops_by_itself():
    st, trace = o.minimise(cases.rosenbrock, np.full(10, -1.2), 100, memory=8)
    assert len(trace) <= 100 and st["active"][0] == 0 and trace[-1] & {"ls_failure", "tol_grad_stop"}
    assert np.abs(st["x0"][0] - 1.0).max() <= 1e-4
    assert st["best_loss"][0] == st["f0"][0] and np.array_equal(st["best_x"][0], st["x0"][0])


def test_column_scales_precondition():
    """The method works in z = x / c: on f(x) = 1/2 sum_j a_j x_j^2 the scales c_j = a_j^-1/2 make the problem's Hessian the identity
    in z, and the search converges in a handful of evaluations where the unscaled one needs many."""
    a = np.logspace(0, 4, 12)
    fun = lambda x: (0.5 * np.sum(a * x * x), a * x)
    xs = np.ones(12)
    plain, _ = o.minimise(fun, xs, 8, memory=8)
    scaled, _ = o.minimise(fun, xs, 8, memory=8, col_scale=(a ** -0.5).astype(np.float32))
    assert fun(scaled["x0"][0])[0] <= 1e-10 * fun(xs)[0] < 1e-6 * fun(plain["x0"][0])[0]


# ---- the host side ------------------------------------------------------------------------------------------------------------
def test_lbfgs_record_and_mode():
    assert fitting.Lbfgs() == fitting.Lbfgs(memory=8, c1=1e-4, max_ls=10, tol_grad=0.0, lr=1.0)
    assert fitting.check_mode("lbfgs") == fitting.Lbfgs() and fitting.check_mode("keras") is None and fitting.check_mode("torch") is None
    opt = fitting.Lbfgs(memory=16, max_ls=0)
    assert fitting.check_mode(opt) is opt
    for bad in (dict(memory=0), dict(memory=17), dict(memory=2.5), dict(memory=True), dict(c1=0.0), dict(c1=1.0), dict(max_ls=-1),
                dict(tol_grad=-1.0), dict(tol_grad=float("nan")), dict(lr=0.0), dict(lr=float("inf"))):
        with pytest.raises(ValueError):
            fitting.Lbfgs(**bad)
    for bad in ("adam", "LBFGS", None, 1):
        with pytest.raises(ValueError, match="mode"):
            fitting.check_mode(bad)
    with pytest.raises(ValueError, match="Adam only"):
        fitting.check_mode("lbfgs", lbfgs=False)


def test_state_new_and_restart_on_cpu_tensors():
    x = torch.arange(12, dtype=torch.float64).reshape(3, 4)
    st = fitting.LbfgsState.new(x, memory=5)
    assert st.memory == 5 and st.S.shape == (3, 5, 4) and st.Y.shape == (3, 5, 4) and st.x.dtype == torch.float32
    assert not hasattr(st, "m") and not hasattr(st, "v")
    names = {f.name for f in __import__("dataclasses").fields(fitting.FitState)} - {"m", "v"}
    assert names <= {f.name for f in __import__("dataclasses").fields(st)}
    assert torch.equal(st.x0, st.x) and st.x0.data_ptr() != st.x.data_ptr() and torch.equal(st.best_x, st.x)
    assert int(st.phase.sum()) == 0 and int(st.pairs.sum()) == 0 and bool(st.active.all()) and bool(torch.isinf(st.best_loss).all())
    for bad in (0, 17, 1.5):
        with pytest.raises(ValueError, match="memory"):
            fitting.LbfgsState.new(x, memory=bad)
    st.phase[:] = torch.tensor([1, 0, 1], dtype=torch.uint8)
    st.x += 100.0
    st.pairs[:] = torch.tensor([3, 9, 0], dtype=torch.int32)
    st.ls[:] = 2
    st.t[:] = 7
    st.best_loss[:] = 0.5
    ref = o.restart(o.from_tensors(st))
    keep = st.clone()
    assert st.restart() is st
    assert torch.equal(st.x[0], keep.x0[0]) and torch.equal(st.x[1], keep.x[1]) and torch.equal(st.x[2], keep.x0[2])
    assert int(st.pairs.abs().sum()) == 0 and int(st.ls.abs().sum()) == 0 and int(st.phase.sum()) == 0
    assert torch.equal(st.t, keep.t) and torch.equal(st.best_loss, keep.best_loss) and torch.equal(st.S, keep.S)
    for k, v in o.from_tensors(st).items():
        assert np.array_equal(v, ref[k]), k


def test_result_names_its_optimizer():
    x = torch.zeros(2, 3)
    z = torch.zeros(2)
    kw = dict(x=x, loss=z, step=z, final_x=x, nonfinite=z, active=z.bool(), history=None, steps=0)
    assert fitting.FitResult(state=fitting.FitState.new(x), **kw).optimizer == "adam"
    assert fitting.FitResult(state=fitting.LbfgsState.new(x), **kw).optimizer == "lbfgs"


def test_fit_refuses_groups_and_bad_modes_before_touching_a_device(smpl_model):
    f = fitting.KeypointFitter(smpl_model)
    K = f.spec.K
    target, conf = torch.zeros(4, K, 2), torch.ones(4, K)
    for mode in ("adam", "lbfgs2", None):
        with pytest.raises(ValueError, match="mode"):
            f.fit(target, conf, mode=mode)
    with pytest.raises(ValueError, match="memory"):
        f.fit(target, conf, mode=fitting.Lbfgs(memory=0))
    # (the data check comes first on CPU tensors; the loop's own checks are `_fit`'s)
    kw = dict(steps=4, lr=1.0, mode="lbfgs", stages=None, patience=0, grad_scale=1.0, graph=False, check_every=0, history=False,
              beta1=0.9, beta2=0.999, eps=1e-7, graph_steps=4, prior=None, prior_weights=None, tie=("shape",))
    for grp in (dict(group_size=2, smooth=None), dict(group_size=1, smooth=fitting.smooth_weights(pose=1.0)),
                dict(group_size=4, smooth=fitting.smooth_weights(pose=1.0))):
        with pytest.raises(ValueError, match="lbfgs"):
            f._fit(4, torch.device("cpu"), lambda: None, lambda: None, [], **kw, **grp)
    with pytest.raises(ValueError, match="Adam only"):
        fitting._fit_args(dict(mode="lbfgs"))


def test_lbfgs_step_checks_its_operands_on_the_host():
    st = fitting.LbfgsState.new(torch.zeros(2, 5))
    g, loss = torch.zeros(2, 5), torch.zeros(2, 7)
    with pytest.raises(TypeError, match="LbfgsState"):
        fitting.lbfgs_step(fitting.FitState.new(torch.zeros(2, 5)), g, loss)
    with pytest.raises(RuntimeError):
        fitting.lbfgs_step(st, g, loss)                    # CPU tensors: HIP tensors only
