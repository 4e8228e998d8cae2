"""Groups of rows in the fit step without a GPU: the float64 oracle (tests/_fit_group_oracle.py) against the plain step's
oracle and against autograd on a problem with a genuinely shared parameter; `tie_mask`, `smooth_weights` and `fit`'s argument
errors; smplr_fit_step_group's refusals (nothing is launched); the torch op's Meta kernel."""
import ctypes

import numpy as np
import pytest
import torch

import _fit_group_oracle as go
import _fitting_oracle as fo
from ilps_amd import fitting


def test_group_of_one_without_smoothing_is_the_plain_oracle():
    rng = np.random.default_rng(0)
    B, P, N, Ns, calls = 5, 86, 37, 19, 7
    for mode, with_silh in (("keras", False), ("torch", True)):
        a = fo.new_state(rng.normal(0.0, 1.0, (B, P)).astype(np.float32))
        b = {k: v.copy() for k, v in a.items()}
        ha, hb = np.full((calls, B), np.nan), np.full((calls, B), np.nan)
        cs = rng.uniform(0.0, 3.0, P).astype(np.float32)
        cs[[3, 50]] = 0.0
        tie = np.zeros(P, np.uint8)
        tie[76:] = 1
        base, base_s = rng.exponential(0.05, (B, N)), rng.exponential(0.3, (B, Ns))
        odd = np.arange(B)[:, None] % 2
        for k in range(calls):
            g = (rng.normal(0.0, 1.0, (B, P)) * 10.0 ** rng.uniform(-6, 1, (B, P))).astype(np.float32)
            g[rng.random((B, P)) < 0.1] = 0.0
            if k == 2:
                g[1, 5] = np.nan
            loss = (base * np.where(odd, 1.0 + 0.3 * k, 1.0 - 0.1 * k)).astype(np.float32)      # even rows fall, odd rows rise
            silh = (base_s * np.where(odd, 1.0 + 0.3 * k, 1.0 - 0.1 * k)).astype(np.float32) if with_silh else None
            if k == 4:
                loss[3, 0] = np.inf
            kw = dict(lr=2e-3, beta1=0.9, beta2=0.999, eps=1e-7, gscale=0.3, mode=mode, patience=2)
            a, La, terms = fo.fit_step(a, g, loss, silh, 0.7, cs, ha, **kw)
            b, info = go.fit_step_group(b, g, loss, silh, 0.7, cs, hb, G=1, tie=tie, smooth=None, **kw)
            for key in fo.FLOAT_KEYS + fo.INT_KEYS:
                assert np.array_equal(a[key], b[key], equal_nan=True), (key, k)
            assert np.array_equal(La, info["L_rows"], equal_nan=True) and np.array_equal(La, info["L"], equal_nan=True)
            for key in ("m_mag", "v_mag", "dx_mag"):
                assert np.array_equal(terms[key], info[key], equal_nan=True), (key, k)
        assert np.array_equal(ha, hb, equal_nan=True)
        assert a["bad"].sum() == 2 and (a["active"] == 0).any() and (a["active"] == 1).any()


def test_tied_sum_and_smoothness_gradient_are_autograd_of_a_shared_parameter():
    """G rows that genuinely share their last 4 columns (one torch parameter w, expanded) and have their own first 5 (u);
    f = sum_r f_r([u_r | w]) + sum_j smooth_j sum_r (x_r - x_r-1)^2 in float64.  Autograd's df/dw is the oracle's tied sum,
    df/du_r is g_r + s_r, and the penalty's value is E_s."""
    rng = np.random.default_rng(1)
    G, K, Pu, Pw = 4, 2, 5, 4
    P, B = Pu + Pw, 2 * 4
    tie = np.array([0] * Pu + [1] * Pw, np.uint8)
    smooth = np.array([0.5, 0.0, 2.0, 0.25, 1.0] + [3.0] * Pw, np.float32)          # (the weights on tied columns are ignored)
    a = torch.tensor(rng.normal(0.0, 1.0, (B, P)))
    u = torch.tensor(rng.normal(0.0, 1.0, (B, Pu)).astype(np.float32).astype(np.float64), requires_grad=True)
    w = torch.tensor(rng.normal(0.0, 1.0, (K, Pw)).astype(np.float32).astype(np.float64), requires_grad=True)
    rows = torch.cat([u, w.repeat_interleave(G, 0)], 1)                            # (B, P): what the decoder consumes
    # the per-row gradients a decoder would return: rows as independent copies
    xr = rows.detach().clone().requires_grad_(True)
    data = lambda x: (torch.sin(a * x) + 0.1 * x ** 3).sum()
    (g_rows,) = torch.autograd.grad(data(xr), xr)
    g32 = g_rows.numpy().astype(np.float32)                                        # the kernel's input: fp32
    sw = torch.tensor(smooth.astype(np.float64) * (1 - tie))

    def penalty(x):
        xg = x.reshape(K, G, P)
        return (sw * ((xg[:, 1:] - xg[:, :-1]) ** 2).sum(1)).sum(1)
    pen = penalty(rows)
    f = (torch.sin(a * rows) + 0.1 * rows ** 3).sum() + pen.sum()
    du, dw = torch.autograd.grad(f, [u, w])
    state = fo.new_state(rows.detach().numpy())
    _, info = go.fit_step_group(state, g32, np.ones((B, 3), np.float32), G=G, tie=tie, smooth=smooth)
    assert np.allclose(info["E_s"], pen.detach().numpy(), rtol=1e-13, atol=0)
    # fp32 rounding of the incoming gradient is the only difference
    tol = 2.0 ** -23
    got_u = info["g_upd"][:, :Pu]
    assert np.all(np.abs(got_u - du.numpy()) <= tol * info["A"][:, :Pu] + 1e-300)
    got_w = info["g_upd"][:, Pu:].reshape(K, G, Pw)
    for r in range(G):
        assert np.array_equal(got_w[:, r], got_w[:, 0])                            # the group's sum, repeated on its rows
    assert np.all(np.abs(got_w[:, 0] - dw.numpy()) <= tol * info["A"][:, Pu:].reshape(K, G, Pw)[:, 0])
    # s_r alone: the penalty's gradient, with exact zeros on tied and unweighted columns
    (ds,) = torch.autograd.grad(penalty(torch.cat([u, w.repeat_interleave(G, 0)], 1)).sum(), [u])
    assert np.allclose(info["s"][:, :Pu], ds.numpy(), rtol=1e-13, atol=1e-15)
    assert not info["s"][:, Pu:].any() and not info["s"][:, 1].any() and info["s"][:, 0].any()
    # tied columns stay equal across a group after the update; untied ones do not
    new, _ = go.fit_step_group(state, g32, np.ones((B, 3), np.float32), G=G, tie=tie, smooth=smooth)
    xn = new["x"].reshape(K, G, P)
    assert np.array_equal(xn[:, :, Pu:], np.repeat(xn[:, :1, Pu:], G, 1)) and not np.array_equal(xn[:, 0, :Pu], xn[:, 1, :Pu])
    assert not np.array_equal(new["x"], state["x"])


def test_group_rules_of_the_oracle():
    """Two groups of three rows: a NaN in one row's gradient is a bad call of its whole group and of nothing else; the group's
    loss decides for all its rows; patience stops a group as one."""
    rng = np.random.default_rng(2)
    G, B, P = 3, 6, 8
    s = fo.new_state(rng.normal(0.0, 1.0, (B, P)).astype(np.float32))
    tie = np.array([0] * 4 + [1] * 4, np.uint8)
    hist = np.full((4, B), np.nan)
    # group 0: the sum falls, although row 1's own loss rises; group 1: the sum never improves after call 0
    script = [np.array([3.0, 1.0, 2.0, 1.0, 1.0, 1.0]), np.array([1.0, 2.0, 1.0, 1.0, 2.0, 1.0]),
              np.array([0.5, 2.5, 0.5, 1.0, 1.0, 2.0]), np.array([0.5, 0.5, 0.5, 1.0, 1.0, 1.0])]
    for k, L in enumerate(script):
        g = rng.normal(0.0, 1.0, (B, P)).astype(np.float32)
        if k == 1:
            g[4, 2] = np.nan
        before = s
        s, info = go.fit_step_group(s, g, L[:, None].astype(np.float32), G=G, tie=tie, history=hist, patience=2)
        assert np.array_equal(info["L"], [L[:3].sum(), L[3:].sum()])
        if k == 1:
            assert s["bad"].tolist() == [0, 0, 0, 1, 1, 1]
            for key in ("x", "m", "v", "t", "stall", "best_loss"):
                assert np.array_equal(s[key][3:], before[key][3:]) and not np.array_equal(s[key][:3], before[key][:3]) or key == "stall"
        for key in fo.INT_KEYS + ("best_loss",):
            assert len(set(s[key][:3].tolist())) == 1 and len(set(s[key][3:].tolist())) == 1, key
    assert np.array_equal(hist, np.array(script))
    assert s["best_step"].tolist() == [3, 3, 3, 0, 0, 0] and s["best_loss"].tolist() == [1.5] * 3 + [3.0] * 3
    assert s["active"].tolist() == [1, 1, 1, 0, 0, 0] and s["t"].tolist() == [4, 4, 4, 2, 2, 2]
    assert s["calls"].tolist() == [4] * 6


def test_tie_mask_and_smooth_weights():
    t = fitting.tie_mask()
    assert t.dtype == torch.uint8 and tuple(t.shape) == (86,) and t[76:].all() and not t[:76].any()
    t = fitting.tie_mask(shape=False, pose=True, num_cam=3)
    assert tuple(t.shape) == (85,) and t[6:75].all() and not t[:6].any() and not t[75:].any()
    t = fitting.tie_mask(shape=True, pose=True, global_rot=True, cam=True)
    assert t.all() and t.is_contiguous()
    assert fitting.tie_mask(shape=False, global_rot=True).nonzero().flatten().tolist() == [4, 5, 6]
    assert fitting.tie_mask(shape=False, cam=True, num_cam=0).sum() == 0 and fitting.tie_mask(num_cam=174).shape[0] == 256
    for bad in (dict(num_cam=-1), dict(num_cam=175), dict(shape=1.5), dict(pose="yes")):
        with pytest.raises(ValueError):
            fitting.tie_mask(**bad)
    s = fitting.smooth_weights(cam=0.5, global_rot=1.0, pose=2.0, shape=4.0)
    assert s.dtype == torch.float32 and tuple(s.shape) == (86,)
    assert s[:4].tolist() == [0.5] * 4 and s[4:7].tolist() == [1.0] * 3 and s[7:76].tolist() == [2.0] * 69 and s[76:].tolist() == [4.0] * 10
    assert not fitting.smooth_weights().any() and fitting.smooth_weights(pose=1.0, num_cam=174).shape[0] == 256
    for bad in (dict(pose=-1.0), dict(cam=float("nan")), dict(shape=float("inf")), dict(global_rot=1e39), dict(num_cam=200)):
        with pytest.raises(ValueError):
            fitting.smooth_weights(**bad)
    # names or a mask
    assert torch.equal(fitting.check_tie(("shape", "pose"), 86), fitting.tie_mask(pose=True))
    assert torch.equal(fitting.check_tie("shape", 86), fitting.tie_mask())
    assert torch.equal(fitting.check_tie(fitting.tie_mask(cam=True).bool(), 86), fitting.tie_mask(cam=True))
    assert not fitting.check_tie((), 86).any()
    for bad in (("torso",), np.zeros(85, np.uint8), np.full(86, 2), np.zeros(86, np.float32)):
        with pytest.raises(ValueError):
            fitting.check_tie(bad, 86)
    with pytest.raises(ValueError):
        fitting.check_tie(("shape",), 90, num_cam=4)


def test_fit_refuses_bad_groups_before_touching_a_device():
    f = object.__new__(fitting.ParamFitter)                              # (no decoder: every call below fails its checks first)
    f.img_wh, f.num_cam, f.P, f.with_silhouette, f.silh_wh, f.silh_weight = 48, 4, 86, False, 64, 1.0
    labels = torch.zeros((6, 48, 48), dtype=torch.int32)
    for kw in (dict(group_size=4), dict(group_size=0), dict(group_size=17), dict(group_size=-2),
               dict(group_size=3, tie=("torso",)), dict(group_size=3, tie=np.zeros(80, np.uint8)),
               dict(group_size=3, smooth=np.full(86, -1.0)), dict(group_size=2, smooth=np.zeros(85)),
               dict(group_size=1, smooth=np.full(86, np.nan))):
        with pytest.raises(ValueError):
            f.fit(labels, steps=1, **kw)
    with pytest.raises(RuntimeError):
        f.fit(labels, steps=1, group_size=3)                              # valid groups; CPU labels: there is no CPU path
    with pytest.raises(ValueError):
        fitting.check_group(10, 3)
    assert fitting.check_group(0, 5) == 5 and fitting.check_group(32, 16) == 16


def test_fit_step_group_argument_errors_launch_nothing():
    from ilps_amd import _lib
    lib = _lib.load()
    one = ctypes.c_void_p(16)          # a non-null pointer that is never dereferenced: every call below fails its checks first

    def call(P=86, N=2304, mode=0, B=6, G=3, tie=one, smooth=None, ptr=one, prior=None, num_cam=4, K=0, A=0, beta1=0.9):
        pr = [prior] * 7
        return lib.smplr_fit_step_group(ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, N, None, 0, 1.0, ptr, None,
                                        0, B, P, 1e-3, beta1, 0.999, 1e-7, 1.0, mode, 0, num_cam, pr[0], pr[1], pr[2], pr[3],
                                        pr[4], pr[5], K, A, pr[6], G, tie, smooth, None)
    for kw, word in ((dict(G=0), b"G=0"), (dict(G=17), b"G=17"), (dict(G=-1), b"G=-1"), (dict(B=7), b"no multiple"),
                     (dict(B=16, G=3), b"no multiple"), (dict(tie=None), b"tie"), (dict(P=257), b"P=257"), (dict(N=0), b"N=0"),
                     (dict(mode=2), b"mode 2"), (dict(B=-3), b"negative batch"), (dict(beta1=1.0), b"beta1"),
                     (dict(ptr=None), b"null pointer"), (dict(prior=one, K=0), b"K=0"), (dict(prior=one, K=1, P=90), b"num_cam + 82")):
        assert call(**kw) == -1, kw
        err = lib.smplr_last_error()
        assert word in err and b"smplr_fit_step_group" in err, (kw, err)
    assert call(B=0, ptr=None, tie=None) == 0                                   # an empty batch is a no-op
    assert call(B=0, G=16) == 0


def test_fit_step_group_op_meta_kernel():
    from ilps_amd import torch_ops
    ns = torch_ops.load()
    assert str(ns.fit_step_group.default._schema) == torch_ops.SCHEMAS["fit_step_group"]
    assert ns.fit_step_group.default._schema.is_mutable

    def args(dev="meta", B=6, P=86, N=2304, tie_dt=torch.uint8, tie_n=None, smooth_n=86, prior=False):
        f = lambda *s: torch.zeros(*s, dtype=torch.float32, device=dev)
        i = lambda: torch.zeros(B, dtype=torch.int32, device=dev)
        a = [f(B, P), f(B, P), f(B, P), f(B, P), i(), i(), i(), i(), i(), torch.ones(B, dtype=torch.uint8, device=dev), f(B),
             f(B, P), f(B, N), None, f(P), f(5, B), torch.zeros(P if tie_n is None else tie_n, dtype=tie_dt, device=dev),
             None if smooth_n is None else f(smooth_n)]
        pr = [f(2, 69), f(2, 69, 69), f(2), torch.zeros(4, dtype=torch.int32, device=dev), f(4), f(10), f(3)] if prior else [None] * 7
        return a + pr
    assert ns.fit_step_group(*args(), 3) is None
    assert ns.fit_step_group(*args(smooth_n=None, prior=True), 2, 1e-3, 0.9, 0.999, 1e-8, 0.5, 2.0, 1, 3, 4) is None
    for bad, G in ((dict(), 4), (dict(), 0), (dict(), 17), (dict(tie_dt=torch.int32), 3), (dict(tie_n=85), 3),
                   (dict(smooth_n=80), 3), (dict(P=257), 3), (dict(N=0), 3), (dict(prior=True, P=90), 3)):
        with pytest.raises(RuntimeError):
            ns.fit_step_group(*args(**bad), G)
    a = args(prior=True)
    a[20] = None                                                               # the prior's tensors go together
    with pytest.raises(RuntimeError):
        ns.fit_step_group(*a, 3)
    with pytest.raises((RuntimeError, NotImplementedError)):
        ns.fit_step_group(*args("cpu"), 3)                                     # a CPU tensor: no kernel registered for it
