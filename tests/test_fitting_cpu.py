"""`ilps_amd.fitting` without a GPU: the float64 oracle of smplr_fit_step against torch.optim.Adam and against Keras'
first step written out by hand; the Python helpers; the launcher's argument errors (nothing is launched); the torch op's
schema and Meta kernel."""
import ctypes

import numpy as np
import pytest
import torch

import _fitting_oracle as fo
from ilps_amd import fitting


def _f32(a):
    return float(np.float32(a))


def test_oracle_torch_mode_is_torch_adam_in_float64():
    """Six steps on random (4, 86) gradients: the oracle's "torch" mode and torch.optim.Adam in float64 agree to 1e-12.
    Both get the scalars the kernel gets (rounded to fp32)."""
    rng = np.random.default_rng(0)
    x0 = rng.normal(0.0, 1.0, (4, 86)).astype(np.float32)
    lr, b1, b2, eps = _f32(1e-3), _f32(0.9), _f32(0.999), _f32(1e-8)
    p = torch.tensor(x0, dtype=torch.float64, requires_grad=True)
    opt = torch.optim.Adam([p], lr=lr, betas=(b1, b2), eps=eps)
    s = fo.new_state(x0)
    loss = np.ones((4, 16), np.float32)
    for k in range(6):
        g = (rng.normal(0.0, 1.0, (4, 86)) * 10.0 ** rng.uniform(-6, 1, (4, 86))).astype(np.float32)
        p.grad = torch.tensor(g, dtype=torch.float64)
        opt.step()
        s, _, _ = fo.fit_step(s, g, loss - 0.01 * k, lr=lr, beta1=b1, beta2=b2, eps=eps, mode="torch")
        assert np.max(np.abs(s["x"] - p.detach().numpy())) <= 1e-12
    assert np.all(s["t"] == 6) and np.all(s["calls"] == 6) and np.all(s["bad"] == 0)


def test_oracle_keras_mode_first_step_by_hand():
    """Keras 2 Adam at t = 1 from m = v = 0: dx = -lr sqrt(1 - b2) / (1 - b1) (1 - b1) g / (sqrt((1 - b2) g^2) + eps)."""
    rng = np.random.default_rng(1)
    x0 = rng.normal(0.0, 1.0, (3, 86)).astype(np.float32)
    g = (rng.normal(0.0, 1.0, (3, 86)) * 10.0 ** rng.uniform(-8, 2, (3, 86))).astype(np.float32)
    lr, b1, b2, eps = _f32(1e-3), _f32(0.9), _f32(0.999), _f32(1e-7)
    s, L, _ = fo.fit_step(fo.new_state(x0), g, np.full((3, 9), 2.0, np.float32), lr=lr, beta1=b1, beta2=b2, eps=eps, mode="keras")
    g64 = g.astype(np.float64)
    dx = -lr * np.sqrt(1.0 - b2) / (1.0 - b1) * (1.0 - b1) * g64 / (np.sqrt((1.0 - b2) * g64 * g64) + eps)
    assert np.max(np.abs(s["x"] - (x0.astype(np.float64) + dx))) <= 1e-15
    assert np.all(L == 2.0) and np.all(s["best_loss"] == 2.0) and np.all(s["best_x"] == x0.astype(np.float64))
    # the two modes differ where the gradient is small against eps: torch's effective eps at t = 1 is sqrt(1 - b2) times Keras'
    st, _, _ = fo.fit_step(fo.new_state(x0), g, np.full((3, 9), 2.0, np.float32), lr=lr, beta1=b1, beta2=b2, eps=eps, mode="torch")
    small = np.abs(g64) < 1e-6
    assert small.any() and np.all(np.abs(st["x"] - x0)[small] > np.abs(s["x"] - x0)[small])


def test_oracle_row_rules():
    """Steps 2-4 of the semantics on three rows: a bad row changes nothing but `bad` and `calls`; a stalled row stops."""
    x0 = np.arange(6, dtype=np.float32).reshape(3, 2)
    s = fo.new_state(x0)
    hist = np.full((4, 3), np.nan)
    g = np.ones((3, 2), np.float32)
    for k, losses in enumerate(([3.0, 3.0, 3.0], [2.0, 4.0, np.inf], [1.0, 5.0, 2.0], [0.5, 1.0, 1.0])):
        s, _, _ = fo.fit_step(s, g, np.array(losses, np.float32)[:, None], history=hist, patience=2)
    assert s["t"].tolist() == [4, 2, 3] and s["calls"].tolist() == [4, 4, 4] and s["bad"].tolist() == [0, 0, 1]
    assert s["active"].tolist() == [1, 0, 1] and s["best_step"].tolist() == [3, 0, 2] and s["best_loss"].tolist() == [0.5, 3.0, 1.0]
    assert np.array_equal(s["best_x"][1], x0[1]) and np.isinf(hist[1, 2]) and hist[3, 1] == 1.0


def test_column_scale_and_stage_lists():
    s = fitting.column_scale(cam=20.0, pose=0.5, shape=0.0)
    assert s.dtype == torch.float32 and tuple(s.shape) == (86,)
    assert s[:4].tolist() == [20.0] * 4 and s[4:76].tolist() == [0.5] * 72 and s[76:].tolist() == [0.0] * 10
    assert tuple(fitting.column_scale(num_cam=3).shape) == (85,) and bool((fitting.column_scale() == 1).all())
    with pytest.raises(ValueError):
        fitting.column_scale(cam=-1.0)
    with pytest.raises(ValueError):
        fitting.column_scale(pose=float("nan"))
    st = fitting.check_stages([(3, s), [5, np.ones(86)]], 86)
    assert [n for n, _ in st] == [3, 5] and torch.equal(st[0][1], s) and st[1][1].dtype == torch.float32
    one = fitting.check_stages(None, 86, steps=7)
    assert len(one) == 1 and one[0][0] == 7 and bool((one[0][1] == 1).all())
    for bad in ([(3, torch.ones(85))], [(-1, s)], [(3,)], [(3, -s - 1)]):
        with pytest.raises(ValueError):
            fitting.check_stages(bad, 86)
    with pytest.raises(ValueError):
        fitting.check_stages(None, 86)


def test_fit_state_initial_values():
    x0 = torch.arange(10 * 86, dtype=torch.float64).reshape(10, 86)
    s = fitting.FitState.new(x0)
    assert s.x.dtype == torch.float32 and torch.equal(s.x, x0.float()) and torch.equal(s.best_x, s.x)
    assert s.x.data_ptr() != s.best_x.data_ptr() != x0.data_ptr()
    assert not s.m.any() and not s.v.any() and s.m.shape == s.v.shape == s.x.shape
    for k in ("t", "calls", "stall", "bad", "best_step"):
        a = getattr(s, k)
        assert a.dtype == torch.int32 and tuple(a.shape) == (10,) and not a.any()
    assert s.active.dtype == torch.uint8 and bool((s.active == 1).all())
    assert s.best_loss.dtype == torch.float32 and bool(torch.isposinf(s.best_loss).all())
    with pytest.raises(ValueError):
        fitting.FitState.new(torch.zeros(2, 257))
    with pytest.raises(ValueError):
        fitting.FitState.new(torch.zeros(86))
    with pytest.raises(RuntimeError):
        fitting.fit_step(s, torch.zeros(10, 86), torch.zeros(10, 4))          # CPU tensors: there is no CPU path


def test_fit_step_argument_errors_launch_nothing():
    from ilps_amd import _lib
    lib = _lib.load()
    one = ctypes.c_void_p(16)          # a non-null pointer that is never dereferenced: every call below fails its checks first

    def call(P=86, N=2304, mode=0, B=1, Ns=0, silh=None, H=0, patience=0, beta1=0.9, eps=1e-7, ptr=one, lr=1e-3):
        return lib.smplr_fit_step(ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, N, silh, Ns, 1.0, ptr, None, H,
                                  B, P, lr, beta1, 0.999, eps, 1.0, mode, patience, None)
    for kw, word in ((dict(P=257), b"P=257"), (dict(P=0), b"P=0"), (dict(N=0), b"N=0"), (dict(N=-3), b"N=-3"),
                     (dict(mode=2), b"mode 2"), (dict(mode=-1), b"mode -1"), (dict(B=-1), b"negative batch"),
                     (dict(silh=one, Ns=0), b"Ns=0"), (dict(H=-1), b"negative history"), (dict(patience=-2), b"patience -2"),
                     (dict(beta1=1.0), b"beta1"), (dict(eps=-1.0), b"eps"), (dict(lr=float("nan")), b"finite"),
                     (dict(ptr=None), b"null pointer")):
        assert call(**kw) == -1, kw
        assert word in lib.smplr_last_error(), (kw, lib.smplr_last_error())
    assert call(B=0, ptr=None) == 0                                            # an empty batch is a no-op


def test_fit_step_op_schema_and_meta_kernel():
    from ilps_amd import torch_ops
    ns = torch_ops.load()
    assert "fit_step" in torch_ops.SCHEMAS
    assert str(ns.fit_step.default._schema) == torch_ops.SCHEMAS["fit_step"]
    assert ns.fit_step.default._schema.is_mutable

    def args(dev, B=3, P=86, N=2304, Ns=None, H=5):
        f = lambda *s: torch.zeros(*s, dtype=torch.float32, device=dev)
        i = lambda: torch.zeros(B, dtype=torch.int32, device=dev)
        return [f(B, P), f(B, P), f(B, P), f(B, P), i(), i(), i(), i(), i(), torch.ones(B, dtype=torch.uint8, device=dev), f(B),
                f(B, P), f(B, N), None if Ns is None else f(B, Ns), f(P), None if H is None else f(H, B)]
    assert ns.fit_step(*args("meta")) is None
    assert ns.fit_step(*args("meta", Ns=4096, H=None), 1e-3, 0.9, 0.999, 1e-8, 0.5, 2.0, 1, 3) is None
    for bad in (dict(P=257), dict(N=0)):
        with pytest.raises(RuntimeError):
            ns.fit_step(*args("meta", **bad))
    a = args("meta")
    a[4] = a[4].long()
    with pytest.raises(RuntimeError):
        ns.fit_step(*a)                                                          # t must be int32
    a = args("meta")
    a[14] = torch.zeros(85, device="meta")
    with pytest.raises(RuntimeError):
        ns.fit_step(*a)                                                          # col_scale must be (P,)
    with pytest.raises(RuntimeError):
        ns.fit_step(*args("meta"), mode=2)
    with pytest.raises((RuntimeError, NotImplementedError)):
        ns.fit_step(*args("cpu"))                                                # a CPU tensor: no kernel registered for it


# ---- the public surface of the fitters: `inspect.signature` of every public callable, as literals ----------------------------
SIGNATURES = {
    "ParamFitter.__init__": ("(self, smpl_path=None, img_wh=48, gamma=5.0, weight_classes=False, with_silhouette=False, "
        "silh_wh=None, silh_weight=1.0, vertex_sampling=None, deterministic=False, penetration=None, "
        "collide=None, keypoints=None, kp_sigma=None)"),
    "ParamFitter.initial": "(self, B, init=None, generator=None, device=None)",
    "ParamFitter.losses": ("(self, x, labels, silh_labels=None, prior=None, prior_weights=None, pen_weight=None, keypoints=None,"
        " kp_weight=None)"),
    "ParamFitter.fit": ("(self, labels, init=None, steps=1601, lr=0.001, mode='keras', stages=None, silh_labels=None, "
        "patience=0, grad_scale=1.0, graph=False, check_every=0, history=False, beta1=0.9, beta2=0.999, "
        "eps=1e-07, graph_steps=4, generator=None, prior=None, prior_weights=None, group_size=1, "
        "tie=('shape',), smooth=None, pen_weight=None, keypoints=None, kp_weight=None)"),
    "ScanFitter.__init__": ("(self, smpl_path=None, topo=None, m2p_weight=1.0, sigma=None, directions=('p2m', 'm2p'), "
        "penetration=None, collide=None)"),
    "ScanFitter.initial": "(self, B, init=None, device=None)",
    "ScanFitter.place": "(self, x, offsets=None)",
    "ScanFitter.terms": "(self, x, points, counts=None, verts=None, offsets=None)",
    "ScanFitter.losses": "(self, x, points, counts=None, prior=None, prior_weights=None, pen_weight=None)",
    "ScanFitter.fit": ("(self, points, counts=None, init=None, steps=200, lr=0.01, mode='torch', stages=None, patience=0, "
        "grad_scale=1.0, graph=False, check_every=0, history=False, beta1=0.9, beta2=0.999, eps=1e-07, "
        "graph_steps=4, prior=None, prior_weights=None, group_size=1, tie=('shape',), smooth=None, "
        "pen_weight=None)"),
    "KeypointFitter.__init__": "(self, smpl_path=None, spec=None, sigma=None, img_wh=48, penetration=None, collide=None)",
    "KeypointFitter.initial": "(self, B, init=None, device=None)",
    "KeypointFitter.terms": "(self, x, target, conf)",
    "KeypointFitter.losses": "(self, x, target, conf, prior=None, prior_weights=None, pen_weight=None)",
    "KeypointFitter.fit": ("(self, target, conf, init=None, steps=200, lr=0.01, mode='torch', stages=None, patience=0, "
        "grad_scale=1.0, graph=False, check_every=0, history=False, beta1=0.9, beta2=0.999, eps=1e-07, "
        "graph_steps=4, prior=None, prior_weights=None, group_size=1, tie=('shape',), smooth=None, "
        "pen_weight=None)"),
    "OffsetFitter.__init__": "(self, scan_fitter, spec, penetration=None)",
    "OffsetFitter.template": "(self, device)",
    "OffsetFitter.row_loss": "(self, x, D, points, counts, wts, pen_w=None)",
    "OffsetFitter.fit": ("(self, points, counts, x, steps=200, lr=0.001, lap_weight=1.0, edge_weight=1.0, offset_weight=0.0, "
        "stages=None, fit_params=False, history=False, graph=False, offsets=None, mode='torch', beta1=0.9, "
        "beta2=0.999, eps=1e-07, x_lr=None, pen_weight=None)"),
    "fit_step": ("(state, grad, loss, silh_loss=None, silh_weight=1.0, col_scale=None, history=None, lr=0.001, "
        "beta1=0.9, beta2=0.999, eps=1e-07, grad_scale=1.0, mode='keras', patience=0, prior=None, "
        "prior_weights=None, num_cam=4, group_size=1, tie=None, smooth=None)"),
    "offset_step": "(D, grad, m, v, t, bad, loss, lr=0.001, beta1=0.9, beta2=0.999, eps=1e-07, mode='torch')",
}
RESULT_FIELDS = {
    "FitResult": ("x", "loss", "step", "final_x", "nonfinite", "active", "history", "steps", "state", "group_size"),
    "OffsetFitResult": ("offsets", "x", "history", "bad", "steps", "t", "state"),
}


def test_public_signatures_are_the_recorded_ones():
    """Names, order and defaults of what callers and tools use: a change to the fitters' host side leaves them alone."""
    import dataclasses
    import inspect
    for name, want in SIGNATURES.items():
        obj = fitting
        for part in name.split("."):
            obj = getattr(obj, part)
        assert str(inspect.signature(obj)) == want, name
    for name, want in RESULT_FIELDS.items():
        assert tuple(f.name for f in dataclasses.fields(getattr(fitting, name))) == want, name
