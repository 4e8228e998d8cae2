"""The probabilistic head without a GPU: the float64 oracle (tests/_prob_oracle.py) against float64 autograd of the torch
restatements in `prob.py`; the C ABI's entries, refusals and no-ops; the torch ops' schemas and Meta kernels; the regressor's
option."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _prob_oracle as o  # noqa: E402
from ilps_amd import prob  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("smplr_prob_sample_fwd", "smplr_prob_sample_bwd", "smplr_prob_nll_fwd", "smplr_prob_nll_bwd", "smplr_prob_fuse",
         "smplr_prob_spread")
OPS = ("prob_sample_fwd", "prob_sample_bwd", "prob_nll_fwd", "prob_nll_bwd", "prob_fuse", "prob_spread")


def close(got, want, mag, tol=1e-12):
    """|got - want| <= tol * the magnitude sum (NaN where both are NaN)."""
    got, want = np.asarray(got), np.asarray(want)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    k = ~np.isnan(want)
    assert (np.abs(got - want)[k] <= tol * mag[k] + 1e-300).all(), np.abs(got - want)[k].max()


@pytest.mark.parametrize("mean_first", [False, True])
@pytest.mark.parametrize("B,S,D", [(1, 1, 5), (3, 4, 7), (2, 9, 86)])
def test_samples_oracle_is_autograd_of_the_restatement(B, S, D, mean_first):
    rng = np.random.default_rng(B * 100 + S)
    mu, s, eps, g = rng.normal(size=(B, D)), rng.uniform(-6, 6, (B, D)), rng.normal(size=(B, S, D)), rng.normal(size=(B, S, D))
    mask = (rng.random(D) < 0.7).astype(np.uint8)
    mask[:2] = 0
    eps[:, :, :2] = np.nan                                   # never read
    if mean_first:
        eps[:, 0] = np.nan
    mt, st = torch.tensor(mu, requires_grad=True), torch.tensor(s, requires_grad=True)
    x = prob.gaussian_samples_torch(mt, st, torch.tensor(eps), mask, mean_first)
    want, status, mag = o.samples(mu, s, eps, mask, mean_first)
    assert (status == 0).all() and x.dtype == torch.float64 and x.shape == (B, S, D)
    close(x.detach().numpy(), want, mag)
    drawn = o.drawn_mask(S, D, mask, mean_first)
    assert np.array_equal(x.detach().numpy()[:, ~drawn], np.broadcast_to(mu[:, None], (B, S, D))[:, ~drawn])
    x.backward(torch.tensor(g))
    dmu, ds, mag_mu, mag_s = o.samples_backward(s, eps, g, mask, mean_first)
    close(mt.grad.numpy(), dmu, mag_mu)
    close(st.grad.numpy(), ds, mag_s)
    assert (ds[:, mask == 0] == 0).all() and (st.grad.numpy()[:, mask == 0] == 0).all()


def nll_case(seed, B, D, G):
    rng = np.random.default_rng(seed)
    groups = rng.integers(-1, G, D)
    if G >= 3:
        groups[groups == 1] = 0                              # an empty group
    groups[0] = -1
    row_w = rng.uniform(0.5, 2.0, (B, G))
    row_w[rng.random((B, G)) < 0.3] = 0.0
    return rng.normal(size=(B, D)), rng.uniform(-6, 6, (B, D)), rng.normal(size=(B, D)), groups, row_w


@pytest.mark.parametrize("with_w", [False, True])
@pytest.mark.parametrize("B,D,G", [(1, 5, 1), (4, 86, 3), (3, 158, 8)])
def test_nll_oracle_is_autograd_of_the_restatement(B, D, G, with_w):
    mu, s, t, groups, row_w = nll_case(B + D, B, D, G)
    if not with_w:
        row_w = None
    else:
        row_w[0, 0] = 0.0
        t[0, groups == 0] = np.nan                           # under a zero weight: not read
    mt, st = torch.tensor(mu, requires_grad=True), torch.tensor(s, requires_grad=True)
    wt = None if row_w is None else torch.tensor(row_w)
    if wt is None and G > groups.max() + 1:                  # (the restatement takes G from row_w or the largest id)
        wt = torch.ones((B, G), dtype=torch.float64)
    got = prob.gaussian_nll_torch(mt, st, torch.tensor(t), groups, wt)
    want, status, mag = o.nll(mu, s, t, groups, G, row_w)
    assert (status == 0).all() and got.shape == (B, G)
    close(got.detach().numpy(), want, mag)
    g = np.random.default_rng(1).normal(size=(B, G))
    got.backward(torch.tensor(g))
    dmu, ds, mag_mu, mag_s = o.nll_backward(mu, s, t, groups, G, g, row_w)
    close(mt.grad.numpy(), dmu, mag_mu)
    close(st.grad.numpy(), ds, mag_s)
    assert (dmu[:, groups < 0] == 0).all() and (ds[:, groups < 0] == 0).all()


@pytest.mark.parametrize("B,G", [(3, 1), (4, 2), (32, 16)])
def test_fusion_oracle_is_the_restatement_and_the_product_of_gaussians(B, G):
    rng = np.random.default_rng(B)
    mu, s = rng.normal(size=(B, 11)), rng.uniform(-200, 200, (B, 11))
    mu_f, s_f, status, mag_mu, mag_s = o.fuse(mu, s, G)
    a, b = prob.fuse_gaussians_torch(torch.tensor(mu), torch.tensor(s), G)
    assert (status == 0).all()
    close(a.numpy(), mu_f, mag_mu)
    close(b.numpy(), s_f, mag_s)
    if G == 1:
        assert np.array_equal(mu_f, mu) and np.array_equal(s_f, s)
    # the product of Gaussians: precisions add, the mean is precision-weighted (log-variances small enough for exp)
    s = rng.uniform(-3, 3, (B, 11))
    mu_f, s_f = o.fuse(mu, s, G)[:2]
    prec = np.exp(-s).reshape(B // G, G, 11)
    assert np.allclose(np.exp(-s_f), prec.sum(1), rtol=1e-12)
    assert np.allclose(mu_f, (mu.reshape(B // G, G, 11) * prec).sum(1) / prec.sum(1), rtol=1e-10, atol=1e-12)


@pytest.mark.parametrize("B,S,N", [(1, 1, 1), (2, 2, 7), (3, 5, 65)])
def test_spread_oracle_is_the_restatement(B, S, N):
    rng = np.random.default_rng(N)
    p = (1e3 + 1e-3 * rng.normal(size=(B * S, N, 3))).astype(np.float32)
    mean, rms, status, mag = o.spread(p, S)
    a, b = prob.sample_spread_torch(torch.tensor(p, dtype=torch.float64), S)
    assert (status == 0).all()
    close(a.numpy(), mean, mag)
    if S == 1:
        assert (rms == 0).all() and np.array_equal(mean, p.astype(np.float64).reshape(B, N, 3))
    else:
        # float64 on unshifted data at 1e3: 1e-13 absolute on each coordinate against an rms of 1e-3
        assert np.abs(b.numpy() - rms).max() <= 1e-9 * rms.max()


def test_header_ctypes_and_schemas_agree():
    from ilps_amd import _lib, torch_ops
    lib = _lib.load()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "smplraster.h")).read(), flags=re.S)
    for name in NAMES:
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        m = re.search(r"\bint %s\s*\(([^)]*)\)" % name, header)
        assert m and m.group(1).count(",") + 1 == len(_lib.SIGNATURES[name][1]), name
    assert "#define SMPLR_ABI_VERSION 7" in header
    assert "#define SMPLR_PROB_NONFINITE %d" % prob.NONFINITE in header and prob.NONFINITE == o.NONFINITE == 1
    assert "#define SMPLR_PROB_MAX_D %d" % prob.MAX_D in header
    ns = torch_ops.load()
    for op in OPS:
        assert str(getattr(ns, op).default._schema) == torch_ops.SCHEMAS[op]


def test_refusals_name_their_entry_point_and_launch_nothing():
    from ilps_amd import _lib
    lib = _lib.load()
    one, err = 1, lib.smplr_last_error                      # (pointer values that are never dereferenced)
    ids = (ctypes.c_int8 * 256)(*([0] * 256))

    def sample_fwd(mu=one, B=2, S=3, D=86, stride=86):
        return lib.smplr_prob_sample_fwd(mu, stride, one, stride, one, None, 0, B, S, D, one, one, None)

    def sample_bwd(s=one, B=2, S=3, D=86, stride=86):
        return lib.smplr_prob_sample_bwd(s, stride, one, None, 0, one, one, B, S, D, one, one, None)

    def nll_fwd(mu=one, B=2, D=86, G=2, groups=ids, stride=86):
        return lib.smplr_prob_nll_fwd(mu, stride, one, stride, one, stride, groups, None, B, D, G, one, one, None)

    def nll_bwd(mu=one, B=2, D=86, G=2, groups=ids, stride=86):
        return lib.smplr_prob_nll_bwd(mu, stride, one, stride, one, stride, groups, None, one, one, B, D, G, one, one, None)

    def fuse(mu=one, B=4, D=86, G=2, stride=86):
        return lib.smplr_prob_fuse(mu, stride, one, stride, B, D, G, one, one, one, None)

    def spread(points=one, B=2, S=3, N=7):
        return lib.smplr_prob_spread(points, B, S, N, one, one, one, None)

    for fn, name in ((sample_fwd, b"smplr_prob_sample_fwd"), (sample_bwd, b"smplr_prob_sample_bwd"), (nll_fwd, b"smplr_prob_nll_fwd"),
                     (nll_bwd, b"smplr_prob_nll_bwd"), (fuse, b"smplr_prob_fuse")):
        assert fn(D=257, stride=257) == -1 and b"D=257" in err() and name in err()
        assert fn(D=0) == -1 and name in err()
        assert fn(stride=85) == -1 and b"stride" in err() and name in err()
        assert fn(None) == -1 and b"null" in err() and name in err()
        assert fn(B=-1) == -1 and b"B=-1" in err() and name in err()
        assert fn(None, B=0) == 0                            # an empty batch is a no-op
    for fn, name in ((sample_fwd, b"smplr_prob_sample_fwd"), (sample_bwd, b"smplr_prob_sample_bwd"), (spread, b"smplr_prob_spread")):
        assert fn(S=0) == -1 and b"S=0" in err() and name in err()
    assert spread(None) == -1 and b"null" in err() and b"smplr_prob_spread" in err()
    assert spread(N=0) == -1 and b"N=0" in err() and spread(None, B=0) == 0
    assert fuse(G=17, B=34) == -1 and b"G=17" in err() and b"smplr_prob_fuse" in err()
    assert fuse(G=3, B=4) == -1 and b"B=4" in err() and b"multiple" in err() and b"smplr_prob_fuse" in err()
    assert fuse(G=0) == -1
    for fn, name in ((nll_fwd, b"smplr_prob_nll_fwd"), (nll_bwd, b"smplr_prob_nll_bwd")):
        bad = (ctypes.c_int8 * 86)(*([0] * 85 + [8]))
        assert fn(groups=bad, G=8) == -1 and b"group id 8" in err() and name in err()
        assert fn(groups=(ctypes.c_int8 * 86)(*([-2] + [0] * 85))) == -1 and b"group id -2" in err()
        assert fn(groups=(ctypes.c_int8 * 86)(*([2] + [0] * 85)), G=2) == -1 and b"group id 2" in err()
        assert fn(G=9) == -1 and b"G=9" in err() and name in err()
        assert fn(groups=None) == -1 and b"null" in err()


def test_meta_shapes_and_cpu_tensors():
    from ilps_amd import torch_ops
    ns = torch_ops.load()
    m = lambda *sh, dt=torch.float32: torch.empty(*sh, dtype=dt, device="meta")
    for B, S, D in ((2, 3, 86), (0, 4, 158), (5, 1, 256)):
        x, status = ns.prob_sample_fwd(m(B, D), m(B, D), m(B, S, D), [1] * D, True)
        assert x.shape == (B, S, D) and x.dtype == torch.float32 and status.shape == (B,) and status.dtype == torch.int32
        dmu, ds = ns.prob_sample_bwd(m(B, D), m(B, S, D), None, False, status, m(B, S, D))
        assert dmu.shape == ds.shape == (B, D)
        groups = [-1] * 4 + [0] * (D - 14) + [1] * 10
        nll, status = ns.prob_nll_fwd(m(B, D), m(B, D), m(B, D), groups, 2, m(B, 2))
        assert nll.shape == (B, 2) and status.shape == (B,)
        dmu, ds = ns.prob_nll_bwd(m(B, D), m(B, D), m(B, D), groups, 2, None, status, m(B, 2))
        assert dmu.shape == ds.shape == (B, D)
    mu_f, s_f, status = ns.prob_fuse(m(6, 200)[:, 5:91], m(6, 86), 3)           # a column slice: strided rows
    assert mu_f.shape == s_f.shape == (2, 86) and status.shape == (2,) and status.dtype == torch.int32
    mean, rms, status = ns.prob_spread(m(12, 6890, 3), 4)
    assert mean.shape == (3, 6890, 3) and rms.shape == (3, 6890) and status.shape == (3,)
    # the Python entries give the same shapes for meta tensors
    assert prob.gaussian_samples(m(2, 86), m(2, 86), m(2, 3, 86)).shape == (2, 3, 86)
    assert prob.gaussian_nll(m(2, 86), m(2, 86), m(2, 86), [0] * 86).shape == (2, 1)
    assert prob.sample_spread(m(6, 24, 3), 3)[1].shape == (2, 24)
    for bad in (lambda: ns.prob_sample_fwd(m(2, 257), m(2, 257), m(2, 3, 257), None, False),
                lambda: ns.prob_sample_fwd(m(2, 86), m(2, 86), m(2, 0, 86), None, False),
                lambda: ns.prob_sample_fwd(m(2, 86), m(2, 86), m(2, 3, 86), [1] * 85, False),
                lambda: ns.prob_nll_fwd(m(2, 86), m(2, 86), m(2, 86), [8] * 86, 8, None),
                lambda: ns.prob_nll_fwd(m(2, 86), m(2, 86), m(2, 86), [0] * 86, 9, None),
                lambda: ns.prob_fuse(m(4, 86), m(4, 86), 3), lambda: ns.prob_fuse(m(34, 86), m(34, 86), 17),
                lambda: ns.prob_spread(m(6, 7, 3), 4), lambda: ns.prob_spread(m(6, 7, 3), 0),
                lambda: ns.prob_spread(m(6, 7, 3, dt=torch.float64), 3)):
        with pytest.raises(RuntimeError):
            bad()
    z = torch.zeros
    with pytest.raises((RuntimeError, NotImplementedError)):
        ns.prob_spread(z(4, 7, 3), 2)                        # a CPU tensor: no kernel registered for it
    with pytest.raises((RuntimeError, NotImplementedError)):
        ns.prob_fuse(z(4, 86), z(4, 86), 2)
    for call in (lambda: prob.gaussian_samples(z(2, 86), z(2, 86), z(2, 3, 86)), lambda: prob.gaussian_nll(z(2, 86), z(2, 86), z(2, 86), [0] * 86),
                 lambda: prob.fuse_gaussians(z(4, 86), z(4, 86), 2), lambda: prob.sample_spread(z(4, 7, 3), 2),
                 lambda: prob.fuse_shape(z(4, 86), z(4, 86), 2)):
        with pytest.raises(RuntimeError, match="HIP device"):
            call()
    with pytest.raises(ValueError):
        prob.gaussian_nll(z(2, 86), z(2, 86), z(2, 86), [8] * 86)
    with pytest.raises(ValueError):
        prob.fuse_gaussians(z(4, 86), z(4, 86), 3)
    with pytest.raises(ValueError):
        prob.sample_spread(z(4, 7, 3), 0)
    with pytest.raises(ValueError):
        prob.gaussian_samples(z(2, 257), z(2, 257), z(2, 3, 257))


def test_lazy_exports():
    import ilps_amd
    for name in ("gaussian_samples", "gaussian_nll", "fuse_gaussians", "fuse_shape", "sample_spread"):
        assert getattr(ilps_amd, name) is not None


def test_regressor_option_keeps_the_default_and_samples_on_meta():
    import inspect
    import math
    from ilps_amd.model import SMPLRegressor, build_model
    from ilps_amd.training import ProbabilisticTrainer, SupervisedTrainer
    for arch in ("enet", "resnet50"):
        for ief in (False, True):
            a = {k: tuple(v.shape) for k, v in SMPLRegressor(48, arch, ief).state_dict().items()}
            b = {k: tuple(v.shape) for k, v in SMPLRegressor(48, arch, ief, probabilistic=False).state_dict().items()}
            assert a == b and not any(k.startswith("spread") for k in a)
    assert inspect.signature(SMPLRegressor.__init__).parameters["probabilistic"].default is False
    assert inspect.signature(build_model).parameters["probabilistic"].default is False
    assert issubclass(ProbabilisticTrainer, SupervisedTrainer)
    for repr_, nout in (("axis_angle", 86), ("rot6d", 158)):
        plain = SMPLRegressor(48, "enet", True, pose_repr=repr_).state_dict()
        net = SMPLRegressor(48, "enet", True, pose_repr=repr_, probabilistic=True, init_sigma=0.2)
        sd = net.state_dict()
        assert set(sd) - set(plain) == {"spread.weight", "spread.bias"} and set(plain) <= set(sd)
        assert sd["spread.weight"].shape == (nout, 2048) and (sd["spread.weight"] == 0).all()
        assert torch.allclose(sd["spread.bias"], torch.full((nout,), 2 * math.log(0.2)))
        assert net.stochastic == (0,) * 4 + (1,) * (nout - 4) and net.mean is None and net.log_var is None
        with pytest.raises(RuntimeError, match="forward"):
            net.sample(torch.zeros(2, 3, nout))
        net.mean = torch.empty(2, nout, device="meta")
        net.log_var = torch.empty(2, nout, device="meta")
        out = net.sample(torch.empty(2, 3, nout, device="meta"))
        assert out.shape == (6, 86) and out.dtype == torch.float32
    with pytest.raises(ValueError, match="init_sigma"):
        SMPLRegressor(48, "enet", probabilistic=True, init_sigma=0.0)


def test_regressor_keeps_its_distribution_on_the_cpu():
    """The forward leaves mean and log_var, fp32 and in the graph; the returned vector is made from the mean."""
    from ilps_amd.model import SMPLRegressor

    class Stub(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.fc = torch.nn.Linear(3 * 8 * 8, 2048)

        def forward(self, x):
            return self.fc(x.flatten(1))
    for ief in (False, True):
        torch.manual_seed(0)
        net = SMPLRegressor(48, "enet", ief, probabilistic=True)
        net.backbone = Stub()
        out = net(torch.randn(2, 3, 8, 8))
        assert out.shape == (2, 86) and torch.equal(net.mean, out) and net.log_var.shape == (2, 86)
        assert net.log_var.dtype == torch.float32 and torch.allclose(net.log_var, torch.full((2, 86), 2 * np.log(0.1)), atol=1e-6)
        net.log_var.sum().backward()
        assert net.spread.bias.grad is not None and (net.spread.bias.grad == 2).all()
