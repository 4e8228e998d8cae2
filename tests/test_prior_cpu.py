"""The pose and shape priors without a GPU: the float64 oracle (tests/_prior_oracle.py) against closed forms and finite
differences; `fitting.PosePrior`'s constructors and validation; both launchers' argument errors (nothing is launched); the
torch ops' schemas and Meta kernels; the kernels' scratch and LDS as the built library reports them."""
import ctypes
import importlib
import os
import pickle
import sys

import numpy as np
import pytest
import torch

import _prior_oracle as po
from ilps_amd.smpl_model import load_mean_params

fitting = importlib.import_module("ilps_amd.fitting")     # (the one copy of the module that `ilps_amd.*` imports share)
MEAN_POSE = load_mean_params()[0]
PosePrior = fitting.PosePrior


def plain(K=1, A=0, seed=0):
    return po.make_prior(K, A, seed, MEAN_POSE)


def test_isotropic_single_gaussian_closed_form():
    """K = 1, A = I / sigma, c = 0: E = |d|^2 / (2 sigma^2) and the gradient d / sigma^2; every other column exactly 0."""
    sigma = 0.37
    p = plain()
    p["factor"] = (np.eye(69) / sigma)[None].astype(np.float32)
    p["offset"] = np.zeros(1, np.float32)
    x = po.make_rows(p, 4, 4, seed=1)
    o = po.prior(x, 4, p, (1.0, 0.0, 0.0))
    s = float(np.float32(1.0 / sigma))                        # the factor's entries as the kernel gets them
    d = x[:, 7:76].astype(np.float64) - p["mean"][0].astype(np.float64)
    assert np.allclose(o["E_pose"], 0.5 * s * s * (d * d).sum(1), rtol=1e-13, atol=0)
    assert np.allclose(o["grad"][:, 7:76], s * s * d, rtol=1e-13, atol=1e-300)
    assert not o["grad"][:, :7].any() and not o["grad"][:, 76:].any()
    assert np.array_equal(o["E"], o["E_pose"]) and not o["E_angle"].any() and not o["E_shape"].any() and not o["comp"].any()


@pytest.mark.parametrize("K,A,num_cam", [(1, 0, 4), (3, 4, 4), (8, 16, 0), (2, 4, 3)])
def test_oracle_gradient_is_the_finite_difference_of_its_energy(K, A, num_cam):
    p = plain(K, A, seed=K + A)
    x = po.make_rows(p, 2, num_cam, seed=5)
    w = (0.7, 1.3, 2.1)
    o = po.prior(x, num_cam, p, w)
    h = 2.0 ** -10                                            # exact in fp32 beside values of order 1
    for b in range(2):
        for j in range(num_cam + 82):
            xp, xm = x.copy(), x.copy()
            xp[b, j] += h
            xm[b, j] -= h
            step = float(xp[b, j]) - float(xm[b, j])
            op, om = po.prior(xp, num_cam, p, w), po.prior(xm, num_cam, p, w)
            if op["comp"][b] != o["comp"][b] or om["comp"][b] != o["comp"][b]:
                continue                                       # (the max-mixture has a kink where the component changes)
            fd = (op["E"][b] - om["E"][b]) / step
            assert abs(fd - o["grad"][b, j]) <= 1e-4 * max(1.0, o["grad_mag"][b, j]), (b, j, fd, o["grad"][b, j])
    assert not o["grad"][:, :num_cam].any()


def test_mixture_factors_and_offsets():
    rng = np.random.default_rng(3)
    K = 4
    M = rng.normal(0.0, 0.2, (K, 69, 69))
    covs = np.einsum("kij,klj->kil", M, M) + 0.05 * np.eye(69)
    w = np.array([0.1, 0.4, 0.3, 0.2])
    means = rng.normal(0.0, 0.3, (K, 69))
    factor, offset = fitting.mixture_terms(covs, w)
    for k in range(K):
        assert np.abs(factor[k].T @ factor[k] @ covs[k] - np.eye(69)).max() <= 1e-9
        assert np.array_equal(factor[k], np.triu(factor[k]))
    logdet = np.array([np.linalg.slogdet(c)[1] for c in covs])
    assert np.allclose(offset, -np.log(w) + 0.5 * (logdet - logdet.min()), rtol=1e-12, atol=1e-12) and (offset >= 0).all()
    p = PosePrior.mixture(means, covs, w)
    assert p.K == K and p.A == 0 and p.mean.dtype == p.factor.dtype == p.offset.dtype == torch.float32
    assert torch.equal(p.factor, torch.as_tensor(factor.astype(np.float32))) and torch.equal(p.offset, torch.as_tensor(offset.astype(np.float32)))
    assert p.angle_idx.dtype == torch.int32 and tuple(p.shape_mean.shape) == (10,) and not p.shape_mean.any()
    g = PosePrior.gaussian(means[0], covs[0])
    assert g.K == 1 and float(g.offset[0]) == 0.0 and torch.equal(g.factor[0], p.factor[0])
    s = PosePrior.from_samples(rng.normal(0.0, 0.3, (20, 69)), shrink=0.2)       # fewer samples than dimensions
    assert s.K == 1 and bool(torch.isfinite(s.factor).all())
    mp = PosePrior.mean_pose(0.5)
    assert torch.equal(mp.mean[0], torch.as_tensor(MEAN_POSE[3:].astype(np.float32))) and float(mp.factor[0, 5, 5]) == 2.0
    a = mp.with_angles().with_shape_mean(np.arange(10.0))
    assert a.angle_idx.tolist() == [55, 58, 12, 15] == list(fitting.SMPLIFY_ANGLE_IDX) and a.angle_scale.tolist() == [1.0, -1.0, -1.0, -1.0]
    assert a.shape_mean.tolist() == list(range(10)) and mp.A == 0
    assert torch.equal(a.to("cpu").factor, a.factor) and a.to("cpu").angle_idx.dtype == torch.int32


def test_first_minimum_wins_and_nan_stays():
    p = plain(3, 0, seed=2)
    p["mean"][1], p["factor"][1], p["offset"][1] = p["mean"][0], p["factor"][0], p["offset"][0]
    p["offset"][2] = 50.0
    x = po.make_rows(p, 6, 4, seed=2)
    x[:, 7:76] = p["mean"][0] + 0.01
    assert po.prior(x, 4, p, (1.0, 1.0, 1.0))["comp"].tolist() == [0] * 6     # two identical components: the first
    x[0, 9] = np.nan
    o = po.prior(x, 4, p, (1.0, 0.0, 0.0))
    assert o["comp"][0] == 0 and np.isnan(o["E"][0]) and np.isfinite(o["E"][1:]).all()


def test_zero_weight_skips_a_term_that_would_overflow():
    p = plain(2, 4, seed=4)
    x = po.make_rows(p, 2, 4, seed=4)
    x[0, 4 + int(p["angle_idx"][1])] = 400.0
    p["angle_scale"][1] = 2.0                                  # exp(800) = inf
    x[1, 80] = np.float32(3e38)                                # E_shape = 9e76: finite in float64, beyond fp32
    on = po.prior(x, 4, p, (1.0, 1.0, 1.0))
    assert np.isinf(on["E_angle"][0]) and np.isinf(on["E"][0]) and on["E_shape"][1] > 3.5e38 and np.isfinite(on["E"][1])
    off = po.prior(x, 4, p, (1.0, 0.0, 0.0))
    assert not off["E_angle"].any() and not off["E_shape"].any() and np.array_equal(off["E"], off["E_pose"])
    assert np.isfinite(off["E"]).all() and np.isfinite(off["grad"]).all() and not off["grad"][:, 76:].any()
    none = po.prior(x, 4, p, (0.0, 0.0, 0.0))
    assert not none["E"].any() and not none["grad"].any() and not none["comp"].any()


def test_from_pickle_reads_arrays_and_refuses_foreign_globals(tmp_path):
    rng = np.random.default_rng(8)
    K = 3
    M = rng.normal(0.0, 0.2, (K, 69, 69))
    dd = {"means": rng.normal(0.0, 0.3, (K, 69)), "covars": np.einsum("kij,klj->kil", M, M) + 0.05 * np.eye(69),
          "weights": np.array([0.2, 0.5, 0.3])}
    path = tmp_path / "gmm.pkl"
    with open(path, "wb") as f:
        pickle.dump(dd, f, protocol=2)
    p = PosePrior.from_pickle(str(path))
    want = PosePrior.mixture(dd["means"], dd["covars"], dd["weights"])
    assert p.K == K and torch.equal(p.mean, want.mean) and torch.equal(p.factor, want.factor) and torch.equal(p.offset, want.offset)
    marker = tmp_path / "ran"
    evil = tmp_path / "evil.pkl"
    with open(evil, "wb") as f:                                # a pickle that names os.system: refused at the global, never called
        f.write(b"cos\nsystem\n(S'touch " + str(marker).encode() + b"'\ntR.")
    with pytest.raises(pickle.UnpicklingError):
        PosePrior.from_pickle(str(evil))
    assert not marker.exists()
    import collections
    with open(evil, "wb") as f:
        pickle.dump(collections.OrderedDict(dd), f, protocol=2)
    with pytest.raises(pickle.UnpicklingError):
        PosePrior.from_pickle(str(evil))
    with open(evil, "wb") as f:
        pickle.dump({"means": dd["means"]}, f, protocol=2)
    with pytest.raises(ValueError):
        PosePrior.from_pickle(str(evil))


def test_validation_errors():
    p = plain(2, 2, seed=1)
    ok = PosePrior(**{k: p[k] for k in p})
    assert ok.K == 2 and ok.A == 2
    big = plain(17, 0, seed=1)
    with pytest.raises(ValueError, match="K"):
        PosePrior(mean=big["mean"], factor=big["factor"], offset=big["offset"])
    with pytest.raises(ValueError, match="0..71"):
        ok.with_angles([5, 72], [1.0, 1.0])
    with pytest.raises(ValueError, match="0..71"):
        ok.with_angles([-1], [1.0])
    with pytest.raises(ValueError):
        ok.with_angles(list(range(17)), [1.0] * 17)
    with pytest.raises(ValueError):
        ok.with_angles([5, 6], [1.0])
    bad = p["factor"].copy()
    bad[1, 3, 4] = np.inf
    with pytest.raises(ValueError, match="finite"):
        PosePrior(mean=p["mean"], factor=bad, offset=p["offset"])
    with pytest.raises(ValueError):
        PosePrior(mean=p["mean"], factor=p["factor"], offset=-p["offset"] - 1.0)
    with pytest.raises(ValueError):
        PosePrior(mean=p["mean"], factor=p["factor"][:, :68], offset=p["offset"])
    with pytest.raises(ValueError):
        ok.with_shape_mean(np.zeros(9))
    for w in ((1.0, -0.5, 1.0), (1.0, float("nan"), 1.0), (1.0, 1.0), (float("inf"), 0.0, 0.0)):
        with pytest.raises(ValueError):
            fitting.check_prior_weights(w)
    assert fitting.check_prior_weights((0.0, 2.0, 0.5)).tolist() == [0.0, 2.0, 0.5]
    with pytest.raises(ValueError):
        PosePrior.mixture(np.zeros((1, 69)), -np.eye(69)[None], [1.0])
    with pytest.raises(RuntimeError):
        fitting.prior_energy(torch.zeros(2, 86), ok)           # CPU tensors: there is no CPU path


def test_layout_check_before_a_launch():
    """`check_prior_layout` (run by every Python entry point before its launch) on priors whose fields were replaced behind
    the constructor's back: the kernels would read K * 69 * 69, A and 10 elements on trust."""
    p = plain(2, 2, seed=1)
    good = PosePrior(**p)
    assert fitting.check_prior_layout(good) is good and fitting.check_prior_layout(good.to("cpu")) is not None
    broken = dict(factor=good.factor[:, :68].contiguous(), factor_t=good.factor.transpose(1, 2), mean=good.mean[:, :68].contiguous(),
                  offset=good.offset[:1].contiguous(), angle_scale=good.angle_scale[:1].contiguous(), idx64=good.angle_idx.long(),
                  shape_mean=good.shape_mean[:9].contiguous(), angle_idx=None, mean64=good.mean.double())
    for name, value in broken.items():
        bad = good.to("cpu")
        setattr(bad, {"factor_t": "factor", "idx64": "angle_idx", "mean64": "mean"}.get(name, name), value)
        with pytest.raises(RuntimeError):
            fitting.check_prior_layout(bad)
    with pytest.raises(TypeError):
        fitting.check_prior_layout(p)
    # `.to()` alone skips the constructor's validation, and only for fields that passed it
    assert torch.equal(good.to("cpu").factor, good.factor) and good.to("cpu").factor.data_ptr() == good.factor.data_ptr()


def test_launchers_argument_errors_launch_nothing():
    from ilps_amd import _lib
    lib = _lib.load()
    one = ctypes.c_void_p(16)          # a non-null pointer that is never dereferenced: every call below fails its checks first

    def energy(B=1, P=86, num_cam=4, K=8, A=4, ptr=one, aptr=one, out=one):
        return lib.smplr_prior_energy(ptr, B, P, num_cam, ptr, ptr, ptr, aptr, aptr, ptr, K, A, ptr, out, out, None, None)

    def step(B=1, P=86, num_cam=4, K=8, A=4, ptr=one, aptr=one, pptr=one, N=2304, mode=0):
        return lib.smplr_fit_step_prior(ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, N, None, 0, 1.0, ptr, None, 0,
                                        B, P, 1e-3, 0.9, 0.999, 1e-7, 1.0, mode, 0, num_cam, pptr, pptr, pptr, aptr, aptr, pptr, K, A,
                                        pptr, None)
    for fn, name in ((energy, b"smplr_prior_energy"), (step, b"smplr_fit_step_prior")):
        for kw, word in ((dict(P=85), b"P=85"), (dict(P=86, num_cam=3), b"num_cam=3"), (dict(num_cam=-1, P=81), b"num_cam=-1"),
                         (dict(P=257, num_cam=175), b"P=257"), (dict(K=0), b"K=0"), (dict(K=17), b"K=17"), (dict(A=-1), b"A=-1"),
                         (dict(A=17), b"A=17"), (dict(B=-1), b"negative batch"), (dict(aptr=None), b"null pointer"),
                         (dict(ptr=None, aptr=None), b"null pointer")):
            assert fn(**kw) == -1, (name, kw)
            assert word in lib.smplr_last_error() and name in lib.smplr_last_error(), (kw, lib.smplr_last_error())
        assert fn(B=0, ptr=None, aptr=None) == 0               # an empty batch is a no-op
        assert fn(B=0, K=17) == -1                             # ... of a valid call only
    assert energy(out=None) == -1 and b"null pointer" in lib.smplr_last_error()
    assert step(pptr=None) == -1 and b"null pointer" in lib.smplr_last_error()
    assert step(N=0) == -1 and b"N=0" in lib.smplr_last_error()
    assert step(mode=2) == -1 and b"mode 2" in lib.smplr_last_error()
    assert lib.smplr_abi_version() == 7


def test_op_schemas_and_meta_kernels():
    from ilps_amd import torch_ops
    ns = torch_ops.load()
    for name in ("prior_energy", "fit_step_prior"):
        assert str(getattr(ns, name).default._schema) == torch_ops.SCHEMAS[name]
    assert ns.fit_step_prior.default._schema.is_mutable and not ns.prior_energy.default._schema.is_mutable
    f = lambda *s, dev="meta": torch.zeros(*s, dtype=torch.float32, device=dev)

    def prior(dev="meta", K=8, A=4):
        return [f(K, 69, dev=dev), f(K, 69, 69, dev=dev), f(K, dev=dev), torch.zeros(A, dtype=torch.int32, device=dev), f(A, dev=dev),
                f(10, dev=dev), f(3, dev=dev)]
    energy, comp, grad = ns.prior_energy(f(5, 86), *prior())
    assert tuple(energy.shape) == (5, 4) and tuple(comp.shape) == (5,) and comp.dtype == torch.int32 and tuple(grad.shape) == (5, 86)
    assert tuple(ns.prior_energy(f(5, 85), *prior(K=1, A=0), 3, False)[2].shape) == (0, 85)
    assert tuple(ns.prior_energy(f(0, 82), *prior(K=16, A=16), num_cam=0)[0].shape) == (0, 4)
    for bad in (dict(K=17), dict(K=0), dict(A=17)):
        with pytest.raises(RuntimeError):
            ns.prior_energy(f(5, 86), *prior(**bad))
    with pytest.raises(RuntimeError):
        ns.prior_energy(f(5, 86), *prior(), num_cam=3)         # P != num_cam + 82
    a = prior()
    a[3] = a[3].long()
    with pytest.raises(RuntimeError):
        ns.prior_energy(f(5, 86), *a)                          # angle_idx must be int32
    a = prior()
    a[6] = f(2)
    with pytest.raises(RuntimeError):
        ns.prior_energy(f(5, 86), *a)                          # weights must be (3,)
    with pytest.raises((RuntimeError, NotImplementedError)):
        ns.prior_energy(f(5, 86, dev="cpu"), *prior("cpu"))    # CPU tensors: no kernel registered for them

    def state(B=3, P=86, N=2304, dev="meta"):
        i = lambda: torch.zeros(B, dtype=torch.int32, device=dev)
        return [f(B, P, dev=dev), f(B, P, dev=dev), f(B, P, dev=dev), f(B, P, dev=dev), i(), i(), i(), i(), i(),
                torch.ones(B, dtype=torch.uint8, device=dev), f(B, dev=dev), f(B, P, dev=dev), f(B, N, dev=dev), None, f(P, dev=dev),
                f(5, B, dev=dev)]
    assert ns.fit_step_prior(*state(), *prior()) is None
    assert ns.fit_step_prior(*state(P=85), *prior(K=1, A=0), 1e-3, 0.9, 0.999, 1e-8, 0.5, 2.0, 1, 3, 3) is None
    with pytest.raises(RuntimeError):
        ns.fit_step_prior(*state(P=85), *prior())              # P != num_cam + 82
    with pytest.raises(RuntimeError):
        ns.fit_step_prior(*state(), *prior(K=17))
    with pytest.raises(RuntimeError):
        ns.fit_step_prior(*state(N=0), *prior())
    with pytest.raises(RuntimeError):
        ns.fit_step_prior(*state(), *prior(), mode=2)
    with pytest.raises((RuntimeError, NotImplementedError)):
        ns.fit_step_prior(*state(dev="cpu"), *prior("cpu"))


def test_prior_kernels_use_no_scratch():
    """What the code objects say (no GPU): no scratch and no spills in the three kernels of csrc/fit.hip, under 4 KB of LDS
    per workgroup with the prior, and the kernel behind smplr_fit_step carries none of the prior's LDS."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import kernel_resources as kr
    ks = kr.kernels()
    hit = {n: k for n, k in ks.items() if "prior_kernel" in n or "fit_step_kernel" in n}
    assert len(hit) == 3, sorted(hit)
    for name, k in hit.items():
        assert k["scratch"] == 0 and k["agpr"] == 0 and k["max_threads"] >= 256, (name, k)
        assert kr.waves_per_simd(k) >= 2, (name, k)          # two 4-wave workgroups per CU
        plain_step = "fit_step_kernelILb0E" in name
        assert (k["lds"] < 512) if plain_step else (3000 < k["lds"] <= 4096), (name, k["lds"])
