"""The 6D rotation pose head without a GPU: the float64 oracle (tests/_rot6d_oracle.py) against exact Rodrigues, central
differences and autograd of the Gram-Schmidt map; `rot6d.params_from_rot6d_torch` against the oracle; the conversions; the
regressor in 6D space with the torch restatement in the kernels' place; the C ABI's refusals and the ops' Meta kernels."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _rot6d_oracle as o  # noqa: E402
from ilps_amd import rot6d  # noqa: E402
from ilps_amd.supervised import rodrigues  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ANGLES = (0.0, 1e-9, 1e-6, 1e-3, 1.0, 3.0, np.pi - 1e-3, np.pi - 1e-6, np.pi)


def ladder(seed=0, angles=ANGLES):
    """Every angle at the scales 1, 1e-3 and 1e3, sheared: (27, 6) and the angles."""
    return o.ladder_inputs(np.random.default_rng(seed), angles)


def test_exact_rodrigues_of_the_oracles_theta_is_the_gram_schmidt_matrix():
    a, phis = ladder()
    theta, flags = o.joint_forward(a)
    assert (flags == 0).all()
    assert np.abs(o.rodrigues_exact(theta) - o.matrix(a)).max() <= 1e-12
    # the angle comes back (atan2 of the quaternion, not acos of the trace): absolute 1e-12 at every rung
    assert np.abs(np.linalg.norm(theta, axis=-1) - phis).max() <= 1e-12
    assert (np.linalg.norm(theta, axis=-1) <= np.pi * (1 + 1e-15)).all()       # (phi <= pi; the norm of phi v / |v| rounds)
    assert (theta[phis == 0] == 0).all()                                        # exactly


def test_oracle_gradient_matches_central_differences():
    a, phis = ladder(1)
    keep = phis <= np.pi - 1e-3
    a = np.concatenate([a[keep], np.random.default_rng(2).normal(size=(16, 6))])
    g = np.random.default_rng(3).normal(size=(a.shape[0], 3))
    da = o.joint_backward(a, g)
    scale = np.abs(a).max(1)                                                    # (the inputs span six decades)
    num = np.zeros_like(a)
    for i in range(6):
        h = np.zeros_like(a)
        h[:, i] = 1e-6 * scale
        num[:, i] = ((o.joint_forward(a + h)[0] - o.joint_forward(a - h)[0]) * g).sum(-1) / (2e-6 * scale)
    # central differences at a relative step of 1e-6: truncation 1e-12, rounding 1e-16 / 1e-6 = 1e-10, both relative
    err = np.abs(num - da).max(1) / np.abs(da).max(1)
    print("central differences, worst relative deviation %.3g" % err.max())
    assert err.max() <= 1e-7


def test_oracle_gradient_through_rodrigues_is_autograd_of_gram_schmidt():
    """L = sum(W . R): through theta (the package's Rodrigues, then the oracle's backward) and directly (autograd of the
    Gram-Schmidt map).  Relative to each joint's gradient norm; the package's Rodrigues shifts theta by 1e-8 per component,
    which is all of the deviation (float64 autograd of the torch restatement meets the oracle to 1e-15): 9.7e-8 at the worst
    joint, a rung at 1e-9 rad where the shift is ten times the angle, below 4e-8 from 1e-3 rad up."""
    rng = np.random.default_rng(4)
    a, phis = ladder(5)
    a = np.concatenate([a[phis <= np.pi - 1e-3], rng.normal(size=(43, 6))])
    W = rng.normal(size=(a.shape[0], 3, 3))
    at = torch.tensor(a, requires_grad=True)
    (torch.tensor(W) * rot6d.rot6d_to_matrix(at)).sum().backward()
    theta = torch.tensor(o.joint_forward(a)[0], requires_grad=True)
    (torch.tensor(W) * rodrigues(theta)).sum().backward()
    da = o.joint_backward(a, theta.grad.numpy())
    want = at.grad.numpy()
    err = np.linalg.norm(da - want, axis=1) / np.linalg.norm(want, axis=1)
    print("through Rodrigues against Gram-Schmidt's autograd, worst relative deviation %.3g" % err.max())
    assert err.max() <= 1e-7


def rows(seed, B, num_cam):
    rng = np.random.default_rng(seed)
    a, _ = ladder(seed)
    aa = np.concatenate([a, rng.normal(size=(B * 24 - a.shape[0], 6))])[rng.permutation(B * 24)]
    return np.concatenate([rng.normal(size=(B, num_cam)), aa.reshape(B, 144), rng.normal(size=(B, 10))], 1)


@pytest.mark.parametrize("num_cam", [0, 4, 8])
def test_torch_restatement_in_float64_is_the_oracle(num_cam):
    y = rows(6, 3, num_cam)
    yt = torch.tensor(y, requires_grad=True)
    x = rot6d.params_from_rot6d_torch(yt, num_cam)
    want, status = o.forward(y, num_cam)
    assert (status == 0).all() and x.shape == (3, num_cam + 82) and x.dtype == torch.float64
    assert np.abs(x.detach().numpy() - want).max() <= 1e-12
    assert np.array_equal(x.detach().numpy()[:, :num_cam], y[:, :num_cam]) and np.array_equal(x.detach().numpy()[:, -10:], y[:, -10:])
    dx = np.random.default_rng(7).normal(size=want.shape)
    x.backward(torch.tensor(dx))
    dy, got = o.backward(y, dx, num_cam), yt.grad.numpy()
    j = slice(num_cam, num_cam + 144)
    err = np.abs(got[:, j] - dy[:, j]).reshape(-1, 6).max(1) / np.abs(dy[:, j]).reshape(-1, 6).max(1)
    assert err.max() <= 1e-10, err.max()
    assert np.array_equal(got[:, :num_cam], dx[:, :num_cam]) and np.array_equal(got[:, -10:], dx[:, -10:])


def test_torch_restatement_on_hostile_joints():
    y = rows(8, 2, 4)
    y[0, 4:10] = [0, 1, 0, 0, 0, 0]                     # a1 = 0
    y[0, 10:16] = [1, 2, 2, 4, -1, -2]                  # a2 parallel to a1
    y[1, 4:10] = [1, 0, 0, 0, 0, 0]                     # a2 = 0
    x = rot6d.params_from_rot6d_torch(torch.tensor(y)).numpy()
    want, status = o.forward(y)
    assert status.tolist() == [o.DEGENERATE, o.DEGENERATE]
    assert (x[0, 4:10] == 0).all() and (x[1, 4:7] == 0).all() and np.abs(x - want).max() <= 1e-12
    y[1, 16] = np.nan
    x = rot6d.params_from_rot6d_torch(torch.tensor(y)).numpy()
    want, status = o.forward(y)
    assert status.tolist() == [o.DEGENERATE, o.DEGENERATE | o.NONFINITE]
    assert np.isnan(x[1, 10:13]).all() and np.isnan(want[1, 10:13]).all()
    keep = np.ones(86, bool)
    keep[10:13] = False
    assert np.isfinite(x[:, keep]).all() and np.abs(x[:, keep] - want[:, keep]).max() <= 1e-12
    da = o.backward(y, np.ones((2, 86)))
    assert (da[0, 4:16] == 0).all() and (da[1, 4:10] == 0).all() and np.isnan(da[1, 16:22]).all()
    assert np.isfinite(np.delete(da, np.s_[16:22], 1)).all()


def test_axis_angle_to_rot6d_and_back():
    rng = np.random.default_rng(9)
    theta = rng.normal(size=(200, 3))
    theta *= (rng.uniform(0, np.pi - 1e-3, (200, 1)) / np.linalg.norm(theta, axis=1, keepdims=True))
    theta[0] = 0
    a = rot6d.axis_angle_to_rot6d(torch.tensor(theta))
    assert a.shape == (200, 6)
    back, flags = o.joint_forward(a.numpy())
    # (the package's Rodrigues moves theta by up to 1e-8 |(1, 1, 1)| before it takes the angle)
    assert (flags == 0).all() and np.abs(back - theta).max() <= 5e-8
    R = rodrigues(torch.tensor(theta))
    assert torch.equal(a.reshape(200, 3, 2), R[:, :, :2])
    # (that Rodrigues' axis theta / |theta + 1e-8| is not quite a unit vector: R is orthonormal to (1 - cos) 2e-8 / phi <= 6e-8)
    assert (rot6d.rot6d_to_matrix(a) - R).abs().max() <= 1e-7
    assert np.abs(rot6d.rot6d_to_matrix(a).numpy() - o.matrix(a.numpy())).max() <= 1e-15


def test_mean_row_is_mean86_in_6d():
    from ilps_amd.smpl_model import mean86
    row = rot6d.mean_rot6d_row(48)
    assert row.shape == (1, 158) and row.dtype == torch.float32 and rot6d.mean_rot6d_row(48) is row
    m = mean86(48)
    assert np.array_equal(row[0, :4].numpy(), m[:4].astype(np.float32)) and np.array_equal(row[0, 148:].numpy(), m[76:].astype(np.float32))
    back = o.forward(row.numpy().astype(np.float64))[0][0]
    assert np.abs(back[4:76] - m[4:76]).max() <= 2e-7                           # (fp32 storage of the 6-vectors)


def models_rot6d():
    """The `rot6d` module object that model.py's `from .rot6d import ...` reads.  `ilps_amd` is an alias of the hyphenated
    package directory, so `from ilps_amd.model import ...` and `from ilps_amd import rot6d` can load a submodule under two
    names, as two objects: a patch has to go to the one in the model's own package."""
    import importlib
    from ilps_amd.model import SMPLRegressor
    return importlib.import_module(sys.modules[SMPLRegressor.__module__].__package__ + ".rot6d")


class _Stub(torch.nn.Module):
    """(N, 3, 64, 64) -> (N, 2048): a stand-in for the backbones, which take 256 x 256 (ENet) or 224 .. 287 (ResNet50)."""

    def __init__(self):
        super().__init__()
        self.fc = torch.nn.Linear(3 * 64 * 64, 2048)

    def forward(self, x):
        return self.fc(x.flatten(1))


@pytest.mark.parametrize("use_IEF", [True, False])
def test_regressor_in_6d_space_on_the_cpu(monkeypatch, use_IEF):
    from ilps_amd.model import SMPLRegressor
    from ilps_amd.smpl_model import mean86
    calls = []

    def head(y, num_cam=4, return_status=False):
        calls.append(tuple(y.shape))
        assert y.dtype == torch.float32 and return_status
        return rot6d.params_from_rot6d_torch(y, num_cam), torch.zeros(y.shape[0], dtype=torch.int32)
    monkeypatch.setattr(models_rot6d(), "params_from_rot6d", head)
    torch.manual_seed(0)
    net = SMPLRegressor(64, "enet", use_IEF, pose_repr="rot6d")
    sd = net.state_dict()
    if use_IEF:
        assert sd["IEF_layer_1.weight"].shape == (1024, 2048 + 158) and sd["IEF_layer_3.weight"].shape == (158, 1024)
    else:
        assert sd["mlp.4.weight"].shape == (158, 1024)
    net.backbone = _Stub()
    assert net.pose_status is None
    images = torch.randn(2, 3, 64, 64)
    out = net(images)
    assert out.shape == (2, 86) and out.dtype == torch.float32 and calls == [(2, 158)]
    assert net.pose_status.shape == (2,) and net.pose_status.dtype == torch.int32
    out.square().sum().backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in net.parameters())
    # a regressor that regresses nothing gives the mean pose: scaledown applies to the 158-delta
    last = net.IEF_layer_3 if use_IEF else net.mlp[4]
    with torch.no_grad():
        last.weight.zero_()
        last.bias.zero_()
        assert np.abs(net(images)[0].numpy() - mean86(64)).max() <= 2e-6
        last.bias.fill_(1.0)
        y = rot6d.mean_rot6d_row(64) + net.scaledown * (3 if use_IEF else 1)
        assert torch.allclose(net(images)[:1], rot6d.params_from_rot6d_torch(y), atol=1e-6)
    with pytest.raises(ValueError, match="pose_repr"):
        SMPLRegressor(64, "enet", pose_repr="quaternion")


def test_enet_backbone_with_the_158_wide_head_on_the_cpu(monkeypatch):
    """The real ENet branch (256 x 256, the only size it takes) in front of the 6D regression module, B = 1."""
    from ilps_amd.model import SMPLRegressor
    monkeypatch.setattr(models_rot6d(), "params_from_rot6d",
                        lambda y, num_cam=4, return_status=False: (rot6d.params_from_rot6d_torch(y, num_cam),
                                                                   torch.zeros(y.shape[0], dtype=torch.int32)))
    torch.manual_seed(1)
    net = SMPLRegressor(48, "enet", True, pose_repr="rot6d").eval()
    with torch.no_grad():
        out = net(torch.randn(1, 256, 256, 3))                                  # NHWC accepted
    assert out.shape == (1, 86) and torch.isfinite(out).all()
    assert torch.allclose(out[0, :4], torch.tensor([24.0, 24.0, 24.0, 30.0]), atol=0.5)


def test_row_strides_beyond_int32_are_made_contiguous():
    """The launchers take the row stride as an int: the autograd path copies such a view, as the torch op refuses it."""
    far = torch.empty_strided((2, 158), (2 ** 31, 1), device="meta")
    assert rot6d._rows32(far).stride() == (158, 1)
    near = torch.empty_strided((2, 158), (2 ** 31 - 1, 1), device="meta")
    assert rot6d._rows32(near).stride() == (2 ** 31 - 1, 1)
    assert rot6d._rows32(torch.empty_strided((1, 158), (2 ** 31, 1), device="meta")).shape == (1, 158)


def test_default_regressor_keeps_its_state_dict():
    """(tests/test_synthetic_cpu.py holds the default's keys and shapes against the recorded ones; here: the new argument's
    default is that regressor, and only "rot6d" widens the head.)"""
    import inspect
    from ilps_amd.model import SMPLRegressor, build_model
    for arch in ("enet", "resnet50"):
        for ief in (False, True):
            a = {k: tuple(v.shape) for k, v in SMPLRegressor(48, arch, ief).state_dict().items()}
            b = {k: tuple(v.shape) for k, v in SMPLRegressor(48, arch, ief, pose_repr="axis_angle").state_dict().items()}
            assert a == b and not any("158" in str(s) for s in a.values())
            assert a["IEF_layer_3.weight" if ief else "mlp.4.weight"] == (86, 1024)
            if ief:
                assert a["IEF_layer_1.weight"] == (1024, 2048 + 86)
    assert inspect.signature(build_model).parameters["pose_repr"].default == "axis_angle"
    assert inspect.signature(SMPLRegressor.__init__).parameters["pose_repr"].default == "axis_angle"


def test_abi_symbols_constants_and_refusals_without_launching():
    from ilps_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "smplraster.h")).read()
    for name in ("smplr_rot6d_fwd", "smplr_rot6d_bwd"):
        assert name in _lib.SIGNATURES and hasattr(lib, name) and "int %s(" % name in header
    assert "#define SMPLR_ABI_VERSION 7" in header
    assert "#define SMPLR_ROT6D_NONFINITE %d" % rot6d.NONFINITE in header and rot6d.NONFINITE == o.NONFINITE == 1
    assert "#define SMPLR_ROT6D_DEGENERATE %d" % rot6d.DEGENERATE in header and rot6d.DEGENERATE == o.DEGENERATE == 2
    one, err = 1, lib.smplr_last_error                  # (pointer values that are never dereferenced: nothing is launched)

    def fwd(y=one, stride=158, B=2, num_cam=4, x=one, status=one):
        return lib.smplr_rot6d_fwd(y, stride, B, num_cam, x, status, None)

    def bwd(y=one, stride=158, B=2, num_cam=4, x=one, status=one, dstride=86):
        return lib.smplr_rot6d_bwd(y, stride, status, x, dstride, B, num_cam, one, None)
    for fn, name in ((fwd, b"smplr_rot6d_fwd"), (bwd, b"smplr_rot6d_bwd")):
        assert fn(y=None) == -1 and b"null" in err() and name in err()
        assert fn(x=None) == -1 and fn(status=None) == -1 and b"null" in err()
        assert fn(num_cam=9) == -1 and b"num_cam=9" in err() and name in err()
        assert fn(num_cam=-1) == -1 and fn(B=-1) == -1 and b"B=-1" in err()
        assert fn(stride=157) == -1 and b"y_stride=157" in err() and fn(stride=161, num_cam=8) == -1
        assert fn(B=0, y=None, x=None, status=None) == 0                        # an empty batch is a no-op
    assert bwd(dstride=85) == -1 and b"dx_stride=85" in err()
    assert lib.smplr_rot6d_bwd(one, 158, one, one, 86, 2, 4, None, None) == -1 and b"null" in err()


def test_torch_ops_have_meta_kernels_and_refuse_cpu_tensors():
    from ilps_amd import torch_ops
    ns = torch_ops.load()
    m = lambda *s, dt=torch.float32: torch.empty(*s, dtype=dt, device="meta")
    for B, nc in ((2, 4), (0, 0), (5, 8)):
        x, status = ns.rot6d_fwd(m(B, nc + 154), nc)
        assert x.shape == (B, nc + 82) and x.dtype == torch.float32 and status.shape == (B,) and status.dtype == torch.int32
        assert ns.rot6d_bwd(m(B, nc + 154), status, m(B, nc + 82), nc).shape == (B, nc + 154)
    x, status = ns.rot6d_fwd(m(3, 200)[:, 7:165])                               # a column slice of a wider tensor
    assert x.shape == (3, 86)
    for bad in (lambda: ns.rot6d_fwd(m(2, 157)), lambda: ns.rot6d_fwd(m(2, 163), 9), lambda: ns.rot6d_fwd(m(2, 158, dt=torch.float64)),
                lambda: ns.rot6d_bwd(m(2, 158), m(2, dt=torch.int32), m(2, 85)), lambda: ns.rot6d_bwd(m(2, 158), m(3, dt=torch.int32), m(2, 86)),
                lambda: ns.rot6d_fwd(m(4, 316)[:, ::2])):
        with pytest.raises(RuntimeError):
            bad()
    with pytest.raises((RuntimeError, NotImplementedError)):
        ns.rot6d_fwd(torch.zeros(1, 158))                                       # a CPU tensor: no kernel registered for it
    with pytest.raises((RuntimeError, NotImplementedError)):
        ns.rot6d_bwd(torch.zeros(1, 158), torch.zeros(1, dtype=torch.int32), torch.zeros(1, 86))
    with pytest.raises(RuntimeError, match="HIP device"):
        rot6d.params_from_rot6d(torch.zeros(1, 158))
    with pytest.raises(ValueError, match="num_cam"):
        rot6d.params_from_rot6d(torch.zeros(1, 163), num_cam=9)
    with pytest.raises(ValueError, match="158"):
        rot6d.params_from_rot6d(torch.zeros(1, 157))
