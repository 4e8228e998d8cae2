"""csrc/rot6d.hip on the device against the float64 oracle (tests/_rot6d_oracle.py): the angle ladder at three scales, sheared
and not, over batches with a partial last group and rows across workgroups, every camera width; strided rows through ctypes and
through torch.ops.smplraster; a row alone and inside a batch; hostile joints; the refusals; the chain into `SMPLLayer` against
the float64 chain from rotation matrices; a regressor in 6D space under both trainers."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _rot6d_oracle as o  # noqa: E402
from ilps_amd import rot6d  # noqa: E402
from ilps_amd.rot6d import params_from_rot6d  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
ANGLES = (0.0, 1e-9, 1e-6, 1e-3, 1.0, 3.0, np.pi - 1e-3, np.pi - 1e-6, np.pi)
HALF_TURNS = ((1, 0, 0, -1, 0, 0), (-1, 0, 0, 1, 0, 0), (-1, 0, 0, -1, 0, 0))      # w == 0 exactly: about x, y and z


def t(a, dtype=torch.float32):
    return torch.as_tensor(np.asarray(a), dtype=dtype).to(DEV)


def bits(a):
    return a.detach().contiguous().view(torch.int32)


def problem(B, num_cam, seed):
    """y (B, num_cam + 154) fp32 and dx (B, num_cam + 82) fp32: the ladder at the scales 1, 1e-3 and 1e3, sheared (27 joints) and
    not (27 more: in fp32 a shear swallows an angle below 1e-7), the three exact half turns, the rest Gaussian; shuffled over
    the B x 24 joints (B = 1 holds the first 24 of that order).  |a1| and |u| stay within [1e-3, 1e3]: scale 1e3 times at
    most 2 (1 + 0.8) is cut to 1e3 where it passes, scale 1e-3 times at least 0.5 is raised likewise."""
    rng = np.random.default_rng(seed)
    a = np.concatenate([o.ladder_inputs(rng, ANGLES)[0], o.ladder_inputs(rng, ANGLES, shear=False)[0], np.asarray(HALF_TURNS, float),
                        rng.normal(size=(max(B * 24 - 57, 0), 6))])
    a = a[rng.permutation(a.shape[0])][:B * 24].astype(np.float32)
    _, _, _, n1, nu, _ = o.gram_schmidt(a)
    for n, col in ((n1, 0), (nu, 1)):
        f = np.clip(n[:, 0], 1e-3 * 1.001, 1e3 / 1.001) / n[:, 0]
        a[:, col::2] = (a[:, col::2] * f[:, None]).astype(np.float32)
    _, _, _, n1, nu, _ = o.gram_schmidt(a)
    assert 1e-3 <= min(n1.min(), nu.min()) and max(n1.max(), nu.max()) <= 1e3
    y = np.concatenate([rng.normal(0, 20, (B, num_cam)), a.reshape(B, 144), rng.normal(size=(B, 10))], 1).astype(np.float32)
    dx = rng.normal(size=(B, num_cam + 82)).astype(np.float32)
    return y, dx


def run(y, dx, num_cam, rows=None):
    """The op on the device -> x, status, dy (numpy would lose the bits of a NaN's payload: tensors)."""
    if rows is not None:
        y, dx = y[rows], dx[rows]
    yt = t(y).requires_grad_(True)
    x, status = params_from_rot6d(yt, num_cam, return_status=True)
    assert not status.requires_grad and x.dtype == torch.float32 and status.dtype == torch.int32
    x.backward(t(dx))
    torch.cuda.synchronize()
    return x.detach(), status, yt.grad


def check_against_oracle(y, dx, num_cam, x, status, dy):
    B, nc = y.shape[0], num_cam
    x, status, dy = x.cpu().numpy(), status.cpu().numpy(), dy.cpu().numpy()
    want, st = o.forward(y, nc)
    dwant = o.backward(y, dx, nc)
    assert x.shape == (B, nc + 82) and dy.shape == (B, nc + 154) and status.tolist() == st.tolist() == [0] * B
    # cam and beta: bit copies in both directions
    for got, src, width in ((x, y, 72), (dy, dx, 144)):
        assert np.array_equal(got[:, :nc].view(np.int32), src[:, :nc].view(np.int32))
        assert np.array_equal(got[:, nc + width:].view(np.int32), src[:, -10:].view(np.int32))
    th, tw = x[:, nc:nc + 72].reshape(-1, 3).astype(np.float64), want[:, nc:nc + 72].reshape(-1, 3)
    phi = np.linalg.norm(tw, axis=1)
    seam = phi > np.pi - 1e-6
    err = np.abs(th - tw).max(1) / np.maximum(1.0, phi)
    print("B %d num_cam %d: theta worst %.3g of 1.2e-7 (%d joints at the seam), phi from %.3g" % (
        B, nc, err[~seam].max() if (~seam).any() else 0.0, seam.sum(), phi[phi > 0].min() if (phi > 0).any() else 0.0))
    assert (err[~seam] <= 1.2e-7).all()
    a = y[:, nc:nc + 144].reshape(-1, 6)
    if seam.any():                                                 # where the sign convention decides: the rotation itself
        assert np.abs(o.rodrigues_exact(th[seam]) - o.matrix(a[seam])).max() <= 5e-7
        assert (np.linalg.norm(th[seam], axis=1) <= np.pi * (1 + 2e-7)).all()
    # gradients; at the seam against the oracle with the sign the kernel's theta took (theta and -theta are one rotation there)
    sign = np.where(seam & ((th * tw).sum(1) < 0), -1.0, 1.0)
    g = dx[:, nc:nc + 72].reshape(-1, 3)
    flipped = o.joint_backward(a, g, sign=sign)
    dwant_a = np.where((sign < 0)[:, None], flipped, dwant[:, nc:nc + 144].reshape(-1, 6))
    got_a = dy[:, nc:nc + 144].reshape(-1, 6).astype(np.float64)
    gerr = np.abs(got_a - dwant_a).max(1) / np.abs(dwant_a).max(1)
    print("    gradient worst %.3g of 2.4e-7 (%d joints took the other sign)" % (gerr.max(), (sign < 0).sum()))
    assert (gerr <= 2.4e-7).all()


# ---- values and gradients --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("num_cam", [0, 3, 4, 8])
@pytest.mark.parametrize("B", [1, 3, 65, 130])
def test_forward_and_backward_against_the_oracle(B, num_cam):
    y, dx = problem(B, num_cam, seed=100 * B + num_cam)
    check_against_oracle(y, dx, num_cam, *run(y, dx, num_cam))


def test_exact_half_turns_and_the_identity():
    """w == 0 stays as Shepperd's candidate gives it: pi about +x, +y, +z; the identity gives exact zeros."""
    y = np.zeros((1, 158), np.float32)
    a = np.tile(np.asarray([1, 0, 0, 1, 0, 0], np.float32), (24, 1))
    a[:3] = HALF_TURNS
    a[3] *= 0.001
    a[4, 3] = 1000.0
    y[0, 4:148] = a.reshape(-1)
    x, status, dy = run(y, np.ones((1, 86), np.float32), 4)
    th = x.cpu().numpy()[0, 4:76].reshape(24, 3)
    assert int(status[0]) == 0 and np.array_equal(th[:3], np.float32(np.pi) * np.eye(3, dtype=np.float32)) and (th[3:] == 0).all()
    assert torch.isfinite(dy).all()
    check_against_oracle(y, np.ones((1, 86), np.float32), 4, x, status, dy)


# ---- strided rows ----------------------------------------------------------------------------------------------------------

def test_strided_rows_through_ctypes_and_the_torch_ops():
    from ilps_amd import torch_ops
    ns = torch_ops.load()
    B, nc = 67, 3
    y, dx = problem(B, nc, seed=7)
    x0, s0, dy0 = run(y, dx, nc)
    wide_y = torch.full((B, nc + 154 + 13), float("nan"), device=DEV)
    wide_dx = torch.full((B, nc + 82 + 9), float("nan"), device=DEV)
    wide_y[:, 5:5 + nc + 154] = t(y)
    wide_dx[:, 2:2 + nc + 82] = t(dx)
    ys, ds = wide_y[:, 5:5 + nc + 154], wide_dx[:, 2:2 + nc + 82]
    assert not ys.is_contiguous() and not ds.is_contiguous()
    # the autograd path (ctypes) on the views
    yv = wide_y.clone().requires_grad_(True)
    x1, s1 = params_from_rot6d(yv[:, 5:5 + nc + 154], nc, return_status=True)
    x1.backward(ds)
    g = yv.grad
    assert torch.equal(bits(x1), bits(x0)) and torch.equal(s1, s0) and torch.equal(bits(g[:, 5:5 + nc + 154]), bits(dy0))
    assert (g[:, :5] == 0).all() and (g[:, 5 + nc + 154:] == 0).all()
    # torch.ops
    x2, s2 = ns.rot6d_fwd(ys, nc)
    dy2 = ns.rot6d_bwd(ys, s2, ds, nc)
    assert torch.equal(bits(x2), bits(x0)) and torch.equal(s2, s0) and torch.equal(bits(dy2), bits(dy0))
    x3, s3 = ns.rot6d_fwd(t(y), nc)
    assert torch.equal(bits(x3), bits(x0)) and torch.equal(bits(ns.rot6d_bwd(t(y), s3, t(dx), nc)), bits(dy0))


# ---- a row alone and inside a batch ----------------------------------------------------------------------------------------

def test_a_row_alone_inside_a_batch_and_twice():
    B, nc = 130, 4
    y, dx = problem(B, nc, seed=9)
    x0, s0, dy0 = run(y, dx, nc)
    x1, s1, dy1 = run(y, dx, nc)
    assert torch.equal(bits(x0), bits(x1)) and torch.equal(s0, s1) and torch.equal(bits(dy0), bits(dy1))
    for b in (0, 7, 8, 64, 129):
        xr, sr, dyr = run(y, dx, nc, rows=[b])
        assert torch.equal(bits(xr[0]), bits(x0[b])) and int(sr[0]) == int(s0[b]) and torch.equal(bits(dyr[0]), bits(dy0[b]))
    xr, sr, dyr = run(y, dx, nc, rows=[129, 3, 64])
    assert torch.equal(bits(xr), bits(x0[[129, 3, 64]])) and torch.equal(bits(dyr), bits(dy0[[129, 3, 64]]))


# ---- hostile rows ----------------------------------------------------------------------------------------------------------

def test_hostile_joints_touch_nothing_else():
    B, nc = 11, 4
    y, dx = problem(B, nc, seed=13)
    clean = run(y, dx, nc)
    bad = y.copy()
    cases = {(0, 0): ([0, 1, 0, 2, 0, 3], rot6d.DEGENERATE),                    # a1 = 0
             (0, 23): ([1, -2, 2, -4, -1, 2], rot6d.DEGENERATE),                # a2 parallel to a1
             (3, 5): ([1, 0, 2, 0, 3, 0], rot6d.DEGENERATE),                    # a2 = 0
             (3, 6): ([1e-7, 0, 0, 1, 0, 0], rot6d.DEGENERATE),                 # |a1| below 1e-6
             (8, 11): ([1, 0, np.nan, 1, 0, 0], rot6d.NONFINITE),
             (9, 1): ([1, 0, 0, 1, np.inf, 0], rot6d.NONFINITE),
             (9, 2): ([0, 0, 0, 0, 0, 0], rot6d.DEGENERATE),
             (10, 0): ([-np.inf, 0, 0, 0, 0, 0], rot6d.NONFINITE)}
    want_status = np.zeros(B, np.int32)
    for (b, j), (six, flag) in cases.items():
        bad[b, nc + 6 * j:nc + 6 * j + 6] = six
        want_status[b] |= flag
    x, status, dy = run(bad, dx, nc)
    assert status.cpu().numpy().tolist() == want_status.tolist() and want_status[9] == 3
    st = o.forward(bad, nc)[1]
    assert st.tolist() == want_status.tolist()
    xs, dys, x0, dy0 = x.clone(), dy.clone(), clean[0].clone(), clean[2].clone()
    for (b, j), (six, flag) in cases.items():
        th, da = x[b, nc + 3 * j:nc + 3 * j + 3], dy[b, nc + 6 * j:nc + 6 * j + 6]
        if flag == rot6d.NONFINITE:
            assert torch.isnan(th).all() and torch.isnan(da).all()
        else:
            assert (bits(th) == 0).all() and (bits(da) == 0).all()               # +0.0, all nine
        for buf, w in ((xs, 3), (x0, 3), (dys, 6), (dy0, 6)):
            buf[b, nc + w * j:nc + w * j + w] = 0
    assert torch.equal(bits(xs), bits(x0)) and torch.equal(bits(dys), bits(dy0))  # every other joint, cam and beta: a clean run's bits
    # the backward recomputes each joint's flags from y: a stale, all-clean status gives the same bits
    from ilps_amd import torch_ops
    assert torch.equal(bits(torch_ops.load().rot6d_bwd(t(bad), torch.zeros_like(status), t(dx), nc)), bits(dy))


# ---- refusals --------------------------------------------------------------------------------------------------------------

def test_refusals_and_the_empty_batch():
    from ilps_amd import _lib, torch_ops
    ns, lib = torch_ops.load(), _lib.load()
    y = torch.zeros(2, 158, device=DEV)
    with pytest.raises(RuntimeError, match="HIP device"):
        params_from_rot6d(torch.zeros(2, 158))
    with pytest.raises((RuntimeError, NotImplementedError)):
        ns.rot6d_fwd(torch.zeros(2, 158))
    with pytest.raises(ValueError, match="158"):
        params_from_rot6d(y[:, :157])
    with pytest.raises(RuntimeError, match="158"):
        ns.rot6d_fwd(y[:, :157])
    with pytest.raises(ValueError, match="num_cam"):
        params_from_rot6d(torch.zeros(2, 163, device=DEV), num_cam=9)
    with pytest.raises(RuntimeError, match="num_cam"):
        ns.rot6d_fwd(torch.zeros(2, 163, device=DEV), 9)
    with pytest.raises(RuntimeError, match="float32"):
        params_from_rot6d(y.double())
    # the launchers themselves: -1 and a message, nothing launched (the outputs keep their fill)
    x, status = torch.full((2, 86), 7.0, device=DEV), torch.full((2,), 7, dtype=torch.int32, device=DEV)
    p = lambda a: a.data_ptr()
    assert lib.smplr_rot6d_fwd(p(y), 158, 2, 9, p(x), p(status), None) == -1 and b"num_cam=9" in lib.smplr_last_error()
    assert lib.smplr_rot6d_fwd(p(y), 157, 2, 4, p(x), p(status), None) == -1 and b"y_stride=157" in lib.smplr_last_error()
    assert lib.smplr_rot6d_fwd(None, 158, 2, 4, p(x), p(status), None) == -1 and b"null" in lib.smplr_last_error()
    assert lib.smplr_rot6d_bwd(p(y), 158, p(status), p(x), 85, 2, 4, p(y), None) == -1
    assert lib.smplr_rot6d_fwd(p(y), 158, 0, 4, p(x), p(status), None) == 0
    torch.cuda.synchronize()
    assert (x == 7).all() and (status == 7).all()
    # B = 0 through every path
    e = torch.zeros(0, 158, device=DEV, requires_grad=True)
    x0, s0 = params_from_rot6d(e, return_status=True)
    assert x0.shape == (0, 86) and s0.shape == (0,)
    x0.sum().backward()
    assert e.grad.shape == (0, 158)
    x0, s0 = ns.rot6d_fwd(e.detach())
    assert x0.shape == (0, 86) and ns.rot6d_bwd(e.detach(), s0, x0).shape == (0, 158)


# ---- the chain into the decoder --------------------------------------------------------------------------------------------

def _chain_inputs(B=4, seed=21):
    """y: the mean pose in 6D, perturbed (sigma 0.15 on the six numbers: unnormalised, sheared), beta sigma 1."""
    rng = np.random.default_rng(seed)
    y = np.tile(rot6d.mean_rot6d_row(48).numpy(), (B, 1)).astype(np.float64)
    y[:, 4:148] += rng.normal(0, 0.15, (B, 144))
    y[:, 4:148] *= rng.uniform(0.5, 2.0, (B, 24, 1)).repeat(6, 2).reshape(B, 144)
    y[:, 148:] += rng.normal(0, 1.0, (B, 10))
    return y.astype(np.float32)


def _smpl_from_matrices(smpl, Rs, betas):
    """oracle/torch_oracle.TorchSMPL.__call__ with the rotations given as matrices (its lines after batch_rodrigues)."""
    from oracle.torch_oracle import batch_global_rigid_transformation
    N, V = Rs.shape[0], smpl.V
    v_shaped = (betas @ smpl.shapedirs).reshape(-1, V, 3) + smpl.v_template
    J = torch.stack([v_shaped[:, :, c] @ smpl.J_regressor for c in range(3)], dim=2)
    pose_feature = (Rs[:, 1:] - torch.eye(3, dtype=Rs.dtype)).reshape(-1, 207)
    v_posed = (pose_feature @ smpl.posedirs).reshape(-1, V, 3) + v_shaped
    _, A = batch_global_rigid_transformation(Rs, J, smpl.parents)
    T = (smpl.lbs_weights.repeat(N, 1).reshape(N, -1, 24) @ A.reshape(N, 24, 16)).reshape(N, -1, 4, 4)
    return (T @ torch.cat([v_posed, torch.ones(N, V, 1, dtype=Rs.dtype)], dim=2).unsqueeze(-1))[:, :, :3, 0]


def chain_reference(model, y, W):
    """dL/dy in float64 for L = sum(W . verts), verts from `rot6d_to_matrix` of y's six-vectors: no theta anywhere."""
    from oracle.torch_oracle import TorchSMPL
    yt = torch.tensor(y, dtype=torch.float64, requires_grad=True)
    Rs = rot6d.rot6d_to_matrix(yt[:, 4:148].reshape(-1, 24, 6))
    (torch.tensor(W) * _smpl_from_matrices(TorchSMPL(model), Rs, yt[:, 148:])).sum().backward()
    return yt.grad.numpy()


def chain_on_the_cpu(model, y, W, decoder_dtype):
    """The device's chain on the CPU: the oracle's forward rounded to fp32, oracle/torch_oracle.TorchSMPL at `decoder_dtype`
    with autograd, its dx rounded to fp32, the oracle's backward rounded to fp32."""
    from oracle.torch_oracle import TorchSMPL
    x = torch.tensor(o.forward(y)[0].astype(np.float32).astype(np.float64), dtype=decoder_dtype, requires_grad=True)
    (torch.tensor(W, dtype=decoder_dtype) * TorchSMPL(model, decoder_dtype)(x)).sum().backward()
    dx = x.grad.numpy().astype(np.float32)
    return o.backward(y, dx).astype(np.float32)


CHAIN_TOL = 4 * 8.22e-8


def chain_deviation(dy, want):
    """The worst of a row's pose block and its shape block, each max |dy - want| over max |want|."""
    dy, want = np.asarray(dy, np.float64), np.asarray(want, np.float64)
    dev = [np.abs(dy[:, c] - want[:, c]).max(1) / np.abs(want[:, c]).max(1) for c in (slice(4, 148), slice(148, 158))]
    return float(np.max(dev))


def test_chain_into_the_smpl_layer_against_float64_from_matrices(smpl_model):
    """The bar is 4 x the worst deviation the same chain shows on the CPU in float64 (`chain_on_the_cpu`: the oracle for the
    head, rounded to fp32 at its output, at the gradient into it and at dy, around oracle/torch_oracle.TorchSMPL in float64):
    8.22e-8, the same on every host, so 3.29e-7.  Seen on an MI355X: 3.1e-7.  Printed beside it: that CPU run again, and the
    one with TorchSMPL in fp32 (6e-7 to 2e-6 by the host's threads), neither of which the assertion uses."""
    from ilps_amd.keras_smpl.batch_smpl import SMPLLayer
    y = _chain_inputs()
    W = np.random.default_rng(22).normal(size=(4, smpl_model.v_template.shape[0], 3))
    want = chain_reference(smpl_model, y, W)
    cpu64 = chain_deviation(chain_on_the_cpu(smpl_model, y, W, torch.float64), want)
    cpu32 = chain_deviation(chain_on_the_cpu(smpl_model, y, W, torch.float32), want)
    print("chain on the CPU: deviation %.3g with the decoder in float64, %.3g in fp32" % (cpu64, cpu32))
    yt = t(y).requires_grad_(True)
    x, status = params_from_rot6d(yt, return_status=True)
    (t(W) * SMPLLayer(smpl_model)(x)).sum().backward()
    assert status.cpu().tolist() == [0] * 4
    dev = chain_deviation(yt.grad.cpu().numpy(), want)
    print("chain: deviation %.3g of %.3g" % (dev, CHAIN_TOL))
    assert (yt.grad[:, :4] == 0).all() and dev <= CHAIN_TOL


# ---- a regressor in 6D space -----------------------------------------------------------------------------------------------

def test_regressor_in_6d_space_takes_a_step_of_each_trainer(smpl_model):
    """ENet + IEF, 256 x 256 images (the ENet branch takes nothing else) -> 64 x 64 label maps, B = 2."""
    from ilps_amd import synthetic as syn
    from ilps_amd.keras_smpl.batch_smpl import SMPLLayer
    from ilps_amd.keypoints import KeypointSpec
    from ilps_amd.training import SegTrainer, SupervisedTrainer
    layer = SMPLLayer(smpl_model)
    bt = syn.SyntheticBatches(layer, 2, 256, 64, topology=syn.hull_topology(smpl_model), device=DEV, truth=True, seed=3,
                              spec=KeypointSpec.from_model(layer, "cocoplus"), sampler=syn.BodySampler(layer, fill=(0.5, 0.8)))
    images, labels, _, truth = next(bt)
    for cls, kw, args in ((SupervisedTrainer, dict(spec=KeypointSpec.smpl_joints(), root=0), (None, None, truth)),
                          (SegTrainer, {}, (labels,))):
        torch.manual_seed(0)
        tr = cls(smpl_model, output_wh=64, encoder_architecture="enet", use_IEF=True, device=DEV, in_channels=bt.in_channels,
                 pose_repr="rot6d", **kw)
        tr.smpl_model.train()
        assert tr.smpl_model.IEF_layer_3.out_features == 158 and tr.smpl_model.pose_status is None
        loss = tr.step(images, *args)
        assert torch.isfinite(loss) and all(p.grad is not None for p in tr.smpl_model.parameters())
        assert all(torch.isfinite(p.grad).all() for p in tr.smpl_model.parameters())
        st = tr.smpl_model.pose_status
        assert st.is_cuda and st.shape == (2,) and st.dtype == torch.int32 and (st == 0).all()
        assert float(tr.smpl_model.IEF_layer_3.weight.grad.abs().sum()) > 0
        with torch.no_grad():
            assert tr.smpl_model.eval()(images).shape == (2, 86)
