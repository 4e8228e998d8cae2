"""The pose regimes' reference side, without a GPU: the generator emits what it says, the float64 oracles are finite
on every row, the float32 oracle's own error - the bar of tests/test_gpu_pose_regimes.py - stays under grad_close's
ceiling in every regime, and the float64 Rodrigues matrix is a rotation as far as the reference's formula lets it."""
import numpy as np
import torch

import _pose_regimes as pr


def test_generator_emits_the_regimes():
    x, rows = pr.regime_batch()
    x2, _ = pr.regime_batch()
    assert x.dtype == np.float32 and x.shape == (len(rows), 86) and np.array_equal(x, x2) and 65 <= len(rows) <= 80
    th = x[:, 4:76].reshape(-1, 24, 3).astype(np.float64)
    mags = dict(pr.MAGNITUDES)
    seen = set()
    for n, (label, kind) in enumerate(rows):
        seen.add((label, kind))
        norm = np.linalg.norm(th[n], axis=1)
        if kind == "all":
            assert np.allclose(norm, mags[label], rtol=2e-7, atol=0) and (mags[label] > 0 or not th[n].any())
        elif kind.startswith("joint"):
            j = int(kind[5:])
            assert np.isclose(norm[j], mags[label], rtol=2e-7, atol=0)
            assert (np.delete(norm, j) > 1e-2).all()                   # the others are make_x's
        elif kind.startswith("axis"):
            ax = "xyz".index(kind[-1])
            want = np.zeros((24, 3), np.float32)
            want[:, ax] = np.float32(mags[label]) * (1 if kind[4] == "+" else -1)
            assert np.array_equal(th[n], want)
        else:
            from ilps_amd.smpl_model import mean86
            assert kind == "tpose" and not th[n, 1:].any() and np.array_equal(th[n, 0], mean86(pr.W)[4:7].astype(np.float32))
    assert len(seen) == len(rows)
    for label, _ in pr.MAGNITUDES:
        assert {(label, "all")} | {(label, "joint%d" % j) for j in pr.SINGLE_JOINTS} <= seen
    assert len([1 for _, k in rows if k.startswith("axis")]) == 18
    assert mags["pi"] == float(np.float32(np.pi)) and mags["2pi"] == float(np.float32(2 * np.pi))
    assert not (x[:, 4:76].reshape(-1, 3) == np.float32(-1e-8)).all(axis=1).any()


def test_float64_oracles_are_finite_on_every_row(smpl_model):
    from oracle import np_oracle as o
    r = pr.reference(smpl_model)
    ref = o.smpl_layer_call(r["x"].astype(np.float64), smpl_model, return_all=True)
    assert all(np.isfinite(ref[k]).all() for k in ("verts", "J_transformed", "A", "Rs"))
    assert np.isfinite(r["d64"]).all() and np.isfinite(r["d32"]).all()
    assert np.isfinite(r["verts"]).all() and np.isfinite(r["J_transformed"]).all()
    # the two float64 oracles are one function written twice
    assert np.abs(ref["verts"] - r["verts"]).max() <= 1e-12 and np.abs(ref["J_transformed"] - r["J_transformed"]).max() <= 1e-12
    assert np.abs(ref["Rs"] - r["Rs"]).max() <= 1e-14
    assert np.all(r["d64"][:, :, :4] == 0) and np.abs(r["d64"][:, :, 4:]).max(axis=(0, 2)).min() > 0


def test_the_cap_never_decides(smpl_model):
    """4 x ref_err < 2e-3 for every regime and block, so each regime's bar is the float32 oracle's own error and not
    grad_close's ceiling.  (Measured: theta block 4e-7 .. 1.5e-6 except 9.5e-6 at 1e-5, 1.0e-4 at 1e-4, 4.6e-5 at
    1e-3; beta block 6e-7 .. 2.1e-6.  No magnitude of the issue's list had to be dropped.)"""
    r = pr.reference(smpl_model)
    for b in pr.BLOCKS:
        for reg in pr.REGIMES:
            e = r["ref_err"][b][reg]
            print("%-9s %-5s ref_err %.3e bar %.3e" % (reg, b, e, r["bar"][b][reg]))
            assert 0 < e and pr.FACTOR * e < pr.CAP, (reg, b, e)
            assert r["bar"][b][reg] == pr.FACTOR * e


def test_float64_rodrigues_is_a_rotation(smpl_model):
    """batch_rodrigues in float64 on every regime angle.  The reference's formula normalises theta by |theta + 1e-8|
    (batch_smpl.py:265-266), so its axis r has rho = |r|^2 = 1 + O(1e-8 / |theta|), not 1, and
        R R^T - I = (rho - 1) (sin^2 I + (1 - cos)^2 r r^T)
    exactly: up to 3e-8 at |theta| ~ pi, 3e-12 at 1e-4.  A plain `R R^T = I to 1e-12` is therefore false for the
    formula under test (it holds only for |theta| <= 1e-5 and at 0).  What is asserted to 1e-12 instead, on ALL angles:
    R R^T equals that closed form, det R equals the closed form's positive root, and where the defect's bound is below
    1e-13 the plain identity and det = 1."""
    from oracle import torch_oracle as to
    r = pr.reference(smpl_model)
    th = r["x"][:, 4:76].reshape(-1, 3).astype(np.float64)
    R = to.batch_rodrigues(torch.tensor(th)).numpy()
    angle = np.sqrt(((th + 1e-8) ** 2).sum(axis=1))
    ax = th / angle[:, None]
    rho = (ax * ax).sum(axis=1)
    s2, oc2 = np.sin(angle) ** 2, (1.0 - np.cos(angle)) ** 2
    eye = np.eye(3)
    defect = (rho - 1.0)[:, None, None] * (s2[:, None, None] * eye + oc2[:, None, None] * ax[:, :, None] * ax[:, None, :])
    RRt = R @ R.transpose(0, 2, 1)
    assert np.abs(RRt - eye - defect).max() <= 1e-12
    det = np.linalg.det(R)
    want = np.sqrt((1.0 + (rho - 1.0) * (s2 + oc2 * rho)) * (1.0 + (rho - 1.0) * s2) ** 2)
    assert np.abs(det - want).max() <= 1e-12 and (det > 0).all()
    small = np.abs(rho - 1.0) * np.maximum(s2, oc2 * rho) < 1e-13
    assert small.sum() >= 24 * 4                                     # magnitudes 0 .. 1e-5, T-pose joints
    assert np.abs(RRt - eye)[small].max() <= 1e-12 and np.abs(det[small] - 1.0).max() <= 1e-12
    # and the defect is the size the formula predicts, nothing larger hides in it
    assert np.abs(defect).max() <= 4e-8
