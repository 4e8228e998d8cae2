"""csrc/supervised.hip on the device against the float64 oracle (tests/_supervised_oracle.py) under the package's rounding
bar |got - want| <= 2^-24 |want| + 2^-28 T: small shapes around every size at which the kernels take another path (the
forward's pass of 1 024 lanes x 4 floats = 1 365.33 vertices, the backward's workgroup of 1 024 vertices), the packing cases of
test_keypoints_cpu.regressor, strided x through torch.ops.smplraster, exact zeros, a further full turn, reproducibility, a
row alone and inside a batch, hostile rows, the refusals, the chain through `SMPLLayer` and `UncertaintyWeights`, and
`SyntheticBatches(truth=True)`."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _supervised_oracle as orc  # noqa: E402
from test_keypoints_cpu import check_bar  # noqa: E402
from test_supervised_cpu import (check_abi_refusals, full_turn_problem, oracle_rows, poison, problem, spec_of,  # noqa: E402
                                 tensors)
from ilps_amd.keypoints import KeypointSpec  # noqa: E402
from ilps_amd.supervised import UncertaintyWeights, supervised_terms, supervised_terms_torch  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
BWD_V = 1024                      # vertices a backward workgroup takes (SUP_BV)
FWD_V = (1365, 1366)              # one forward pass covers 4 096 floats: 1 365 vertices and a third


def t(a, dtype=torch.float32):
    return torch.as_tensor(np.asarray(a), dtype=dtype).to(DEV)


def bits(a):
    return a.detach().contiguous().view(torch.int32)


def rows_of(p, rows):
    per_row = ("x", "x_t", "verts", "verts_t", "jtr", "jtr_t", "row_w", "g")
    return {k: (v[rows] if k in per_row and v is not None else v) for k, v in p.items()}


def run(p, root, g=None, rows=None, use_row_w=True):
    """The op on the device for problem p (rows: a list of row indices, None = all) -> (terms, status, dverts, djtr, dx)."""
    q = p if rows is None else rows_of(p, rows)
    x, verts, jtr, truth, row_w, cam_scale = tensors(q, DEV, grad=g is not None)
    terms, status = supervised_terms(x, verts, jtr, truth, spec_of(p), root, row_w if use_row_w else None,
                                     cam_scale if p["num_cam"] else None, p["num_cam"], return_status=True)
    if g is None:
        return terms, status, None, None, None
    terms.backward(t(g if rows is None else g[rows]))
    torch.cuda.synchronize()
    return terms.detach(), status, verts.grad, None if jtr is None else jtr.grad, x.grad


def check_against_oracle(p, root, out, g, use_row_w=True):
    terms, status, dverts, djtr, dx = (None if o is None else o.cpu().numpy() for o in out)
    B, V, nc = len(p["x"]), p["V"], p["num_cam"]
    assert status.tolist() == [0] * B
    for b, (fw, gr) in enumerate(oracle_rows(p, root, use_row_w, g)):
        assert fw["status"] == 0
        check_bar(terms[b], fw["terms"], fw["T_terms"], "terms")
        check_bar(dverts[b], gr["dverts"], gr["T_dverts"], "dverts")
        check_bar(dx[b], gr["dx"], gr["T_dx"], "dx")
        if djtr is not None:
            check_bar(djtr[b], gr["djtr"], gr["T_djtr"], "djtr")
        on = fw["on"]
        assert (terms[b][~on] == 0).all()
        # exact zeros: dx columns nothing feeds, dverts rows no joint uses when term 0 gives nothing
        for term, cols in ((4, slice(0, nc)), (2, slice(nc, nc + 72)), (3, slice(nc + 72, nc + 82))):
            if not on[term] or g[b, term] == 0:
                assert (dx[b, cols].view(np.int32) << 1 == 0).all()
        assert (dx[b, nc + 82:] == 0).all()
        if not on[0] or g[b, 0] == 0:
            used = (p["R"][:, :V] != 0).any(0) if on[1] else np.zeros(V, bool)
            assert (dverts[b][~used].view(np.int32) << 1 == 0).all()
            assert not used.any() or g[b, 1] == 0 or root >= 0 or (dverts[b][used] != 0).any()


# ---- values and gradients --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K", [0, 1, 5, 64])
@pytest.mark.parametrize("V", [1, 65, 300, BWD_V - 1, BWD_V, BWD_V + 1, FWD_V[0], FWD_V[1]])
@pytest.mark.parametrize("B", [1, 3])
def test_small_shapes_against_the_oracle(B, V, K):
    for with_joints in ((False, True) if K else (False,)):
        for root, num_cam in ((-1, 4), (0, 0), (K - 1, 4)) if K else ((-1, 4), (-1, 0)):
            p = poison(problem(B, V, K, with_joints, seed=B + V + K, num_cam=num_cam))
            if K >= 3:                                           # the rows the packing must get right
                spec = spec_of(p)
                assert spec.off[1] == spec.off[0] and spec.off[2] - spec.off[1] == 1 and spec.off[3] - spec.off[2] == V
                assert spec.t_off[V // 2 + 1] - spec.t_off[V // 2] == K - 1
            g = p["g"].copy()
            g[B - 1, 0] = 0.0                                    # (the last row: term 0 gives no gradient)
            check_against_oracle(p, root, run(p, root, g), g)
            if root == -1:                                       # ... and with every term counted
                q = problem(B, V, K, with_joints, seed=B + V + K + 1, num_cam=num_cam, zero_w=False)
                check_against_oracle(q, root, run(q, root, g, use_row_w=False), g, use_row_w=False)


@pytest.mark.parametrize("with_joints", [False, True])
def test_strided_x_through_the_torch_ops(with_joints):
    """x rows 93 floats apart for 86 columns, through torch.ops.smplraster.sup_fwd / sup_bwd: the same numbers as the
    oracle's, every pad column of dx an exact zero, and the bits of the autograd path on a strided view."""
    from ilps_amd import torch_ops
    ns = torch_ops.load()
    B, V, K, C, root = 3, 300, 5, 93, 2
    p = problem(B, V, K, with_joints, seed=11, cols=C)
    spec = spec_of(p)
    d = spec.on(DEV)
    x, verts, jtr, truth, row_w, cam_scale = tensors(p, DEV)
    terms, status, ws = ns.sup_fwd(x, truth["x"], verts, truth["verts"], jtr, truth["J_transformed"] if with_joints else None,
                                   d["off"], d["idx"], d["w"], K, root, row_w, cam_scale)
    dverts, djtr, dx = ns.sup_bwd(x, truth["x"], verts, truth["verts"], d["t_off"], d["t_joint"], d["t_w"], K, root, row_w,
                                  cam_scale, status, ws, t(p["g"]), with_joints)
    assert dx.shape == (B, C) and djtr.shape == ((B, 24, 3) if with_joints else (0, 24, 3))
    check_against_oracle(p, root, (terms, status, dverts, djtr if with_joints else None, dx), p["g"])
    xv = x.clone().requires_grad_(True)
    vv, jv = verts.clone().requires_grad_(True), None if jtr is None else jtr.clone().requires_grad_(True)
    tr = {"x": truth["x"][:, :86], "verts": truth["verts"], "J_transformed": truth["J_transformed"]}
    t2, s2 = supervised_terms(xv[:, :86], vv, jv, tr, spec, root, row_w, cam_scale, return_status=True)
    t2.backward(t(p["g"]))
    assert torch.equal(bits(t2), bits(terms)) and torch.equal(bits(vv.grad), bits(dverts))
    assert torch.equal(bits(xv.grad[:, :86]), bits(dx[:, :86])) and (xv.grad[:, 86:] == 0).all()
    if with_joints:
        assert torch.equal(bits(jv.grad), bits(djtr))


def test_full_size_with_the_model_specs_and_the_device_restatement(smpl_model):
    """V = 6 890, B = 2: the cocoplus spec and the 24 posed joints, against the oracle; `supervised_terms_torch` in fp32 on
    the device (what tools/supervised_time.py times the kernels against) lands within fp32 rounding of the same numbers."""
    for spec, root in ((KeypointSpec.from_model(smpl_model), 0), (KeypointSpec.smpl_joints(), 3)):
        p = problem(2, 6890, 0, spec.with_joints, seed=8)
        p.update(R=spec.dense(), K=spec.K)
        out = run(p, root, p["g"])
        check_against_oracle(p, root, out, p["g"])
        x, verts, jtr, truth, row_w, cam_scale = tensors(p, DEV)
        ref = supervised_terms_torch(x, verts, jtr, truth, spec, root, row_w, cam_scale)
        np.testing.assert_allclose(ref.cpu().numpy(), out[0].cpu().numpy(), rtol=2e-4, atol=1e-9)


# ---- properties ------------------------------------------------------------------------------------------------------------

def test_rotation_matrices_do_not_see_a_further_full_turn():
    p = full_turn_problem()
    terms, status, *_ = run(p, -1, use_row_w=False)
    fw = orc.forward(None, p["x"][0], p["x_t"][0], p["verts"][0], p["verts_t"][0], cam_scale=p["cam_scale"])
    got = float(terms[0, 2])
    print("T2 = %.3g, bar around 0 = %.3g" % (got, 2.0 ** -28 * fw["T_terms"][2]))
    assert int(status[0]) == 0 and 0.0 <= got <= 2.0 ** -28 * fw["T_terms"][2]
    assert ((p["x"][0, 4:76] - p["x_t"][0, 4:76]) ** 2).mean() > 10.0
    check_bar(terms[0].cpu().numpy(), fw["terms"], fw["T_terms"], "terms")


@pytest.fixture(scope="module")
def batch_case():
    """B = 5, V = 1 366 (two backward workgroups, a forward tail), K = 64 with joint sources, root 63."""
    return problem(5, FWD_V[1], 64, True, seed=21), 63


def test_launches_repeat_and_a_row_does_not_see_its_batch(batch_case):
    p, root = batch_case
    a, b = run(p, root, p["g"]), run(p, root, p["g"])
    for x, y in zip(a, b):
        assert torch.equal(bits(x), bits(y))
    for row in (0, 2, 4):
        alone = run(p, root, p["g"], rows=[row])
        for x, y in zip(a, alone):
            assert torch.equal(bits(x[row]), bits(y[0]))
    order = [3, 0, 4, 1, 2]                                       # any position
    c = run(p, root, p["g"], rows=order)
    for x, y in zip(a, c):
        assert torch.equal(bits(x[order]), bits(y))


def test_a_zero_weight_hides_its_targets(batch_case):
    p, root = batch_case
    h = poison(p)
    assert sum(int(np.isnan(h[k]).sum() + np.isinf(h[k]).sum()) for k in ("x_t", "verts_t", "jtr_t")) > 0
    clean, hid = run(p, root, p["g"]), run(h, root, p["g"])
    assert hid[1].cpu().tolist() == [0] * 5
    for x, y in zip(clean, hid):
        assert torch.equal(bits(x), bits(y)) and torch.isfinite(y.float()).all()
    off = t(p["row_w"]) == 0
    assert off.any(1).all() and (bits(hid[0])[off] == 0).all()


def test_hostile_rows(batch_case):
    p, root = batch_case
    h = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in p.items()}
    h["row_w"][:] = 1.0
    clean = run(h, root, p["g"])
    h["verts"][0, 5, 1] = np.nan                                  # row 0: a predicted vertex
    h["x_t"][1, 4 + 30] = np.inf                                  # row 1: a true angle
    h["jtr_t"][3, [j for j in range(24) if p["R"][:, p["V"] + j].any()][0], 2] = np.nan      # row 3: a used true joint
    h["row_w"][4, 3] = np.inf                                     # row 4: an infinite weight
    out = run(h, root, p["g"])
    assert out[1].cpu().tolist() == [1, 1, 0, 1, 1]
    for b in (0, 1, 3, 4):
        for x in (out[0], out[2], out[3], out[4]):
            assert torch.isnan(x[b]).all()
    alone = run(h, root, p["g"], rows=[2])
    for x, y, z in zip(out, alone, clean):
        assert torch.equal(bits(x[2]), bits(y[0])) and torch.equal(bits(x[2]), bits(z[2]))


def test_refusals_launch_nothing_and_an_empty_batch_is_a_no_op():
    check_abi_refusals()
    p = problem(2, 9, 5, True, seed=1)
    x, verts, jtr, truth, row_w, cam_scale = tensors(rows_of(p, []), DEV, grad=True)
    terms, status = supervised_terms(x, verts, jtr, truth, spec_of(p), 0, row_w, cam_scale, return_status=True)
    assert terms.shape == (0, 5) and status.shape == (0,)
    terms.sum().backward()
    assert verts.grad.shape == (0, 9, 3) and x.grad.shape == (0, 86)
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match="HIP device"):
        supervised_terms(x.cpu(), verts.cpu(), jtr.cpu(), {k: v.cpu() for k, v in truth.items()}, spec_of(p))


# ---- the chain through SMPLLayer -------------------------------------------------------------------------------------------

def test_chain_through_the_smpl_layer_and_the_uncertainty_weights(smpl_model):
    """d loss / dx for x -> SMPLLayer -> supervised_terms -> UncertaintyWeights -> sum at V = 6 890, B = 2, against the float64
    chain (oracle/torch_oracle.TorchSMPL, float64 autograd of `supervised_terms_torch`), under the bars
    test_gpu_keypoints.py uses for its own chain through SMPLLayer (test_gpu_parity's `grad_close` per column block): it
    is the same SMPL backward."""
    from _inputs import make_x
    from oracle.torch_oracle import TorchSMPL
    from test_gpu_keypoints import mixed_spec
    from test_gpu_parity import grad_close
    from ilps_amd.keras_smpl.batch_smpl import SMPLLayer
    spec, root, B = mixed_spec(smpl_model), 8, 2
    layer = SMPLLayer(smpl_model)
    x, x_t = make_x(B, 48, seed=5), make_x(B, 48, seed=6)
    with torch.no_grad():
        vt, jt, _ = TorchSMPL(smpl_model)(torch.tensor(x_t, dtype=torch.float64), return_all=True)
    truth32 = {"x": torch.tensor(x_t), "verts": vt.to(torch.float32), "J_transformed": jt.to(torch.float32)}
    cam_scale = (0.05, 0.05, 0.02, 0.02)
    s = torch.tensor([0.1, -0.2, 0.3, 0.0, -0.1])
    uw64, uw = UncertaintyWeights().double(), UncertaintyWeights().to(DEV)
    with torch.no_grad():
        uw64.s.copy_(s)
        uw.s.copy_(s)
    xo = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    vo, jo, _ = TorchSMPL(smpl_model)(xo, return_all=True)
    to = supervised_terms_torch(xo, vo, jo, {k: v.double() for k, v in truth32.items()}, spec, root, None, cam_scale)
    uw64(to).sum().backward()
    xg = t(x).requires_grad_(True)
    verts = layer(xg)
    terms, status = supervised_terms(xg, verts, layer.J_transformed, {k: v.to(DEV) for k, v in truth32.items()}, spec, root, None,
                                     cam_scale, return_status=True)
    uw(terms).sum().backward()
    assert status.cpu().tolist() == [0] * B and (to[:, :4] > 0).all()
    np.testing.assert_allclose(terms.detach().cpu().numpy(), to.detach().numpy(), rtol=2e-3, atol=1e-6)
    got, want = xg.grad.cpu().numpy(), xo.grad.numpy()
    grad_close(got[:, :4], want[:, :4], name="dcam")
    grad_close(got[:, 4:76], want[:, 4:76], name="dtheta")
    grad_close(got[:, 76:], want[:, 76:], name="dbeta")
    np.testing.assert_allclose(uw.s.grad.cpu().numpy(), uw64.s.grad.numpy(), rtol=2e-3, atol=1e-5)


# ---- batches that hand over their truth ------------------------------------------------------------------------------------

def test_synthetic_batches_hand_over_their_truth(smpl_model):
    from ilps_amd import synthetic as syn
    from ilps_amd.keras_smpl.batch_smpl import SMPLLayer
    layer = SMPLLayer(smpl_model)
    kw = dict(topology=syn.hull_topology(smpl_model), device=DEV, spec=KeypointSpec.from_model(layer, "cocoplus"),
              sampler=syn.BodySampler(layer, fill=(0.5, 0.8)), corruption={}, seed=5)
    with_truth = syn.SyntheticBatches(layer, 3, 32, 16, truth=True, **kw)
    plain, plain2 = syn.SyntheticBatches(layer, 3, 32, 16, **kw), syn.SyntheticBatches(layer, 3, 32, 16, truth=False, **kw)
    for _ in range(2):
        item, a, b = next(with_truth), next(plain), next(plain2)
        assert len(item) == 4 and item[2] is None and len(a) == 2 and len(b) == 2
        images, labels, _, truth = item
        assert set(truth) == {"x", "verts", "J_transformed", "joints"}
        last = with_truth.last
        for k in truth:                                           # the very tensors the sampler made
            assert truth[k] is last[k] and truth[k].data_ptr() == last[k].data_ptr()
        assert truth["x"].shape == (3, 86) and truth["verts"].shape == (3, 6890, 3) and truth["J_transformed"].shape == (3, 24, 3)
        assert not truth["verts"].requires_grad and truth["joints"].shape == (3, 19, 2)
        for u, v in zip(a, b):                                    # the same seed: the same draws, with or without truth
            assert torch.equal(u, v)
        assert torch.equal(images, a[0]) and torch.equal(labels, a[1])
    silh = syn.SyntheticBatches(layer, 2, 32, 16, truth=True, silh_wh=8, **kw)
    assert next(silh)[2].shape == (2, 8, 8)
    # the truth of a batch against itself: every term an exact zero
    terms = supervised_terms(truth["x"], truth["verts"], truth["J_transformed"], truth, KeypointSpec.smpl_joints(), 0)
    assert (terms == 0).all()
