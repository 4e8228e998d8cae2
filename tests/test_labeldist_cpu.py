"""The label-map distance term without a GPU: `label_distance_torch` and the autograd Function on CPU tensors against the
numpy oracle (tests/_labeldist_oracle.py) - indices and status exactly, floats to the keypoint oracle's bar; finite
differences of the float64 restatement away from ties; the prep against a stable argsort; the frame convention on a map
with one labelled pixel; hostile rows; the spec, the argument errors and the C ABI (no launch); and the sign table of the
issue: where the focal loss's camera gradient points the wrong way, both directions of this term point the right way."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ilps_amd  # noqa: E402,F401
from ilps_amd.labeldist import (LabelDistanceSpec, LabelTargets, label_distance, label_distance_torch,  # noqa: E402
                                prep_torch, silhouette_labels)
import _labeldist_cases as cases  # noqa: E402
import _labeldist_oracle as orc  # noqa: E402

KEYS = ("e_m2i", "e_i2m", "near_pix", "near_vert", "d2_v", "d2_p", "proj", "status")


def tens(p, grad=False):
    verts, cam = torch.tensor(p["verts"]), torch.tensor(p["cam"])
    if grad:
        verts.requires_grad_(True)
        cam.requires_grad_(True)
    return (verts, cam, LabelDistanceSpec(p["vclass"], p["C"]), LabelTargets(torch.tensor(p["labels"]), p["C"]),
            None if p["vweight"] is None else torch.tensor(p["vweight"]))


def run_op(p, sigma, slack, g_seed=5):
    """The public op on CPU tensors, forward and backward under seeded cotangents -> (got dict, (dverts, dcam), g_v, g_p)."""
    verts, cam, spec, targets, vw = tens(p, grad=True)
    (e_v, e_p), det = label_distance(verts, cam, spec, targets, vw, sigma, slack, return_details=True)
    rng = np.random.default_rng(g_seed)
    g_v, g_p = rng.normal(size=tuple(e_v.shape)).astype(np.float32), rng.normal(size=tuple(e_p.shape)).astype(np.float32)
    torch.autograd.backward([e_v, e_p], [torch.tensor(g_v), torch.tensor(g_p)])       # (one backward: each gradient rounded once)
    got = dict(det, e_m2i=e_v.detach(), e_i2m=e_p.detach())
    return {k: v.numpy() for k, v in got.items()}, (verts.grad.numpy(), cam.grad.numpy()), g_v, g_p


@pytest.mark.parametrize("B,V,W,C", [(1, 1, 1, 2), (3, 65, 7, 2), (3, 257, 7, 32), (1, 600, 48, 32), (3, 600, 7, 32)])
@pytest.mark.parametrize("sigma,slack", [(None, 0.5), (3.0, 0.0)])
def test_cpu_path_matches_the_oracle(B, V, W, C, sigma, slack):
    p = cases.problem(B, V, W, C, seed=1)
    got, grads, g_v, g_p = run_op(p, sigma, slack)
    fw, gr = cases.reference(p, sigma, slack, g_v=g_v, g_p=g_p)
    worst = cases.compare(got, fw, gr, grads)
    print("worst error / bar: %.3g" % worst)
    # the float64 restatement itself, before any rounding to fp32
    verts, cam, spec, targets, vw = tens(p)
    o = label_distance_torch(verts, cam, spec, targets, vw, sigma, slack)
    cases.compare({k: o[k].numpy() for k in KEYS}, fw)


def test_exact_ties_occur_and_go_to_the_lower_index():
    p = cases.problem(3, 600, 7, 32, seed=1)
    fw, _ = cases.reference(p)
    assert sum(f["ties"][0] for f in fw) > 0 and sum(f["ties"][1] for f in fw) > 0
    verts, cam, spec, targets, vw = tens(p)
    _, det = label_distance(verts, cam, spec, targets, vw, return_details=True)
    pts = orc.points(7)
    for b, f in enumerate(fw):
        pr = f["proj"]
        for i in np.nonzero(f["near_pix"] >= 0)[0][:200]:                   # no lower pixel of the class is as close
            q = int(det["near_pix"][b, i])
            assert q == f["near_pix"][i]
            lab = p["labels"][b].reshape(-1)
            lower = np.nonzero(lab[:q] == p["vclass"][i])[0]
            d2 = ((pr[i] - pts[lower]) ** 2).sum(1)
            assert (d2 > f["d2_v"][i]).all()


def test_one_direction_and_no_weights():
    p = cases.problem(3, 65, 7, 2, seed=2, weights=False)
    verts, cam, spec, targets, _ = tens(p)
    fw, _ = cases.reference(p)
    for d in ("m2i", "i2m"):
        e, det = label_distance(verts, cam, spec, targets, directions=d, return_details=True)
        assert isinstance(e, torch.Tensor)
        other = {"m2i": ("near_vert", "d2_p"), "i2m": ("near_pix", "d2_v")}[d]
        assert all(det[k] is None for k in other)
        cases.compare(dict({k: (v.numpy() if v is not None else None) for k, v in det.items()}, **{"e_" + d: e.numpy()}), fw)


def test_finite_differences_away_from_ties():
    p = cases.problem(2, 65, 7, 32, seed=3, ties=False)
    fw, _ = cases.reference(p, 3.0, 0.5)
    assert min(f["margin"] for f in fw) > 1e-6
    d2 = np.concatenate([np.concatenate([f["d2_v"], f["d2_p"]]) for f in fw])
    assert np.abs(d2[np.isfinite(d2)] - 0.5).min() > 1e-4                   # (and no residual sits on the slack's kink)
    _, _, spec, targets, vw = tens(p)
    v0 = torch.tensor(p["verts"], dtype=torch.float64, requires_grad=True)
    c0 = torch.tensor(p["cam"], dtype=torch.float64, requires_grad=True)

    def f(v, c):
        o = label_distance_torch(v, c, spec, targets, vw, 3.0, 0.5)
        return torch.nan_to_num(o["e_m2i"]).sum(1), o["e_i2m"].sum((1, 2))
    assert torch.autograd.gradcheck(f, (v0, c0), eps=1e-6, atol=1e-6, rtol=1e-5)


def test_prep_is_a_stable_sort_by_class():
    p = cases.problem(3, 65, 48, 32, seed=4)
    off, pix = prep_torch(torch.tensor(p["labels"]), 32)
    for b in range(3):
        o, q = orc.prep(p["labels"][b], 32)
        assert np.array_equal(off[b].numpy(), o) and np.array_equal(pix[b].numpy(), q)
        lab = p["labels"][b].reshape(-1).astype(np.int64)
        key = np.where((lab >= 0) & (lab < 32), lab, 32)
        order = np.argsort(key, kind="stable")
        n = int((key < 32).sum())
        assert n < 48 * 48 and np.array_equal(q[:n], order[:n]) and (q[n:] == -1).all()


@pytest.mark.parametrize("flip", [True, False])
def test_frame_convention_one_labelled_pixel(flip):
    """Stored pixel (r, c) = (1, 3) of a 5 x 5 map sits at (3, 5 - 1 - 1) = (3, 3) of the projection frame, or at (3, 1)
    without flip_rows: a vertex projected exactly there is at distance 0, one a pixel to the right at distance 1."""
    labels = torch.zeros((1, 5, 5), dtype=torch.int64)
    labels[0, 1, 3] = 1
    point = (3.0, 3.0) if flip else (3.0, 1.0)
    verts = torch.tensor([[[point[0], point[1], 7.0], [point[0] + 1.0, point[1], -7.0]]])
    cam = torch.tensor([[1.0, 1.0, 0.0, 0.0]])
    spec, targets = LabelDistanceSpec.silhouette(2), LabelTargets(labels, 2, flip_rows=flip)
    (e_v, e_p), det = label_distance(verts, cam, spec, targets, slack=0.0, return_details=True)
    assert det["near_pix"].tolist() == [[8, 8]] and det["d2_v"].tolist() == [[0.0, 1.0]] and e_v.tolist() == [[0.0, 1.0]]
    assert int(det["near_vert"][0, 1, 3]) == 0 and float(det["d2_p"][0, 1, 3]) == 0.0
    assert int((det["near_vert"] >= 0).sum()) == 1 and float(e_p.sum()) == 0.0
    f = orc.forward(verts[0].numpy(), cam[0].numpy(), labels[0].numpy(), spec.vclass, 2, None, None, 0.0, flip)
    assert f["near_pix"].tolist() == [8, 8] and f["d2_v"].tolist() == [0.0, 1.0]


def test_hostile_rows_leave_their_neighbours_alone():
    p = cases.problem(3, 65, 7, 32, seed=6)
    clean, cgrads, g_v, g_p = run_op(p, 3.0, 0.5)
    counted = (p["vclass"] >= 1) & (p["vclass"] < 32) & (p["vweight"][1] > 0)
    i_c, i_u = int(np.nonzero(counted)[0][0]), int(np.nonzero(~counted)[0][0])

    def variant(edit):
        q = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in p.items()}
        edit(q)
        return q, run_op(q, 3.0, 0.5)

    def same(a, b, rows):
        for k in a[0]:
            assert np.array_equal(a[0][k][rows], b[0][k][rows], equal_nan=True), k
        for x, y in zip(a[1], b[1]):
            assert np.array_equal(x[rows], y[rows], equal_nan=True)
    for edit in (lambda q: q["verts"].__setitem__((1, i_c, 0), np.nan), lambda q: q["cam"].__setitem__((1, 3), np.inf)):
        q, r = variant(edit)
        got, grads = r[0], r[1]
        assert got["status"].tolist() == [0, 1, 0]
        assert (got["near_pix"][1] == -1).all() and (got["near_vert"][1] == -1).all()
        for k in ("e_m2i", "e_i2m", "d2_v", "d2_p", "proj"):
            assert np.isnan(got[k][1]).all(), k
        assert np.isnan(grads[0][1]).all() and np.isnan(grads[1][1]).all()
        same(r, (clean, cgrads), [0, 2])
        fw, gr = cases.reference(q, 3.0, 0.5, g_v=g_v, g_p=g_p)
        cases.compare(got, fw, gr, grads)
    # a NaN in a vertex that is not counted, and in Z, does nothing (but to that vertex's own proj)
    q, r = variant(lambda q: (q["verts"].__setitem__((1, i_u, 0), np.nan), q["verts"].__setitem__((1, i_c, 2), np.nan)))
    assert r[0]["status"].tolist() == [0, 0, 0]
    keep = np.ones(65, bool)
    keep[i_u] = False
    for k in ("e_m2i", "near_pix", "d2_v", "e_i2m", "near_vert", "d2_p"):
        assert np.array_equal(r[0][k], clean[k]), k
    assert np.array_equal(r[0]["proj"][:, keep], clean["proj"][:, keep]) and np.isnan(r[0]["proj"][1, i_u, 0])
    assert np.array_equal(r[1][0], cgrads[0]) and np.array_equal(r[1][1], cgrads[1])
    # a row whose vweight is all 0: zero outputs, zero gradients
    q, r = variant(lambda q: q["vweight"].__setitem__(1, 0.0))
    assert r[0]["status"].tolist() == [0, 0, 0]
    assert (r[0]["e_m2i"][1] == 0).all() and (r[0]["e_i2m"][1] == 0).all() and (r[0]["near_pix"][1] == -1).all()
    assert (r[0]["near_vert"][1] == -1).all() and (r[1][0][1] == 0).all() and (r[1][1][1] == 0).all()
    same(r, (clean, cgrads), [0, 2])


def test_spec_constructors_and_slot_order():
    from ilps_amd.render import vertex_parts
    from ilps_amd.smpl_model import load_part_tables
    tables = load_part_tables(1)
    spec = LabelDistanceSpec.from_parts(tables, 6890)
    assert spec.num_classes == 32 and np.array_equal(spec.vclass, vertex_parts(tables, 6890) + 1)
    assert sorted(spec.order[spec.order >= 0].tolist()) == list(range(6890))           # every vertex once
    tiles = spec.order[:len(spec.order) // 256 * 256].reshape(-1, 256)
    classed = [set(spec.vclass[t[t >= 0]].tolist()) for t in tiles]
    assert all(len(s) <= 1 for s in classed[:-1])                                       # a tile holds one class
    assert spec.voff[0] == spec.voff[1] == 0 and spec.voff[-1] == len(spec.vrun) == int((spec.vclass >= 1).sum())
    for c in range(1, 32):
        run = spec.vrun[spec.voff[c]:spec.voff[c + 1]]
        assert np.array_equal(run, np.nonzero(spec.vclass == c)[0])
    sil = LabelDistanceSpec.silhouette(10)
    assert sil.num_classes == 2 and (sil.vclass == 1).all()
    lab = torch.tensor([[[0, 5, 31], [32, 255, -1], [1, 0, 7]]])
    assert silhouette_labels(lab).tolist() == [[[0, 1, 1], [32, 255, -1], [1, 0, 1]]]


def test_argument_errors():
    p = cases.problem(2, 65, 7, 32, seed=7)
    verts, cam, spec, targets, vw = tens(p)
    with pytest.raises(ValueError, match="num_classes"):
        LabelDistanceSpec(p["vclass"], 33)
    with pytest.raises(ValueError, match="num_classes"):
        LabelTargets(torch.tensor(p["labels"]), 1)
    with pytest.raises(ValueError, match="integer"):
        LabelTargets(torch.zeros(2, 7, 7), 32)
    with pytest.raises(ValueError, match="W"):
        LabelTargets(torch.zeros(1, 161, 161, dtype=torch.int32), 32)
    with pytest.raises(TypeError):
        label_distance(verts, cam, None, targets)
    with pytest.raises(ValueError, match="vertices"):
        label_distance(verts[:, :64], cam, spec, targets)
    with pytest.raises(ValueError, match="rows"):
        label_distance(verts[:1], cam[:1], spec, targets)
    with pytest.raises(ValueError, match="classes"):
        label_distance(verts, cam, LabelDistanceSpec(np.ones(65, np.int32), 2), targets)
    with pytest.raises(RuntimeError, match="float32"):
        label_distance(verts.double(), cam, spec, targets)
    with pytest.raises(ValueError, match="vweight"):
        label_distance(verts, cam, spec, targets, vw[:, :3])
    with pytest.raises(ValueError, match="slack"):
        label_distance(verts, cam, spec, targets, slack=-1.0)
    with pytest.raises(ValueError, match="sigma"):
        label_distance(verts, cam, spec, targets, sigma=0.0)
    with pytest.raises(ValueError, match="directions"):
        label_distance(verts, cam, spec, targets, directions=("m2i", "up"))


def test_c_abi_refuses_bad_arguments_without_a_launch():
    from ilps_amd import _lib
    lib = _lib.load()
    assert lib.smplr_ld_prep(None, 0, 48, 32, None, None, None) == 0                   # B = 0: a no-op
    assert lib.smplr_ld_prep(None, 1, 161, 32, None, None, None) == -1 and b"smplr_ld_prep" in lib.smplr_last_error()
    assert lib.smplr_ld_prep(None, 1, 48, 33, None, None, None) == -1
    assert lib.smplr_ld_prep(None, 1, 48, 32, None, None, None) == -1 and b"null" in lib.smplr_last_error()
    n = (None,)
    assert lib.smplr_ld_fwd(*n * 10, 0, 6890, 48, 32, 7000, 6800, 1, 0.0, 0.5, *n * 9) == 0
    assert lib.smplr_ld_fwd(*n * 10, 1, 6890, 48, 32, 7000, 6800, 1, 0.0, 0.5, *n * 9) == -1
    assert b"smplr_ld_fwd" in lib.smplr_last_error()
    assert lib.smplr_ld_fwd(*n * 10, 1, 6890, 48, 32, 7000, 6800, 1, -1.0, 0.5, *n * 9) == -1 and b"sigma" in lib.smplr_last_error()
    assert lib.smplr_ld_fwd(*n * 10, 1, 6890, 48, 32, 7000, 6891, 1, 0.0, 0.5, *n * 9) == -1 and b"nrun" in lib.smplr_last_error()
    assert lib.smplr_ld_bwd(*n * 12, 0, 6890, 48, 32, 7000, 1, 0.0, 0.5, *n * 4) == 0
    assert lib.smplr_ld_bwd(*n * 12, 1, 6890, 48, 32, 7000, 1, 0.0, float("inf"), *n * 4) == -1 and b"slack" in lib.smplr_last_error()
    assert lib.smplr_ld_bwd(*n * 12, 1, 6890, 48, 32, 7000, 1, 0.0, 0.5, *n * 4) == -1 and b"smplr_ld_bwd" in lib.smplr_last_error()


def test_evaluate_label_distance_by_hand():
    from ilps_amd.evaluation import evaluate_label_distance
    p = cases.problem(3, 65, 7, 32, seed=8)
    p["cam"][1, 0] = np.nan
    verts, cam, spec, targets, vw = tens(p)
    _, det = label_distance(verts, cam, spec, targets, vw, return_details=True)
    r = evaluate_label_distance(det, targets)
    assert r["nonfinite_rows"] == 1
    for d, key in (("m2i", "d2_v"), ("i2m", "d2_p")):
        d2 = det[key][[0, 2]].double().reshape(-1)
        dist = d2[torch.isfinite(d2)].sqrt().numpy()
        assert r[d]["count"] == len(dist) > 0
        assert r[d]["mean_px"] == pytest.approx(dist.mean()) and r[d]["median_px"] == pytest.approx(np.median(dist))
        assert r[d]["within_1px"] == pytest.approx((dist <= 1.0).mean())


def test_sign_table_both_directions_point_home_where_the_focal_loss_does_not():
    """The issue's table, restated through the float64 oracle: the synthetic model at x* = make_x(1, 48, seed=0), mask all
    ones, labels = arg-max of the scores at x*; x* shifted by -16 .. +16 px along u0 or v0.  d(mean e)/d(that column) of
    either direction (sigma None, slack 0: plain squared distances) has the sign of the shift in all twelve cases; the focal
    loss (gamma 5, mean over the pixels) is printed beside it - at +-16 px it points the wrong way in three of four."""
    from _inputs import make_x
    from ilps_amd.smpl_model import load_part_tables, synthetic_smpl_model
    from oracle import torch_oracle as T
    W = 48
    model = synthetic_smpl_model(1234)
    ids, off = load_part_tables(1)
    x = torch.tensor(make_x(1, W, seed=0), dtype=torch.float64)
    verts = T.TorchSMPL(model)(x).detach()
    ones = torch.ones((1, verts.shape[1]), dtype=torch.float64)
    seg = T.projects_to_seg(T.orthographic_project(verts, x), ones, W, ids, off)
    labels = seg.argmax(-1)
    onehot = torch.nn.functional.one_hot(labels.reshape(1, -1), 32).to(torch.float64)
    spec, targets = LabelDistanceSpec.from_parts((ids, off), verts.shape[1]), LabelTargets(labels, 32)
    wrong_focal = 0
    for col in (2, 3):
        for shift in (-16, -8, -4, 4, 8, 16):
            xs = x.clone()
            xs[0, col] += shift
            cam = xs[:, :4].clone().requires_grad_(True)
            xc = torch.cat([cam, xs[:, 4:]], 1)
            focal = T.softmax_focal_loss(T.projects_to_seg(T.orthographic_project(verts, xc), ones, W, ids, off), onehot, 5.0).mean()
            (gf,) = torch.autograd.grad(focal, cam)
            o = label_distance_torch(verts, cam, spec, targets, None, None, 0.0)
            (gm,) = torch.autograd.grad(o["e_m2i"].mean(), cam, retain_graph=True)
            (gi,) = torch.autograd.grad(o["e_i2m"].mean(), cam)
            print("col %d shift %+3d px: focal %+.2e  m2i %+.3f  i2m %+.5f" % (col, shift, gf[0, col], gm[0, col], gi[0, col]))
            assert np.sign(float(gm[0, col])) == np.sign(shift) and np.sign(float(gi[0, col])) == np.sign(shift)
            wrong_focal += np.sign(float(gf[0, col])) != np.sign(shift)
    print("focal loss: wrong sign in %d of 12" % wrong_focal)
