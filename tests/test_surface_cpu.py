"""The dense surface-correspondence term without a GPU: the float64 torch restatement (`surface_energy_torch`, the CPU path of
`surface_energy`) against tests/_surface_oracle.py under its rounding bar, its autograd gradient against the oracle's closed
form, `SurfaceTargets`' packing, the vertex -> (face, corner) lists, and `pixel_barycentrics`.  Also the problems that
tests/test_gpu_surface.py runs on the device."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _surface_oracle as orc  # noqa: E402
from ilps_amd.render import MeshTopology  # noqa: E402
from ilps_amd.surface import (SurfaceTargets, pixel_barycentrics, surface_energy, surface_energy_torch,  # noqa: E402
                              vertex_corners)

TOPOLOGIES = ("tri", "v65", "v300")
CASES = ("random", "oneface", "perface", "corner")


def check_bar(got, want, T, what):
    ok, worst = orc.within(got, want, T)
    print("%s: worst error / bar = %.3g" % (what, worst))
    assert ok, "%s: error %.3g times the bar" % (what, worst)
    return worst


def topology(kind):
    """-> (faces (F, 3) int32, V).  "tri": one face.  "v65": 100 random faces over vertices 0 .. 59 (60 .. 64 are in no face),
    face 7 repeats a vertex.  "v300": 500 random faces."""
    rng = np.random.default_rng(len(kind))
    if kind == "tri":
        return np.array([[0, 1, 2]], np.int32), 3
    if kind == "v65":
        f = rng.integers(0, 60, (100, 3)).astype(np.int32)
        f[7] = (5, 5, 9)
        return f, 65
    return rng.integers(0, 300, (500, 3)).astype(np.int32), 300


def problem(B, kind, N, D, case="random", seed=0):
    """A seeded problem as float32 / int32 numpy: faces, V, verts (B, V, 3), cam (B, 4) or None, face (B, N), bary (B, N, 3),
    target (B, N, D), conf (B, N).  Weights are negative and non-normalised except in "corner" ((1, 0, 0)); "oneface" puts
    every correspondence on one face, "perface" one on each face (then padding); "random" scatters padding through the row.
    With B = 3 row 1 is all padding.  Entries with conf = 0 hold NaN targets; the targets of the rest lie on both sides of
    sigma = 3 of the model's points."""
    rng = np.random.default_rng(seed)
    faces, V = topology(kind)
    F = len(faces)
    verts = rng.normal(0, 1.0, (B, V, 3)).astype(np.float32)
    cam = None
    if D == 2:
        cam = np.stack([rng.uniform(8, 12, B), rng.uniform(8, 12, B), rng.uniform(20, 28, B), rng.uniform(20, 28, B)], 1).astype(np.float32)
    if case == "oneface":
        face = np.full((B, N), F // 2, np.int32)
    elif case == "perface":
        face = np.tile(np.where(np.arange(N) < F, np.arange(N), -1).astype(np.int32), (B, 1))
    else:
        face = rng.integers(0, F, (B, N)).astype(np.int32)
        if case == "random":
            face[rng.uniform(size=(B, N)) < 0.15] = -1
    if B == 3:
        face[1] = -1
    bary = rng.normal(0.3, 0.8, (B, N, 3)).astype(np.float32)
    if case == "corner":
        bary[:] = (1.0, 0.0, 0.0)
    conf = rng.uniform(0.2, 1.0, (B, N)).astype(np.float32)
    conf[rng.uniform(size=(B, N)) < 0.2] = 0.0
    P = (bary[..., None].astype(np.float64) * verts[np.arange(B)[:, None, None], faces[np.maximum(face, 0)]].astype(np.float64)).sum(2)
    if D == 2:
        P = np.stack([cam[:, 2, None] + cam[:, 0, None] * P[..., 0], cam[:, 3, None] + cam[:, 1, None] * P[..., 1]], -1)
    far = rng.uniform(size=(B, N, 1)) < 0.5
    off = np.where(far, rng.uniform(4.0, 9.0, (B, N, D)), rng.uniform(0.1, 1.5, (B, N, D))) * rng.choice([-1.0, 1.0], (B, N, D))
    target = (P + off).astype(np.float32)
    target[conf == 0] = np.nan
    return dict(faces=faces, V=V, verts=verts, cam=cam, face=face, bary=bary, target=target, conf=conf)


def take(p, rows):
    return {k: (v[rows] if isinstance(v, np.ndarray) and k != "faces" else v) for k, v in p.items()}


def tens(p, device, grad=False):
    """-> (verts, cam or None, SurfaceTargets) on `device`."""
    t = lambda a: torch.as_tensor(a).to(device)
    verts = t(p["verts"]).requires_grad_(grad)
    cam = None if p["cam"] is None else t(p["cam"]).requires_grad_(grad)
    topo = MeshTopology(p["faces"], p["V"])
    return verts, cam, SurfaceTargets(topo, t(p["face"]), t(p["bary"]), t(p["target"]), t(p["conf"]))


def oracle_row(p, b, sigma, g=None):
    fw = orc.forward(p["faces"], p["verts"][b], None if p["cam"] is None else p["cam"][b], p["face"][b], p["bary"][b],
                     p["target"][b], p["conf"][b], sigma)
    gr = None if g is None or fw["status"] else orc.grads(fw, None if p["cam"] is None else p["cam"][b], p["conf"][b], g[b], sigma)
    return fw, gr


# ---- the torch restatement against the oracle ----------------------------------------------------------------------------

@pytest.mark.parametrize("D", [2, 3])
@pytest.mark.parametrize("sigma", [None, 3.0])
def test_torch_restatement_and_its_gradient_against_the_oracle(D, sigma):
    for kind in TOPOLOGIES:
        for case in CASES:
            B, N = 3, 65
            p = problem(B, kind, N, D, case, seed=11)
            g = np.random.default_rng(5).normal(size=(B, N)).astype(np.float32)
            verts, cam, targets = tens(p, "cpu", grad=True)
            out = surface_energy_torch(verts, cam, targets, sigma)
            (out["e"] * torch.as_tensor(g, dtype=torch.float64)).sum().backward()
            e32, det = surface_energy(verts.detach(), None if cam is None else cam.detach(), targets, sigma, return_details=True)
            assert out["status"].tolist() == [0] * B and det["status"].tolist() == [0] * B
            for b in range(B):
                fw, gr = oracle_row(p, b, sigma, g)
                check_bar(out["e"][b].detach().numpy(), fw["e"], fw["T_e"], "e")
                check_bar(out["d2"][b].detach().numpy(), fw["d2"], fw["T_d2"], "d2")
                check_bar(out["point"][b].detach().numpy(), fw["point"], fw["T_point"], "point")
                check_bar(e32[b].numpy(), fw["e"], fw["T_e"], "e (fp32 op)")
                check_bar(verts.grad[b].numpy(), gr["dverts"], gr["T_dverts"], "dverts (autograd)")
                if D == 2:
                    check_bar(cam.grad[b].numpy(), gr["dcam"], gr["T_dcam"], "dcam (autograd)")
                assert (out["e"][b].detach().numpy()[~fw["counted"]] == 0).all()
            assert (out["e"][1] == 0).all() and (verts.grad[1] == 0).all()          # (the row that is all padding)


@pytest.mark.parametrize("D", [2, 3])
def test_cpu_op_backward_is_the_closed_form(D):
    p = problem(3, "v65", 63, D, "random", seed=2)
    g = np.random.default_rng(3).normal(size=(3, 63)).astype(np.float32)
    verts, cam, targets = tens(p, "cpu", grad=True)
    surface_energy(verts, cam, targets, 3.0).backward(torch.as_tensor(g))
    for b in range(3):
        _, gr = oracle_row(p, b, 3.0, g)
        check_bar(verts.grad[b].numpy(), gr["dverts"], gr["T_dverts"], "dverts")
        if D == 2:
            check_bar(cam.grad[b].numpy(), gr["dcam"], gr["T_dcam"], "dcam")
    unused = np.ones(65, bool)
    unused[p["faces"].reshape(-1)] = False
    assert unused.sum() >= 5 and (verts.grad[:, unused] == 0).all()


def test_hostile_rows_on_the_cpu_path():
    p = problem(4, "v65", 64, 2, "perface", seed=8)
    p["conf"][:, :4] = 1.0
    p["target"][:, :4] = 20.0
    p["conf"][:, 5] = 0.0
    p["verts"][0, p["faces"][0, 0], 1] = np.nan                  # row 0: a NaN vertex under a counted correspondence
    p["verts"][1, p["faces"][5, 0], 0] = np.nan                  # row 1: a NaN vertex ...
    lone = [n for n in range(64) if n != 5 and p["faces"][5, 0] in p["faces"][n]]
    p["conf"][1, lone] = 0.0                                     # ... that only uncounted correspondences use
    p["cam"][2, 3] = np.inf                                      # row 2: an Inf cam column
    verts, cam, targets = tens(p, "cpu", grad=True)
    e, det = surface_energy(verts, cam, targets, 3.0, return_details=True)
    e.backward(torch.ones_like(e))
    assert det["status"].tolist() == [1, 0, 1, 0]
    assert [orc.forward(p["faces"], p["verts"][b], p["cam"][b], p["face"][b], p["bary"][b], p["target"][b], p["conf"][b], 3.0)["status"]
            for b in range(4)] == [1, 0, 1, 0]
    for b in (0, 2):
        assert torch.isnan(e[b]).all() and torch.isnan(det["d2"][b]).all() and torch.isnan(verts.grad[b]).all() and torch.isnan(cam.grad[b]).all()
    for b in (1, 3):
        assert torch.isfinite(e[b]).all() and torch.isfinite(det["d2"][b]).all() and torch.isfinite(verts.grad[b]).all()


# ---- the packing ---------------------------------------------------------------------------------------------------------

def test_surface_targets_packing():
    p = problem(3, "v65", 257, 2, "random", seed=4)
    F = len(p["faces"])
    _, _, t = tens(p, "cpu")
    assert (t.B, t.N, t.D) == (3, 257, 2) and t.order.dtype == torch.int32 and t.c_off.dtype == torch.int32
    for b in range(3):
        face, order = p["face"][b], t.order[b].numpy()
        key = np.where(face >= 0, face, F)
        assert np.array_equal(order, np.argsort(key, kind="stable"))          # stable, padding last
        assert np.array_equal(t.s_face[b].numpy(), face[order]) and np.array_equal(t.s_conf[b].numpy(), p["conf"][b][order])
        assert np.array_equal(t.s_bary[b].numpy(), p["bary"][b][order])
        assert np.array_equal(t.s_target[b].numpy(), p["target"][b][order], equal_nan=True)
        on_mesh = int((face >= 0).sum())
        c_off = t.c_off[b].numpy()
        assert c_off[0] == 0 and c_off[F] == on_mesh and (np.diff(c_off) >= 0).all()
        assert np.array_equal(np.diff(c_off), np.bincount(face[face >= 0], minlength=F))
        assert (t.s_face[b].numpy()[on_mesh:] == -1).all()
        counted = int(((face >= 0) & (p["conf"][b] > 0)).sum())
        assert int(t.counted()[b].sum()) == counted and counted <= on_mesh      # (c_off counts the uncounted on the mesh too)
    assert int(t.c_off[1, F]) == 0                                              # the row that is all padding


def test_surface_targets_refusals():
    faces, V = topology("v65")
    topo = MeshTopology(faces, V)
    face = torch.zeros((2, 5), dtype=torch.int32)
    bary, target, conf = torch.zeros((2, 5, 3)), torch.zeros((2, 5, 2)), torch.ones((2, 5))
    SurfaceTargets(topo, face, bary, target, conf)
    SurfaceTargets(topo, face.long(), bary, torch.zeros((2, 5, 3)))             # (integer faces of any width; conf None: ones)
    with pytest.raises(ValueError, match="below F"):
        SurfaceTargets(topo, face + len(faces), bary, target, conf)
    with pytest.raises(ValueError, match="integer"):
        SurfaceTargets(topo, face.float(), bary, target, conf)
    with pytest.raises(ValueError, match="bary"):
        SurfaceTargets(topo, face, bary[:, :4], target, conf)
    with pytest.raises(ValueError, match="D = 2"):
        SurfaceTargets(topo, face, bary, torch.zeros((2, 5, 4)), conf)
    with pytest.raises(ValueError, match="conf"):
        SurfaceTargets(topo, face, bary, target, conf[:1])
    with pytest.raises(RuntimeError, match="float32"):
        SurfaceTargets(topo, face, bary.double(), target, conf)
    with pytest.raises(RuntimeError, match="float32"):
        SurfaceTargets(topo, face, bary, target.double(), conf)
    with pytest.raises(ValueError, match="correspondences per row"):
        SurfaceTargets(topo, face[:, :0], bary[:, :0], target[:, :0], conf[:, :0])
    with pytest.raises(TypeError):
        SurfaceTargets(faces, face, bary, target, conf)
    t = SurfaceTargets(topo, face, bary, target, conf)
    verts = torch.zeros((2, V, 3))
    with pytest.raises(ValueError, match="cam"):
        surface_energy(verts, None, t)                                          # image targets need a camera
    with pytest.raises(ValueError, match="rows"):
        surface_energy(verts[:1], torch.zeros((1, 4)), t)
    with pytest.raises(ValueError, match="vertices"):
        surface_energy(verts[:, :10], torch.zeros((2, 4)), t)
    with pytest.raises(ValueError, match="sigma"):
        surface_energy(verts, torch.zeros((2, 4)), t, sigma=-1.0)


def test_vertex_corner_lists_with_a_repeated_vertex_and_a_vertex_in_no_face():
    faces = np.array([[0, 1, 2], [2, 2, 3], [3, 0, 2], [4, 4, 4]], np.int32)    # vertex 5: in no face
    off, face, corner = vertex_corners(MeshTopology(faces, 6))
    assert off.tolist() == [0, 2, 3, 7, 9, 12, 12]
    pairs = [list(zip(face[off[i]:off[i + 1]].tolist(), corner[off[i]:off[i + 1]].tolist())) for i in range(6)]
    assert pairs == [[(0, 0), (2, 1)], [(0, 1)], [(0, 2), (1, 0), (1, 1), (2, 2)], [(1, 2), (2, 0)], [(3, 0), (3, 1), (3, 2)], []]
    f65, V = topology("v65")
    off, face, corner = vertex_corners(MeshTopology(f65, V))
    assert off[-1] == 300 and (np.diff(off)[60:] == 0).all()
    assert np.array_equal(f65[face, corner], np.repeat(np.arange(V), np.diff(off)))
    key = face.astype(np.int64) * 4 + corner
    for i in range(V):
        assert (np.diff(key[off[i]:off[i + 1]]) > 0).all()                      # faces increase, corners within a face
    k5 = list(zip(face[off[5]:off[6]].tolist(), corner[off[5]:off[6]].tolist()))
    assert (7, 0) in k5 and (7, 1) in k5


def test_pixel_barycentrics_reproduce_the_pixel_centre():
    verts = torch.tensor([[[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [1.0, 1.0, 0.5]],
                          [[0.1, 0.2, 0.0], [0.9, 0.1, 0.0], [0.2, 0.8, 0.0], [1.0, 1.1, 0.5]]])
    faces = np.array([[0, 1, 2], [1, 3, 2]], np.int32)
    cam = torch.tensor([[4.0, 4.0, 1.0, 1.0], [5.0, 3.0, 0.5, 1.5]])
    H, W = 6, 7
    fm = torch.full((2, H, W), -1, dtype=torch.int32)
    fm[0, 3, 2], fm[0, 4, 1], fm[0, 1, 4], fm[1, 2, 2], fm[1, 0, 5] = 0, 0, 1, 0, 1     # (a hand-made map: inside or not)
    bary, centre = pixel_barycentrics(verts, faces, cam, fm)
    assert bary.dtype == torch.float64 and tuple(bary.shape) == (2, H, W, 3)
    assert (bary[fm < 0] == 0).all()
    for b, r, j in ((0, 3, 2), (0, 4, 1), (0, 1, 4), (1, 2, 2), (1, 0, 5)):
        f = faces[int(fm[b, r, j])]
        c = cam[b].double().numpy()
        v = verts[b].double().numpy()
        p = np.stack([c[2] + c[0] * v[f, 0], c[3] + c[1] * v[f, 1]], 1)
        w = bary[b, r, j].numpy()
        assert abs(w.sum() - 1.0) <= 4 * np.finfo(np.float64).eps * np.abs(w).sum()
        got, want = w @ p, np.array([j, H - 1 - r], np.float64)
        assert np.array_equal(centre[b, r, j].numpy(), want)
        assert (np.abs(got - want) <= 16 * np.finfo(np.float64).eps * (np.abs(w) @ np.abs(p) + np.abs(want))).all(), (got, want)
    fm2 = torch.zeros((1, 2, 2), dtype=torch.int32)                             # a face without area: zeros, not NaN
    flat = torch.tensor([[[0.0, 0.0, 0.0], [1.0, 1.0, 0.0], [2.0, 2.0, 0.0]]])
    b2, _ = pixel_barycentrics(flat, np.array([[0, 1, 2]]), cam[:1], fm2)
    assert (b2 == 0).all()
