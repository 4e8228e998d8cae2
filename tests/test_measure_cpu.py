"""Mesh measurements without a GPU: the oracle (tests/_measure_oracle.py) pinned on the generated spheres and checked
against finite differences and the homogeneity identities; the package's CPU path (`measure.mesh_measures` on CPU tensors)
against the oracle; `MeasureSpec` validation, `planes_through`, `joint_planes`, `evaluation.evaluate_measurements` on a stub
model, and the C launchers' and torch ops' argument handling (no launch)."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ilps_amd  # noqa: E402,F401
from ilps_amd import measure  # noqa: E402
from ilps_amd.measure import MeasureSpec, joint_planes, mesh_measures, planes_through  # noqa: E402
from ilps_amd.render import MeshTopology  # noqa: E402
import _measure_oracle as orc  # noqa: E402
from _render_oracle import soup, uv_sphere  # noqa: E402


def _rel(a, b):
    return abs(a - b) / abs(b)


def test_oracle_on_the_smpl_sized_sphere():
    v, f = uv_sphere()
    assert v.shape == (6890, 3) and f.shape == (13776, 3)
    ring40 = v[1 + 40 * 84, 1]
    m = orc.measures(v, f, planes=[[0, 1, 0, 0], [0, 1, 0, ring40], [1, 2, 3, 0.5]])
    assert _rel(m["volume"], 4.18338653889078) < 1e-12
    assert _rel(m["area"], 12.558263515555925) < 1e-12
    assert _rel(m["girth"][0], 6.280595724661316) < 1e-12 and m["counted"][0] == 168
    # the plane through ring 40 touches 84 vertices (d = 0 counts as above): the same cut, half its faces zero-length
    assert _rel(m["girth"][1], 6.280595724661316) < 1e-12 and m["counted"][1] == 168 and m["zero_len"][1] == 84
    assert _rel(m["girth"][2], 6.2247655666491735) < 1e-12 and m["counted"][2] == 322
    # pole to pole exactly 2; 82 rings put none on the equator, so x and z fall short by 1 - sin(41 pi / 83)
    np.testing.assert_allclose(m["extent"], [2 * np.sin(41 * np.pi / 83), 2, 2 * np.sin(41 * np.pi / 83)], rtol=0, atol=1e-15)
    assert list(m["ext_idx"][[1, 4]]) == [6889, 0]


def test_oracle_on_the_small_sphere():
    v, f = uv_sphere(8, 5)
    assert v.shape == (42, 3) and f.shape == (80, 3)
    m = orc.measures(v, f, planes=[[0, 1, 0, 0], [0, 1, 0, v[9, 1]]])
    assert _rel(m["volume"], 3.5186112450195792) < 1e-12
    assert _rel(m["area"], 11.525753893285291) < 1e-12
    assert _rel(m["girth"][0], 6.122934917841436) < 1e-12 and m["counted"][0] == 16
    assert _rel(m["girth"][1], 5.302617184569468) < 1e-12 and m["counted"][1] == 16
    assert m["volume_T"] >= abs(m["volume"]) and m["area_T"] == m["area"]


PLANE = np.array([0.3, 1.0, -0.2, 0.137])            # touches no vertex of the 42-vertex sphere


def test_oracle_gradient_against_central_differences():
    v, f = uv_sphere(8, 5)
    assert np.abs(orc.plane_dist(v, PLANE)).min() > 1e-3
    gv, ga, ge, gg = 0.7, -1.3, np.array([0.5, -0.25, 2.0]), np.array([1.1])
    g = orc.grads(v, f, planes=[PLANE], g_volume=gv, g_area=ga, g_extent=ge, g_girth=gg)

    def total(vv, pl):
        m = orc.measures(vv, f, planes=[pl])
        return gv * m["volume"] + ga * m["area"] + ge @ m["extent"] + gg @ m["girth"]
    h = 1e-6
    rng = np.random.default_rng(0)
    picks = [(0, 1), (41, 1), (9, 0)] + [(int(i), int(c)) for i, c in zip(rng.integers(0, 42, 12), rng.integers(0, 3, 12))]
    for i, c in picks:
        vp, vm = v.copy(), v.copy()
        vp[i, c] += h
        vm[i, c] -= h
        fd = (total(vp, PLANE) - total(vm, PLANE)) / (2 * h)
        assert abs(fd - g["dverts"][i, c]) < 1e-7 * max(1.0, abs(fd)), (i, c, fd, g["dverts"][i, c])
    for c in range(4):
        pp, pm = PLANE.copy(), PLANE.copy()
        pp[c] += h
        pm[c] -= h
        fd = (orc.measures(v, f, planes=[pp])["girth"][0] - orc.measures(v, f, planes=[pm])["girth"][0]) / (2 * h)
        assert abs(fd - g["dgirth_dplane"][0, c]) < 1e-7 * max(1.0, abs(fd))


def homogeneity(v, vol, area, girth, o, dvol, darea, dgirth, dgdp, planes):
    """The four identities as residuals relative to the quantities: volume is homogeneous of degree 3 in the vertices, area
    of degree 2, a girth of degree 1 in (vertices, o), and of degree 0 in the plane (n, o)."""
    v = np.asarray(v, np.float64)
    return (abs((v * dvol).sum() - 3 * vol) / abs(vol), abs((v * darea).sum() - 2 * area) / area,
            abs((v * dgirth).sum() + o * dgdp[3] - girth) / girth,
            abs(planes[:3] @ dgdp[:3] + o * dgdp[3]) / girth)


def test_oracle_gradient_homogeneity():
    v, f = uv_sphere(8, 5)
    m = orc.measures(v, f, planes=[PLANE])
    gvol = orc.grads(v, f, g_volume=1.0)["dverts"]
    gar = orc.grads(v, f, g_area=1.0)["dverts"]
    gg = orc.grads(v, f, planes=[PLANE], g_girth=[1.0])
    res = homogeneity(v, m["volume"], m["area"], m["girth"][0], PLANE[3], gvol, gar, gg["dverts"], gg["dgirth_dplane"][0], PLANE)
    assert max(res) < 1e-13, res


def _case(seed, B, kind):
    if kind == "sphere42":
        v, f = uv_sphere(8, 5)
        rng = np.random.default_rng(seed)
        verts = np.stack([v * rng.uniform(0.6, 1.2, 3) + rng.uniform(-0.2, 0.2, 3) for _ in range(B)]).astype(np.float32)
        fp = (np.arange(len(f)) % 5).astype(np.uint8)
    else:
        v, f = soup(seed)
        rng = np.random.default_rng(seed + 1)
        verts = np.stack([v * rng.uniform(0.6, 1.2, 3) for _ in range(B)]).astype(np.float32)
        fp = rng.integers(0, 32, len(f)).astype(np.uint8)
    return verts, f, fp


@pytest.mark.parametrize("kind,B,per_mesh", [("sphere42", 3, False), ("sphere42", 2, True), ("soup", 2, True)])
def test_cpu_path_matches_the_oracle(kind, B, per_mesh):
    verts, f, fp = _case(11, B, kind)
    V = verts.shape[1]
    rng = np.random.default_rng(5)
    K = 3
    planes = np.concatenate([rng.normal(size=(B, K, 3)), rng.uniform(-0.2, 0.2, (B, K, 1))], -1).astype(np.float32)
    planes[:, 1] = [0, 1, 0, 5.0]                                  # misses the mesh
    if not per_mesh:
        planes = planes[0]
    masks = [0xFFFFFFFF, 0xFFFFFFFF, 0b10110]
    topo = MeshTopology(f, V, face_part=fp)
    spec = MeasureSpec(topo, planes=None if per_mesh else planes, part_mask=masks)
    tv = torch.from_numpy(verts).requires_grad_(True)
    tp = torch.from_numpy(planes).requires_grad_(True)
    out = mesh_measures(tv, spec, planes=tp)
    assert out["status"].tolist() == [0] * B and out["volume"].dtype == torch.float32 and out["girth"].shape == (B, K)
    gv, ga = rng.normal(size=B), rng.normal(size=B)
    ge, gg = rng.normal(size=(B, 3)), rng.normal(size=(B, K))
    (out["volume"] @ torch.from_numpy(gv).float() + out["area"] @ torch.from_numpy(ga).float()
     + (out["extent"] * torch.from_numpy(ge).float()).sum() + (out["girth"] * torch.from_numpy(gg).float()).sum()).backward()
    gvf, gaf, gef, ggf = (np.asarray(a, np.float32).astype(np.float64) for a in (gv, ga, ge, gg))
    dplanes = np.zeros(planes.shape)
    for b in range(B):
        pb = planes[b] if per_mesh else planes
        m = orc.measures(verts[b], f, fp, pb, masks)
        # float64 arithmetic in another order than the oracle's, then one rounding to fp32
        for key, T in (("volume", m["volume_T"]), ("area", m["area_T"]), ("girth", m["girth_T"])):
            ok, worst = orc.within(out[key][b].detach().numpy(), m[key], T, absT=2.0 ** -40)
            assert ok, (key, b, worst)
        np.testing.assert_array_equal(out["extent"][b].detach().numpy(), m["extent"].astype(np.float32))
        np.testing.assert_array_equal(out["ext_idx"][b].numpy(), m["ext_idx"])
        assert m["girth"][1] == 0 and m["counted"][0] > 0
        g = orc.grads(verts[b], f, fp, pb, masks, gvf[b], gaf[b], gef[b], ggf[b])
        np.testing.assert_allclose(tv.grad[b].numpy(), g["dverts"], rtol=1e-5, atol=1e-6 * np.abs(g["dverts_T"]).max())
        if per_mesh:
            dplanes[b] = ggf[b][:, None] * g["dgirth_dplane"]
        else:
            dplanes += ggf[b][:, None] * g["dgirth_dplane"]
    np.testing.assert_allclose(tp.grad.numpy(), dplanes, rtol=1e-4, atol=1e-5 * np.abs(dplanes).max())


def test_cpu_path_edge_cases():
    v, f = uv_sphere(8, 5)
    topo = MeshTopology(f, 42)
    verts = torch.from_numpy(np.stack([v, v * 0.5, v + 1]).astype(np.float32))
    # K = 0
    out = mesh_measures(verts, MeasureSpec(topo))
    assert out["girth"].shape == (3, 0) and out["status"].tolist() == [0, 0, 0]
    # a plane through the vertices of ring 1 (d = 0 is above), and the null normal: nothing is cut
    spec = MeasureSpec(topo, planes=[[0, 1, 0, float(np.float32(v[9, 1]))], [0, 0, 0, 0.1], [0, 0, 0, -0.1]])
    out = mesh_measures(verts[:1], spec)
    m = orc.measures(verts[0].numpy(), f, planes=spec.planes.numpy())
    assert m["counted"].tolist() == [16, 0, 0] and m["zero_len"][0] == 8
    assert orc.within(out["girth"][0].numpy(), m["girth"], m["girth_T"])[0] and out["girth"][0, 1:].tolist() == [0, 0]
    # a NaN in mesh 1: its outputs and gradient rows NaN, the others bit-equal to the clean batch
    clean = mesh_measures(verts, spec)
    hurt = verts.clone()
    hurt[1, 17, 2] = float("nan")
    hurt.requires_grad_(True)
    out = mesh_measures(hurt, spec)
    assert out["status"].tolist() == [0, measure.NONFINITE, 0] and out["ext_idx"][1].tolist() == [-1] * 6
    (out["volume"].sum() + out["girth"].sum()).backward()
    for k in ("volume", "area", "extent", "girth"):
        assert torch.isnan(out[k][1]).all()
        assert torch.equal(out[k][[0, 2]], clean[k][[0, 2]])
    assert torch.isnan(hurt.grad[1]).all() and torch.isfinite(hurt.grad[[0, 2]]).all()
    # all-degenerate faces: area 0, finite (zero) gradients
    deg = MeshTopology(np.array([[0, 0, 1], [2, 3, 3], [4, 4, 4], [5, 6, 7]], np.int32), 8)
    line = torch.arange(8, dtype=torch.float32)[:, None] * torch.tensor([[1.0, 2.0, -1.0]])    # collinear vertices
    x = line[None].clone().requires_grad_(True)
    out = mesh_measures(x, MeasureSpec(deg, planes=[[1, 0, 0, 2.5]]))
    (out["area"].sum() + out["girth"].sum() + out["volume"].sum()).backward()
    assert out["area"].item() == 0 and out["girth"].item() == 0 and torch.isfinite(x.grad).all()


def test_spec_validation():
    v, f = uv_sphere(8, 5)
    topo = MeshTopology(f, 42)
    with pytest.raises(TypeError, match="MeshTopology"):
        MeasureSpec(f)
    with pytest.raises(ValueError, match=r"\(K, 4\)"):
        MeasureSpec(topo, planes=np.zeros((2, 3)))
    with pytest.raises(ValueError, match="at most 16"):
        MeasureSpec(topo, planes=np.zeros((17, 4)))
    with pytest.raises(ValueError, match="2\\^32"):
        MeasureSpec(topo, planes=np.zeros((1, 4)), part_mask=[1 << 32])
    with pytest.raises(ValueError, match="2\\^32"):
        MeasureSpec(topo, planes=np.zeros((1, 4)), part_mask=[-1])
    with pytest.raises(ValueError, match="disagree"):
        MeasureSpec(topo, planes=np.zeros((2, 4)), part_mask=[1])
    with pytest.raises(ValueError, match="disagree"):
        MeasureSpec(topo, planes=np.zeros((2, 4)), names=["chest"])
    with pytest.raises(ValueError, match="integers"):
        MeasureSpec(topo, part_mask=[0.5])
    spec = MeasureSpec(topo, planes=np.zeros((16, 4)), part_mask=[0xFFFFFFFF] * 16)
    assert spec.num_planes == 16 and spec.on("cpu")["part_mask"].dtype == torch.int32 and spec.on("cpu")["part_mask"][0] == -1
    assert MeasureSpec(topo, part_mask=[3, 5]).num_planes == 2 and MeasureSpec(topo).num_planes == 0
    verts = torch.zeros(2, 42, 3)
    with pytest.raises(ValueError, match="vertices"):
        mesh_measures(torch.zeros(2, 41, 3), spec)
    with pytest.raises(ValueError, match="planes must be"):
        mesh_measures(verts, spec, planes=torch.zeros(3, 4))
    with pytest.raises(ValueError, match="planes must be"):
        mesh_measures(verts, spec, planes=torch.zeros(3, 16, 4))
    with pytest.raises(ValueError, match="pass planes"):
        mesh_measures(verts, MeasureSpec(topo, part_mask=[1]))
    with pytest.raises(ValueError, match=r"\(B, V, 3\)"):
        mesh_measures(torch.zeros(42, 3), spec)


def test_planes_through_and_joint_planes():
    rng = np.random.default_rng(2)
    p, n = torch.from_numpy(rng.normal(size=(3, 5, 3))), torch.from_numpy(rng.normal(size=(3, 5, 3)))
    pl = planes_through(p, n)
    assert pl.shape == (3, 5, 4) and torch.equal(pl[..., :3], n)
    d = (pl[..., :3] * p).sum(-1) - pl[..., 3]                  # the plane passes through its point
    assert d.abs().max() < 1e-15
    assert planes_through(p[0], n[0]).shape == (5, 4)
    with pytest.raises(ValueError):
        planes_through(p, n[:, :4])
    J = torch.from_numpy(rng.normal(size=(2, 24, 3))).requires_grad_(True)
    pl = joint_planes(J, anchors=[3, 0], along=[(3, 6), (0, 3)])
    assert pl.shape == (2, 2, 4)
    Jd = J.detach()
    assert torch.allclose(pl[:, 0, :3], Jd[:, 6] - Jd[:, 3]) and torch.allclose(pl[:, 1, :3], Jd[:, 3] - Jd[:, 0])
    assert torch.allclose(pl[:, 0, 3], ((Jd[:, 6] - Jd[:, 3]) * Jd[:, 3]).sum(-1))
    pl.sum().backward()
    assert J.grad is not None and J.grad[:, [0, 3, 6]].abs().min() > 0 and J.grad[:, 1].abs().max() == 0
    with pytest.raises(ValueError, match="one entry per plane"):
        joint_planes(Jd, [3], [(3, 6), (0, 3)])
    with pytest.raises(ValueError, match="lie in"):
        joint_planes(Jd, [24], [(3, 6)])
    with pytest.raises(ValueError, match="different"):
        joint_planes(Jd, [3], [(3, 3)])


class _StubRegressor(torch.nn.Module):
    def forward(self, images):
        return images


class _CpuLayer:
    """A CPU stand-in for SMPLLayer: the float64 NumPy oracle of the SMPL forward."""
    num_cam = 4

    def __init__(self, model):
        self.model = model

    def __call__(self, x):
        sys.path.insert(0, ROOT)
        from oracle import np_oracle as o
        return torch.from_numpy(o.smpl_layer_call(x.numpy().astype(np.float64), self.model).astype(np.float32))


def _params(n, seed):
    from ilps_amd.smpl_model import mean86
    rng = np.random.default_rng(seed)
    x = np.tile(mean86(48), (n, 1))
    x[:, 4:76] += rng.normal(0, 0.2, (n, 72))
    x[:, 76:] += rng.normal(0, 1.0, (n, 10))
    return torch.from_numpy(x.astype(np.float32))


def test_evaluate_measurements_on_a_stub_model():
    from ilps_amd.evaluation import evaluate_measurements
    from ilps_amd.smpl_model import synthetic_smpl_model
    model = synthetic_smpl_model(1234, num_verts=600)
    layer, reg = _CpuLayer(model), _StubRegressor()
    _, f = soup(3, n=200)                                     # any valid faces over the 600 vertices
    topo = MeshTopology(f, 600)
    spec = MeasureSpec(topo, planes=[[0, 1, 0, 0.0], [1, 0, 0, 0.05]], names=["a", "b"])
    xs, ys = [_params(2, 1), _params(3, 2)], [_params(2, 8), _params(3, 9)]
    # the prediction's own shape as ground truth: in the T-pose every error is zero, whatever the poses were
    res = evaluate_measurements(reg, layer, [(x, (y[:, 4:76], x[:, 76:86])) for x, y in zip(xs, ys)], spec)
    assert res["count"] == 5 and res["nonfinite"] == 0 and res["names"] == ["a", "b"]
    assert res["volume"] == 0 and res["area"] == 0 and res["extent"] == [0, 0, 0] and res["girth"] == [0, 0]
    # other shapes: the means of the per-body absolute differences, by hand
    res = evaluate_measurements(reg, layer, [(x, (y[:, 4:76], y[:, 76:86])) for x, y in zip(xs, ys)], spec)
    x, y = torch.cat(xs).clone(), torch.cat(ys).clone()
    x[:, 4:76] = 0
    y[:, 4:76] = 0
    mp, mg = mesh_measures(layer(x), spec), mesh_measures(layer(y), spec)
    assert abs(res["volume"] - float((mp["volume"] - mg["volume"]).abs().double().mean())) < 1e-12 and res["area"] > 0
    want = (mp["girth"] - mg["girth"]).abs().double().mean(0)
    assert all(abs(a - float(b)) < 1e-12 for a, b in zip(res["girth"], want)) and len(res["extent"]) == 3
    # with the poses kept the same shapes differ as well
    res2 = evaluate_measurements(reg, layer, [(x, (y[:, 4:76], x[:, 76:86])) for x, y in zip(xs, ys)], spec, tpose=False)
    assert res2["area"] > 0 and res2["count"] == 5
    # a NaN prediction is left out and counted
    bad = xs[0].clone()
    bad[1, 80] = float("nan")
    res = evaluate_measurements(reg, layer, [(bad, (ys[0][:, 4:76], ys[0][:, 76:86]))], spec)
    assert res["count"] == 1 and res["nonfinite"] == 1 and np.isfinite(res["volume"])
    with pytest.raises(ValueError, match="no batches"):
        evaluate_measurements(reg, layer, [], spec)
    with pytest.raises(ValueError, match="gt_pose"):
        evaluate_measurements(reg, layer, [(xs[0], (xs[0][:, 4:70], xs[0][:, 76:86]))], spec)


def test_launchers_refuse_bad_arguments_without_launching():
    from ilps_amd import _lib
    lib = _lib.load()
    one = 1                                            # (a non-null pointer value that is never dereferenced: no launch)
    fwd = lambda verts=one, K=3, B=2, V=42, F=80, vol=one: lib.smplr_mesh_measures(
        verts, one, one, one, 0, one, B, V, F, K, vol, one, one, one, one, None, one, None)
    bwd = lambda verts=one, K=3, B=2, V=42, F=80, dv=one: lib.smplr_mesh_measures_bwd(
        verts, one, one, one, 240, one, one, 0, one, one, one, None, None, None, one, B, V, F, K, dv, None)
    for fn, name in ((fwd, b"smplr_mesh_measures"), (bwd, b"smplr_mesh_measures_bwd")):
        assert fn(verts=None) == -1 and b"null" in lib.smplr_last_error() and name in lib.smplr_last_error()
        assert fn(K=17) == -1 and b"K=17" in lib.smplr_last_error()
        assert fn(K=-1) == -1
        assert fn(V=0) == -1 and b"V=0" in lib.smplr_last_error()
        assert fn(V=(1 << 24) + 1) == -1 and fn(F=(1 << 24) + 1) == -1 and fn(F=-1) == -1 and fn(B=-1) == -1
        assert fn(B=0, verts=None) == 0                 # an empty batch is a no-op
    assert fwd(vol=None) == -1 and b"null" in lib.smplr_last_error()
    assert bwd(dv=None) == -1 and b"null" in lib.smplr_last_error()
    # K > 0 needs the planes, the masks and the face parts
    assert lib.smplr_mesh_measures(one, one, None, one, 0, one, 2, 42, 80, 1, one, one, one, one, one, None, one, None) == -1
    assert lib.smplr_mesh_measures(one, one, one, one, 2, one, 2, 42, 80, 1, one, one, one, one, one, None, one, None) == -1
    assert b"plane_bstride" in lib.smplr_last_error()
    header = open(os.path.join(ROOT, "include", "smplraster.h")).read()
    assert "int smplr_mesh_measures(" in header and "int smplr_mesh_measures_bwd(" in header
    assert "#define SMPLR_ABI_VERSION 7" in header and "#define SMPLR_MM_NONFINITE 1" in header


def test_torch_ops_meta_shapes_and_cpu_refusal():
    from ilps_amd import torch_ops
    ns = torch_ops.load()
    for name in ("mesh_measures", "mesh_measures_bwd"):
        assert str(getattr(ns, name).default._schema) == torch_ops.SCHEMAS[name]
    m = lambda *s, dt=torch.float32: torch.empty(*s, dtype=dt, device="meta")
    i32, u8 = torch.int32, torch.uint8
    outs = ns.mesh_measures(m(5, 42, 3), m(80, 3, dt=i32), m(80, dt=u8), m(5, 3, 4), m(3, dt=i32))
    assert [tuple(o.shape) for o in outs] == [(5,), (5,), (5, 3), (5, 6), (5, 3), (5, 3, 4), (5,)]
    assert outs[3].dtype == i32 and outs[6].dtype == i32
    outs = ns.mesh_measures(m(5, 42, 3), m(80, 3, dt=i32), m(80, dt=u8), m(3, 4), m(3, dt=i32), False)
    assert tuple(outs[4].shape) == (5, 3) and outs[5].numel() == 0
    assert tuple(ns.mesh_measures(m(0, 42, 3), m(80, 3, dt=i32))[4].shape) == (0, 0)
    dv = ns.mesh_measures_bwd(m(5, 42, 3), m(80, 3, dt=i32), m(43, dt=i32), m(240, dt=i32), m(80, dt=u8), m(3, 4),
                              m(3, dt=i32), m(5, 6, dt=i32), m(5, dt=i32), None, m(5), None, m(5, 3))
    assert tuple(dv.shape) == (5, 42, 3)
    with pytest.raises(RuntimeError, match="16 planes"):
        ns.mesh_measures(m(5, 42, 3), m(80, 3, dt=i32), m(80, dt=u8), m(17, 4), m(17, dt=i32))
    with pytest.raises(RuntimeError, match="part_mask"):
        ns.mesh_measures(m(5, 42, 3), m(80, 3, dt=i32), m(80, dt=u8), m(3, 4), m(2, dt=i32))
    with pytest.raises(RuntimeError, match="g_girth"):
        ns.mesh_measures_bwd(m(5, 42, 3), m(80, 3, dt=i32), m(43, dt=i32), m(240, dt=i32), m(80, dt=u8), m(3, 4),
                             m(3, dt=i32), m(5, 6, dt=i32), m(5, dt=i32), None, None, None, m(5, 2))
    with pytest.raises((RuntimeError, NotImplementedError)):
        ns.mesh_measures(torch.zeros(1, 42, 3), torch.zeros(80, 3, dtype=i32))          # CPU tensors: no kernel registered
    with pytest.raises((RuntimeError, NotImplementedError)):
        ns.mesh_measures_bwd(torch.zeros(1, 42, 3), torch.zeros(80, 3, dtype=i32), torch.zeros(43, dtype=i32),
                             torch.zeros(240, dtype=i32), None, None, None, torch.zeros(1, 6, dtype=i32),
                             torch.zeros(1, dtype=i32), torch.zeros(1), None, None, None)


def test_kernels_fit_their_launch():
    """Registers, LDS and scratch from the built code object: no scratch, static LDS far below 64 KB, and the forward's 512
    lanes (eight waves, two per SIMD) fit a CU."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr
    ks = {n: k for n, k in kr.kernels().items() if "measure_" in n}
    assert len(ks) == 2
    for name, k in ks.items():
        assert k["scratch"] == 0, "%s spills %d B per lane" % (name, k["scratch"])
        assert k["lds"] <= 64 * 1024
        if "measure_fwd" in name:
            assert k["max_threads"] >= 512 and kr.waves_per_simd(k) >= 2
