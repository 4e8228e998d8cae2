"""Mesh measurements on the GPU (csrc/measure.hip through `measure.mesh_measures` and `torch.ops.smplraster.mesh_measures*`)
against the float64 oracle of tests/_measure_oracle.py.

The rounding model behind the bars: the kernels take every product and sum in fp64 on the fp32 inputs and round each
output to fp32 once.  A sum of n <= 2^24 fp64 terms is off by at most n 2^-53 <= 2^-29 of T = sum |terms|, the rounding adds
2^-24 of the value: |got - ref| <= 2^-24 |ref| + 2^-28 T.  For a girth (and the gradients that go through a cut) this holds
where the cut is well conditioned: t = d_i / (d_i - d_j) loses what d_i - d_j cancels, so every case first asserts - on the
CPU, from the oracle alone - that c = max over cut edges of (|n| |v| + |o|) / |d_i - d_j| stays below 2^20.
A gradient component obeys the same bar with T = the sum of |per-face, per-term contributions| at that vertex.
"""
import functools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _measure_oracle as orc  # noqa: E402
from _inputs import make_x  # noqa: E402
from _render_oracle import posed_sphere, soup, uv_sphere  # noqa: E402

pytestmark = pytest.mark.gpu

ALL = 0xFFFFFFFF
COND_MAX = 2.0 ** 20


def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def t(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(dev())


# ---- cases ------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def mesh(kind, B):
    """-> verts (B, V, 3) float32, faces, face_part (uint8 or None: the topology's own rule)."""
    if kind == "sphere42":
        v, f = uv_sphere(8, 5)
        rng = np.random.default_rng(21)
        verts = np.stack([v @ np.linalg.qr(rng.normal(size=(3, 3)))[0] * rng.uniform(0.6, 1.2, 3) + rng.uniform(-0.2, 0.2, 3)
                          for _ in range(B)]).astype(np.float32)
        return verts, f, (np.arange(len(f)) % 5).astype(np.uint8)
    if kind == "posed":
        verts, f = posed_sphere(33, B)
        return verts, f, None
    v, f = soup(7)
    rng = np.random.default_rng(8)
    verts = np.stack([v * rng.uniform(0.6, 1.2, 3) for _ in range(B)]).astype(np.float32)
    return verts, f, rng.integers(0, 32, len(f)).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def topology(kind):
    from ilps_amd.render import MeshTopology
    verts, f, fp = mesh(kind, 1)
    return MeshTopology(f, verts.shape[1], face_part=fp)


@functools.lru_cache(maxsize=None)
def planes_for(kind, B, K, per_mesh):
    """(B, K, 4) or (K, 4) float32: plane 0 passes through a vertex (axis-aligned, so d = 0 there to the bit), plane 1
    misses the mesh, plane 2 has n = 0, the rest are random cuts near the middle."""
    verts = mesh(kind, B)[0]
    rng = np.random.default_rng(100 + K)
    out = np.zeros((B, K, 4), np.float32)
    for b in range(B if per_mesh else 1):
        for k in range(K):
            if k == 0:
                out[b, k] = [0, 1, 0, verts[b, 9 if kind == "sphere42" else 500, 1]]
            elif k == 1:
                out[b, k] = [0.5, 1, 0, 50.0]
            elif k == 2:
                out[b, k] = [0, 0, 0, 0.25 if b % 2 else -0.25]
            else:
                n = rng.normal(size=3)
                out[b, k] = [*(n * rng.uniform(0.5, 2.0)), rng.uniform(-0.15, 0.15)]
    return out if per_mesh else out[0]


def masks_for(K, subset):
    return tuple((0x5A5A5A5B >> (k % 3)) & ALL if subset else ALL for k in range(K))


@functools.lru_cache(maxsize=None)
def reference(kind, B, K, per_mesh, subset):
    verts = mesh(kind, B)[0]
    topo = topology(kind)
    pl = planes_for(kind, B, K, per_mesh)
    return [orc.measures(verts[b], topo.faces, topo.face_part, pl[b] if per_mesh else pl, masks_for(K, subset)) for b in range(B)]


def spec_for(kind, K, subset, planes=None):
    from ilps_amd.measure import MeasureSpec
    return MeasureSpec(topology(kind), planes=planes, part_mask=masks_for(K, subset))


def run(kind, B, K, per_mesh, subset, requires_grad=False):
    from ilps_amd.measure import mesh_measures
    verts = t(mesh(kind, B)[0]).requires_grad_(requires_grad)
    pl = planes_for(kind, B, K, per_mesh)
    if per_mesh:
        planes = t(pl).requires_grad_(requires_grad and K > 0)
        out = mesh_measures(verts, spec_for(kind, K, subset), planes=planes)
    else:
        planes = None
        out = mesh_measures(verts, spec_for(kind, K, subset, planes=pl))
    return out, verts, planes


def assert_conditioned(ref):
    for m in ref:
        assert (m["cond"] < COND_MAX).all(), "the case's cuts are ill conditioned: c = %s" % m["cond"]


def check_bar(got, want, T, what):
    ok, worst = orc.within(got, want, T)
    print("%s: worst error / bar = %.3g" % (what, worst))
    assert ok, "%s: error %.3g times the bar" % (what, worst)


VALUE_CASES = [("sphere42", B, K, False, False) for B in (1, 3, 7) for K in (0, 1, 3, 16)] + [
    ("sphere42", 3, 16, True, True), ("soup", 1, 1, False, False), ("soup", 7, 3, False, True), ("soup", 3, 16, True, True),
    ("posed", 7, 0, False, False), ("posed", 3, 3, True, True), ("posed", 1, 16, False, False)]


@pytest.mark.parametrize("kind,B,K,per_mesh,subset", VALUE_CASES)
def test_values_against_the_oracle(kind, B, K, per_mesh, subset):
    ref = reference(kind, B, K, per_mesh, subset)
    assert_conditioned(ref)
    if K >= 3:
        assert all(m["counted"][0] > 0 and m["counted"][1] == 0 and m["counted"][2] == 0 for m in ref)
        pl = planes_for(kind, B, K, per_mesh)                     # plane 0 passes through a vertex: d = 0 there, to the bit
        assert all((orc.plane_dist(mesh(kind, B)[0][b].astype(np.float64), (pl[b] if per_mesh else pl)[0].astype(np.float64)) == 0).any()
                   for b in range(B if per_mesh else 1))
    out, _, _ = run(kind, B, K, per_mesh, subset)
    torch.cuda.synchronize()
    assert out["girth"].shape == (B, K) and out["extent"].shape == (B, 3) and out["volume"].dtype == torch.float32
    assert out["status"].cpu().tolist() == [0] * B and out["status"].dtype == torch.int32
    np.testing.assert_array_equal(out["ext_idx"].cpu().numpy(), np.stack([m["ext_idx"] for m in ref]))
    for key in ("volume", "area", "girth"):
        check_bar(out[key].cpu().numpy(), np.stack([m[key] for m in ref]), np.stack([m[key + "_T"] for m in ref]), key)
    # an extent is one fp64 difference of two fp32 values, rounded once
    np.testing.assert_array_equal(out["extent"].cpu().numpy(), np.stack([m["extent"] for m in ref]).astype(np.float32))
    if K >= 3:
        assert (out["girth"][:, 1:3] == 0).all()


GRAD_CASES = [("sphere42", 3, 3, False, False), ("soup", 3, 16, True, True), ("posed", 3, 3, True, True)]
MODES = ("volume", "area", "extent", "girth", "all", "some")


@pytest.mark.parametrize("kind,B,K,per_mesh,subset", GRAD_CASES)
def test_gradients_against_the_oracle(kind, B, K, per_mesh, subset):
    """dverts for each cotangent alone, for all together (random weights) and with some absent; the plane gradient against
    the oracle's with unit cotangents (g_girth = 1: the multiply in torch is exact, so dplanes is dgirth_dplane itself)."""
    ref = reference(kind, B, K, per_mesh, subset)
    assert_conditioned(ref)
    topo, masks = topology(kind), masks_for(K, subset)
    vnp = mesh(kind, B)[0]
    pl = planes_for(kind, B, K, per_mesh)
    rng = np.random.default_rng(3)
    w = {"volume": rng.normal(size=B), "area": rng.normal(size=B), "extent": rng.normal(size=(B, 3)), "girth": rng.normal(size=(B, K))}
    w = {k: v.astype(np.float32) for k, v in w.items()}
    for mode in MODES:
        use = {"all": ("volume", "area", "extent", "girth"), "some": ("area", "girth")}.get(mode, (mode,))
        out, verts, planes = run(kind, B, K, per_mesh, subset, requires_grad=True)
        loss = sum((out[k] * (t(w[k]) if mode in ("all", "some") else 1.0)).sum() for k in use)
        loss.backward()
        got = verts.grad.cpu().numpy()
        for b in range(B):
            cot = {("g_" + k): ((w[k][b] if mode in ("all", "some") else np.ones_like(w[k][b])) if k in use else None) for k in w}
            g = orc.grads(vnp[b], topo.faces, topo.face_part, pl[b] if per_mesh else pl, masks, **cot)
            check_bar(got[b], g["dverts"], g["dverts_T"], "%s dverts[%d] (%s)" % (kind, b, mode))
            if mode == "girth" and per_mesh:
                check_bar(planes.grad[b].cpu().numpy(), g["dgirth_dplane"], g["dgirth_dplane_T"], "dplanes[%d]" % b)
        if mode in ("volume", "area", "extent") and planes is not None:
            assert planes.grad is None or (planes.grad == 0).all()


def test_shared_planes_gradient_sums_over_the_batch():
    from ilps_amd.measure import mesh_measures
    kind, B, K = "sphere42", 3, 3
    pl = planes_for(kind, B, K, False)
    verts, planes = t(mesh(kind, B)[0]), t(pl).requires_grad_(True)
    out = mesh_measures(verts, spec_for(kind, K, False), planes=planes)
    gg = t(np.random.default_rng(1).normal(size=(B, K)))
    (out["girth"] * gg).sum().backward()
    topo = topology(kind)
    want = sum(gg[b].cpu().numpy().astype(np.float64)[:, None]
               * orc.grads(mesh(kind, B)[0][b], topo.faces, topo.face_part, pl, masks_for(K, False))["dgirth_dplane"] for b in range(B))
    # fp32 products and an fp32 sum over the batch on top of the kernel's single rounding
    np.testing.assert_allclose(planes.grad.cpu().numpy(), want, rtol=1e-5, atol=1e-6 * np.abs(want).max())


@pytest.mark.parametrize("kind", ["sphere42", "posed"])
def test_homogeneity_identities_on_the_device(kind):
    """sum v . dvolume/dv = 3 volume, sum v . darea/dv = 2 area, sum v . dgirth/dv + o dgirth/do = girth and
    n . dgirth/dn + o dgirth/do = 0, on the fp32 results.  Every gradient entry and every value carries one fp32 rounding
    (2^-24 relative), so a residual is bounded by 2^-24 of the sum of |terms| on both sides; the bar allows twice that for
    the fp64 sums' own error and the 2^-28 T part of the value bar."""
    from ilps_amd.measure import mesh_measures
    B, K = 2, 4
    pl = planes_for(kind, B, K, True)[:, [0, 3]]                     # through a vertex, and a random cut
    spec = spec_for(kind, 2, False)
    v64 = mesh(kind, B)[0].astype(np.float64)
    res = {}
    for key, col in (("volume", None), ("area", None), ("girth", 0), ("girth", 1)):
        verts, planes = t(mesh(kind, B)[0]).requires_grad_(True), t(pl).requires_grad_(True)
        out = mesh_measures(verts, spec, planes=planes)
        val = out[key] if col is None else out[key][:, col]
        val.sum().backward()
        res[(key, col)] = (val.detach().cpu().numpy().astype(np.float64), verts.grad.cpu().numpy().astype(np.float64),
                           planes.grad.cpu().numpy().astype(np.float64))
    for b in range(B):
        for (key, col), deg in ((("volume", None), 3), (("area", None), 2)):
            val, dv, _ = res[(key, col)]
            terms = v64[b] * dv[b]
            assert abs(terms.sum() - deg * val[b]) <= 2.0 ** -23 * (np.abs(terms).sum() + deg * abs(val[b])), (key, b)
        for col in (0, 1):
            val, dv, dp = res[("girth", col)]
            p, g = pl[b, col].astype(np.float64), dp[b, col]
            terms = v64[b] * dv[b]
            assert val[b] > 0
            assert abs(terms.sum() + p[3] * g[3] - val[b]) <= 2.0 ** -23 * (np.abs(terms).sum() + abs(p[3] * g[3]) + val[b]), (col, b)
            assert abs(p[:3] @ g[:3] + p[3] * g[3]) <= 2.0 ** -23 * (np.abs(p[:3] * g[:3]).sum() + abs(p[3] * g[3])), (col, b)


def _all_outputs(kind, B, K, per_mesh, rows=None):
    """Values and gradients (random cotangents) of the case, or of its rows alone, as a list of CPU tensors."""
    from ilps_amd.measure import mesh_measures
    rows = list(range(B)) if rows is None else rows
    verts = t(mesh(kind, B)[0][rows]).requires_grad_(True)
    pl = planes_for(kind, B, K, per_mesh)
    planes = t(pl[rows] if per_mesh else pl).requires_grad_(True)
    out = mesh_measures(verts, spec_for(kind, K, True), planes=planes)
    rng = np.random.default_rng(9)
    w = {k: rng.normal(size=(B,) + tuple(out[k].shape[1:])).astype(np.float32)[rows] for k in ("volume", "area", "extent", "girth")}
    sum((out[k] * t(w[k])).sum() for k in w).backward()
    res = [out[k].detach().cpu() for k in ("volume", "area", "extent", "girth", "ext_idx", "status")] + [verts.grad.cpu()]
    return res + ([planes.grad.cpu()] if per_mesh else [])


@pytest.mark.parametrize("kind,K", [("posed", 3), ("soup", 16)])
def test_bits_do_not_depend_on_the_launch_or_the_batch(kind, K):
    B = 7
    a, b = _all_outputs(kind, B, K, True), _all_outputs(kind, B, K, True)
    for x, y in zip(a, b):
        assert torch.equal(x, y), "two launches differ"
    for r in range(B):
        for x, y in zip(a, _all_outputs(kind, B, K, True, rows=[r])):
            assert torch.equal(x[r:r + 1], y), "row %d alone differs from row %d of the batch" % (r, r)


def test_hostile_rows():
    from ilps_amd.measure import MeasureSpec, mesh_measures
    from ilps_amd.render import MeshTopology
    kind, B, K = "posed", 3, 3
    clean = _all_outputs(kind, B, K, True)
    vnp = mesh(kind, B)[0].copy()
    vnp[1, 4321, 2] = np.nan
    pl = planes_for(kind, B, K, True).copy()
    verts, planes = t(vnp).requires_grad_(True), t(pl).requires_grad_(True)
    out = mesh_measures(verts, spec_for(kind, K, True), planes=planes)
    rng = np.random.default_rng(9)
    w = {k: rng.normal(size=(B,) + tuple(out[k].shape[1:])).astype(np.float32) for k in ("volume", "area", "extent", "girth")}
    sum((out[k] * t(w[k])).sum() for k in w).backward()
    assert out["status"].cpu().tolist() == [0, 1, 0] and out["ext_idx"][1].cpu().tolist() == [-1] * 6
    got = [out[k].detach().cpu() for k in ("volume", "area", "extent", "girth", "ext_idx", "status")] + [verts.grad.cpu(), planes.grad.cpu()]
    for i, (x, y) in enumerate(zip(got, clean)):
        assert torch.equal(x[[0, 2]], y[[0, 2]]), "output %d of the clean rows changed" % i
        if x.dtype == torch.float32:
            assert torch.isnan(x[1]).all(), "output %d of the NaN row" % i
    # an infinite plane entry does the same to its mesh
    pl[2, 0, 3] = np.inf
    out = mesh_measures(t(mesh(kind, B)[0]), spec_for(kind, K, True), planes=t(pl))
    assert out["status"].cpu().tolist() == [0, 0, 1] and torch.isnan(out["girth"][2]).all() and torch.isnan(out["volume"][2])
    assert torch.equal(out["girth"][:2].cpu(), clean[3][:2])
    # all-degenerate faces (repeated corners, collinear vertices): area 0, no NaN, finite gradients
    deg = MeshTopology(np.array([[0, 0, 1], [2, 3, 3], [4, 4, 4], [5, 6, 7], [7, 6, 5]], np.int32), 8)
    line = torch.arange(8, dtype=torch.float32)[:, None] * torch.tensor([[1.0, 2.0, -1.0]])
    x = torch.stack([line, line * 0.5 + 1]).to(dev()).requires_grad_(True)
    out = mesh_measures(x, MeasureSpec(deg, planes=[[1, 0, 0, 2.5], [0, 1, 0, 11.0]]))
    (out["area"].sum() + out["girth"].sum() + out["volume"].sum() + out["extent"].sum()).backward()
    assert out["status"].cpu().tolist() == [0, 0] and (out["area"] == 0).all() and (out["girth"] == 0).all()
    assert torch.isfinite(x.grad).all() and all(torch.isfinite(out[k]).all() for k in ("volume", "extent"))
    ref = orc.grads(line.numpy(), deg.faces, None, None, None, g_volume=1.0, g_area=1.0, g_extent=np.ones(3))
    # (the collinear faces' volume terms cancel completely in exact arithmetic, so T is no scale here: the oracle's own
    # cross products, of coordinates up to 17, keep up to 17^2 2^-52 = 7e-14 where the exact answer is 0)
    np.testing.assert_allclose(x.grad[0].cpu().numpy(), ref["dverts"], rtol=2.0 ** -23, atol=1e-12)


def grad_close(a, b, rtol=2e-3, name="", elem_rtol=None, elem_atol=2e-4, per_column=True):
    """The metric of tests/test_gpu_parity.py (copied).  (1) max-norm: max|a-b| <= rtol * max|b|.  (2) element-wise:
    |a-b| <= elem_rtol*|b| + elem_atol*scale, scale = the RMS of the reference over the batch axis per trailing index."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, "%s: shapes %s vs %s" % (name, a.shape, b.shape)
    if b.size == 0:
        return
    scale = np.abs(b).max() + 1e-30
    err = np.abs(a - b).max() / scale
    assert err <= rtol, "%s: max|diff|/max|ref| = %.3e > %.1e" % (name, err, rtol)
    er = rtol if elem_rtol is None else elem_rtol
    col = np.sqrt(np.mean(b * b, axis=0, keepdims=True)) if (b.ndim >= 2 and per_column) else np.sqrt(np.mean(b * b))
    col = np.maximum(col, 1e-3 * np.sqrt(np.mean(b * b)) + 1e-30)
    bad = np.abs(a - b) > er * np.abs(b) + elem_atol * col
    assert not bad.any(), "%s: %d of %d entries outside |d| <= %.1e|ref| + %.1e*rms; worst %.3e vs ref %.3e" % (
        name, int(bad.sum()), b.size, er, elem_atol, float(np.abs(a - b)[bad].max()),
        float(np.abs(b)[bad][np.abs(a - b)[bad].argmax()]))


def test_chain_through_the_smpl_layer(smpl_model):
    """SMPLLayer (synthetic model) -> mesh_measures with the sphere's faces (any valid topology over 6 890 vertices):
    d(volume + sum girth)/dx against the float64 SMPL oracle chained with the measurement oracle."""
    from ilps_amd.keras_smpl.batch_smpl import SMPLLayer
    from ilps_amd.measure import MeasureSpec, mesh_measures
    from ilps_amd.render import MeshTopology
    from oracle.torch_oracle import TorchSMPL
    _, f = uv_sphere()
    topo = MeshTopology(f, 6890)
    pl = np.array([[0, 1, 0, 0.0], [1, 0, 0, 0.1], [0.3, 0.2, 1, 0.05]], np.float32)
    spec = MeasureSpec(topo, planes=pl)
    B = 4
    x = make_x(B, 48, seed=11)
    xo = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    vo, _, _ = TorchSMPL(smpl_model)(xo, return_all=True)
    total = 0.0
    sel = np.ones(len(f), bool)
    for b in range(B):
        corners = vo[b][torch.from_numpy(f.astype(np.int64))]
        total = total + (corners[:, 0] * torch.linalg.cross(corners[:, 1], corners[:, 2])).sum() / 6.0
        for k in range(3):
            total = total + orc._girth_corners(corners, torch.from_numpy(pl[k].astype(np.float64)), sel)
    total.backward()
    xg = t(x).requires_grad_(True)
    out = mesh_measures(SMPLLayer(smpl_model)(xg), spec)
    assert (out["girth"] > 0).all() and out["status"].cpu().tolist() == [0] * B
    (out["volume"].sum() + out["girth"].sum()).backward()
    got, want = xg.grad.cpu().numpy(), xo.grad.numpy()
    assert np.all(got[:, :4] == 0)
    grad_close(got[:, 4:76], want[:, 4:76], name="dtheta")
    grad_close(got[:, 76:], want[:, 76:], name="dbeta")


def test_torch_ops():
    from ilps_amd import torch_ops
    from ilps_amd.measure import mesh_measures
    ns = torch_ops.load()
    kind, B, K = "sphere42", 3, 3
    out, _, _ = run(kind, B, K, True, True)
    spec = spec_for(kind, K, True)
    d = spec.on(dev())
    verts, planes = t(mesh(kind, B)[0]), t(planes_for(kind, B, K, True))
    vol, area, ext, idx, girth, dgdp, status = ns.mesh_measures(verts, d["faces"], d["face_part"], planes, d["part_mask"])
    for a, b in ((vol, out["volume"]), (area, out["area"]), (ext, out["extent"]), (idx, out["ext_idx"]), (girth, out["girth"]),
                 (status, out["status"])):
        assert torch.equal(a, b)
    assert dgdp.shape == (B, K, 4) and ns.mesh_measures(verts, d["faces"], d["face_part"], planes, d["part_mask"], False)[5].numel() == 0
    gg = t(np.random.default_rng(2).normal(size=(B, K)))
    dv = ns.mesh_measures_bwd(verts, d["faces"], d["vf_off"], d["vf_face"], d["face_part"], planes, d["part_mask"], idx, status,
                              None, None, None, gg)
    v2 = verts.clone().requires_grad_(True)
    (mesh_measures(v2, spec, planes=planes)["girth"] * gg).sum().backward()
    assert torch.equal(dv, v2.grad)
    # K = 0 and B = 0
    o0 = ns.mesh_measures(verts, d["faces"])
    assert o0[4].shape == (B, 0) and torch.equal(o0[0], vol)
    assert ns.mesh_measures(verts[:0], d["faces"])[2].shape == (0, 3)
    # Meta shapes
    m = lambda *s, dt=torch.float32: torch.empty(*s, dtype=dt, device="meta")
    outs = ns.mesh_measures(m(5, 42, 3), m(80, 3, dt=torch.int32), m(80, dt=torch.uint8), m(5, 3, 4), m(3, dt=torch.int32))
    assert [tuple(o.shape) for o in outs] == [(5,), (5,), (5, 3), (5, 6), (5, 3), (5, 3, 4), (5,)]
    # refusals: CPU tensors, a CPU operand beside device ones, wrong dtypes
    with pytest.raises((RuntimeError, NotImplementedError)):
        ns.mesh_measures(verts.cpu(), d["faces"].cpu())
    with pytest.raises(RuntimeError):
        ns.mesh_measures(verts, d["faces"], d["face_part"], planes.cpu(), d["part_mask"])
    with pytest.raises(RuntimeError):
        ns.mesh_measures(verts.double(), d["faces"])
    with pytest.raises(RuntimeError):
        ns.mesh_measures_bwd(verts, d["faces"], d["vf_off"], d["vf_face"], d["face_part"], planes, d["part_mask"], idx, status,
                             None, None, None, gg.cpu())
    with pytest.raises(RuntimeError, match="planes"):
        mesh_measures(verts, spec, planes=planes.cpu())
