"""Scan distances without a GPU: the oracle (tests/_scan_oracle.py) pinned on hand-computed closest points of one triangle
(the seven Voronoi regions, a collinear triangle, a triangle of three equal corners); the package's CPU path
(`scan.surface_distance` on CPU tensors) against the oracle, hostile rows included; the envelope gradient against central
differences in float64; `sample_surface`; `evaluation.evaluate_scans` on a stub model; the C ABI of the three launchers and
their argument handling (no launch); the kernels' registers, LDS and scratch from the built code object."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ilps_amd  # noqa: E402,F401
from ilps_amd import scan  # noqa: E402
from ilps_amd.render import MeshTopology  # noqa: E402
from ilps_amd.scan import sample_surface, surface_distance  # noqa: E402
import _scan_oracle as orc  # noqa: E402
from _render_oracle import soup, uv_sphere  # noqa: E402

TRI = np.array([[0.0, 0, 0], [2, 0, 0], [0, 2, 0]])


@pytest.mark.parametrize("name, p, q, w, which", [
    ("interior", (0.5, 0.5, 1.0), (0.5, 0.5, 0), (0.5, 0.25, 0.25), 3),
    ("edge 01", (1.0, -1.0, 0.5), (1, 0, 0), (0.5, 0.5, 0), 0),
    ("edge 12", (2.0, 2.0, 0.0), (1, 1, 0), (0, 0.5, 0.5), 1),
    ("edge 20", (-1.0, 1.0, 0.0), (0, 1, 0), (0.5, 0, 0.5), 2),
    ("corner 0", (-1.0, -1.0, 0.0), (0, 0, 0), (1, 0, 0), 0),
    ("corner 1", (3.0, -0.5, 0.0), (2, 0, 0), (0, 1, 0), 0),
    ("corner 2", (-0.5, 3.0, 1.0), (0, 2, 0), (0, 0, 1), 1),
])
def test_oracle_on_the_seven_regions_of_one_triangle(name, p, q, w, which):
    r = orc.point_face(p, TRI)
    np.testing.assert_allclose(r["q"], q, rtol=0, atol=1e-15, err_msg=name)
    np.testing.assert_allclose(r["w"], w, rtol=0, atol=1e-15, err_msg=name)
    assert abs(r["d2"] - np.sum((np.asarray(p) - q) ** 2)) < 1e-15 and r["which"] == which
    # the same point under every relabelling of the corners: one q, the weights permuted with them
    for perm in ((1, 2, 0), (2, 0, 1), (0, 2, 1)):
        rp = orc.point_face(p, TRI[list(perm)])
        np.testing.assert_allclose(rp["q"], q, rtol=0, atol=1e-15)
        np.testing.assert_allclose(rp["w"], np.asarray(w)[list(perm)], rtol=0, atol=1e-15)


def test_oracle_on_degenerate_triangles():
    # three collinear corners: the segment from 0 to 3 on the x axis
    tri = np.array([[0.0, 0, 0], [1, 0, 0], [3, 0, 0]])
    r = orc.point_face((2.0, 1.0, 0.0), tri)
    np.testing.assert_allclose(r["q"], (2, 0, 0), rtol=0, atol=1e-15)
    assert abs(r["d2"] - 1) < 1e-15 and r["which"] == 1 and (r["w"] >= 0).all() and abs(r["w"].sum() - 1) < 1e-15
    np.testing.assert_allclose(r["w"] @ tri, (2, 0, 0), rtol=0, atol=1e-15)
    r = orc.point_face((-1.0, 0.0, 2.0), tri)                            # beyond the end
    np.testing.assert_allclose(r["q"], (0, 0, 0), rtol=0, atol=0)
    assert r["d2"] == 5.0
    # two equal corners: a segment
    r = orc.point_face((0.5, 1.0, 0.0), np.array([[0.0, 0, 0], [0, 0, 0], [1, 0, 0]]))
    np.testing.assert_allclose(r["q"], (0.5, 0, 0), rtol=0, atol=1e-15)
    # three equal corners: a point
    r = orc.point_face((1.0, 2.0, 5.0), np.array([[1.0, 2, 3]] * 3))
    assert r["d2"] == 4.0 and list(r["q"]) == [1, 2, 3] and list(r["w"]) == [1, 0, 0] and r["which"] == 0
    # on a corner to the bit: zero, not a rounding of it
    r = orc.point_face(TRI[1], TRI)
    assert r["d2"] == 0.0 and list(r["w"]) == [0, 1, 0]


def test_oracle_brute_force_and_ties():
    v, f = uv_sphere(8, 5)
    rng = np.random.default_rng(3)
    p = rng.normal(0, 1, (40, 3))
    M = orc.pair_d2(v, f, p)
    assert M.shape == (40, 80)
    # against an independent minimisation: projected gradient descent over the simplex is overkill - sample the triangle
    lam = rng.dirichlet(np.ones(3), 4000)
    for n in range(0, 40, 7):
        for fi in (0, 17, 79):
            d_samp = (((lam @ v[f[fi]]) - p[n]) ** 2).sum(1).min()
            assert M[n, fi] <= d_samp + 1e-12 and M[n, fi] > d_samp * 0.9 - 1e-3
    # a face listed twice: the lower index wins; a face naming a vertex outside the mesh is no candidate
    f2 = np.concatenate([f, f[:1], [[0, 1, 99]]])
    r1, r2 = orc.surface_distance(v, f, p), orc.surface_distance(v, f2, p)
    assert np.array_equal(r1["face"], r2["face"]) and np.array_equal(r1["d2"], r2["d2"])
    # a point listed twice: the lower index wins
    r3 = orc.surface_distance(v, f, np.concatenate([p, p]))
    assert r3["vpoint"].max() < 40 and np.array_equal(r3["vd2"], r1["vd2"])


def _mesh(kind, B):
    rng = np.random.default_rng(11)
    if kind == "sphere42":
        v, f = uv_sphere(8, 5)
    else:
        v, f = soup(5, n=60)
        v, f = v.astype(np.float64), f.copy()
        v[3 * 7 + 2] = v[3 * 7 + 1]                                      # a segment
        v[3 * 20: 3 * 20 + 3] = v[3 * 20]                                # a point
        v[3 * 31 + 2] = 0.25 * v[3 * 31] + 0.75 * v[3 * 31 + 1]          # collinear (up to the fp32 rounding below)
    verts = np.stack([v * rng.uniform(0.7, 1.2, 3) + rng.uniform(-0.2, 0.2, 3) for _ in range(B)]).astype(np.float32)
    return verts, np.asarray(f, np.int32)


def _cloud(verts, f, N, seed):
    """Points on the surface, near it, far outside, at a corner to the bit."""
    rng = np.random.default_rng(seed)
    B = verts.shape[0]
    out = np.empty((B, N, 3), np.float32)
    for b in range(B):
        fi = rng.integers(0, len(f), N)
        w = rng.dirichlet(np.ones(3), N)
        on = np.einsum("nk,nkc->nc", w, verts[b][f[fi]].astype(np.float64))
        kind = np.arange(N) % 4
        p = on + np.where(kind[:, None] == 1, rng.normal(0, 0.02, (N, 3)), 0) + np.where(kind[:, None] == 2, rng.normal(0, 3.0, (N, 3)), 0)
        p[kind == 3] = verts[b][f[fi, 0]][kind == 3]
        out[b] = p
    return out


@pytest.mark.parametrize("kind, B, N", [("sphere42", 1, 37), ("sphere42", 3, 64), ("soup", 2, 90)])
def test_cpu_path_matches_the_oracle(kind, B, N):
    verts, f = _mesh(kind, B)
    pts = _cloud(verts, f, N, 5)
    counts = np.array([N, N // 2, 0][:B], np.int32)
    topo = MeshTopology(f, verts.shape[1])
    out = surface_distance(torch.from_numpy(verts), topo, torch.from_numpy(pts), counts)
    assert out["d2"].dtype == torch.float32 and out["face"].dtype == torch.int32 and out["status"].dtype == torch.int32
    for b in range(B):
        ref = orc.surface_distance(verts[b], f, pts[b], counts[b])
        # the indices may differ from the oracle's on exact ties of rounded numbers only: compare distances first
        for k in ("d2", "vd2"):
            np.testing.assert_allclose(out[k][b].numpy(), ref[k], rtol=2.0 ** -23, atol=0, err_msg="%s mesh %d" % (k, b))
        same = out["face"][b].numpy() == ref["face"]
        assert same.mean() > 0.9
        np.testing.assert_allclose(out["resid"][b].numpy()[same], ref["resid"][same], rtol=0, atol=1e-6)
        np.testing.assert_allclose(out["bary"][b].numpy()[same], ref["bary"][same], rtol=0, atol=1e-5)
        assert (out["face"][b, counts[b]:] == -1).all() and (out["d2"][b, counts[b]:] == 0).all()
        if counts[b] == 0:
            assert torch.isinf(out["vd2"][b]).all() and (out["vpoint"][b] == -1).all()
    only = surface_distance(torch.from_numpy(verts), topo, torch.from_numpy(pts), counts, directions="m2p")
    assert sorted(only) == ["status", "vd2", "vpoint"] and torch.equal(only["vd2"], out["vd2"])
    only = surface_distance(torch.from_numpy(verts), topo, torch.from_numpy(pts), counts, directions=("p2m",))
    assert sorted(only) == ["bary", "d2", "face", "resid", "status"] and torch.equal(only["face"], out["face"])


def test_cpu_path_hostile_rows():
    verts, f = _mesh("sphere42", 3)
    pts = _cloud(verts, f, 20, 9)
    topo = MeshTopology(f, 42)
    clean = surface_distance(torch.from_numpy(verts), topo, torch.from_numpy(pts))
    bad_v = verts.copy()
    bad_v[1, 17, 2] = np.nan
    bad_p = pts.copy()
    bad_p[0, 3, 1] = np.inf
    bad_p[2, 0, 0] = np.nan
    V = torch.from_numpy(bad_v).requires_grad_(True)
    P = torch.from_numpy(bad_p).requires_grad_(True)
    out = surface_distance(V, topo, P)
    assert out["status"].tolist() == [0, scan.NONFINITE, 0]
    for k in ("d2", "bary", "resid", "vd2"):
        assert torch.isnan(out[k][1]).all(), k
    assert (out["face"][1] == -1).all() and (out["vpoint"][1] == -1).all()
    # a non-finite point: NaN / -1, no candidate of m2p; every other point as in the clean batch, bit for bit
    for b, n in ((0, 3), (2, 0)):
        assert torch.isnan(out["d2"][b, n]) and torch.isnan(out["bary"][b, n]).all() and torch.isnan(out["resid"][b, n]).all()
        assert out["face"][b, n] == -1 and (out["vpoint"][b] != n).all()
        keep = torch.arange(20) != n
        for k in ("d2", "face", "bary", "resid"):
            assert torch.equal(out[k][b][keep], clean[k][b][keep]), k
        ref = orc.surface_distance(bad_v[b], f, bad_p[b])
        assert np.array_equal(out["vpoint"][b].numpy(), ref["vpoint"])
    g_d2 = torch.where(torch.isnan(out["d2"]), torch.zeros(()), torch.ones(()))
    g_vd2 = torch.where(torch.isnan(out["vd2"]), torch.zeros(()), torch.ones(()))
    torch.autograd.backward([out["d2"], out["vd2"]], [g_d2 * 1.5, g_vd2 * 0.5])
    assert torch.isnan(V.grad[1]).all() and torch.isfinite(V.grad[[0, 2]]).all()
    assert (P.grad[0, 3] == 0).all() and (P.grad[2, 0] == 0).all() and torch.isfinite(P.grad[[0, 2]]).all()
    # no faces: +Inf, -1; m2p unaffected
    none = surface_distance(torch.from_numpy(verts), MeshTopology(np.zeros((0, 3), np.int32), 42), torch.from_numpy(pts))
    assert torch.isinf(none["d2"]).all() and (none["face"] == -1).all() and torch.equal(none["vd2"], clean["vd2"])
    # validation
    with pytest.raises(ValueError, match="vertices"):
        surface_distance(torch.zeros(1, 41, 3), topo, torch.zeros(1, 5, 3))
    with pytest.raises(ValueError, match="points"):
        surface_distance(torch.zeros(1, 42, 3), topo, torch.zeros(2, 5, 3))
    with pytest.raises(ValueError, match="counts"):
        surface_distance(torch.zeros(1, 42, 3), topo, torch.zeros(1, 5, 3), counts=[-1])
    with pytest.raises(ValueError, match="counts"):
        surface_distance(torch.zeros(1, 42, 3), topo, torch.zeros(1, 5, 3), counts=[6])
    with pytest.raises(ValueError, match="directions"):
        surface_distance(torch.zeros(1, 42, 3), topo, torch.zeros(1, 5, 3), directions=("p2p",))


def _gap_cloud(v, f, N, seed, lift):
    """Points offset along the normal from face interiors by `lift` inradii: the nearest face is that face, by a gap."""
    rng = np.random.default_rng(seed)
    fi = rng.integers(0, len(f), N)
    w = rng.dirichlet(np.full(3, 6.0), N)                                  # well inside
    t = v[f[fi]]
    n = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    area2 = np.linalg.norm(n, axis=1)
    per = sum(np.linalg.norm(t[:, k] - t[:, (k + 1) % 3], axis=1) for k in range(3))
    inr = area2 / per
    return np.einsum("nk,nkc->nc", w, t) + (n / area2[:, None]) * (lift * inr)[:, None], fi


def test_envelope_gradient_against_central_differences():
    """d (sum g_d2 d2 + sum g_vd2 vd2) / d (verts, points) by the definition's formula against central differences of the
    brute-force oracle in float64, where the minimiser does not switch: the second-best DISTINCT closest point is farther
    by a clear gap (asserted)."""
    v, f = uv_sphere(8, 5)
    v = v * np.array([0.9, 1.1, 1.0]) + 0.05
    p, fi = _gap_cloud(v, f, 30, 2, 0.08)
    M, D = orc.pair_d2(v, f, p), orc.pair_vd2(v, p)
    r = orc.surface_distance(v, f, p)
    assert np.array_equal(r["face"], fi)
    # distinct closest points: faces whose q is the same point (an edge shared with the best face) are the same minimiser
    q_best = p - r["resid"]
    for n in range(len(p)):
        tri = v[f]
        c = orc.closest(tri[:, 0] - p[n], tri[:, 1] - p[n], tri[:, 2] - p[n])
        distinct = np.linalg.norm((p[n] + c["q"]) - q_best[n], axis=1) > 1e-9
        assert np.sqrt(M[n][distinct].min()) - np.sqrt(r["d2"][n]) > 1e-3
    srt = np.sort(D, axis=1)
    assert (np.sqrt(srt[:, 1]) - np.sqrt(srt[:, 0])).min() > 1e-4
    rng = np.random.default_rng(4)
    g_d2, g_vd2 = rng.normal(size=len(p)), rng.normal(size=len(v))
    dv, dp, _ = orc.grads(v, f, p, r["face"], r["bary"], r["resid"], r["vpoint"], g_d2, g_vd2)

    def total(vv, pp):
        o = orc.surface_distance(vv, f, pp)
        return g_d2 @ o["d2"] + g_vd2 @ o["vd2"]
    h = 1e-6
    for i, c in [(int(a), int(b)) for a, b in zip(rng.integers(0, 42, 14), rng.integers(0, 3, 14))] + [(0, 1), (41, 1)]:
        vp, vm = v.copy(), v.copy()
        vp[i, c] += h
        vm[i, c] -= h
        fd = (total(vp, p) - total(vm, p)) / (2 * h)
        assert abs(fd - dv[i, c]) < 1e-7 * max(1.0, abs(fd)), (i, c, fd, dv[i, c])
    for n, c in [(int(a), int(b)) for a, b in zip(rng.integers(0, 30, 10), rng.integers(0, 3, 10))]:
        pp, pm = p.copy(), p.copy()
        pp[n, c] += h
        pm[n, c] -= h
        fd = (total(v, pp) - total(v, pm)) / (2 * h)
        assert abs(fd - dp[n, c]) < 1e-7 * max(1.0, abs(fd)), (n, c, fd, dp[n, c])
    # the package's CPU path has the same gradient (teacher-forced on its own outputs, float32 roundings apart)
    V = torch.from_numpy(v.astype(np.float32)).requires_grad_(True)[None]
    P = torch.from_numpy(p.astype(np.float32)).requires_grad_(True)[None]
    V.retain_grad(), P.retain_grad()
    out = surface_distance(V, MeshTopology(f, 42), P)
    torch.autograd.backward([out["d2"], out["vd2"]], [torch.from_numpy(g_d2.astype(np.float32))[None],
                                                        torch.from_numpy(g_vd2.astype(np.float32))[None]])
    rv, rp, T = orc.grads(V[0].detach().numpy(), f, P[0].detach().numpy(), out["face"][0].numpy(), out["bary"][0].numpy(),
                          out["resid"][0].numpy(), out["vpoint"][0].numpy(), g_d2.astype(np.float32), g_vd2.astype(np.float32))
    assert (np.abs(V.grad[0].numpy() - rv) <= 2.0 ** -24 * np.abs(rv) + 2.0 ** -28 * T).all()
    np.testing.assert_allclose(P.grad[0].numpy(), rp, rtol=2.0 ** -23, atol=1e-12)


def test_sample_surface():
    v, f = uv_sphere(8, 5)
    verts = torch.from_numpy(np.stack([v, 0.5 * v + 0.1]).astype(np.float32))
    topo = MeshTopology(f, 42)
    g = torch.Generator().manual_seed(7)
    pts, face, bary = sample_surface(verts, topo, 2000, g)
    assert pts.shape == (2, 2000, 3) and pts.dtype == torch.float32 and face.shape == (2, 2000) and bary.shape == (2, 2000, 3)
    assert (bary >= 0).all() and (bary.sum(-1) - 1).abs().max() < 1e-12
    out = surface_distance(verts, topo, pts)
    assert float(out["d2"].max()) < 1e-12                                 # on the surface (to fp32 rounding)
    # area-weighted: the faces' share of the samples follows their share of the area
    tri = v[f]
    area = np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=1)
    share = np.bincount(face[0].numpy(), minlength=80) / 2000.0
    assert np.abs(share - area / area.sum()).max() < 0.02
    pts2, _, _ = sample_surface(verts, topo, 2000, torch.Generator().manual_seed(7))
    assert torch.equal(pts, pts2)
    with pytest.raises(ValueError, match="no faces"):
        sample_surface(verts, MeshTopology(np.zeros((0, 3), np.int32), 42), 5)


class _StubRegressor(torch.nn.Module):
    def forward(self, images):
        return images


class _StubLayer:
    """A CPU stand-in for SMPLLayer: a fixed mesh scaled by column 76 and shifted by columns 1..3."""
    num_cam = 4

    def __init__(self, v):
        self.v = torch.from_numpy(v.astype(np.float32))

    def __call__(self, x):
        return (1.0 + 0.1 * x[:, 76, None, None]) * self.v[None] + x[:, None, 1:4]


def test_evaluate_scans_on_a_stub_model():
    from ilps_amd.evaluation import evaluate_scans
    v, f = uv_sphere(8, 5)
    topo, layer, reg = MeshTopology(f, 42), _StubLayer(v), _StubRegressor()
    rng = np.random.default_rng(0)
    xs = [torch.from_numpy(rng.normal(0, 0.3, (n, 86)).astype(np.float32)) for n in (2, 3)]
    pts = [torch.from_numpy(rng.normal(0, 1, (n, 25, 3)).astype(np.float32)) for n in (2, 3)]
    cnts = [torch.tensor([25, 11], dtype=torch.int32), torch.tensor([0, 25, 7], dtype=torch.int32)]
    res = evaluate_scans(reg, layer, [(x, (p, c)) for x, p, c in zip(xs, pts, cnts)], topo)
    s_p = s_v = 0.0
    n_p = n_v = 0
    for x, p, c in zip(xs, pts, cnts):
        out = surface_distance(layer(x), topo, p, c)
        for b in range(len(x)):
            k = int(c[b])
            s_p += float(out["d2"][b, :k].double().sqrt().sum())
            n_p += k
            if k:
                s_v += float(out["vd2"][b].double().sqrt().sum())
                n_v += 42
    assert res["points"] == n_p == 68 and res["vertices"] == n_v == 4 * 42 and res["count"] == 5 and res["nonfinite"] == 0
    assert abs(res["scan_to_mesh"] - s_p / n_p) < 1e-12 and abs(res["mesh_to_scan"] - s_v / n_v) < 1e-12
    # a NaN prediction is left out and counted; a NaN point is left out of both means
    bad = xs[0].clone()
    bad[1, 76] = float("nan")
    p0 = pts[0].clone()
    p0[0, 4, 2] = float("nan")
    res = evaluate_scans(reg, layer, [(bad, (p0, None))], topo)
    assert res["count"] == 1 and res["nonfinite"] == 1 and res["points"] == 24 and res["vertices"] == 42
    assert np.isfinite(res["scan_to_mesh"]) and np.isfinite(res["mesh_to_scan"])
    with pytest.raises(ValueError, match="no batches"):
        evaluate_scans(reg, layer, [], topo)
    with pytest.raises(ValueError, match="points"):
        evaluate_scans(reg, layer, [(xs[0], (pts[1], None))], topo)


def test_abi_symbols_and_launchers_refuse_bad_arguments_without_launching():
    from ilps_amd import _lib
    lib = _lib.load()
    for name in ("smplr_scan_p2m", "smplr_scan_m2p", "smplr_scan_bwd"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    one = 1                                            # (a non-null pointer value that is never dereferenced: no launch)
    p2m = lambda verts=one, B=2, V=42, F=80, N=50, d2=one: lib.smplr_scan_p2m(verts, one, one, None, B, V, F, N, d2, one, one,
                                                                            one, one, None)
    m2p = lambda verts=one, B=2, V=42, F=80, N=50, d2=one: lib.smplr_scan_m2p(verts, one, None, B, V, N, d2, one, one, None)
    bwd = lambda verts=one, B=2, V=42, F=80, N=50, d2=one: lib.smplr_scan_bwd(verts, one, one, one, one, one, one, one, one, one,
                                                                            B, V, F, N, d2, None)
    for fn, name in ((p2m, b"smplr_scan_p2m"), (m2p, b"smplr_scan_m2p"), (bwd, b"smplr_scan_bwd")):
        assert fn(verts=None) == -1 and b"null" in lib.smplr_last_error() and name in lib.smplr_last_error()
        assert fn(d2=None) == -1 and b"null" in lib.smplr_last_error()
        assert fn(V=0) == -1 and b"V=0" in lib.smplr_last_error()
        assert fn(V=(1 << 24) + 1) == -1 and fn(N=(1 << 24) + 1) == -1 and fn(N=-1) == -1 and fn(B=-1) == -1
        assert fn(B=0, verts=None) == 0                 # an empty batch is a no-op
    assert p2m(F=(1 << 24) + 1) == -1 and p2m(F=-1) == -1 and bwd(F=(1 << 24) + 1) == -1
    # a cotangent needs what its term reads
    assert lib.smplr_scan_bwd(one, one, one, None, one, one, one, one, one, None, 2, 42, 80, 50, one, None) == -1
    assert b"g_d2" in lib.smplr_last_error()
    assert lib.smplr_scan_bwd(one, one, one, one, one, one, None, one, None, one, 2, 42, 80, 50, one, None) == -1
    assert b"g_vd2" in lib.smplr_last_error()
    header = open(os.path.join(ROOT, "include", "smplraster.h")).read()
    assert all("int %s(" % n in header for n in ("smplr_scan_p2m", "smplr_scan_m2p", "smplr_scan_bwd"))
    assert "#define SMPLR_ABI_VERSION 7" in header and "#define SMPLR_SCAN_NONFINITE 1" in header


def test_kernels_fit_their_launch():
    """Registers, LDS and scratch from the built code object: no scratch, static LDS below 64 KB, 256 lanes per workgroup,
    and the search kernels keep at least four waves per SIMD (their loops hide LDS latency by occupancy)."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr
    ks = {n: k for n, k in kr.kernels().items() if "scan_p2m_kernel" in n or "scan_m2p_kernel" in n or "scan_bwd_kernel" in n}
    assert len(ks) == 3
    for name, k in ks.items():
        assert k["scratch"] == 0, "%s spills %d B per lane" % (name, k["scratch"])
        assert k["lds"] <= 64 * 1024
        assert k["max_threads"] >= 256 and kr.waves_per_simd(k) >= 4
