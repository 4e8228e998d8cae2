"""Scan distances on the GPU (csrc/scan.hip through `scan.surface_distance`, `fitting.ScanFitter`,
`evaluation.evaluate_scans`) against the float64 brute-force oracle of tests/_scan_oracle.py.

The rounding model behind the bars (u = 2^-24; DESIGN.md section 19 derives the constants):
  values    d2, resid and vd2 are the fp64 evaluation on the fp32 inputs for the CHOSEN index, rounded once:
            |got - ref(chosen)| <= u |ref|, per component.  bary >= 0, |sum bary - 1| <= 4 u, and sum_k bary_k v_k (one fp64
            evaluation on the fp32 bary) reproduces p - resid within u |resid| + u sum_k |bary_k| |v_k| per component: the
            rounding of resid, and of the three stored weights each times its corner (sized by |v_k|, not by distances from p).
  choice    the search is fp32 in coordinates relative to p: dist_ref(chosen) <= dist_min + K_P2M u M, M = the largest corner
            distance from p over the two faces; vd2_ref(chosen) <= vd2_min (1 + K_M2P u).  Observed / bar is printed.
  gradient  teacher-forced on the op's own face, bary, resid, vpoint: fp64 sums rounded once, |got - ref| <= u |ref| + 2^-28 T,
            T = the sum of |terms| of that component.
"""
import functools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _scan_oracle as orc  # noqa: E402
from _render_oracle import soup, uv_sphere  # noqa: E402

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
K_P2M = 64          # 8 (any face is never under-estimated by more) + 22 (vertex and edge regions) or
                    # + 14 + 20 / sin^2(angle at corner 0) (interior) for the nearest face, <= 64 from 39 to 141 degrees
K_M2P = 11          # 5 u on either squared distance
TILE = 256          # csrc/scan.hip SC_T: faces (points) per LDS tile, points (vertices) per workgroup


def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def t(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(dev())


# ---- cases ------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def mesh(kind, B):
    """-> verts (B, V, 3) float32, faces (F, 3) int32."""
    rng = np.random.default_rng(21)
    if kind == "sphere42":
        v, f = uv_sphere(8, 5)
    elif kind == "smpl":
        v, f = uv_sphere()
    else:                                                # "soup255" ...: an open triangle soup with zero-area faces mixed in
        n = int(kind[4:])
        v, f = soup(7, n=n, span=0.6)
        v, f = v.astype(np.float64), f.copy()
        for k in range(3, n, 17):
            v[3 * k + 2] = v[3 * k + 1]                                       # a segment
        for k in range(5, n, 29):
            v[3 * k: 3 * k + 3] = v[3 * k]                                    # a point
        for k in range(8, n, 23):
            v[3 * k + 2] = 0.25 * v[3 * k] + 0.75 * v[3 * k + 1]              # collinear, up to the fp32 rounding
        f[11] = (f[11, 0], f[11, 0], f[11, 1])                                # a face that lists one vertex twice
    verts = np.stack([v @ np.linalg.qr(rng.normal(size=(3, 3)))[0] * rng.uniform(0.7, 1.2, 3) + rng.uniform(-0.2, 0.2, 3)
                      for _ in range(B)]).astype(np.float32)
    return verts, np.asarray(f, np.int32)


@functools.lru_cache(maxsize=None)
def topology(kind):
    from ilps_amd.render import MeshTopology
    verts, f = mesh(kind, 1)
    return MeshTopology(f, verts.shape[1])


@functools.lru_cache(maxsize=None)
def cloud(kind, B, N, seed=5):
    """Points on the surface, near it, far outside, at a face's corner to the bit (= coincident with a vertex); ragged
    counts including 0 from B = 3 on."""
    verts, f = mesh(kind, B)
    rng = np.random.default_rng(seed + N)
    out = np.empty((B, N, 3), np.float32)
    for b in range(B):
        fi = rng.integers(0, len(f), N)
        w = rng.dirichlet(np.ones(3), N)
        on = np.einsum("nk,nkc->nc", w, verts[b][f[fi]].astype(np.float64))
        kind_n = (np.arange(N) + b) % 4
        p = on + np.where(kind_n[:, None] == 1, rng.normal(0, 0.02, (N, 3)), 0) + np.where(kind_n[:, None] == 2, rng.normal(0, 3.0, (N, 3)), 0)
        p[kind_n == 3] = verts[b][f[fi, 0]][kind_n == 3]
        if kind.startswith("soup") and N >= 8:              # some points on and near the face that lists one vertex twice
            p[:4] = np.einsum("nk,kc->nc", rng.dirichlet(np.ones(3), 4), verts[b][f[11]].astype(np.float64))
            p[2:4] += rng.normal(0, 1e-4, (2, 3))
        out[b] = p
    counts = np.array([N, (N + 1) // 2, 0][:B], np.int32) if B > 1 else None
    return out, counts


@functools.lru_cache(maxsize=None)
def reference(kind, B, N):
    """The oracle's full pair matrices, once per case: per mesh (M (count, F) squared distances, D (V, N))."""
    verts, f = mesh(kind, B)
    pts, counts = cloud(kind, B, N)
    out = []
    for b in range(B):
        c = N if counts is None else int(counts[b])
        out.append((orc.pair_d2(verts[b], f, pts[b, :c]), orc.pair_vd2(verts[b], pts[b], c)))
    return out


def run(kind, B, N, directions=("p2m", "m2p"), grad=False):
    from ilps_amd.scan import surface_distance
    verts, _ = mesh(kind, B)
    pts, counts = cloud(kind, B, N)
    V, P = t(verts), t(pts)
    if grad:
        V.requires_grad_(True)
        P.requires_grad_(True)
    out = surface_distance(V, topology(kind), P, None if counts is None else t(counts, torch.int32), directions)
    return V, P, out


def to_np(out):
    return {k: v.detach().cpu().numpy() for k, v in out.items()}


def check_forward(kind, B, N, out):
    """Every forward check of the module's docstring; returns the largest observed / bar of the two choice bars."""
    verts, f = mesh(kind, B)
    pts, counts = cloud(kind, B, N)
    ref = reference(kind, B, N)
    F, V = len(f), verts.shape[1]
    worst_p = worst_v = 0.0
    for b in range(B):
        c = N if counts is None else int(counts[b])
        M, D = ref[b]
        v64, p64 = verts[b].astype(np.float64), pts[b].astype(np.float64)
        d2, face, bary, resid = out["d2"][b], out["face"][b], out["bary"][b].astype(np.float64), out["resid"][b].astype(np.float64)
        # beyond counts: zeros and -1
        assert (d2[c:] == 0).all() and (face[c:] == -1).all() and (bary[c:] == 0).all() and (resid[c:] == 0).all()
        assert out["status"][b] == 0
        if c:
            fc = face[:c]
            assert ((fc >= 0) & (fc < F)).all()
            r = orc.at_faces(v64, f, p64[:c], fc)
            assert (np.abs(d2[:c] - r["d2"]) <= U * r["d2"]).all(), "d2 is not the chosen face's, rounded once"
            assert (np.abs(resid[:c] - r["resid"]) <= U * np.abs(r["resid"])).all(), "resid is not the chosen face's, rounded once"
            assert (bary[:c] >= 0).all() and (np.abs(bary[:c].sum(1) - 1) <= 4 * U).all()
            corners = v64[f[fc]]                                                          # (c, 3, 3)
            recon = (bary[:c, :, None] * corners).sum(1)
            bound = U * np.abs(resid[:c]) + U * (np.abs(bary[:c, :, None]) * np.abs(corners)).sum(1)
            assert (np.abs(recon - (p64[:c] - resid[:c])) <= bound).all(), "sum bary v does not reproduce p - resid"
            assert (np.abs(recon - r["q"]) <= U * (np.abs(bary[:c, :, None]) * np.abs(corners)).sum(1) + 2.0 ** -50).all()
            # the choice
            fmin = M.argmin(1)
            dist_c, dist_min = np.sqrt(M[np.arange(c), fc]), np.sqrt(M[np.arange(c), fmin])
            assert np.array_equal(M[np.arange(c), fc], r["d2"])                          # (one evaluation, two routes)
            Mx = np.maximum(np.linalg.norm(corners - p64[:c, None], axis=2).max(1),
                            np.linalg.norm(v64[f[fmin]] - p64[:c, None], axis=2).max(1))
            over, bar = dist_c - dist_min, K_P2M * U * Mx                                # (Mx = 0: p on a face that is one point)
            assert (over <= bar).all(), "a chosen face is farther than the nearest by %.2f bars" % (over[bar > 0] / bar[bar > 0]).max()
            if (bar > 0).any():
                worst_p = max(worst_p, float((over[bar > 0] / bar[bar > 0]).max()))
        vd2, vp = out["vd2"][b], out["vpoint"][b]
        if c == 0 or not np.isfinite(D).any():
            assert np.isinf(vd2).all() and (vd2 > 0).all() and (vp == -1).all()
        else:
            assert ((vp >= 0) & (vp < c)).all()
            rv = D[np.arange(V), vp]
            assert (np.abs(vd2 - rv) <= U * rv).all(), "vd2 is not the chosen point's, rounded once"
            vmin = D.min(1)
            ok = rv <= vmin * (1 + K_M2P * U)
            assert ok.all()
            nz = vmin > 0
            if nz.any():
                worst_v = max(worst_v, float(((rv[nz] / vmin[nz] - 1) / (K_M2P * U)).max()))
    print("%s B=%d N=%d: choice observed / bar: p2m %.3f (k = %d), m2p %.3f (k' = %d)" % (kind, B, N, worst_p, K_P2M, worst_v, K_M2P))
    return worst_p, worst_v


CASES = [("sphere42", 1, 1), ("sphere42", 3, 63), ("sphere42", 1, 64), ("sphere42", 3, 65), ("sphere42", 1, 255),
         ("sphere42", 3, 256), ("sphere42", 1, 257), ("sphere42", 3, 700),
         ("soup%d" % (TILE - 1), 3, 257), ("soup%d" % TILE, 1, 256), ("soup%d" % (TILE + 1), 3, 65), ("soup%d" % (TILE + 1), 1, 700),
         ("smpl", 2, 300)]


@pytest.mark.parametrize("kind, B, N", CASES)
def test_forward_against_the_pair_matrices(kind, B, N):
    _, _, out = run(kind, B, N)
    check_forward(kind, B, N, to_np(out))


@pytest.mark.parametrize("kind, B, N", [("sphere42", 3, 257), ("soup%d" % (TILE + 1), 3, 300)])
def test_one_direction_only(kind, B, N):
    _, _, both = run(kind, B, N)
    _, _, p = run(kind, B, N, directions=("p2m",))
    _, _, m = run(kind, B, N, directions="m2p")
    assert sorted(p) == ["bary", "d2", "face", "resid", "status"] and sorted(m) == ["status", "vd2", "vpoint"]
    for one in (p, m):
        for k in one:
            assert torch.equal(one[k].view(torch.int32), both[k].view(torch.int32)), k


def test_ties_go_to_the_lower_index():
    """Every face and every point listed twice: the copies compute the same numbers, and the first one is named."""
    from ilps_amd.render import MeshTopology
    from ilps_amd.scan import surface_distance
    verts, f = mesh("sphere42", 3)
    pts, _ = cloud("sphere42", 3, 257)
    a = surface_distance(t(verts), topology("sphere42"), t(pts))
    b = surface_distance(t(verts), MeshTopology(np.concatenate([f, f]), 42), t(np.concatenate([pts, pts], 1)))
    assert int(b["face"].max()) < len(f) and int(b["vpoint"].max()) < 257
    assert torch.equal(b["face"][:, :257], a["face"]) and torch.equal(b["face"][:, 257:], a["face"])
    assert torch.equal(b["vpoint"], a["vpoint"]) and torch.equal(b["d2"][:, :257], a["d2"]) and torch.equal(b["vd2"], a["vd2"])


def gap_cloud(verts, f, N, seed, lift):
    """Points offset along the normal from face interiors by `lift` inradii (< 1 / 10)."""
    rng = np.random.default_rng(seed)
    tri_all = verts[f].astype(np.float64)
    area2_all = np.linalg.norm(np.cross(tri_all[:, 1] - tri_all[:, 0], tri_all[:, 2] - tri_all[:, 0]), axis=1)
    good = np.flatnonzero(area2_all > 1e-4 * area2_all.max())
    fi = good[rng.integers(0, len(good), N)]
    w = rng.dirichlet(np.full(3, 6.0), N)
    tri = tri_all[fi]
    n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    per = sum(np.linalg.norm(tri[:, k] - tri[:, (k + 1) % 3], axis=1) for k in range(3))
    inr = area2_all[fi] / per
    return (np.einsum("nk,nkc->nc", w, tri) + (n / area2_all[fi][:, None]) * (lift * inr)[:, None]).astype(np.float32), fi


@pytest.mark.parametrize("kind, N", [("sphere42", 300), ("smpl", 300)])
def test_clear_gap_inputs_name_the_oracles_indices(kind, N):
    from ilps_amd.scan import surface_distance
    verts, f = mesh(kind, 1)
    pts, fi = gap_cloud(verts[0], f, N, 3, 0.08)
    out = to_np(surface_distance(t(verts), topology(kind), t(pts[None])))
    # closed and convex: the face below the point is the nearest (the oracle's arg-min, checked by brute force on the small mesh)
    assert np.array_equal(out["face"][0], fi)
    if kind == "sphere42":
        assert np.array_equal(orc.pair_d2(verts[0], f, pts).argmin(1), fi)
    r = orc.at_faces(verts[0], f, pts, fi)
    assert (np.abs(out["d2"][0] - r["d2"]) <= U * r["d2"]).all()
    D = orc.pair_vd2(verts[0], pts)
    srt = np.sort(D, axis=1)
    clear = np.sqrt(srt[:, 1]) - np.sqrt(srt[:, 0]) > 1e-5
    assert clear.mean() > 0.99 and np.array_equal(out["vpoint"][0][clear], D.argmin(1)[clear])


def grads_ref(kind, B, N, out, g_d2, g_vd2):
    verts, f = mesh(kind, B)
    pts, _ = cloud(kind, B, N)
    return [orc.grads(verts[b], f, pts[b], out["face"][b], out["bary"][b], out["resid"][b], out["vpoint"][b],
                      None if g_d2 is None else g_d2[b], None if g_vd2 is None else g_vd2[b]) for b in range(B)]


@pytest.mark.parametrize("kind, B, N, which", [("sphere42", 3, 700, "both"), ("sphere42", 1, 257, "p2m"), ("soup%d" % (TILE + 1), 3, 300, "both"),
                                               ("soup%d" % TILE, 1, 256, "m2p"), ("smpl", 2, 300, "both")])
def test_gradient_teacher_forced(kind, B, N, which):
    """dverts and dpoints against the definition evaluated in float64 on the op's own outputs.  The sphere's 700 points
    share 42 vertices (a vertex is a corner of many matched faces, and a quarter of the points sit ON vertices); the
    soups hold a face that lists one vertex twice (its points add to that vertex once per corner)."""
    V, P, out = run(kind, B, N, grad=True)
    rng = np.random.default_rng(9)
    verts = mesh(kind, B)[0]
    g_d2 = rng.normal(size=(B, N)).astype(np.float32) if which != "m2p" else None
    g_vd2 = rng.normal(size=(B, verts.shape[1])).astype(np.float32) if which != "p2m" else None
    o = to_np(out)
    fin = np.isfinite(o["vd2"])
    outs, gs = [], []
    if g_d2 is not None:
        outs.append(out["d2"]); gs.append(t(g_d2))
    if g_vd2 is not None:
        g_vd2 = np.where(fin, g_vd2, 0).astype(np.float32)                  # (a mesh without points: vd2 = +Inf, no gradient)
        outs.append(out["vd2"]); gs.append(t(g_vd2))
    torch.autograd.backward(outs, gs)
    dv, dp = V.grad.cpu().numpy(), P.grad.cpu().numpy()
    if kind.startswith("soup"):
        f = mesh(kind, B)[1]
        assert f[11, 0] == f[11, 1] and (o["face"] == 11).any(), "no point matched the face that lists a vertex twice"
    worst = 0.0
    for b, (rv, rp, T) in enumerate(grads_ref(kind, B, N, o, g_d2, g_vd2)):
        bar = U * np.abs(rv) + 2.0 ** -28 * T
        err = np.abs(dv[b] - rv)
        assert (err <= bar).all(), "dverts mesh %d: %d components outside the bar" % (b, int((err > bar).sum()))
        worst = max(worst, float((err[bar > 0] / bar[bar > 0]).max()) if (bar > 0).any() else 0.0)
        np.testing.assert_allclose(dp[b], rp, rtol=2.0 ** -22, atol=1e-9)
    print("%s B=%d N=%d %s: dverts observed / bar %.3f" % (kind, B, N, which, worst))


@pytest.mark.parametrize("kind, N", [("sphere42", 257), ("soup%d" % (TILE + 1), 300)])
def test_launches_and_batches_agree_bit_for_bit(kind, N):
    from ilps_amd.scan import surface_distance
    B = 3
    verts, _ = mesh(kind, B)
    pts, counts = cloud(kind, B, N)
    rng = np.random.default_rng(2)
    g_d2, g_vd2 = rng.normal(size=(B, N)).astype(np.float32), rng.normal(size=(B, verts.shape[1])).astype(np.float32)
    g_vd2[2] = 0                                                            # (counts[2] = 0: vd2 = +Inf)

    def go(sl):
        V = t(verts[sl]).requires_grad_(True)
        out = surface_distance(V, topology(kind), t(pts[sl]), t(counts[sl], torch.int32))
        torch.autograd.backward([out["d2"], out["vd2"]], [t(g_d2[sl]), t(g_vd2[sl])])
        return {**{k: v.detach() for k, v in out.items()}, "dverts": V.grad}
    bits = lambda x: x.view(torch.int32) if x.dtype == torch.float32 else x
    a, b = go(slice(0, 3)), go(slice(0, 3))
    for k in a:
        assert torch.equal(bits(a[k]), bits(b[k])), "two launches differ in %s" % k
    for i in range(B):
        one = go(slice(i, i + 1))
        for k in a:
            assert torch.equal(bits(a[k][i:i + 1]), bits(one[k])), "mesh %d alone differs from the batch in %s" % (i, k)


def test_hostile_rows():
    from ilps_amd import scan
    from ilps_amd.render import MeshTopology
    from ilps_amd.scan import surface_distance
    kind, B, N = "sphere42", 3, 65
    verts, f = mesh(kind, B)
    pts, _ = cloud(kind, B, N)
    bits = lambda x: x.view(torch.int32) if x.dtype == torch.float32 else x

    def go(v, p, counts=None, topo=None):
        V, P = t(v).requires_grad_(True), t(p).requires_grad_(True)
        out = surface_distance(V, topo or topology(kind), P, counts)
        live = lambda x: torch.where(torch.isfinite(x), torch.ones_like(x), torch.zeros_like(x))
        torch.autograd.backward([out["d2"], out["vd2"]], [1.5 * live(out["d2"]), 0.5 * live(out["vd2"])])
        return {**{k: x.detach() for k, x in out.items()}, "dverts": V.grad, "dpoints": P.grad}
    clean = go(verts, pts)
    # a NaN vertex in mesh 1 of 3
    bad_v = verts.copy()
    bad_v[1, 17, 2] = np.nan
    out = go(bad_v, pts)
    assert out["status"].tolist() == [0, scan.NONFINITE, 0]
    for k in ("d2", "bary", "resid", "vd2", "dverts"):
        assert torch.isnan(out[k][1]).all(), k
    assert (out["face"][1] == -1).all() and (out["vpoint"][1] == -1).all()
    for k in clean:
        for b in (0, 2):
            assert torch.equal(bits(out[k][b]), bits(clean[k][b])), "mesh %d is not bit-equal to the clean batch in %s" % (b, k)
    # an Inf vertex is non-finite as well
    bad_v = verts.copy()
    bad_v[0, 0, 0] = np.inf
    assert go(bad_v, pts)["status"].tolist() == [scan.NONFINITE, 0, 0]
    # a NaN point and an Inf point
    bad_p = pts.copy()
    bad_p[0, 3, 1] = np.nan
    bad_p[2, 64, 0] = -np.inf
    out = go(verts, bad_p)
    assert out["status"].tolist() == [0, 0, 0]
    for b, n in ((0, 3), (2, 64)):
        assert torch.isnan(out["d2"][b, n]) and torch.isnan(out["bary"][b, n]).all() and torch.isnan(out["resid"][b, n]).all()
        assert out["face"][b, n] == -1 and (out["vpoint"][b] != n).all() and (out["dpoints"][b, n] == 0).all()
        keep = torch.arange(N, device=dev()) != n
        for k in ("d2", "face", "bary", "resid"):
            assert torch.equal(bits(out[k][b][keep]), bits(clean[k][b][keep])), k
        ref = orc.surface_distance(verts[b], f, bad_p[b])
        assert np.array_equal(out["vpoint"][b].cpu().numpy(), ref["vpoint"])
        o = {k: x[b].cpu().numpy() for k, x in out.items()}
        rv, _, T = orc.grads(verts[b], f, bad_p[b], o["face"], o["bary"], o["resid"], o["vpoint"],
                             np.where(o["face"] >= 0, 1.5, 0), np.full(42, 0.5))
        assert (np.abs(o["dverts"] - rv) <= U * np.abs(rv) + 2.0 ** -28 * T).all()
    assert torch.equal(bits(out["dverts"][1]), bits(clean["dverts"][1]))
    # counts = 0 in mesh 1
    out = go(verts, pts, t(np.array([N, 0, 7], np.int32), torch.int32))
    assert (out["d2"][1] == 0).all() and (out["face"][1] == -1).all() and (out["bary"][1] == 0).all() and (out["resid"][1] == 0).all()
    assert torch.isinf(out["vd2"][1]).all() and (out["vd2"][1] > 0).all() and (out["vpoint"][1] == -1).all()
    assert (out["dverts"][1] == 0).all() and (out["dpoints"][1] == 0).all() and (out["dpoints"][2, 7:] == 0).all()
    assert (out["vpoint"][2] < 7).all() and torch.equal(bits(out["d2"][0]), bits(clean["d2"][0]))
    # F = 0
    out = go(verts, pts, topo=MeshTopology(np.zeros((0, 3), np.int32), 42))
    assert torch.isinf(out["d2"]).all() and (out["d2"] > 0).all() and (out["face"] == -1).all()
    assert torch.equal(bits(out["vd2"]), bits(clean["vd2"])) and torch.equal(out["vpoint"], clean["vpoint"])


# ---- through the SMPL layer -------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def body_topology():
    """An open triangle soup over the synthetic model's 6 890 vertices (the model carries no faces): consecutive vertices of
    the part tables, three at a time - 2 293 small faces, each inside one body part."""
    from ilps_amd.render import MeshTopology
    from ilps_amd.smpl_model import load_part_tables
    ids, _ = load_part_tables(1)
    f = np.asarray(ids[:(len(ids) // 3) * 3], np.int32).reshape(-1, 3)
    return MeshTopology(f, 6890), f


@pytest.fixture(scope="module")
def layer(smpl_model):
    from ilps_amd.keras_smpl.batch_smpl import SMPLLayer
    return SMPLLayer(smpl_model)


def test_chain_through_the_smpl_layer(layer, smpl_model):
    """d (sum d2 + sum vd2) / dx through SMPLLayer -> surface_distance against the float64 SMPL oracle chained with the scan
    oracle, under test_smpl_backward's bars.  The points have a clear gap (in both directions), so the oracle on its float64
    vertices and the op on the layer's fp32 vertices name the same faces and points."""
    from _inputs import make_x
    from oracle.torch_oracle import TorchSMPL
    from test_gpu_parity import grad_close
    from ilps_amd.scan import surface_distance
    topo, f = body_topology()
    B = 2
    x = make_x(B, 48, seed=11)
    xo = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    vo = TorchSMPL(smpl_model)(xo, return_all=True)[0]
    v64 = vo.detach().numpy()
    pts, keep_n = [], 120
    for b in range(B):
        p, _ = gap_cloud(v64[b], f, 600, 40 + b, 0.08)
        p = p.astype(np.float64)
        M = orc.pair_d2(v64[b], f, p)
        srt = np.sort(np.sqrt(M), axis=1)
        p = p[srt[:, 1] - srt[:, 0] > 1e-3]                                   # p2m: the second face is clearly farther
        for _ in range(20):                                                   # m2p: drop the runner-up of every near tie
            D = orc.pair_vd2(v64[b], p)
            order = np.argsort(D, axis=1)[:, :2]
            d = np.sqrt(np.take_along_axis(D, order, 1))
            tie = d[:, 1] - d[:, 0] <= 1e-4
            if not tie.any():
                break
            p = np.delete(p, np.unique(order[tie, 1]), axis=0)
        assert not tie.any() and len(p) >= keep_n
        pts.append(p[:keep_n])
    pts = np.stack(pts).astype(np.float32)
    dv = np.zeros_like(v64)
    for b in range(B):
        r = orc.surface_distance(v64[b], f, pts[b])
        dv[b] = orc.grads(v64[b], f, pts[b], r["face"], r["bary"], r["resid"], r["vpoint"], np.ones(keep_n), np.ones(6890))[0]
    (vo * torch.tensor(dv)).sum().backward()
    xg = t(x).requires_grad_(True)
    out = surface_distance(layer(xg), topo, t(pts))
    (out["d2"].sum() + out["vd2"].sum()).backward()
    for b in range(B):
        r = orc.surface_distance(v64[b], f, pts[b])
        assert np.array_equal(out["face"][b].cpu().numpy(), r["face"]) and np.array_equal(out["vpoint"][b].cpu().numpy(), r["vpoint"])
    got, want = xg.grad.cpu().numpy(), xo.grad.numpy()
    assert np.all(got[:, :4] == 0)
    grad_close(got[:, 4:76], want[:, 4:76], name="dtheta")
    grad_close(got[:, 76:], want[:, 76:], name="dbeta")


def fit_inputs(smpl_model):
    """The fit tests' data, all made on the CPU (so a CPU reference loop sees the same numbers): B = 2 scans of N = 512
    points sampled by `sample_surface` from the float64 SMPL oracle's vertices of seeded parameters, placed by (s, t), and
    a perturbed start (pose noise, shifted t).  -> x_true, x0 (2, 86) float32, scans (2, 512, 3) float32."""
    from oracle import np_oracle as o
    from ilps_amd.scan import sample_surface
    from ilps_amd.smpl_model import mean86
    topo, _ = body_topology()
    rng = np.random.default_rng(77)
    x_true = np.tile(mean86(1.0), (2, 1))
    x_true[:, 4:76] += rng.normal(0, 0.15, (2, 72))
    x_true[:, 76:] += rng.normal(0, 0.8, (2, 10))
    x_true[:, 0] = (1.0, 1.1)
    x_true[:, 1:4] = rng.normal(0, 0.1, (2, 3))
    x_true = x_true.astype(np.float32)
    v = o.smpl_layer_call(x_true.astype(np.float64), smpl_model)
    v = (x_true[:, 0, None, None].astype(np.float64) * v + x_true[:, None, 1:4]).astype(np.float32)
    scans, _, _ = sample_surface(torch.from_numpy(v), topo, 512, torch.Generator().manual_seed(5))
    x0 = x_true.copy()
    x0[:, 4:76] += rng.normal(0, 0.05, (2, 72)).astype(np.float32)
    x0[:, 1:4] += np.array((0.05, -0.04, 0.03), np.float32)
    return x_true, x0, scans.numpy()


@functools.lru_cache(maxsize=None)
def fit_case():
    from ilps_amd.keras_smpl.batch_smpl import SMPLLayer
    from ilps_amd.fitting import ScanFitter
    from ilps_amd.smpl_model import synthetic_smpl_model
    model = synthetic_smpl_model(1234)
    _, x0, scans = fit_inputs(model)
    return ScanFitter(SMPLLayer(model), body_topology()[0]), t(scans), t(x0)


FIT_KW = dict(lr=0.01, mode="torch")


def test_scan_fitter_one_iteration_is_the_hand_written_composition():
    from ilps_amd.fitting import FitState, fit_step
    from ilps_amd.scan import surface_distance
    fitter, pts, x0 = fit_case()
    r = fitter.fit(pts, init=x0, steps=1, history=True, **FIT_KW)
    B, N, V = 2, 512, 6890
    state = FitState.new(x0)
    x = state.x.detach().requires_grad_(True)
    verts = x[:, 0, None, None] * fitter.layer(x) + x[:, None, 1:4]
    out = surface_distance(verts, fitter.topo, pts)
    (g,) = torch.autograd.grad([out["d2"], out["vd2"]], [x], grad_outputs=[torch.full((B, N), 1.0 / N, device=dev()),
                                                                           torch.full((B, V), 1.0 / V, device=dev())])
    hist = torch.empty((1, B), device=dev())
    fit_step(state, g.contiguous(), out["d2"].detach(), out["vd2"].detach(), 1.0, None, hist, lr=FIT_KW["lr"], mode=FIT_KW["mode"])
    bits = lambda a: a.view(torch.int32)
    assert torch.equal(bits(r.final_x), bits(state.x)) and torch.equal(bits(r.history), bits(hist))
    assert torch.equal(bits(r.loss), bits(state.best_loss)) and torch.equal(bits(r.state.m), bits(state.m))
    assert not torch.equal(r.final_x, x0) and torch.equal(bits(fitter.losses(x0, pts)), bits(hist[0]))


@pytest.mark.parametrize("direction", ["p2m", "m2p"])
def test_scan_fitter_with_one_direction(direction):
    """One direction only: the loss `fit` records is that direction's mean alone, with ragged counts divided by the count."""
    from ilps_amd.fitting import ScanFitter
    from ilps_amd.scan import surface_distance
    full, pts, x0 = fit_case()
    fitter = ScanFitter(full.layer, full.topo, directions=(direction,))
    counts = t(np.array([512, 200], np.int32), torch.int32)
    r = fitter.fit(pts, counts, init=x0, steps=2, history=True, **FIT_KW)
    with torch.no_grad():
        out = surface_distance(fitter.place(x0), fitter.topo, pts, counts, directions=(direction,))
    want = out["d2"].double().sum(1) / counts if direction == "p2m" else out["vd2"].double().mean(1)
    assert r.steps == 2 and (r.nonfinite == 0).all()
    assert ((r.history[0].double() - want).abs() <= 1e-6 * want).all(), (r.history[0].tolist(), want.tolist())


def test_scan_fitter_lowers_every_rows_loss():
    """From the perturbed start (pose noise of 0.05 rad, t shifted by (5, -4, 3) cm) every row's best loss after 50
    iterations is strictly below its initial loss.  lr = 0.01 with torch's Adam was chosen on the CPU: the reference loop -
    the float64 SMPL oracle, scale and shift, the CPU path of `surface_distance`, `torch.optim.Adam(lr=0.01)` on the same
    scans and start - takes the two rows from 4.03e-3 and 5.49e-3 to 0.286 and 0.356 of that in 50 iterations (lr = 0.005:
    0.307 and 0.413; lr = 0.02: 0.277 and 0.314).  The data term does not vanish at the scans' own parameters (1.57e-3 and
    3.22e-3 there): 6 890 vertices look for their nearest of 512 samples.  The ratios are the reference's, not asserted."""
    fitter, pts, x0 = fit_case()
    first = fitter.losses(x0, pts)
    r = fitter.fit(pts, init=x0, steps=50, history=True, **FIT_KW)
    assert r.steps == 50 and (r.nonfinite == 0).all()
    print("ScanFitter: initial", first.tolist(), "best", r.loss.tolist(), "ratio", (r.loss / first).tolist())
    assert torch.equal(r.history[0], first) and (r.loss < first).all()


def test_scan_fitter_graph_replay_equals_eager():
    fitter, pts, x0 = fit_case()
    a = fitter.fit(pts, init=x0, steps=9, history=True, **FIT_KW)
    b = fitter.fit(pts, init=x0, steps=9, history=True, graph=True, graph_steps=4, **FIT_KW)
    bits = lambda z: z.view(torch.int32)
    assert torch.equal(bits(a.final_x), bits(b.final_x)) and torch.equal(bits(a.history), bits(b.history))
    assert torch.equal(bits(a.x), bits(b.x)) and torch.equal(a.step, b.step)


def test_evaluate_scans_equals_the_sums_by_hand(layer):
    from ilps_amd.evaluation import evaluate_scans
    from ilps_amd.scan import surface_distance
    from _inputs import make_x
    topo, _ = body_topology()

    class Identity(torch.nn.Module):
        def forward(self, images):
            return images
    rng = np.random.default_rng(1)
    xs = [t(make_x(n, 48, seed=n)) for n in (2, 3)]
    pts = [t(rng.normal(0, 0.4, (n, 130, 3))) for n in (2, 3)]
    cnts = [None, t(np.array([130, 0, 77], np.int32), torch.int32)]
    xs[1][2, 80] = float("nan")                                              # one prediction is not finite
    res = evaluate_scans(Identity(), layer, [(x, (p, c)) for x, p, c in zip(xs, pts, cnts)], topo)
    s_p = s_v = 0.0
    n_p = n_v = 0
    for x, p, c in zip(xs, pts, cnts):
        out = surface_distance(layer(x), topo, p, c)
        for b in range(len(x)):
            if int(out["status"][b]):
                continue
            k = 130 if c is None else int(c[b])
            s_p += float(out["d2"][b, :k].double().sqrt().sum())
            n_p += k
            if k:
                s_v += float(out["vd2"][b].double().sqrt().sum())
                n_v += 6890
    assert res["count"] == 4 and res["nonfinite"] == 1 and res["points"] == n_p == 390 and res["vertices"] == n_v == 3 * 6890
    assert abs(res["scan_to_mesh"] - s_p / n_p) <= 1e-12 * res["scan_to_mesh"]
    assert abs(res["mesh_to_scan"] - s_v / n_v) <= 1e-12 * res["mesh_to_scan"]
