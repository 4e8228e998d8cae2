"""Self-penetration without a GPU: the oracle (tests/_penetration_oracle.py) pinned on known answers (a vertex inside and
outside a sphere of another part, a vertex in a tangent plane, exact mirror ties, an all-zero table, an asymmetric table);
the package's CPU path (`penetration.self_penetration` on CPU tensors, `self_penetration_torch`) against the oracle, values
and gradient; the default part-pair table; `evaluation.evaluate_penetration`; argument errors and the C ABI of the two
launchers (no launch); the kernels' registers, LDS and scratch from the built code object."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ilps_amd  # noqa: E402,F401
from ilps_amd import penetration  # noqa: E402
from ilps_amd.penetration import part_collision_table, self_penetration, self_penetration_torch  # noqa: E402
from ilps_amd.render import MeshTopology  # noqa: E402
import _penetration_oracle as orc  # noqa: E402
from _render_oracle import uv_sphere  # noqa: E402

ALL2 = np.array([[0, 1], [1, 0]], np.uint8)


def topo_of(faces, part, V=None):
    """A MeshTopology with the given per-vertex parts (the constructor's tables are for SMPL's vertex count only)."""
    t = MeshTopology(faces, len(part) if V is None else V)
    t.vertex_part = np.asarray(part, np.int64)
    return t


def sphere_and_probe(offset):
    """A unit uv_sphere(8, 5) as part 0 and one loose vertex of part 1 at distance 1 + offset from the centre along the
    direction of sphere vertex 10."""
    v, f = uv_sphere(8, 5)
    probe = v[10] * (1.0 + offset)
    return np.concatenate([v, probe[None]]), f, np.array([0] * 42 + [1])


def test_oracle_vertex_inside_and_outside_a_sphere():
    v, f, part = sphere_and_probe(-0.1)
    r = orc.self_penetration(v, f, part, ALL2)
    assert r["near"][42] == 10 and r["inside"][42] and r["e"][42] == r["d2"][42] and abs(r["d2"][42] - 0.01) < 1e-15
    # the sphere's own vertices see the probe from the side their normals point away from: the probe's normal is zero
    assert not r["inside"][:42].any() and (r["near"][:42] == 42).all() and (r["e"][:42] == 0).all()
    v, f, part = sphere_and_probe(+0.1)
    r = orc.self_penetration(v, f, part, ALL2)
    assert r["near"][42] == 10 and not r["inside"][42] and r["e"][42] == 0 and abs(r["d2"][42] - 0.01) < 1e-15


def test_oracle_tangent_plane_ties_and_tables():
    # one triangle in z = 0 wound so that its normal is +z; a probe in that plane next to corner 0: s = 0, not inside
    tri = np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0]])
    f = np.array([[0, 1, 2]])
    v = np.concatenate([tri, [[-0.25, -0.25, 0.0]]])
    r = orc.self_penetration(v, f, [0, 0, 0, 1], ALL2)
    assert r["near"][3] == 0 and r["s"][3] == 0 and not r["inside"][3] and r["e"][3] == 0
    below = v.copy()
    below[3, 2] = -0.125
    r = orc.self_penetration(below, f, [0, 0, 0, 1], ALL2)
    assert r["inside"][3] and r["e"][3] == 0.25 ** 2 * 2 + 0.125 ** 2
    # exact mirror ties: the probe at the origin, candidates at +-x (listed as 2 and 0): the lower index wins
    v = np.array([[-1.0, 0, 0], [0, 0, 0], [1.0, 0, 0], [0, 2.0, 0]])
    r = orc.self_penetration(v, np.zeros((0, 3), int), [0, 1, 0, 0], ALL2)
    assert r["near"].tolist() == [1, 0, 1, 1] and r["d2"][1] == 1.0
    # an all-zero table: no candidates
    v, f, part = sphere_and_probe(-0.1)
    r = orc.self_penetration(v, f, part, np.zeros((2, 2), int))
    assert (r["near"] == -1).all() and np.isinf(r["d2"]).all() and (r["e"] == 0).all() and not r["inside"].any()
    # the diagonal is ignored
    r = orc.self_penetration(v, f, part, np.ones((2, 2), int))
    assert r["near"][42] == 10 and (r["near"][:42] == 42).all()
    # an asymmetric table penalises one side only: two overlapping spheres, part 0 may hit part 1 but not the reverse
    v2, f2, part2 = two_spheres(1.2)
    r = orc.self_penetration(v2, f2, part2, np.array([[0, 1], [0, 0]]))
    assert r["inside"][:42].any() and (r["near"][42:] == -1).all() and (r["e"][42:] == 0).all()
    rs = orc.self_penetration(v2, f2, part2, ALL2)
    assert rs["inside"][:42].any() and rs["inside"][42:].any() and np.array_equal(rs["e"][:42], r["e"][:42])
    # a part outside the table counts as -1
    r = orc.self_penetration(v, f, np.where(part == 1, 7, part), ALL2)
    assert (r["near"] == -1).all()


def two_spheres(shift, n=2, loose=0, seed=0):
    """n copies of uv_sphere(8, 5), copy k shifted by k * shift along x and its part k, plus `loose` vertices of part -1."""
    v, f = uv_sphere(8, 5)
    rng = np.random.default_rng(seed)
    vs = [v + np.array([k * shift, 0.0, 0.0]) for k in range(n)] + [rng.uniform(-1, 1 + n * shift, (loose, 3))]
    fs = [f + 42 * k for k in range(n)]
    part = np.concatenate([np.full(42, k) for k in range(n)] + [np.full(loose, -1)])
    return np.concatenate(vs), np.concatenate(fs).astype(np.int32), part


def batch(n, shift, loose, B, seed):
    v, f, part = two_spheres(shift, n, loose, seed)
    rng = np.random.default_rng(seed + 1)
    verts = np.stack([v @ np.linalg.qr(rng.normal(size=(3, 3)))[0] * rng.uniform(0.7, 1.2) + rng.uniform(-0.2, 0.2, 3)
                      for _ in range(B)]).astype(np.float32)
    return verts, f, part


@pytest.mark.parametrize("n, loose, B, table", [(2, 0, 1, "all"), (3, 5, 2, "all"), (4, 3, 2, "hops1"), (3, 0, 1, "asym")])
def test_cpu_path_equals_the_oracle(n, loose, B, table):
    verts, f, part = batch(n, 1.3, loose, B, 3)
    topo = topo_of(f, part)
    collide = {"all": 1 - np.eye(n, dtype=np.uint8), "hops1": None,
               "asym": np.triu(np.ones((n, n), np.uint8), 1)}[table]
    ref_table = part_collision_table(topo, 1) if collide is None else collide
    out = self_penetration_torch(torch.from_numpy(verts), topo, collide, pairs_per_chunk=1000)
    e, det = self_penetration(torch.from_numpy(verts), topo, collide, return_details=True)
    assert e.dtype == torch.float32 and det["near"].dtype == torch.int32 and det["inside"].dtype == torch.bool
    some = False
    for b in range(B):
        r = orc.self_penetration(verts[b], f, part, ref_table)
        assert np.array_equal(out["near"][b].numpy(), r["near"]) and np.array_equal(out["inside"][b].numpy(), r["inside"])
        assert np.array_equal(out["d2"][b].numpy(), r["d2"].astype(np.float32))
        assert np.array_equal(out["e"][b].numpy(), r["e"].astype(np.float32))
        assert torch.equal(e[b], out["e"][b]) and torch.equal(det["near"][b], out["near"][b])
        some |= bool(r["inside"].any())
    assert some and (det["status"] == 0).all()


def test_cpu_gradient_equals_the_closed_form():
    verts, f, part = batch(3, 1.3, 4, 2, 8)
    topo = topo_of(f, part)
    V = torch.from_numpy(verts).requires_grad_(True)
    e, det = self_penetration(V, topo, 1 - np.eye(3, dtype=np.uint8), return_details=True)
    g = np.random.default_rng(1).normal(size=e.shape).astype(np.float32)
    e.backward(torch.from_numpy(g))
    for b in range(2):
        dv, T = orc.grads(verts[b], det["near"][b].numpy(), det["inside"][b].numpy(), g[b])
        assert np.abs(dv).max() > 0
        assert (np.abs(V.grad[b].numpy() - dv) <= 2.0 ** -24 * np.abs(dv) + 2.0 ** -28 * T).all()
    # the closed form is the derivative of sum g e where the choice does not switch: central differences of the oracle
    v64 = verts[0].astype(np.float64)
    r = orc.self_penetration(v64, f, part, 1 - np.eye(3))
    dv, _ = orc.grads(v64, r["near"], r["inside"], g[0])
    total = lambda vv: float(g[0].astype(np.float64) @ orc.self_penetration(vv, f, part, 1 - np.eye(3))["e"])
    rng = np.random.default_rng(2)
    h = 1e-7
    for i, c in zip(rng.integers(0, len(v64), 12), rng.integers(0, 3, 12)):
        vp, vm = v64.copy(), v64.copy()
        vp[i, c] += h
        vm[i, c] -= h
        fd = (total(vp) - total(vm)) / (2 * h)
        assert abs(fd - dv[i, c]) < 1e-6 * max(1.0, abs(fd)), (i, c, fd, dv[i, c])


def test_cpu_path_hostile_rows():
    verts, f, part = batch(3, 1.3, 4, 3, 5)
    topo = topo_of(f, part)
    tab = 1 - np.eye(3, dtype=np.uint8)
    clean = self_penetration_torch(torch.from_numpy(verts), topo, tab)
    bad = verts.copy()
    bad[1, 17, 2] = np.nan
    V = torch.from_numpy(bad).requires_grad_(True)
    e, det = self_penetration(V, topo, tab, return_details=True)
    assert det["status"].tolist() == [0, penetration.NONFINITE, 0]
    assert torch.isnan(e[1]).all() and torch.isnan(det["d2"][1]).all() and (det["near"][1] == -1).all() and not det["inside"][1].any()
    for b in (0, 2):
        assert torch.equal(e[b], clean["e"][b]) and torch.equal(det["near"][b], clean["near"][b])
    e.backward(torch.where(torch.isnan(e), torch.zeros(()), torch.ones(())))
    assert torch.isnan(V.grad[1]).all() and torch.isfinite(V.grad[[0, 2]]).all()
    # an empty table and a table without parts
    e0, d0 = self_penetration(torch.from_numpy(verts), topo, np.zeros((3, 3), np.uint8), return_details=True)
    assert (e0 == 0).all() and (d0["near"] == -1).all() and torch.isinf(d0["d2"]).all()
    e0, d0 = self_penetration(torch.from_numpy(verts), topo, np.zeros((0, 0), np.uint8), return_details=True)
    assert (e0 == 0).all() and (d0["near"] == -1).all()


def chain_topology():
    """Three spheres in a row that touch through bridging faces (0 - 1, 1 - 2) and a separate fourth."""
    v, f, part = two_spheres(1.9, 4)
    bridges = np.array([[0, 42, 43], [42 + 1, 84, 85]], np.int32)
    return topo_of(np.concatenate([f, bridges]), part)


def test_default_table_on_a_chain_of_parts():
    topo = chain_topology()
    off = lambda *pairs: np.array([[0 if (a == b or (a, b) in pairs or (b, a) in pairs) else 1 for b in range(4)]
                                   for a in range(4)], np.uint8)
    assert np.array_equal(part_collision_table(topo, 0), off())
    assert np.array_equal(part_collision_table(topo, 1), off((0, 1), (1, 2)))
    assert np.array_equal(part_collision_table(topo, 2), off((0, 1), (1, 2), (0, 2)))
    t = part_collision_table(topo)
    assert t.dtype == np.uint8 and np.array_equal(t, part_collision_table(topo, 1))
    with pytest.raises(ValueError, match="hops"):
        part_collision_table(topo, -1)


def test_argument_errors_are_raised_without_a_launch():
    verts, f, part = batch(2, 1.3, 0, 1, 0)
    topo = topo_of(f, part)
    v = torch.from_numpy(verts)
    with pytest.raises(ValueError, match="verts"):
        self_penetration(v[0], topo)
    with pytest.raises(ValueError, match="vertices"):
        self_penetration(v[:, :80], topo)
    with pytest.raises(RuntimeError, match="float32"):
        self_penetration(v.double(), topo)
    with pytest.raises(TypeError, match="MeshTopology"):
        self_penetration(v, f)
    with pytest.raises(ValueError, match=r"\(P, P\)"):
        self_penetration(v, topo, np.zeros((2, 3), np.uint8))
    with pytest.raises(ValueError, match="31"):
        self_penetration(v, topo, np.zeros((32, 32), np.uint8))
    with pytest.raises(ValueError, match="0 / 1"):
        self_penetration(v, topo, np.full((2, 2), 2))
    with pytest.raises(ValueError, match="0 / 1"):
        self_penetration(v, topo, np.full((2, 2), 0.5))


def test_abi_symbols_and_launchers_refuse_bad_arguments_without_launching():
    from ilps_amd import _lib
    lib = _lib.load()
    for name in ("smplr_pen_fwd", "smplr_pen_bwd"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    one = 1                                            # (a non-null pointer value that is never dereferenced: no launch)
    fwd = lambda verts=one, B=2, V=42, F=80, P=4, e=one, perm=one: lib.smplr_pen_fwd(verts, one, one, one, one, one, perm, 512, B, V, F,
                                                                                    P, e, one, one, one, one, None)
    bwd = lambda verts=one, B=2, V=42, e=one: lib.smplr_pen_bwd(verts, one, one, one, one, B, V, e, None)
    for fn, name in ((fwd, b"smplr_pen_fwd"), (bwd, b"smplr_pen_bwd")):
        assert fn(verts=None) == -1 and b"null" in lib.smplr_last_error() and name in lib.smplr_last_error()
        assert fn(e=None) == -1 and b"null" in lib.smplr_last_error()
        assert fn(V=0) == -1 and b"V=0" in lib.smplr_last_error()
        assert fn(V=(1 << 24) + 1) == -1 and fn(B=-1) == -1
        assert fn(B=0, verts=None) == 0                 # an empty batch is a no-op
    assert fwd(P=32) == -1 and b"P=32" in lib.smplr_last_error()
    assert fwd(F=(1 << 24) + 1) == -1 and fwd(F=-1) == -1 and fwd(P=-1) == -1
    assert fwd(V=600) == -1 and b"nperm" in lib.smplr_last_error()      # a perm shorter than the mesh
    header = open(os.path.join(ROOT, "include", "smplraster.h")).read()
    assert all("int %s(" % n in header for n in ("smplr_pen_fwd", "smplr_pen_bwd"))
    assert "#define SMPLR_ABI_VERSION 7" in header and "#define SMPLR_PEN_NONFINITE 1" in header


def test_evaluate_penetration_on_cpu_tensors():
    from ilps_amd.evaluation import evaluate_penetration
    verts, f, part = batch(3, 1.3, 2, 3, 4)
    verts[2] = verts[2] * np.float32(np.nan)
    topo = topo_of(f, part)
    tab = 1 - np.eye(3, dtype=np.uint8)
    res = evaluate_penetration(torch.from_numpy(verts), topo, tab)
    e, det = self_penetration(torch.from_numpy(verts), topo, tab, return_details=True)
    cnt = det["inside"].sum(1)
    assert res["inside"].tolist() == cnt.tolist() and res["inside"][2] == 0 and res["total_inside"] == int(cnt.sum()) > 0
    depth = torch.where(det["inside"], det["d2"].double(), torch.zeros(())).sqrt().amax(1)
    assert torch.equal(res["max_depth"], depth) and res["max_depth_overall"] == float(depth.max())
    assert res["count"] == 2 and res["nonfinite"] == 1 and res["meshes_with_penetration"] == int((cnt > 0).sum())


def test_kernels_fit_their_launch():
    """Registers, LDS and scratch from the built code object: no scratch, static LDS below 64 KB, 256 lanes per workgroup,
    and at least four waves per SIMD (the walks hide LDS latency by occupancy)."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr
    ks = {n: k for n, k in kr.kernels().items() if "pen_fwd_kernel" in n or "pen_bwd_kernel" in n}
    assert len(ks) == 3                                  # the pruned and the plain forward, the backward
    for name, k in ks.items():
        assert k["scratch"] == 0, "%s spills %d B per lane" % (name, k["scratch"])
        assert k["lds"] <= 64 * 1024
        assert k["max_threads"] >= 256 and kr.waves_per_simd(k) >= 4


def test_part_major_order_pads_every_part_to_whole_tiles():
    from ilps_amd.penetration import part_major_order
    part = np.array([2, -1, 0, 2, 7, 0, 0, 1, -1, 2])
    perm = part_major_order(part, 3, tile=4)
    assert perm.tolist() == [2, 5, 6, -1, 7, -1, -1, -1, 0, 3, 9, -1, 1, 4, 8]      # part 7 is outside 0 .. 2: with the -1s
    assert sorted(perm[perm >= 0].tolist()) == list(range(10))
    assert part_major_order(part, 0).tolist() == list(range(10))
    rng = np.random.default_rng(0)
    big = rng.integers(-1, 31, 6890)
    perm = part_major_order(big, 31)
    assert sorted(perm[perm >= 0].tolist()) == list(range(6890)) and len(perm) <= 6890 + 31 * 255
    for t0 in range(0, len(perm), 256):
        ids = perm[t0:t0 + 256]
        assert len(set(big[ids[ids >= 0]].tolist())) <= 1
