"""The mesh regularisers without a GPU: tests/_meshreg_oracle.py (NumPy float64, analytic gradient) against float64 torch
autograd of `meshreg.mesh_reg_torch` and against central differences, `MeshRegSpec`'s construction, and the properties the
definitions promise.  Unit roundoff of float64: U = 2^-53."""
import numpy as np
import pytest
import torch

import _meshreg_oracle as mo
import _render_oracle as ro
from ilps_amd.meshreg import MeshRegSpec, mesh_reg_torch, mesh_regularisers, one_ring
from ilps_amd.render import MeshTopology

U = 2.0 ** -53


def sphere():
    v, f = ro.uv_sphere(8, 5)
    return np.asarray(v, np.float64), np.asarray(f, np.int32)


def soup_with_loose_vertices():
    """soup(7): 300 disjoint triangles; plus a fan of three faces round one edge (non-manifold) and four vertices no face
    names (degree 0)."""
    v, f = ro.soup(7)
    n = len(v)
    extra = np.array([[0.0, 0.0, 0.0], [0.3, 0.0, 0.1], [0.1, 0.4, 0.0], [0.1, -0.3, 0.2], [0.2, 0.1, -0.5]])
    fan = np.array([[n, n + 1, n + 2], [n, n + 1, n + 3], [n + 1, n, n + 4]], np.int32)
    loose = np.array([[2.0, 2.0, 2.0], [-2.0, 1.0, 0.0], [0.5, 0.5, 0.5], [0.0, -1.0, 1.0]])
    return np.concatenate([v.astype(np.float64), extra, loose]), np.concatenate([f, fan])


MESHES = {"sphere": sphere, "soup": soup_with_loose_vertices}


def build(kind, weights="uniform", vweight=False, smooth=False, seed=0):
    ref, faces = MESHES[kind]()
    V = len(ref)
    rng = np.random.default_rng(seed)
    vw = rng.uniform(0.0, 2.0, V) if vweight else None
    spec = MeshRegSpec(MeshTopology(faces, V), ref, weights, vw, smooth)
    verts = (ref + rng.normal(0, 0.05, ref.shape)).astype(np.float32).astype(np.float64)
    return spec, ref, faces, verts


def torch_terms(verts, spec, dtype=torch.float64):
    t = spec.on("cpu")
    return mesh_reg_torch(torch.as_tensor(verts, dtype=dtype), t["nb_off"], t["nb_idx"], t["nb_w"], t["lap_ref"], t["vweight"],
                          spec.num_edges)


CONFIGS = [("sphere", "uniform", False, False), ("sphere", "cotangent", True, False), ("sphere", "cotangent", False, True),
           ("soup", "uniform", True, False), ("soup", "cotangent", False, False)]


@pytest.mark.parametrize("kind,weights,vweight,smooth", CONFIGS)
def test_oracle_gradient_equals_autograd(kind, weights, vweight, smooth):
    """Both sides are float64 evaluations of the same sums in different orders: they differ by at most a few U of the
    magnitudes T the oracle reports (64 covers the longest ring, 3 x 17 products, and the tree above it)."""
    spec, _, _, verts = build(kind, weights, vweight, smooth)
    g = (0.7, 1.3)
    ref = mo.evaluate(verts, spec, g)
    v = torch.tensor(verts[None], dtype=torch.float64, requires_grad=True)
    terms = torch_terms(v, spec)
    (g[0] * terms[0, 0] + g[1] * terms[0, 1]).backward()
    assert np.all(np.abs(terms.detach().numpy()[0] - ref["terms"]) <= 64 * U * ref["T_terms"])
    assert np.all(np.abs(v.grad.numpy()[0] - ref["grad"]) <= 64 * U * ref["T_grad"] + 1e-300)


@pytest.mark.parametrize("kind,weights,vweight,smooth", CONFIGS[:4])
def test_oracle_gradient_equals_central_differences(kind, weights, vweight, smooth):
    """Central differences with h = 2^-14 on energies that are polynomials of degree <= 4 in a coordinate: the truncation
    error is h^2 / 6 |f'''| and the cancellation error U T / h; both stay below 1e-6 of the gradient's scale here."""
    spec, _, _, verts = build(kind, weights, vweight, smooth, seed=3)
    ref = mo.evaluate(verts, spec, (1.0, 1.0))
    h = 2.0 ** -14
    rng = np.random.default_rng(5)
    scale = np.abs(ref["grad"]).max()
    for i in rng.choice(len(verts), 12, replace=False):
        for c in range(3):
            p, m = verts.copy(), verts.copy()
            p[i, c] += h
            m[i, c] -= h
            fd = (mo.evaluate(p, spec)["terms"].sum() - mo.evaluate(m, spec)["terms"].sum()) / (2 * h)
            assert abs(fd - ref["grad"][i, c]) <= 1e-6 * scale, (i, c, fd, ref["grad"][i, c])


@pytest.mark.parametrize("kind", ["sphere", "soup"])
def test_csr_against_brute_force(kind):
    spec, ref, faces, _ = build(kind, "cotangent")
    V = len(ref)
    nb = mo.brute_one_ring(faces, V)
    off, idx = spec.nb_off, spec.nb_idx
    assert off[0] == 0 and off[-1] == len(idx) == spec.nnz
    for i in range(V):
        assert idx[off[i]:off[i + 1]].tolist() == nb[i]
    # the transposed weight and the edge length of entry (i, k) are those of entry (k, i)
    pos = {(i, int(k)): e for i in range(V) for e, k in zip(range(off[i], off[i + 1]), idx[off[i]:off[i + 1]])}
    for (i, k), e in pos.items():
        assert spec.nb_w[e, 1] == spec.nb_w[pos[(k, i)], 0] and spec.nb_w[e, 2] == spec.nb_w[pos[(k, i)], 2]
        l2 = ((ref[i] - ref[k]) ** 2).sum()
        assert spec.nb_w[e, 2] == np.float32(1.0 / l2)
    assert spec.num_edges == sum(1 for (i, k) in pos if i < k)
    o2, i2 = one_ring(faces, V)
    assert np.array_equal(o2, off) and np.array_equal(i2, idx)


@pytest.mark.parametrize("kind,weights", [("sphere", "uniform"), ("soup", "uniform"), ("sphere", "cotangent"), ("soup", "cotangent")])
def test_rows_sum_to_one(kind, weights):
    """Each weight is a float64 quotient rounded to fp32 (2^-24 relative), so a row of positive weights sums to 1 within
    2^-24 of the sum of the weights = 2^-24; a vertex of degree 0 has an empty row."""
    spec, _, _, _ = build(kind, weights)
    a = mo.arrays(spec)
    rs = np.bincount(a["row"], a["w"], minlength=a["V"])
    assert (a["w"] >= 0).all()
    assert np.all(np.abs(rs[a["deg"] > 0] - 1.0) <= 2.0 ** -24)
    assert np.all(rs[a["deg"] == 0] == 0)
    if weights == "uniform":
        assert np.array_equal(a["w"], (1.0 / a["deg"][a["row"]]).astype(np.float32).astype(np.float64))


def test_cotangent_weights_on_a_regular_grid():
    """Right triangles on a square grid: the diagonals face two right angles (cot = 0) and every axis edge two angles of 45
    degrees (cot 1 + 1), so an interior vertex has the five-point stencil - 1/4 on its four axis neighbours, 0 on the two
    diagonal ones."""
    v, f = ro.grid_plane(4, 4, 0.0, 0.0, 0.25, alt=False)
    V = len(v)
    spec = MeshRegSpec(MeshTopology(np.asarray(f, np.int32), V), v, "cotangent")
    a = mo.arrays(spec)
    nx = 5
    for r in range(1, 4):
        for c in range(1, 4):
            i = r * nx + c
            row = {int(k): w for k, w in zip(a["idx"][a["off"][i]:a["off"][i + 1]], a["w"][a["off"][i]:a["off"][i + 1]])}
            assert len(row) == 6
            for k, w in row.items():
                axis = k in (i - 1, i + 1, i - nx, i + nx)
                assert abs(w - (0.25 if axis else 0.0)) <= 2.0 ** -24, (i, k, w)


def test_clamp_and_uniform_fallback():
    # an obtuse triangle: the edge facing the obtuse corner has a negative cotangent and is clamped to 0
    v = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.5, 0.1, 0.0]])
    spec = MeshRegSpec(MeshTopology(np.array([[0, 1, 2]], np.int32), 3), v, "cotangent")
    a = mo.arrays(spec)
    w = {(int(i), int(k)): x for i, k, x in zip(a["row"], a["idx"], a["w"])}
    assert w[(0, 1)] == 0.0 and w[(1, 0)] == 0.0 and w[(0, 2)] == 1.0 and w[(1, 2)] == 1.0
    assert abs(w[(2, 0)] + w[(2, 1)] - 1.0) <= 2.0 ** -24 and w[(2, 0)] > 0 and w[(2, 1)] > 0
    # a face of zero area (collinear corners): every cotangent is left out, every row falls back to uniform
    v = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [3.0, 0.0, 0.0]])
    spec = MeshRegSpec(MeshTopology(np.array([[0, 1, 2]], np.int32), 3), v, "cotangent")
    assert np.array_equal(spec.nb_w[:, 0], np.full(6, 0.5, np.float32))
    # two obtuse triangles back to back: vertex 0's only positive edge is gone when both its edges face obtuse corners
    v = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.5, 0.05, 0.0], [0.5, -0.05, 0.0]])
    spec = MeshRegSpec(MeshTopology(np.array([[0, 1, 2], [1, 0, 3]], np.int32), 4), v, "cotangent")
    a = mo.arrays(spec)
    assert (a["w"] >= 0).all() and np.all(np.abs(np.bincount(a["row"], a["w"]) - 1.0) <= 2.0 ** -24)


def test_degenerate_topologies_give_zero_not_nan():
    one = MeshRegSpec(MeshTopology(np.zeros((0, 3), np.int32), 1), np.array([[0.3, -0.2, 0.1]]))
    assert one.nnz == 0 and one.num_edges == 0
    for v in (np.array([[[0.3, -0.2, 0.1]]]), np.array([[[5.0, 1.0, -2.0]]])):
        t = torch_terms(v, one).numpy()
        assert np.array_equal(t, np.zeros((1, 2)))                   # L(v) of a vertex of degree 0 is 0, and so is lap_ref
        assert np.array_equal(mo.evaluate(v[0], one)["terms"], np.zeros(2))
    loose = MeshRegSpec(MeshTopology(np.zeros((0, 3), np.int32), 5), np.arange(15.0).reshape(5, 3), "cotangent")
    v = torch.randn(2, 5, 3, dtype=torch.float64, requires_grad=True)
    t = torch_terms(v, loose)
    assert np.array_equal(t.detach().numpy(), np.zeros((2, 2)))
    t.sum().backward()
    assert np.array_equal(v.grad.numpy(), np.zeros((2, 5, 3)))
    # degree 0 beside a face: that vertex adds nothing and has a zero gradient
    ref = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [4.0, 4.0, 4.0]])
    spec = MeshRegSpec(MeshTopology(np.array([[0, 1, 2]], np.int32), 4), ref)
    moved = ref.copy()
    moved[3] += 7.0
    assert np.array_equal(mo.evaluate(moved, spec)["terms"], mo.evaluate(ref, spec)["terms"])
    assert np.array_equal(mo.evaluate(moved, spec)["grad"][3], np.zeros(3))
    # a reference edge of zero length is left out of E_edge and of E
    ref = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [1.0, 0.0, 0.0]])
    spec = MeshRegSpec(MeshTopology(np.array([[0, 1, 2]], np.int32), 3), ref)
    assert spec.num_edges == 2 and np.isfinite(torch_terms(ref[None] + 0.1, spec).numpy()).all()


def test_value_errors():
    v, f = sphere()
    topo = MeshTopology(f, len(v))
    with pytest.raises(ValueError):
        MeshRegSpec(topo, v[:-1])
    with pytest.raises(ValueError):
        MeshRegSpec(topo, v.reshape(-1))
    with pytest.raises(ValueError):
        MeshRegSpec(topo, v, vweight=-np.ones(len(v)))
    with pytest.raises(ValueError):
        MeshRegSpec(topo, v, vweight=np.ones(len(v) - 1))
    with pytest.raises(ValueError):
        MeshRegSpec(topo, v, weights="mean-value")
    with pytest.raises(ValueError):
        MeshRegSpec(topo, v, weights=np.ones(3))
    bad = v.copy()
    bad[0, 0] = np.nan
    with pytest.raises(ValueError):
        MeshRegSpec(topo, bad)
    with pytest.raises(TypeError):
        MeshRegSpec(f, v)
    spec = MeshRegSpec(topo, v)
    with pytest.raises(ValueError):
        mesh_regularisers(torch.zeros(2, len(v) + 1, 3), spec)
    with pytest.raises(TypeError):
        mesh_regularisers(torch.zeros(2, len(v), 3), topo)


@pytest.mark.parametrize("kind,weights", [("sphere", "uniform"), ("sphere", "cotangent"), ("soup", "cotangent")])
def test_reference_has_zero_energy(kind, weights):
    """At verts = ref: lap_ref is L(ref) rounded to fp32, so |L(ref)_i - lap_ref_i| <= 2^-24 |L(ref)_i| per coordinate (plus
    the float64 evaluation, 64 U of the magnitudes) and E_lap(ref) <= the mean of the squares of that - nothing else is left;
    with smooth=True the same mesh has E_lap = mean |L(ref)|^2, far above.  E_edge: q = l^2 fl32(1 / l^2) - 1, at most 2^-24
    (+ 4 U) in magnitude per edge, so E_edge(ref) <= (2^-24 + 4 U)^2."""
    ref, faces = MESHES[kind]()
    topo = MeshTopology(faces, len(ref))
    spec = MeshRegSpec(topo, ref, weights)
    o = mo.evaluate(ref, spec)
    plain = mo.evaluate(ref, MeshRegSpec(topo, ref, weights, smooth=True))
    a = mo.arrays(spec)
    s = np.zeros_like(ref)
    np.add.at(s, a["row"], a["w"][:, None] * ref[a["idx"]])
    L = np.where((a["deg"] > 0)[:, None], ref - s, 0.0)
    Mag = np.abs(ref) + np.abs(s)
    bound = (((2.0 ** -24) * np.abs(L) + 64 * U * Mag) ** 2).sum() / len(ref)
    assert o["terms"][0] <= bound
    assert plain["terms"][0] > 1e6 * max(bound, 1e-300)
    assert o["terms"][1] <= (2.0 ** -24 + 4 * U) ** 2
    t = torch_terms(ref[None], spec).numpy()[0]
    assert t[0] <= bound and t[1] <= (2.0 ** -24 + 4 * U) ** 2


@pytest.mark.parametrize("kind,weights,vweight", [("sphere", "cotangent", True), ("soup", "uniform", False)])
def test_invariance_under_rigid_motion(kind, weights, vweight):
    """E_edge sees edge lengths only and is invariant under any rigid motion.  The rows of L sum to 1, so L(v + t) = L(v)
    and L(R v) = R L(v): E_lap is invariant under translations always, and under rotations when lap_ref = 0 (smooth=True) -
    with lap_ref = L(ref) the term compares L(v) with a fixed vector field and is NOT rotation invariant, which is why
    `OffsetFitter` evaluates it in the template's frame (asserted at the end).
    Bound, from float64 rounding alone: the moved coordinates v' = R v + t carry at most eps_v = 4 U (sqrt(3) |v|_max +
    |t|_max) of error each (three products, three sums), which moves an energy by at most eps_v |grad|_1 to first order; each
    of the two evaluations adds 64 U T; a factor 2 covers the second order.  One more term is not rounding of the arithmetic
    but of the DEFINITION: the stored weights are fp32, so a row sums to 1 - d_i with |d_i| up to deg 2^-25, and
    L(v + t)_i = L(v)_i + d_i t exactly.  That moves E_lap by at most 1/V sum_i vweight_i (2 |delta_i| . |d_i t| + |d_i t|^2),
    computed here from the spec's weights (uniform rows of a power-of-two degree have d_i = 0)."""
    rng = np.random.default_rng(11)
    Q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    Q *= np.sign(np.linalg.det(Q))
    shift = rng.uniform(-3, 3, 3)
    for smooth in (True, False):
        spec, ref, faces, verts = build(kind, weights, vweight, smooth, seed=2)
        o = mo.evaluate(verts, spec)

        a = mo.arrays(spec)
        defect = np.abs(np.where(a["deg"] > 0, 1.0 - np.bincount(a["row"], a["w"], minlength=a["V"]), 0.0))
        s = np.zeros_like(verts)
        np.add.at(s, a["row"], a["w"][:, None] * verts[a["idx"]])
        delta = np.abs(np.where((a["deg"] > 0)[:, None], verts - s, 0.0) - a["lref"])

        def bound(t, i, moved):
            eps_v = 4 * U * (np.sqrt(3) * max(np.abs(verts).max(), np.abs(moved).max()) + np.abs(t).max())
            b = 2 * (eps_v * np.abs(o["grad_lap" if i == 0 else "grad_edge"]).sum() + 2 * 64 * U * o["T_terms"][i])
            if i == 0:
                dt = defect[:, None] * np.abs(t)[None]
                b += 2 * (a["vw"][:, None] * (2 * delta.sum(1, keepdims=True) * dt + dt * dt)).sum() / a["V"]
            return b
        moved = verts + shift
        m = mo.evaluate(moved, spec)
        # (T of the moved mesh's Laplacian grows with |t|: bound it with the moved mesh's own magnitudes as well)
        for i in (0, 1):
            assert abs(m["terms"][i] - o["terms"][i]) <= bound(shift, i, moved) + 2 * 64 * U * m["T_terms"][i]
        moved = verts @ Q.T + shift
        m = mo.evaluate(moved, spec)
        assert abs(m["terms"][1] - o["terms"][1]) <= bound(shift, 1, moved) + 2 * 64 * U * m["T_terms"][1]
        if smooth:
            assert abs(m["terms"][0] - o["terms"][0]) <= bound(shift, 0, moved) + 2 * 64 * U * m["T_terms"][0]
        else:
            assert abs(m["terms"][0] - o["terms"][0]) > 1e3 * (bound(shift, 0, moved) + 2 * 64 * U * m["T_terms"][0])
        got = torch_terms(np.stack([verts, verts + shift]), spec).numpy()
        for i in (0, 1):
            assert abs(got[1, i] - got[0, i]) <= bound(shift, i, verts + shift) + 2 * 64 * U * m["T_terms"][i] + 64 * U * got[0, i]


def test_cpu_tensors_take_the_torch_path():
    spec, _, _, verts = build("sphere", "cotangent", True)
    v32 = torch.tensor(np.stack([verts, verts * 1.1]), dtype=torch.float32, requires_grad=True)
    terms = mesh_regularisers(v32, spec, return_terms=True)
    assert terms.dtype == torch.float32 and tuple(terms.shape) == (2, 2)
    ref = mo.evaluate(verts, spec)
    # fp64 sums, one rounding to fp32: the GPU bar
    assert np.all(np.abs(terms.detach().numpy()[0].astype(np.float64) - ref["terms"]) <= 2.0 ** -24 * ref["terms"] + 2.0 ** -28 * ref["T_terms"])
    e = mesh_regularisers(v32, spec, lap_weight=3.0, edge_weight=0.5)
    assert torch.equal(e, 3.0 * terms[:, 0] + 0.5 * terms[:, 1])
    e.sum().backward()
    g = mo.evaluate(verts, spec, (3.0, 0.5))
    assert np.all(np.abs(v32.grad.numpy()[0] - g["grad"]) <= 2.0 ** -23 * np.abs(g["grad"]) + 2.0 ** -28 * g["T_grad"])


def test_offsets_reach_the_public_interface():
    """The SMPL+D plumbing that needs no GPU: the layer and the scan fitter take `offsets`, the offset node refuses CPU
    tensors (no CPU path, no fallback), `OffsetFitter` checks what it is built from, the oracle's Adam is Adam."""
    import inspect
    from ilps_amd import ops
    from ilps_amd.fitting import OffsetFitter, ScanFitter, offset_step
    from ilps_amd.keras_smpl.batch_smpl import SMPLLayer
    from ilps_amd.evaluation import evaluate_registration
    assert "offsets" in inspect.signature(SMPLLayer.forward).parameters
    assert "offsets" in inspect.signature(ScanFitter.place).parameters and "offsets" in inspect.signature(ScanFitter.terms).parameters
    assert callable(evaluate_registration) and callable(offset_step)
    layer = SMPLLayer(None)
    with pytest.raises(RuntimeError):
        layer(torch.zeros(1, 86), offsets=torch.zeros(1, 6890, 3))
    assert issubclass(ops.BatchSMPLOffsetFn, torch.autograd.Function)
    v, f = sphere()
    with pytest.raises(TypeError):
        OffsetFitter(object(), MeshRegSpec(MeshTopology(f, len(v)), v))
    D, m, vv, t = mo.adam(np.zeros(3), np.array([1.0, -2.0, 0.0]), np.zeros(3), np.zeros(3), 0, 0.1, 0.9, 0.999, 0.0, "torch")
    assert np.allclose(D, [-0.1, 0.1, 0.0]) and t == 1                  # the first Adam step is lr sign(g)


def test_kernels_use_no_scratch():
    """What the code objects say (no GPU): the three regulariser kernels and the offset step have no scratch frame and no
    AGPRs, and fit eight waves per SIMD; the forward's only LDS is the 4 x 2 fp64 wave sums."""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import kernel_resources as kr
    ks = kr.kernels()
    hit = {n: k for n, k in ks.items() if "meshreg_" in n or "offset_adam_kernel" in n}
    assert len(hit) == 4, sorted(hit)
    for name, k in hit.items():
        assert k["scratch"] == 0 and k["agpr"] == 0, (name, k)
        assert kr.waves_per_simd(k) >= 8, (name, k)
        assert k["lds"] == (64 if "meshreg_fwd_kernel" in name else 0), (name, k["lds"])
