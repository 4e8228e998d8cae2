"""The mesh regularisers on the GPU (csrc/meshreg.hip through `meshreg.mesh_regularisers` and
`torch.ops.smplraster.mesh_reg_fwd / _bwd`) against tests/_meshreg_oracle.py (NumPy float64).

The rounding model behind the bars is the one tests/test_gpu_measure.py states: the kernels take every product and sum in
fp64 on the fp32 inputs and round each output to fp32 once.  A sum of n <= 2^24 fp64 terms is off by at most n 2^-53 <= 2^-29
of T = the sum of the magnitudes of its terms, the rounding adds 2^-24 of the value: |got - ref| <= 2^-24 |ref| + 2^-28 T.
A gradient component obeys the same bar with T = the sum of |per-neighbour, per-edge contributions| at that vertex.  T comes
from the oracle (`evaluate`'s T_terms, T_grad).

Meshes: V = 1 (no face); one triangle; uv_sphere(8, 5), 42 vertices; soup(7) with a non-manifold fan and four vertices of
degree 0 (909 vertices, four blocks); uv_sphere(15, 17), 257 vertices: the per-mesh sum crosses a 256-lane block by one
vertex; and once uv_sphere(), 6 890 vertices, B = 3.  B = 1 and 5 otherwise; uniform and cotangent weights, with and without
vweight and lap_ref.

`mesh_reg_torch` on the device computes in float64 and rounds once to fp32 as the kernel does, so its fp32 error is that one
rounding: it agrees with the kernel within the bar above plus 2^-24 |ref| + 2^-28 T of its own.  The largest
|restatement - oracle| / (2^-24 |ref|) is printed (RESTATEMENT lines); it cannot exceed 1 + the fp64 part, and measured
0.79 on an MI355X when this file was written (the kernels' own worst error was 0.92 of their bar: the one rounding)."""
import functools

import numpy as np
import pytest
import torch

import _meshreg_oracle as mo
import _render_oracle as ro
from test_gpu_parity import dev, t

pytestmark = pytest.mark.gpu


def _soup():
    v, f = ro.soup(7)
    n = len(v)
    extra = np.array([[0.0, 0.0, 0.0], [0.3, 0.0, 0.1], [0.1, 0.4, 0.0], [0.1, -0.3, 0.2], [0.2, 0.1, -0.5]])
    fan = np.array([[n, n + 1, n + 2], [n, n + 1, n + 3], [n + 1, n, n + 4]], np.int32)
    loose = np.array([[2.0, 2.0, 2.0], [-2.0, 1.0, 0.0], [0.5, 0.5, 0.5], [0.0, -1.0, 1.0]])
    return np.concatenate([v.astype(np.float64), extra, loose]), np.concatenate([f, fan])


def _sphere(s, r):
    v, f = ro.uv_sphere(s, r)
    return np.asarray(v, np.float64), np.asarray(f, np.int32)


MESHES = {
    "one": lambda: (np.array([[0.3, -0.2, 0.1]]), np.zeros((0, 3), np.int32)),
    "triangle": lambda: (np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.2], [0.2, 0.9, 0.0]]), np.array([[0, 1, 2]], np.int32)),
    "sphere42": lambda: _sphere(8, 5),
    "soup": _soup,
    "sphere257": lambda: _sphere(15, 17),
    "sphere6890": lambda: _sphere(84, 82),
}


@functools.lru_cache(maxsize=None)
def case(kind, weights, vweight, smooth, B):
    """spec, verts (B, V, 3) fp32, g (B, 2) fp32 and the oracle's results per row - computed once, never modified."""
    from ilps_amd.meshreg import MeshRegSpec
    from ilps_amd.render import MeshTopology
    ref, faces = MESHES[kind]()
    V = len(ref)
    rng = np.random.default_rng(100 + V + B)
    spec = MeshRegSpec(MeshTopology(faces, V), ref, weights, rng.uniform(0.0, 2.0, V) if vweight else None, smooth)
    verts = np.stack([(ref * rng.uniform(0.8, 1.2) + rng.normal(0, 0.03, ref.shape) + rng.uniform(-1, 1, 3)) for _ in range(B)])
    verts = verts.astype(np.float32)
    g = rng.uniform(-1.5, 1.5, (B, 2)).astype(np.float32)
    want = [mo.evaluate(verts[b], spec, g[b]) for b in range(B)]
    verts.setflags(write=False)
    g.setflags(write=False)
    return spec, verts, g, want


def run(spec, verts, g):
    """terms (B, 2) and dverts (B, V, 3) of the op, as numpy arrays with their device tensors."""
    from ilps_amd.meshreg import mesh_regularisers
    v = t(np.array(verts)).requires_grad_(True)
    terms = mesh_regularisers(v, spec, return_terms=True)
    terms.backward(t(np.array(g)))
    torch.cuda.synchronize()
    return terms.detach(), v.grad


def within_bar(got, ref, T, what, extra=0.0):
    got = np.asarray(got, np.float64)
    bar = 2.0 ** -24 * np.abs(ref) + 2.0 ** -28 * T + extra
    err = np.abs(got - ref)
    worst = float((err / np.maximum(bar, 1e-300)).max()) if err.size else 0.0
    print("BAR %-40s error / bar %.4f" % (what, worst))
    assert np.all(err <= bar), "%s: %.3f of the bar" % (what, worst)


SMALL = [(k, w, vw, sm, B) for k in ("one", "triangle", "sphere42", "soup", "sphere257") for B in (1, 5)
         for (w, vw, sm) in (("uniform", False, False), ("cotangent", True, False), ("cotangent", False, True), ("uniform", True, True))]
FULL = [("sphere6890", "cotangent", True, False, 3)]
IDS = lambda cs: ["%s-%s-%s-%s-B%d" % (k, w, "vw" if vw else "novw", "smooth" if sm else "lapref", B) for k, w, vw, sm, B in cs]


@pytest.mark.parametrize("kind,weights,vweight,smooth,B", SMALL + FULL, ids=IDS(SMALL + FULL))
def test_terms_and_gradient(kind, weights, vweight, smooth, B):
    spec, verts, g, want = case(kind, weights, vweight, smooth, B)
    terms, dverts = run(spec, verts, g)
    label = "%s %s B=%d" % (kind, weights, B)
    for b in range(B):
        within_bar(terms[b].cpu().numpy(), want[b]["terms"], want[b]["T_terms"], label + " terms row %d" % b)
        within_bar(dverts[b].cpu().numpy(), want[b]["grad"], want[b]["T_grad"], label + " dverts row %d" % b)
    if spec.num_edges == 0:
        assert not terms[:, 1].any(), "E = 0 must give an edge energy of exactly 0"
    assert bool(torch.isfinite(terms).all()) and bool(torch.isfinite(dverts).all())
    # a launch reproduces its bits
    terms2, dverts2 = run(spec, verts, g)
    assert torch.equal(terms, terms2) and torch.equal(dverts, dverts2), label + ": two launches differ"
    # a row does not see its batch
    for b in range(B) if B > 1 else ():
        t1, d1 = run(spec, verts[b:b + 1], g[b:b + 1])
        assert torch.equal(t1[0], terms[b]) and torch.equal(d1[0], dverts[b]), label + ": row %d differs from its solo run" % b


@pytest.mark.parametrize("kind", ["sphere42", "sphere257"])
def test_nan_vertex_stays_in_its_row(kind):
    spec, verts, g, _ = case(kind, "cotangent", True, False, 5)
    verts, g = np.array(verts[:3]), np.array(g[:3])
    verts[1, len(verts[1]) // 2, 1] = np.nan
    terms, dverts = run(spec, verts, g)
    assert bool(torch.isnan(terms[1, 0])) and bool(torch.isnan(terms[1, 1]))
    for b in (0, 2):
        t1, d1 = run(spec, verts[b:b + 1], g[b:b + 1])
        assert torch.equal(t1[0], terms[b]) and torch.equal(d1[0], dverts[b])
        assert bool(torch.isfinite(terms[b]).all()) and bool(torch.isfinite(dverts[b]).all())


@pytest.mark.parametrize("kind,weights,vweight,smooth,B", [c for c in SMALL if c[4] == 5 and c[0] in ("soup", "sphere257")],
                         ids=IDS([c for c in SMALL if c[4] == 5 and c[0] in ("soup", "sphere257")]))
def test_torch_restatement_on_the_device(kind, weights, vweight, smooth, B):
    from ilps_amd.meshreg import mesh_reg_torch
    spec, verts, g, want = case(kind, weights, vweight, smooth, B)
    terms, dverts = run(spec, verts, g)
    d = spec.on(dev())
    v = t(np.array(verts)).requires_grad_(True)
    rt = mesh_reg_torch(v, d["nb_off"], d["nb_idx"], d["nb_w"], d["lap_ref"], d["vweight"], spec.num_edges)
    assert rt.dtype == torch.float32
    rt.backward(t(np.array(g)))
    worst = 0.0
    for b in range(B):
        ref, T = want[b]["terms"], want[b]["T_terms"]
        own = 2.0 ** -24 * np.abs(ref) + 2.0 ** -28 * T
        within_bar(rt[b].detach().cpu().numpy(), terms[b].cpu().numpy().astype(np.float64), T, "restatement terms row %d" % b,
                   extra=own + 2.0 ** -24 * np.abs(ref))
        worst = max(worst, float((np.abs(rt[b].detach().cpu().numpy() - ref) / np.maximum(2.0 ** -24 * np.abs(ref), 1e-300)).max()))
        ref, T = want[b]["grad"], want[b]["T_grad"]
        # (autograd's gradient in fp64 is rounded to fp32 once as well: the same allowance)
        own = 2.0 ** -24 * np.abs(ref) + 2.0 ** -28 * T
        within_bar(v.grad[b].cpu().numpy(), dverts[b].cpu().numpy().astype(np.float64), T, "restatement dverts row %d" % b,
                   extra=own + 2.0 ** -24 * np.abs(ref))
    print("RESTATEMENT %s %s: largest |restatement - oracle| = %.3f x 2^-24 |ref| over the terms" % (kind, weights, worst))


def test_torch_ops_agree_and_check_their_arguments():
    from ilps_amd import torch_ops
    ns = torch_ops.load()
    spec, verts, g, _ = case("sphere257", "cotangent", True, False, 5)
    terms, dverts = run(spec, verts, g)
    d = spec.on(dev())
    args = (d["nb_off"], d["nb_idx"], d["nb_w"], d["lap_ref"], d["vweight"], spec.num_edges)
    v, gg = t(np.array(verts)), t(np.array(g))
    assert torch.equal(ns.mesh_reg_fwd(v, *args), terms)
    assert torch.equal(ns.mesh_reg_bwd(v, *args, gg), dverts)
    meta = lambda x: None if x is None else torch.empty(x.shape, dtype=x.dtype, device="meta")
    assert ns.mesh_reg_fwd(meta(v), *[meta(a) if isinstance(a, torch.Tensor) else a for a in args]).shape == (5, 2)
    assert ns.mesh_reg_bwd(meta(v), *[meta(a) if isinstance(a, torch.Tensor) else a for a in args], meta(gg)).shape == v.shape
    cpu = lambda x: x.cpu() if isinstance(x, torch.Tensor) else x
    with pytest.raises((RuntimeError, NotImplementedError)):
        ns.mesh_reg_fwd(v.cpu(), *[cpu(a) for a in args])
    with pytest.raises((RuntimeError, NotImplementedError)):
        ns.mesh_reg_fwd(v, args[0].cpu(), *args[1:])
    with pytest.raises(RuntimeError):
        ns.mesh_reg_fwd(v[:, :-1], *args)                                     # V disagrees with nb_off
    with pytest.raises(RuntimeError):
        ns.mesh_reg_fwd(v, args[0], args[1], args[2][:, :2].contiguous(), *args[3:])
    with pytest.raises(RuntimeError):
        ns.mesh_reg_fwd(v, args[0], args[1][:-1], *args[2:])                  # nb_w rows != nnz
    with pytest.raises(RuntimeError):
        ns.mesh_reg_fwd(v, *args[:3], args[3][:-1], *args[4:])                # lap_ref (V - 1, 3)
    with pytest.raises(RuntimeError):
        ns.mesh_reg_fwd(v, *args[:5], spec.nnz)                               # 2 E > nnz
    with pytest.raises(RuntimeError):
        ns.mesh_reg_fwd(v.double(), *args)
    with pytest.raises(RuntimeError):
        ns.mesh_reg_bwd(v, *args, gg[:, :1].contiguous())
    with pytest.raises(RuntimeError):
        ns.mesh_reg_bwd(v, *args, gg[:-1])
