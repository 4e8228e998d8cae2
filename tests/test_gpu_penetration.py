"""Self-penetration on the GPU (csrc/penetration.hip through `penetration.self_penetration`, the fitters' `penetration`
option, `evaluation.evaluate_penetration`) against the float64 brute-force oracle of tests/_penetration_oracle.py.

The rounding model behind the bars (u = 2^-24):
  values    d2 and e are the fp64 evaluation on the fp32 inputs for the CHOSEN near, rounded once: |got - ref(chosen)| <=
            u |ref|; inside is the oracle's flag at the chosen near exactly (the same fp64 operations in the same order).
  choice    the search is m2p's fp32 arithmetic in coordinates relative to the query: d2_ref(chosen) <= d2_min (1 + K u),
            K = 11 (5 u on either squared distance).  Observed / bar is printed.  Where every runner-up is farther than the
            bar, near is the oracle's index; an exact tie names the lower index.
  gradient  teacher-forced on the op's own near / inside: fp64 sums rounded once, |got - ref| <= u |ref| + 2^-28 T, T = the sum
            of |terms| of that component.
The meshes are unions of uv_sphere(8, 5) copies (42 vertices, one part each) whose neighbours overlap by a third of a radius,
plus loose vertices of part -1, jittered by 1e-3 so that no two candidates tie; per-mesh random rotations and scales.
"""
import contextlib
import functools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _penetration_oracle as orc  # noqa: E402
from _render_oracle import uv_sphere  # noqa: E402

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
K_CHOICE = 11       # m2p's arithmetic: 5 u on either squared distance
CASES = {"v84": (2, 84), "v255": (6, 255), "v256": (6, 256), "v257": (6, 257), "v513": (12, 513), "p31": (31, 1310)}


def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def t(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(dev())


def bits(a):
    return a.view(torch.int32) if a.dtype == torch.float32 else a


@contextlib.contextmanager
def unpruned():
    """The plain walk of smplr_pen_fwd (natural order, every tile): the launcher reads the variable at every call."""
    os.environ["SMPLR_PEN_UNPRUNED"] = "1"
    try:
        yield
    finally:
        del os.environ["SMPLR_PEN_UNPRUNED"]


# ---- cases ------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def mesh(kind, B):
    """-> verts (B, V, 3) float32, faces (F, 3) int32, part (V,) int64, collide (P, P) uint8.  The copies sit on a zigzag,
    neighbours 5 / 3 apart (unit spheres: an overlap of a third of a radius); the table is random with about three pairs in
    four set, not symmetric (two parts: both directions)."""
    n, V = CASES[kind]
    v, f = uv_sphere(8, 5)
    rng = np.random.default_rng(31 + V)
    step = 5.0 / 3.0
    centres = [np.array([k * step * np.cos(0.5), (k % 2) * step * np.sin(0.5), 0.3 * (k % 3)]) for k in range(n)]
    loose = V - 42 * n
    vs = np.concatenate([v + c for c in centres] + [rng.uniform(-1, 1, (loose, 3)) + centres[n // 2]])
    vs = vs + rng.normal(0, 1e-3, vs.shape)
    faces = np.concatenate([f + 42 * k for k in range(n)]).astype(np.int32)
    part = np.concatenate([np.full(42, k) for k in range(n)] + [np.full(loose, -1)])
    order = rng.permutation(V)                                # the vertices in no particular order: the parts interleave
    inv = np.argsort(order)
    vs, part, faces = vs[order], part[order], inv[faces].astype(np.int32)
    collide = (rng.uniform(size=(n, n)) < 0.75).astype(np.uint8) if n > 2 else np.ones((2, 2), np.uint8)
    verts = np.stack([vs @ np.linalg.qr(rng.normal(size=(3, 3)))[0] * rng.uniform(0.7, 1.2) + rng.uniform(-0.2, 0.2, 3)
                      for _ in range(B)]).astype(np.float32)
    return verts, faces, part, collide


@functools.lru_cache(maxsize=None)
def topology(kind):
    from ilps_amd.render import MeshTopology
    _, faces, part, _ = mesh(kind, 1)
    topo = MeshTopology(faces, len(part))
    topo.vertex_part = part.copy()
    return topo


@functools.lru_cache(maxsize=None)
def reference(kind, B):
    """The oracle's pair matrix per mesh, once per case: (M (V, V) squared distances with +Inf off the candidates)."""
    verts, _, part, collide = mesh(kind, B)
    return [orc.pair_d2(verts[b], part, collide) for b in range(B)]


def run(kind, B, grad=False, verts=None):
    from ilps_amd.penetration import self_penetration
    vs, _, _, collide = mesh(kind, B)
    V = t(vs if verts is None else verts)
    if grad:
        V.requires_grad_(True)
    e, det = self_penetration(V, topology(kind), collide, return_details=True)
    return V, e, det


def check_forward(kind, B, e, det):
    """Every forward check of the module's docstring; returns the largest observed / bar of the choice."""
    verts, faces, part, collide = mesh(kind, B)
    ref = reference(kind, B)
    e, d2, near, inside = (x.cpu().numpy() for x in (e, det["d2"], det["near"], det["inside"]))
    assert det["status"].tolist() == [0] * B
    worst, n_inside = 0.0, 0
    for b in range(B):
        M = ref[b]
        mn = M.min(1)
        has = np.isfinite(mn)
        assert np.array_equal(near[b] >= 0, has) and np.isinf(d2[b][~has]).all() and (e[b][~has] == 0).all()
        assert (part[near[b][has]] >= 0).all() and np.isfinite(M[np.arange(len(M))[has], near[b][has]]).all()   # a candidate
        rd2, _, rin, re = orc.at(verts[b], faces, near[b])
        assert np.array_equal(inside[b], rin)
        assert (np.abs(d2[b][has] - rd2[has]) <= U * rd2[has]).all() and (np.abs(e[b] - re) <= U * re).all()
        bar = mn[has] * (K_CHOICE * U)
        obs = rd2[has] - mn[has]
        assert (obs <= bar).all()
        worst = max(worst, float((obs / np.maximum(bar, 1e-300)).max()))
        # where every runner-up is farther than the bar, the index is the oracle's (the jitter makes that every vertex)
        srt = np.partition(M[has], 1, axis=1)[:, :2]
        clear = srt[:, 1] > srt[:, 0] * (1 + K_CHOICE * U)
        assert clear.all() and np.array_equal(near[b][has], M[has].argmin(1))
        n_inside += int(rin.sum())
    assert n_inside > 0
    return worst


# ---- values, choice, determinism ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("kind", list(CASES))
def test_forward_against_the_oracle_pruned_and_plain(kind, B):
    _, e, det = run(kind, B)
    worst = check_forward(kind, B, e, det)
    print("penetration %s B=%d: choice observed / bar = %.3f" % (kind, B, worst))
    _, e2, det2 = run(kind, B)                                                     # a second launch: the same bits
    with unpruned():
        _, e3, det3 = run(kind, B)
    for other_e, other in ((e2, det2), (e3, det3)):
        assert torch.equal(bits(e), bits(other_e))
        for k in det:
            assert torch.equal(bits(det[k]), bits(other[k])), k


@pytest.mark.parametrize("kind", ["v84", "v257", "v513", "p31"])
def test_gradient_teacher_forced_and_batch_independent(kind):
    B = 3
    verts, faces, part, collide = mesh(kind, B)
    g = np.random.default_rng(9).normal(size=verts.shape[:2]).astype(np.float32)
    V, e, det = run(kind, B, grad=True)
    e.backward(t(g))
    got = V.grad.cpu().numpy()
    near, inside = det["near"].cpu().numpy(), det["inside"].cpu().numpy()
    for b in range(B):
        dv, T = orc.grads(verts[b], near[b], inside[b], g[b])
        assert np.abs(dv).max() > 0
        assert (np.abs(got[b] - dv) <= U * np.abs(dv) + 2.0 ** -28 * T).all()
    V2, e2, _ = run(kind, B, grad=True)                                            # two launches agree bit for bit
    e2.backward(t(g))
    assert torch.equal(bits(V.grad), bits(V2.grad))
    with unpruned():
        V3, e3, _ = run(kind, B, grad=True)
        e3.backward(t(g))
    assert torch.equal(bits(V.grad), bits(V3.grad))
    for b in range(B):                                                             # B = 3 equals three B = 1 launches
        V1, e1, d1 = run(kind, 1, grad=True, verts=verts[b:b + 1])
        e1.backward(t(g[b:b + 1]))
        assert torch.equal(bits(e1[0]), bits(e[b])) and torch.equal(bits(V1.grad[0]), bits(V.grad[b]))
        for k in ("d2", "near", "inside"):
            assert torch.equal(bits(d1[k][0]), bits(det[k][b])), k


def test_exact_ties_name_the_lower_index():
    """Mirror pairs +-p around a query at the origin: their fp32 squared distances are equal to the bit.  The nearest pair is
    (57, 200) with the part-major walk meeting 200 first (part 1) and 57 second (part 2), and (58, 201) the other way round
    for a second query; both walks name the lower index."""
    from ilps_amd.penetration import self_penetration
    from ilps_amd.render import MeshTopology
    rng = np.random.default_rng(4)
    V = 300
    v = rng.normal(size=(V, 3))
    v = v / np.linalg.norm(v, axis=1, keepdims=True) * rng.uniform(2.0, 3.0, (V, 1))
    part = np.where(np.arange(V) % 2 == 0, 1, 2)
    p = np.array([0.5, -0.25, 0.125])
    v[0], part[0] = 0.0, 0
    v[200], part[200], v[57], part[57] = p, 1, -p, 2
    q = np.array([8.0, 0.0, 0.0])
    v[1], part[1] = q, 0
    v[58], part[58], v[201], part[201] = q + p, 1, q - p, 2
    topo = MeshTopology(np.zeros((0, 3), np.int32), V)
    topo.vertex_part = part
    collide = 1 - np.eye(3, dtype=np.uint8)
    ref = orc.self_penetration(v.astype(np.float32), np.zeros((0, 3), int), part, collide)
    assert ref["near"][0] == 57 and ref["near"][1] == 58
    for ctx in (contextlib.nullcontext(), unpruned()):
        with ctx:
            _, det = self_penetration(t(v[None]), topo, collide, return_details=True)
        assert det["near"][0, 0] == 57 and det["near"][0, 1] == 58
        assert np.array_equal(det["near"][0].cpu().numpy(), ref["near"])


# ---- hostile rows -----------------------------------------------------------------------------------------------------

def test_hostile_rows():
    from ilps_amd import penetration
    from ilps_amd.penetration import self_penetration
    from ilps_amd.render import MeshTopology
    kind, B = "v257", 3
    verts, faces, part, collide = mesh(kind, B)
    topo = topology(kind)

    def go(vs, topo=topo, table=collide):
        V = t(vs).requires_grad_(True)
        e, det = self_penetration(V, topo, table, return_details=True)
        e.backward(torch.where(torch.isnan(e), torch.zeros_like(e), torch.full_like(e, 1.5)))
        return {"e": e.detach(), **det, "dverts": V.grad}
    clean = go(verts)
    assert clean["inside"].any()
    # a NaN vertex in mesh 1 of 3
    bad = verts.copy()
    bad[1, 17, 2] = np.nan
    out = go(bad)
    assert out["status"].tolist() == [0, penetration.NONFINITE, 0]
    for k in ("e", "d2", "dverts"):
        assert torch.isnan(out[k][1]).all(), k
    assert (out["near"][1] == -1).all() and not out["inside"][1].any()
    for k in clean:
        for b in (0, 2):
            assert torch.equal(bits(out[k][b]), bits(clean[k][b])), "mesh %d is not bit-equal to the clean batch in %s" % (b, k)
    bad = verts.copy()
    bad[0, 0, 0] = np.inf
    assert go(bad)["status"].tolist() == [penetration.NONFINITE, 0, 0]
    # part ids outside -1 .. P - 1 count as -1
    wild = part.copy()
    wild[part == 2] = 40
    wild[part == 4] = -7
    topo_w = MeshTopology(faces, len(part))
    topo_w.vertex_part = wild
    out = go(verts, topo_w)
    near = out["near"].cpu().numpy()
    for b in range(B):
        ref = orc.self_penetration(verts[b], faces, wild, collide)
        assert np.array_equal(near[b], ref["near"]) and np.array_equal(out["inside"][b].cpu().numpy(), ref["inside"])
        assert (near[b][(part == 2) | (part == 4)] == -1).all() and not np.isin(part[near[b][near[b] >= 0]], (2, 4)).any()
    # an empty table, and a table without parts
    for table in (np.zeros_like(collide), np.zeros((0, 0), np.uint8)):
        out = go(verts, table=table)
        assert (out["near"] == -1).all() and torch.isinf(out["d2"]).all() and (out["d2"] > 0).all()
        assert (out["e"] == 0).all() and (out["dverts"] == 0).all() and out["status"].tolist() == [0, 0, 0]


# ---- full size, the chain through the SMPL layer ---------------------------------------------------------------------------

def test_full_size_forward_and_backward():
    """uv_sphere() at SMPL's counts with the package's UP-S31 part tables (every pair of distinct parts collides), B = 1, one
    forward and one backward against the oracle: sizes only (27 tiles, 27 workgroups, 31 parts)."""
    from ilps_amd.penetration import part_collision_table, self_penetration
    from ilps_amd.render import MeshTopology
    v, f = uv_sphere()
    rng = np.random.default_rng(6)
    v = ((v + rng.normal(0, 1e-3, v.shape)) * np.array([0.3, 0.9, 0.25])).astype(np.float32)
    topo = MeshTopology(f, 6890)
    collide = part_collision_table(topo, 0)
    assert collide.shape == (31, 31) and collide.sum() == 31 * 30
    V = t(v[None]).requires_grad_(True)
    e, det = self_penetration(V, topo, collide, return_details=True)
    g = rng.normal(size=6890).astype(np.float32)
    e.backward(t(g[None]))
    ref = orc.self_penetration(v, f, topo.vertex_part, collide)
    near, inside = det["near"][0].cpu().numpy(), det["inside"][0].cpu().numpy()
    rd2, _, rin, re = orc.at(v, f, near)
    has = near >= 0
    assert np.array_equal(has, ref["near"] >= 0) and has.sum() > 6000
    assert (rd2[has] <= ref["d2"][has] * (1 + K_CHOICE * U)).all() and (near == ref["near"]).mean() > 0.99
    assert np.array_equal(inside, rin) and (np.abs(e[0].detach().cpu().numpy() - re) <= U * re).all()
    dv, T = orc.grads(v, near, inside, g)
    assert (np.abs(V.grad[0].cpu().numpy() - dv) <= U * np.abs(dv) + 2.0 ** -28 * T).all()
    with unpruned():
        e2, det2 = self_penetration(V.detach(), topo, collide, return_details=True)
    assert torch.equal(bits(e2), bits(e.detach())) and torch.equal(det2["near"], det["near"])


@pytest.fixture(scope="module")
def layer(smpl_model):
    from ilps_amd.keras_smpl.batch_smpl import SMPLLayer
    return SMPLLayer(smpl_model)


def test_chain_through_the_smpl_layer(layer, smpl_model):
    """d (sum g e) / dx through SMPLLayer -> self_penetration against the float64 SMPL oracle chained with the penetration
    oracle, under test_smpl_backward's bars.  g is 1 on the vertices whose choice and sign are clear in float64 (the runner-up
    farther by 1e-6 relative, |s| above 1e-9 of |d| |n|) and 0 elsewhere, so the oracle on its float64 vertices and the op on
    the layer's fp32 vertices name the same near and inside wherever the gradient looks.
    The energy does not change under a rigid motion, so its derivative by the global rotation theta[0:3] vanishes up to what
    the model's blend terms leave (1e-6 here, against 1e-1 and more in the other columns): a sum of large terms that cancel.
    `grad_close`'s per-column scale is the column's own RMS and is no scale for such a column (its docstring says so of
    per-vertex tensors), so test_smpl_backward's bars are applied per column to the body pose theta[3:72] and to beta, and to
    all of dtheta, these three columns included, with the tensor's RMS as the scale (per_column=False) - the same rtol and
    atol.  Observed on an MI355X: the three columns differ from the oracle by 1.4e-5 at most."""
    from _inputs import make_x
    from oracle.torch_oracle import TorchSMPL
    from test_gpu_parity import grad_close
    from test_gpu_scan import body_topology
    from ilps_amd.penetration import self_penetration
    topo, f = body_topology()
    part = topo.vertex_part
    collide = np.zeros((31, 31), np.uint8)
    collide[:8, 8:16] = collide[8:16, :8] = 1                      # sixteen parts in two camps: a quarter of the pair matrix
    x = make_x(1, 48, seed=11)
    xo = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    vo = TorchSMPL(smpl_model)(xo, return_all=True)[0]
    v64 = vo.detach().numpy()[0]
    M = orc.pair_d2(v64, part, collide)
    srt = np.partition(M, 1, axis=1)[:, :2]
    r = {"near": np.where(np.isfinite(srt[:, 0]), M.argmin(1), -1)}
    r["d2"], r["s"], r["inside"], _ = orc.at(v64, f, r["near"])
    nrm = np.zeros(6890)
    vf = orc.csr(f, 6890)
    for i in np.nonzero(r["near"] >= 0)[0]:
        nrm[i] = np.linalg.norm(orc.normal(v64, f, r["near"][i], vf))
    has = r["near"] >= 0
    clear = has & (srt[:, 1] > srt[:, 0] * (1 + 1e-6)) & (np.abs(r["s"]) > 1e-9 * np.sqrt(np.where(has, r["d2"], 0.0)) * nrm)
    g = clear.astype(np.float32)
    assert (clear & r["inside"]).sum() > 50
    dv, _ = orc.grads(v64, r["near"], r["inside"], g)
    (vo[0] * torch.tensor(dv)).sum().backward()
    xg = t(x).requires_grad_(True)
    e, det = self_penetration(layer(xg), topo, collide, return_details=True)
    e.backward(t(g[None]))
    assert np.array_equal(det["near"][0].cpu().numpy()[clear], r["near"][clear])
    assert np.array_equal(det["inside"][0].cpu().numpy()[clear], r["inside"][clear])
    got, want = xg.grad.cpu().numpy(), xo.grad.numpy()
    assert np.all(got[:, :4] == 0)
    print("chain: |dtheta| rms %.3e, global rotation columns: want %s, |got - want| %s"
          % (np.sqrt(np.mean(want[:, 4:76] ** 2)), want[0, 4:7].tolist(), np.abs(got - want)[0, 4:7].tolist()))
    grad_close(got[:, 7:76], want[:, 7:76], name="dtheta[3:72]")
    grad_close(got[:, 4:76], want[:, 4:76], name="dtheta", per_column=False)
    grad_close(got[:, 76:], want[:, 76:], name="dbeta")


# ---- behaviour ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("where", ["gpu", "cpu"])
def test_adam_separates_two_overlapping_spheres(where):
    """Two unit spheres 5 / 3 apart, the second sphere's translation the only unknown: 200 steps of torch's Adam on e.sum()
    take the energy to exactly 0, where it stays (no gradient, and what momentum is left moves the spheres further apart)."""
    from ilps_amd.penetration import self_penetration
    from ilps_amd.render import MeshTopology
    v, f = uv_sphere(8, 5)
    device = dev() if where == "gpu" else torch.device("cpu")
    base = torch.as_tensor(np.concatenate([v, v + np.array([5.0 / 3.0, 0.1, 0.05])])[None], dtype=torch.float32, device=device)
    topo = MeshTopology(np.concatenate([f, f + 42]), 84)
    topo.vertex_part = np.repeat([0, 1], 42)
    second = torch.cat([torch.zeros(42), torch.ones(42)]).to(device)[None, :, None]
    shift = torch.zeros(3, device=device, requires_grad=True)
    opt = torch.optim.Adam([shift], lr=0.02)
    energy = []
    for _ in range(200):
        opt.zero_grad()
        E = self_penetration(base + second * shift, topo).sum()
        E.backward()
        opt.step()
        energy.append(float(E.detach()))
    print("two spheres (%s): energy %.4f -> %.4f, first zero at step %d, shift %s"
          % (where, energy[0], energy[-1], energy.index(0.0) if 0.0 in energy else -1, shift.tolist()))
    assert energy[0] > 0 and energy[-1] == 0.0
    first = energy.index(0.0)
    assert all(x == 0.0 for x in energy[first:])


def test_evaluate_penetration_equals_the_sums_by_hand():
    from ilps_amd.evaluation import evaluate_penetration
    kind, B = "v513", 3
    verts, _, _, collide = mesh(kind, B)
    _, e, det = run(kind, B)
    res = evaluate_penetration(t(verts), topology(kind), collide)
    cnt = det["inside"].sum(1)
    depth = torch.where(det["inside"], det["d2"].double(), torch.zeros((), dtype=torch.float64, device=dev())).sqrt().amax(1)
    assert torch.equal(res["inside"], cnt) and torch.equal(res["max_depth"], depth)
    assert res["total_inside"] == int(cnt.sum()) > 0 and res["max_depth_overall"] == float(depth.max()) > 0
    assert res["count"] == 3 and res["nonfinite"] == 0 and res["meshes_with_penetration"] == int((cnt > 0).sum())


# ---- the fitters -----------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def param_case(smpl_model):
    """A ParamFitter with the term (the model carries no faces: the soup of test_gpu_scan.body_topology, every pair of
    distinct parts colliding), one without it that shares its constants, labels and a start."""
    import importlib.util
    from test_gpu_scan import body_topology
    from ilps_amd.fitting import ParamFitter
    spec = importlib.util.spec_from_file_location("fit_time", os.path.join(ROOT, "tools", "fit_time.py"))
    fit_time = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fit_time)
    topo, _ = body_topology()
    with_pen = ParamFitter(smpl_model, img_wh=48, deterministic=True, penetration=topo)
    plain = ParamFitter(smpl_model, img_wh=48, deterministic=True)
    labels, x0, _ = fit_time.problem(plain, 3, 48, seed=0, pose_sigma=0.05, cam_shift=1.5)
    return with_pen, plain, labels, x0


def test_param_fitter_refuses_what_the_term_cannot_use(smpl_model):
    from test_gpu_scan import body_topology
    from ilps_amd.fitting import ParamFitter
    with pytest.raises(ValueError, match="vertex_sampling"):
        ParamFitter(smpl_model, penetration=body_topology()[0], vertex_sampling=5)
    with pytest.raises(ValueError, match="no faces"):
        ParamFitter(smpl_model, penetration=True)
    with pytest.raises(ValueError, match="pen_weight"):
        ParamFitter(smpl_model).fit(torch.zeros((1, 48, 48), dtype=torch.int32, device=dev()), steps=1, pen_weight=1.0)


def test_param_fitter_one_iteration_is_the_hand_written_composition(param_case):
    from ilps_amd.fitting import FitState, fit_step
    from ilps_amd.penetration import self_penetration
    fitter, _, labels, x0 = param_case
    w, B, N, V = 30.0, 3, 48 * 48, 6890
    r = fitter.fit(labels, init=x0, steps=1, lr=1e-2, history=True, pen_weight=w)
    state = FitState.new(x0)
    x = state.x.detach().requires_grad_(True)
    out = fitter.decoder(x, labels.to(torch.int32).reshape(B, 48, 48))
    e = self_penetration(out["verts"], fitter.pen_topo, fitter.pen_collide)
    assert float(e.detach().sum()) > 0
    (g,) = torch.autograd.grad([out["seg_loss"], e], [x], grad_outputs=[torch.full((B, N), 1.0 / N, device=dev()),
                                                                       torch.full((B, V), w / V, device=dev())])
    loss = out["seg_loss"].detach() + (torch.full((1,), w, device=dev()) * e.detach().mean(1))[:, None]
    hist = torch.empty((1, B), device=dev())
    fit_step(state, g.contiguous(), loss, None, 1.0, None, hist, lr=1e-2)
    assert torch.equal(bits(r.final_x), bits(state.x)) and torch.equal(bits(r.history), bits(hist))
    assert torch.equal(bits(r.loss), bits(state.best_loss)) and torch.equal(bits(r.state.m), bits(state.m))
    assert not torch.equal(r.final_x, x0) and torch.equal(bits(fitter.losses(x0, labels, pen_weight=w)), bits(hist[0]))


def test_param_fitter_replay_stage_weights_and_weight_zero(param_case):
    from ilps_amd.fitting import column_scale
    fitter, plain, labels, x0 = param_case
    cs = column_scale(cam=10.0, pose=1.0, shape=0.0)
    stages = [(5, cs), (6, cs)]
    kw = dict(init=x0, stages=stages, lr=1e-2, history=True)
    a = fitter.fit(labels, pen_weight=[0.0, 40.0], **kw)
    b = fitter.fit(labels, pen_weight=[0.0, 40.0], graph=True, graph_steps=2, **kw)
    for k in ("final_x", "history", "x", "loss"):
        assert torch.equal(bits(getattr(a, k)), bits(getattr(b, k))), k
    assert torch.equal(a.step, b.step)
    # the weights take effect under replay: another second-stage weight changes the second stage's losses only
    c = fitter.fit(labels, pen_weight=[0.0, 5.0], graph=True, graph_steps=2, **kw)
    assert torch.equal(bits(c.history[:5]), bits(b.history[:5])) and (c.history[5] < b.history[5]).all()
    # a stage with weight 0 records the loss bits of the term-free sum
    p = plain.fit(labels, **kw)
    assert torch.equal(bits(a.history[0]), bits(p.history[0]))
    assert torch.equal(bits(a.history[0]), bits(plain.losses(x0, labels)))
    assert torch.equal(bits(fitter.losses(x0, labels, pen_weight=0.0)), bits(p.history[0]))


def test_scan_fitter_with_the_term():
    from test_gpu_scan import FIT_KW, fit_case
    from ilps_amd.fitting import FitState, ScanFitter, fit_step
    from ilps_amd.penetration import self_penetration
    from ilps_amd.scan import surface_distance
    full, pts, x0 = fit_case()
    fitter = ScanFitter(full.layer, full.topo, penetration=True)
    w, B, N, V = 20.0, 2, 512, 6890
    r = fitter.fit(pts, init=x0, steps=1, history=True, pen_weight=w, **FIT_KW)
    state = FitState.new(x0)
    x = state.x.detach().requires_grad_(True)
    verts = x[:, 0, None, None] * fitter.layer(x) + x[:, None, 1:4]
    out = surface_distance(verts, fitter.topo, pts)
    e = self_penetration(verts, fitter.topo)
    assert float(e.detach().sum()) > 0
    f32 = lambda n, val: torch.full((B, n), val, device=dev())
    (g,) = torch.autograd.grad([out["d2"], out["vd2"], e], [x], grad_outputs=[f32(N, 1.0 / N), f32(V, 1.0 / V), f32(V, w / V)])
    loss = out["d2"].detach() + (torch.full((1,), w, device=dev()) * e.detach().mean(1))[:, None]
    hist = torch.empty((1, B), device=dev())
    fit_step(state, g.contiguous(), loss, out["vd2"].detach(), 1.0, None, hist, lr=FIT_KW["lr"], mode=FIT_KW["mode"])
    assert torch.equal(bits(r.final_x), bits(state.x)) and torch.equal(bits(r.history), bits(hist))
    assert torch.equal(bits(fitter.losses(x0, pts, pen_weight=w)), bits(hist[0]))
    # replay equals eager, and the stage weights take effect under replay
    kw = dict(init=x0, stages=[(4, torch.ones(86)), (5, torch.ones(86))], history=True, **FIT_KW)
    a = fitter.fit(pts, pen_weight=[0.0, w], **kw)
    b = fitter.fit(pts, pen_weight=[0.0, w], graph=True, graph_steps=2, **kw)
    assert torch.equal(bits(a.final_x), bits(b.final_x)) and torch.equal(bits(a.history), bits(b.history))
    p = full.fit(pts, **kw)
    assert torch.equal(bits(a.history[0]), bits(p.history[0])) and (a.history[4] > p.history[4]).all()
