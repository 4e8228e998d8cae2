"""smplr_offset_step (csrc/fit.hip, through `fitting.offset_step`) and `fitting.OffsetFitter` on the GPU.

smplr_offset_step against a float64 Adam (tests/_meshreg_oracle.adam) in both modes over 3 steps at n = 3, 769 and 3 x 6 890.
The bar is propagated through the steps from the update's operation count, U = 2^-24 (csrc/fit.hip: m takes 3 roundings, v 4,
the step at most 13):
    err_m(t)  = beta1 err_m(t-1) + 3 U (beta1 |m| + (1 - beta1) |g|)           (m may cancel: an absolute bound)
    rel_v(t)  = rel_v(t-1) + 4 U                                                 (v sums non-negative terms: a relative one)
    err_q     = err_m / den + |m / den| (rel_v / 2 + 13 U)                       q = m / den, den = sqrt(v) [/ sqrt(c2)] + eps
    err_D(t)  = err_D(t-1) + step err_q + U |D|                                  D -= step q, one more rounding
so a few ulps of m, v and of the moved D per step.  A row with a non-finite loss keeps the bits of D, m, v, t and counts in
bad; a replayed graph gives the eager bits.

OffsetFitter: the target is the model at x plus a smooth 1 cm bump along the vertex normals of one body part, the scan is
`sample_surface` of the target, the fit starts from D = 0 with x fixed.  Asserted is the direction only - the last recorded
loss below the first, the mean vertex error to the target below the error of D = 0 - plus: the first iteration is the
hand-written composition of the ops, bit for bit; two fits from the same start are bit-equal; a replayed graph gives the
eager bits; with fit_params x moves through `fit_step`.  The ratios reached are printed (FIT lines)."""
import functools

import numpy as np
import pytest
import torch

import _meshreg_oracle as mo
import _render_oracle as ro
from test_gpu_parity import dev, t

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
ADAM = dict(lr=1e-2, beta1=0.9, beta2=0.999, eps=1e-7)


@functools.lru_cache(maxsize=None)
def adam_case(n, mode, B=3, steps=3):
    """D0 and one gradient per step (fp32, read-only; a tenth of the entries have a zero gradient throughout), the float64
    trajectory and the propagated bars after every step."""
    rng = np.random.default_rng(n + len(mode))
    D0 = rng.normal(0, 0.05, (B, n)).astype(np.float32)
    still = rng.uniform(size=(B, n)) < 0.1
    gs = [np.where(still, 0, rng.normal(0, 0.02, (B, n))).astype(np.float32) for _ in range(steps)]
    D, m, v = D0.astype(np.float64), np.zeros((B, n)), np.zeros((B, n))
    err_m, rel_v, err_D = np.zeros((B, n)), 0.0, np.zeros((B, n))
    traj = []
    # (the kernel's scalars are the fp32 values of these: 1 - fl32(0.999) is 500 ulps from 0.001)
    b1, b2, eps, lr = (float(np.float32(ADAM[k])) for k in ("beta1", "beta2", "eps", "lr"))
    for k, g in enumerate(gs):
        g = g.astype(np.float64)
        err_m = b1 * err_m + 3 * U * (b1 * np.abs(m) + (1 - b1) * np.abs(g))
        rel_v = rel_v + 4 * U
        D, m, v, _ = mo.adam(D, g, m, v, k, lr, b1, b2, eps, mode)
        c1, c2 = 1 - b1 ** (k + 1), 1 - b2 ** (k + 1)
        den = np.sqrt(v) + eps if mode == "keras" else np.sqrt(v) / np.sqrt(c2) + eps
        step = lr * np.sqrt(c2) / c1 if mode == "keras" else lr / c1
        err_q = err_m / den + np.abs(m / den) * (rel_v / 2 + 13 * U)
        err_D = err_D + np.where(m != 0, step * err_q + U * np.abs(D), 0.0)
        traj.append(dict(D=D.copy(), m=m.copy(), v=v.copy(), err_D=err_D.copy(), err_m=err_m.copy(), rel_v=rel_v))
    for a in [D0] + gs:
        a.setflags(write=False)
    return D0, gs, still, traj


def device_state(D0):
    B = D0.shape[0]
    D = t(np.array(D0))
    return D, torch.zeros_like(D), torch.zeros_like(D), torch.zeros(B, dtype=torch.int32, device=dev()), \
        torch.zeros(B, dtype=torch.int32, device=dev())


@pytest.mark.parametrize("mode", ["keras", "torch"])
@pytest.mark.parametrize("n", [3, 769, 3 * 6890])
def test_offset_step_against_float64_adam(n, mode):
    from ilps_amd.fitting import offset_step
    D0, gs, still, traj = adam_case(n, mode)
    D, m, v, tt, bad = device_state(D0)
    loss = torch.ones(D0.shape[0], device=dev())
    for k, g in enumerate(gs):
        offset_step(D, t(np.array(g)), m, v, tt, bad, loss, mode=mode, **ADAM)
        torch.cuda.synchronize()
        r = traj[k]
        for name, got, ref, bar in (("D", D, r["D"], r["err_D"]), ("m", m, r["m"], r["err_m"]), ("v", v, r["v"], r["rel_v"] * r["v"])):
            err = np.abs(got.cpu().numpy().astype(np.float64) - ref)
            worst = float((err / np.maximum(bar, 1e-300)).max())
            print("ADAM n=%d %s step %d %s: error / bar %.3f" % (n, mode, k + 1, name, worst))
            assert np.all(err <= bar), (name, k, worst)
        assert (tt == k + 1).all() and (bad == 0).all()
    # an entry whose gradient was zero throughout has m = 0 and was never stored to
    assert np.array_equal(D.cpu().numpy()[still], D0[still])


@pytest.mark.parametrize("mode", ["keras", "torch"])
def test_offset_step_bad_row_and_graph_replay(mode):
    from ilps_amd.fitting import offset_step
    n = 769
    D0, gs, _, _ = adam_case(n, mode)
    # eager, all rows good
    De, me, ve, te, bade = device_state(D0)
    good = torch.ones(3, device=dev())
    for g in gs:
        offset_step(De, t(np.array(g)), me, ve, te, bade, good, mode=mode, **ADAM)
    # row 1 meets a non-finite loss at the second step: it keeps its bits there and is one update behind afterwards
    D, m, v, tt, bad = device_state(D0)
    for k, g in enumerate(gs):
        loss = torch.ones(3, device=dev())
        if k == 1:
            loss[1] = float("nan")
            before = [a[1].clone() for a in (D, m, v, tt)]
        offset_step(D, t(np.array(g)), m, v, tt, bad, loss, mode=mode, **ADAM)
        if k == 1:
            torch.cuda.synchronize()
            assert all(torch.equal(a[1], b) for a, b in zip((D, m, v, tt), before))
            assert bad.tolist() == [0, 1, 0]
    for a, b in ((D, De), (m, me), (v, ve)):
        assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2]) and not torch.equal(a[1], b[1])
    assert tt.tolist() == [3, 2, 3] and bad.tolist() == [0, 1, 0]
    loss = torch.full((3,), float("inf"), device=dev())
    keep = D.clone()
    offset_step(D, t(np.array(gs[0])), m, v, tt, bad, loss, mode=mode, **ADAM)
    assert torch.equal(D, keep) and bad.tolist() == [1, 2, 1] and tt.tolist() == [3, 2, 3]
    # a captured launch replays to the eager bits
    Dg, mg, vg, tg, badg = device_state(D0)
    gbuf = t(np.array(gs[0]))
    side = torch.cuda.Stream(device=dev())
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        scratch = [a.clone() for a in (Dg, mg, vg, tg, badg)]
        offset_step(scratch[0], gbuf, scratch[1], scratch[2], scratch[3], scratch[4], good, mode=mode, **ADAM)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        offset_step(Dg, gbuf, mg, vg, tg, badg, good, mode=mode, **ADAM)
    for g in gs:
        gbuf.copy_(t(np.array(g)))
        graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(Dg, De) and torch.equal(mg, me) and torch.equal(vg, ve) and torch.equal(tg, te)


def test_offset_step_refuses_bad_arguments():
    from ilps_amd.fitting import offset_step
    D, m, v, tt, bad = device_state(np.zeros((2, 5, 3), np.float32))
    loss = torch.ones(2, device=dev())
    g = torch.zeros_like(D)
    with pytest.raises(ValueError):
        offset_step(D, g, m, v, tt, bad, loss, mode="sgd")
    with pytest.raises(RuntimeError):
        offset_step(D, g[:, :4], m, v, tt, bad, loss)
    with pytest.raises(RuntimeError):
        offset_step(D, g, m, v, tt.long(), bad, loss)
    with pytest.raises(RuntimeError):
        offset_step(D, g, m, v, tt, bad, loss[:1])
    with pytest.raises(RuntimeError):
        offset_step(D.cpu(), g.cpu(), m.cpu(), v.cpu(), tt.cpu(), bad.cpu(), loss.cpu())
    with pytest.raises(RuntimeError):
        offset_step(D, g, m, v, tt, bad, loss, beta1=1.0)


# ---------------------------------------------------------------------------------------------------------- OffsetFitter
B, N, V = 2, 4096, 6890
PART = 9
FIT = dict(lr=2e-4, lap_weight=0.1, edge_weight=1e-6, offset_weight=1e-3, mode="torch")


@functools.lru_cache(maxsize=None)
def fit_case():
    """The fitters, the spec, x (B, 86), the target vertices, its scan and the D = 0 vertices, all on the device."""
    from ilps_amd.fitting import OffsetFitter, ScanFitter
    from ilps_amd.keras_smpl.batch_smpl import SMPLLayer
    from ilps_amd.meshreg import MeshRegSpec
    from ilps_amd.render import MeshTopology
    from ilps_amd.scan import sample_surface
    model, part_of = mo.surface_model()
    faces = model.faces
    topo = MeshTopology(faces, V)
    rng = np.random.default_rng(31)
    x = np.zeros((B, 86))
    x[:, 4:76] = rng.normal(0, 0.03, (B, 72))
    x[:, 0] = 1.0
    x = t(x.astype(np.float32))
    sf = ScanFitter(SMPLLayer(model), topo, directions=("p2m",))
    spec = MeshRegSpec(topo, model.v_template, "cotangent")
    with torch.no_grad():
        base = sf.place(x)
    part = np.nonzero(part_of == PART)[0]
    bump = np.zeros((B, V, 3))
    for b in range(B):
        v = base[b].cpu().numpy().astype(np.float64)
        nrm = ro.vertex_normals(v, faces)
        c = v[part[0]]
        r2 = ((v[part] - c) ** 2).sum(1)
        bump[b, part] = 0.01 * np.exp(-r2 / (2 * 0.15 ** 2))[:, None] * nrm[part]
    target = base + t(bump.astype(np.float32))
    pts, _, _ = sample_surface(target, topo, N, torch.Generator(device=dev()).manual_seed(9))
    return OffsetFitter(sf, spec), sf, spec, x, target, pts.contiguous(), base


def test_offset_fitter_moves_towards_the_target():
    fitter, sf, spec, x, target, pts, base = fit_case()
    r = fitter.fit(pts, None, x, steps=40, history=True, **FIT)
    assert r.steps == 40 and (r.bad == 0).all() and (r.t == 40).all() and torch.equal(r.x, x) and r.state is None
    h = r.history
    assert tuple(h.shape) == (40, B) and bool(torch.isfinite(h).all())
    with torch.no_grad():
        got = sf.place(x, r.offsets)
    e0 = (base - target).norm(dim=2).mean(1)
    e1 = (got - target).norm(dim=2).mean(1)
    print("FIT loss first %s last %s ratio %s" % (h[0].tolist(), h[-1].tolist(), (h[-1] / h[0]).tolist()))
    print("FIT mean vertex error D = 0 %s, fitted %s, ratio %s" % (e0.tolist(), e1.tolist(), (e1 / e0).tolist()))
    assert bool((h[-1] < h[0]).all()), "the loss did not fall"
    assert bool((e1 < e0).all()), "the fitted surface is no closer to the target than D = 0"
    # two fits from the same start: the same bits
    r2 = fitter.fit(pts, None, x, steps=40, history=True, **FIT)
    assert torch.equal(r2.offsets, r.offsets) and torch.equal(r2.history, r.history)


def test_first_iteration_is_the_hand_written_composition():
    from ilps_amd.fitting import offset_step
    from ilps_amd.meshreg import mesh_regularisers
    from ilps_amd.scan import surface_distance
    fitter, sf, spec, x, target, pts, base = fit_case()
    r = fitter.fit(pts, None, x, steps=1, history=True, **FIT)
    D = torch.zeros(B, V, 3, device=dev())
    m, v = torch.zeros_like(D), torch.zeros_like(D)
    tt, bad = torch.zeros(B, dtype=torch.int32, device=dev()), torch.zeros(B, dtype=torch.int32, device=dev())
    wts = torch.tensor([FIT["lap_weight"], FIT["edge_weight"], FIT["offset_weight"]], dtype=torch.float32).to(dev())
    Dg = D.detach().requires_grad_(True)
    verts = x[:, 0, None, None] * sf.layer(x, offsets=Dg) + x[:, None, 1:4]
    out = surface_distance(verts, sf.topo, pts, None, ("p2m",))
    L = out["d2"].sum(1) / float(N)
    template = torch.as_tensor(np.asarray(sf.layer._model.v_template), dtype=torch.float32).reshape(1, V, 3).to(dev())
    reg = mesh_regularisers(template + Dg, spec, return_terms=True)
    L = L + wts[0] * reg[:, 0] + wts[1] * reg[:, 1] + wts[2] * ((Dg * Dg).sum((1, 2)) / float(V))
    (g,) = torch.autograd.grad(L.sum(), [Dg])
    offset_step(D, g.contiguous(), m, v, tt, bad, L.detach().contiguous(), lr=FIT["lr"], mode=FIT["mode"])
    torch.cuda.synchronize()
    bits = lambda a: a.view(torch.int32)
    assert torch.equal(bits(r.offsets), bits(D)) and torch.equal(bits(r.history[0]), bits(L.detach()))
    assert bool(D.any()) and r.t.tolist() == [1, 1]


def test_graph_replay_and_fit_params():
    fitter, sf, spec, x, target, pts, base = fit_case()
    eager = fitter.fit(pts, None, x, steps=4, history=True, **FIT)
    graph = fitter.fit(pts, None, x, steps=4, history=True, graph=True, **FIT)
    assert torch.equal(graph.offsets, eager.offsets) and torch.equal(graph.history, eager.history) and (graph.t == 4).all()
    # per-stage weights: two stages of two steps with the same weights are the four steps
    kw = dict(FIT, lap_weight=[FIT["lap_weight"]] * 2, offset_weight=[FIT["offset_weight"]] * 2)
    staged = fitter.fit(pts, None, x, stages=[(2, torch.ones(86)), (2, torch.ones(86))], history=True, **kw)
    assert torch.equal(staged.offsets, eager.offsets) and torch.equal(staged.history, eager.history)
    with pytest.raises(ValueError):
        fitter.fit(pts, None, x, stages=[(2, torch.ones(86))], **kw)            # two weights for one stage
    both = fitter.fit(pts, None, x, steps=4, history=True, fit_params=True, x_lr=1e-3, **FIT)
    assert both.state is not None and not torch.equal(both.x, x) and bool(torch.isfinite(both.x).all())
    assert torch.equal(both.history[0], eager.history[0]) and (both.bad == 0).all()
    with pytest.raises(ValueError):
        fitter.fit(pts, None, x, steps=2, pen_weight=1.0, **FIT)
    with pytest.raises(ValueError):
        fitter.fit(pts, None, x[:, :85], steps=2, **FIT)


def test_evaluate_registration():
    from ilps_amd.evaluation import evaluate_registration
    fitter, sf, spec, x, target, pts, base = fit_case()
    ev = evaluate_registration(target, sf.topo, pts, None, spec)
    # the scan was sampled from the target: its points lie on the surface up to fp32 rounding of the sample
    assert bool((ev["scan_to_mesh"] < 1e-5).all()) and ev["nonfinite"] == 0
    assert tuple(ev["e_lap"].shape) == (B,) and tuple(ev["e_edge"].shape) == (B,) and bool((ev["mesh_to_scan"] > 0).all())
    off = evaluate_registration(base, sf.topo, pts, None, spec)
    assert bool((off["scan_to_mesh"] > ev["scan_to_mesh"]).all())
