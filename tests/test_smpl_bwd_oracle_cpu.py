"""The float64 reference of the fused SMPL backward (tests/_smpl_bwd_oracle.py) checked WITHOUT a GPU:

  * the staged dx (skinning, blend GEMM, pose: three restatements chained by a per-mesh Jacobian) equals float64
    autograd through TorchSMPL + orthographic_project to 1e-12 of its magnitude, at every (V, vertex sampling) of
    test_gpu_smpl_bwd_small.py;
  * the same chain in FLOAT32 arithmetic (TorchSMPL(float32) for the pose part, fp32 running sums for the skinning sums,
    test_gpu_blend_small.py's emulations for the GEMM) lands inside the GPU file's bars at every case, both GEMMs, both
    weight tables: the reference alone leaves room (the worst error / bar is printed);
  * the bars, loose as they are at large V, still catch a wrong term: six mutated references each leave an entry of dx
    outside the bar at every shape;
  * the hand-built slot layouts are what they claim: live records per 1 024-vertex chunk, the slot windows touched, the
    exactly-zero fp32 block sums of the dead records."""
import functools

import numpy as np
import pytest
import torch

import _smpl_bwd_oracle as so
from _smpl_bwd_oracle import CASES, CASE_IDS, Case, U

VVS = [(V, vs) for V in so.SHAPES for vs in (1, 3)]


def _live(V, vs, cap):
    return tuple(min(cap, so.sampled_in_chunk(V, vs, c)) for c in range(so.nchunk(V)))


# ------------------------------------------------------------------------------------ 1. staged == independent autograd
@pytest.mark.parametrize("V,vs", VVS)
def test_staged_dx_equals_autograd_through_the_whole_layer(V, vs):
    from oracle import torch_oracle as to
    B = 3
    worst = 0.0
    for case in (Case(V, B, vs, "all", 0, False, None), Case(V, B, vs, "slots+dproj+dJt", 3, True, _live(V, vs, 64)),
                 Case(V, B, vs, "slots+dverts", 7, False, _live(V, vs, 1024))):
        inp, ref = so.inputs(case), so.reference(case)
        d, _ = so.proj_cotangent(inp)
        x = torch.tensor(so.x_rows(B), dtype=torch.float64, requires_grad=True)
        verts, Jt, _ = to.TorchSMPL(so.model(V), torch.float64)(x, return_all=True)
        proj = to.orthographic_project(verts, x, vs)
        c = lambda a: torch.tensor(np.asarray(a, np.float64))
        loss = (proj * c(d)).sum()
        if inp["dverts"] is not None:
            loss = loss + (verts * c(inp["dverts"])).sum()
        if inp["dJt"] is not None:
            loss = loss + (Jt * c(inp["dJt"])).sum()
        loss.backward()
        err = np.abs(x.grad.numpy() - ref["dx"])
        assert (ref["mag_dx"] >= np.abs(ref["dx"]) * (1 - 1e-12)).all()
        assert (ref["mag_dx"] > 0).all()
        worst = max(worst, float((err / ref["mag_dx"]).max()))
    print("V=%d vs=%d staged vs autograd: worst |diff| / mag_dx %.2e" % (V, vs, worst))
    assert worst <= 1e-12


# ------------------------------------------------------------------------------------ 2. the float32 chain
def skin32(V, B, vs, w, fw, cam, dverts, dproj):
    """Stage S in fp32: every sum a running fp32 sum in vertex / joint order -> dv_posed (B, V, 3), dA (B, 288), dcam."""
    f = np.float32
    A, vp = fw["A"].astype(f).reshape(B, 24, 3, 4), fw["vp"].astype(f)
    T = np.zeros((B, V, 3, 4), f)
    for j in range(24):
        T = T + w[None, :, j, None, None] * A[:, None, j]
    ph = np.concatenate([vp, np.ones((B, V, 1), f)], axis=2)
    g = np.zeros((B, V, 3), f) if dverts is None else dverts.astype(f).copy()
    dcam = np.zeros((B, 4), f)
    if dproj is not None:
        X = (T[:, ::vs, :2, :3] * ph[:, ::vs, None, :3]).astype(f)
        XY = ((X[..., 0] + X[..., 1]) + X[..., 2]) + T[:, ::vs, :2, 3]
        g[:, ::vs, 0] += cam[:, None, 0] * dproj[..., 0]
        g[:, ::vs, 1] += cam[:, None, 1] * dproj[..., 1]
        g[:, ::vs, 2] += dproj[..., 2]
        terms = np.stack([XY[..., 0] * dproj[..., 0], XY[..., 1] * dproj[..., 1], dproj[..., 0], dproj[..., 1]], axis=2)
        dcam = np.cumsum(terms.astype(f), axis=1, dtype=f)[:, -1]
    dvp = np.zeros((B, V, 3), f)
    for r in range(3):
        dvp = dvp + T[:, :, r, :3] * g[:, :, r, None]
    dA = np.zeros((B, 24, 12), f)
    gp = (g[:, :, :, None] * ph[:, :, None, :]).reshape(B, V, 12)
    for v in range(V):
        dA = dA + w[v][None, :, None] * gp[:, v, None, :]
    assert dvp.dtype == f and dA.dtype == f and dcam.dtype == f and g.dtype == f
    return dvp, dA.reshape(B, 288), dcam


@functools.lru_cache(maxsize=None)
def chain32(case, weights):
    """-> {gemm: dx (B, 86)} of the whole chain in float32."""
    from test_gpu_blend_small import emulate1, emulate3
    V, B, vs = case.V, case.B, case.vs
    inp, fw = so.inputs(case), so.forward(V, B, torch.float32)
    d = inp["dproj"]
    if inp["lay"] is not None:
        s = so.gather(inp["lay"], so.block_sum32(inp["lay"]["part"]))
        d = s if d is None else d + s
        assert d.dtype == np.float32
    dvp, dA, dcam = skin32(V, B, vs, so.weights_of(V, weights), fw, so.x_rows(B)[:, :4], inp["dverts"], d)
    bt = np.ascontiguousarray(so.blend_t(V).astype(np.float32))
    z = np.zeros((B, 72), np.float32) if inp["dJt"] is None else inp["dJt"].reshape(B, 72)
    out = {}
    for gemm, mm in (("bf16x3", emulate3), ("f32", emulate1)):
        cot = np.concatenate([mm(np.ascontiguousarray(dvp.reshape(B, 3 * V)), bt), dA, z], axis=1)
        out[gemm] = so.pose_vjp32(V, B, cot, dcam)
    return out


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_float32_chain_is_inside_the_bars(case):
    kp = so.k_pose()
    for weights in so.WEIGHTS:
        if weights == "dense" and case.B > 33:
            continue                                        # (the dense table's room is shown at B <= 33)
        ref, got = so.reference(case, weights), chain32(case, weights)
        for gemm in so.GEMMS:
            K = so.bar_k(case, gemm)
            r = so.ratio(got[gemm], ref, K)
            print("%s %s %s: K = %.1f (K_pose %.1f), float32 chain error / bar %.3f" % (so._id(case), weights, gemm, K, kp, r))
            assert r <= 1.0


def test_float32_chain_worst_case():
    """The worst error / bar of the float32 chain per vertex count (the chains are the cached ones of the test above)."""
    for V in so.SHAPES:
        worst = max((so.ratio(chain32(c, w)[g], so.reference(c, w), so.bar_k(c, g)), so._id(c), w, g)
                    for c in CASES if c.V == V for w in so.WEIGHTS if not (w == "dense" and c.B > 33) for g in so.GEMMS)
        print("V=%d: worst float32 chain error / bar %.3f (%s %s %s)" % ((V,) + worst))
        assert worst[0] <= 1.0


def test_k_pose_is_measured_on_the_float32_pose_stage():
    kp = so.k_pose()
    print("K_pose = %.2f (4 x %.2f)" % (kp, kp / 4))
    assert 4.0 <= kp < 4096.0          # at least one rounding per entry; far from grad_close's 2e-3 / 2^-24 = 33 554


# ------------------------------------------------------------------------------------ 3. the bars catch a wrong term
def _slot_mutants(case):
    """name -> mutated reference dx of a slot-sums-only `case` (sparse weights)."""
    V, B, vs = case.V, case.B, case.vs
    lay, w = so.inputs(case)["lay"], so.weights_of(V, "sparse")
    p64 = lay["part"].astype(np.float64)

    def run(part=p64, w=w, fold=None, edit=lambda s: s):
        s, ms = so.gather(lay, part.sum(1)), so.gather(lay, np.abs(part).sum(1))
        return so.staged(V, B, vs, w, None, edit(s), ms, None, fold_blocks=fold)["dx"]

    if case.nsplit > 1:
        return {"skip the last row block": run(part=p64[:, :-1])}
    share = so.gather(lay, np.abs(p64.sum(1)))[..., :2].sum(-1)                   # |du| + |dv| per sampled vertex
    lo = np.unravel_index(np.argmin(np.where(lay["live"], share, np.inf)), share.shape)
    hi = np.unravel_index(np.argmax(np.where(lay["live"], share, -1.0)), share.shape)

    def drop(s):
        s = s.copy()
        s[lo] = 0
        return s

    def swap(s):
        s = s.copy()
        s[hi][:2] = s[hi][1::-1].copy()
        return s
    t4 = so.top4_of(w)
    w1 = np.zeros_like(w)
    np.add.at(w1, (np.arange(V), t4[:, 4].astype(int)), t4[:, :4].sum(1))
    return {"drop the live record with the smallest share": run(edit=drop),
            "swap du and dv of one record": run(edit=swap),
            "give all four weights to the first joint": run(w=w1),
            # (the last chunk that holds a sampled vertex: at vs = 3 the one-vertex chunk of V = 1 025 / 2 049 holds
            #  none, its partials are zeros and a fold without it is right)
            "fold one block of partials too few (1 024-vertex chunks)": run(fold=(so.CHUNK, (V - 1) // vs * vs // so.CHUNK))}


def _outside(name, dx, ref, K, label):
    r = np.abs(dx - ref["dx"]) / (K * U * ref["mag_dx"])
    print("%s K=%.0f  %-58s %s: %d entries outside, worst |diff| / bar %.2f" % (
        label, K, name, "caught" if (r > 1).any() else "MISSED", int((r > 1).sum()), float(r.max())))
    return bool((r > 1).any())


@pytest.mark.parametrize("V,vs", VVS)
def test_bars_catch_a_wrong_term(V, vs):
    """The bars grow with V (5 V 2^-24 of the magnitude and more), so one term among thousands is below them by
    construction; the cotangents here are the ones a dropped term shows in: N(0, 1) with |value| >= 0.05, on up to 8
    live records per chunk (one row block, so no record's sum is small by cancellation; three for the skipped block)
    or on 17 vertices, the last vertex - the one-vertex block or chunk - among them.  Every mutant must leave an entry
    of dx outside the larger (fp32 GEMM) bar of the shape."""
    label = "V=%d vs=%d" % (V, vs)
    missed = []
    last = (V - 1) // vs * vs                                       # the last sampled vertex owns a live record
    for ns in (1, 3):
        live = list(_live(V, vs, 8))
        case = Case(V, 3, vs, "slots", ns, True, tuple(live))
        assert live[last // so.CHUNK] >= 1
        ref = so.reference(case)
        K = max(so.bar_k(case, g) for g in so.GEMMS)
        missed += [n for n, dx in _slot_mutants(case).items() if not _outside(n, dx, ref, K, label)]
    # a cotangent on 17 vertices
    idx = np.unique(np.r_[np.arange(0, V, max(V // 16, 1))[:16], V - 1])
    dverts = np.zeros((3, V, 3), np.float32)
    dverts[:, idx] = so._normal(np.random.default_rng(V + vs), (3, idx.size, 3))
    w = so.weights_of(V, "sparse")
    ref = so.staged(V, 3, vs, w, dverts, None, None, None)
    K = max(so.k_general(V, 0, g) for g in so.GEMMS) + so.k_pose()
    one = dverts.copy()
    one[:, V - 1] = 0
    nblk = (V + so.BLOCK - 1) // so.BLOCK
    for name, dx in (("drop one vertex", so.staged(V, 3, vs, w, one, None, None, None)["dx"]),
                     ("fold one block of partials too few (256-vertex blocks)",
                      so.staged(V, 3, vs, w, dverts, None, None, None, fold_blocks=(so.BLOCK, nblk - 1))["dx"])):
        if not _outside(name, dx, ref, K, label):
            missed.append(name)
    assert not missed, "%s: the bar does not see: %s" % (label, "; ".join(missed))


# ------------------------------------------------------------------------------------ 4. the layouts
SLOT_CASES = [c for c in CASES if c.live is not None]


@pytest.mark.parametrize("case", SLOT_CASES, ids=[so._id(c) for c in SLOT_CASES])
def test_layout_is_what_it_claims(case):
    lay = so.inputs(case)["lay"]
    V, B, vs = case.V, case.B, case.vs
    VP = (V + vs - 1) // vs
    vslot, part = lay["vslot"].astype(np.int64), lay["part"]
    assert vslot.shape == (B, VP) and part.shape == (B, case.nsplit, so.NSLOT, 2) and part.dtype == np.float32
    assert vslot.min() >= -1 and vslot.max() < so.NSLOT
    for b in range(B):                                             # one slot per record
        s = vslot[b][vslot[b] >= 0]
        assert np.unique(s).size == s.size
    sums = so.gather(lay, so.block_sum32(part))[..., :2]           # what slot_sum returns, per sampled vertex
    live = (vslot >= 0) & ~((sums[..., 0] == 0) & (sums[..., 1] == 0))
    assert np.array_equal(live, lay["live"])
    chunk = (np.arange(VP) * vs) // so.CHUNK
    for c, want in enumerate(case.live):
        assert (live[:, chunk == c].sum(1) == want).all(), "chunk %d" % c
    dead = (vslot >= 0) & ~live
    assert not sums[dead].any() and not np.signbit(sums[dead]).any()                   # exactly +0
    if case.nsplit > 1 and (lay["kind"] == 3).any():
        k3 = so.gather(lay, np.abs(part).sum(1))[..., :2][lay["kind"] == 3]
        assert (k3 > 0).all()                                      # cancelling blocks, not empty ones
    k2 = so.gather(lay, np.abs(part).sum(1))[..., :2][lay["kind"] == 2]
    assert not k2.any()
    nrec = int((vslot[0] >= 0).sum())
    win = set((vslot[vslot >= 0] // 4096).tolist())
    if case.perm:
        assert 4 in win and (nrec < 2 or 1 in win)
    else:
        assert win == set(range((nrec - 1) // 4096 + 1)) and vslot.max() == nrec - 1
    # every slot no record owns is zero in every block (nothing else could be gathered by mistake and go unseen)
    used = np.zeros((B, so.NSLOT), bool)
    for b in range(B):
        used[b, vslot[b][vslot[b] >= 0]] = True
    assert not part.transpose(0, 2, 1, 3)[~used].any()


def test_layouts_cover_what_the_issue_lists():
    counts, kinds, sx0, nsplits = set(), set(), False, set()
    for case in SLOT_CASES:
        lay = so.inputs(case)["lay"]
        counts |= set(case.live)
        kinds |= set(np.unique(lay["kind"]).tolist())
        nsplits.add(case.nsplit)
        s = so.gather(lay, so.block_sum32(lay["part"]))
        sx0 |= bool(((s[..., 0] == 0) & (s[..., 1] != 0) & lay["live"]).any())
    assert counts >= {0, 1, 64, 65, 256, 257, 1024} and kinds == {0, 1, 2, 3} and sx0 and nsplits == {1, 2, 3, 7}
    for V in so.SHAPES:                                            # every axis value meets every skinning path
        for key, vals in (("B", (1, 33)), ("vs", (1, 3))):
            for val in vals:
                cots = {c.cot for c in CASES if c.V == V and getattr(c, key) == val}
                assert cots & {"dverts", "dproj", "all"} and "slots" in cots and cots & {"slots+dverts", "slots+dproj+dJt"}
    for ns in (1, 2, 3, 7):
        cots = {c.cot for c in SLOT_CASES if c.nsplit == ns}
        assert "slots" in cots and cots & {"slots+dverts", "slots+dproj+dJt"}
    assert {c.cot for c in CASES} == set(so.COTS)
