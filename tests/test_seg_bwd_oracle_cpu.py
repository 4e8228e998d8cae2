"""tests/_seg_bwd_oracle.py pinned without a GPU: its two references equal float64 autograd through the oracle's
projects_to_seg (+ softmax_focal_loss) when they are fed that oracle's own arg-min vertices and clip gate - both sides
float64, differing in summation order only, hence 1e-9 of the largest entry; known answers by hand; and the case
builder's arg synthesis contains every pattern the GPU matrix (tests/test_gpu_seg_bwd_forms.py) relies on."""
import numpy as np
import pytest
import torch

import _seg_bwd_oracle as so
from oracle import np_oracle as o
from oracle import torch_oracle as to


def mesh(seed, B, V, P, W):
    """Random float32-exact projections and {1, 500} masks, a partition of the V vertices into P parts; rec with one
    record per vertex (slot = vertex, m^2 = mask^2) and arg from the oracle's arg-min vertices and clip gate."""
    rng = np.random.default_rng(seed)
    proj = rng.uniform(-2.0, W + 2.0, (B, V, 3)).astype(np.float32).astype(np.float64)
    mask = np.where(rng.random((B, V)) < 0.5, 1.0, 500.0)
    ids, off = so.random_table(rng, P, V, V)
    seg, warg = o.projects_to_seg(proj, mask, W, ids, off, return_argmin=True)
    rec = np.zeros((B, V + 1, 4), np.float32)
    rec[:, :V, 0:2] = proj[..., :2]
    rec[:, :V, 2] = mask * mask
    rec.view(np.int32)[:, :V, 3] = np.arange(V)
    arg = np.full((B, W, W, 32), -1, np.int16)
    arg[..., 1:P + 1] = warg
    arg[..., 0] = seg[..., 1:].sum(-1) <= 1.0
    return rng, proj, mask, ids, off, rec, arg, seg


def close(got, want):
    assert np.abs(got - want).max() <= 1e-9 * np.abs(want).max()


def test_plain_reference_is_autograd_of_the_oracle():
    B, V, P, W = 2, 200, 5, 12
    rng, proj, mask, ids, off, rec, arg, seg = mesh(1, B, V, P, W)
    assert 0 < (arg[..., 0] == 1).mean() < 1                  # both states of the clip's gate occur
    dseg = rng.normal(0, 1, (B, W, W, P + 1))
    p = torch.tensor(proj, requires_grad=True)
    (to.projects_to_seg(p, torch.tensor(mask), W, ids, off) * torch.tensor(dseg)).sum().backward()
    ref = so.seg_bwd_ref(dseg, arg, rec, V, W, P + 1)
    close(ref.dproj, p.grad.numpy())
    assert not ref.dproj[..., 2].any() and (ref.mag >= np.abs(ref.dproj)).all()
    assert np.allclose(so.scores_of(arg, rec, W, P + 1)[..., :P + 1], seg, rtol=1e-12, atol=1e-300)


@pytest.mark.parametrize("gamma,weighted", [(0.0, False), (0.0, True), (2.0, False), (2.0, True)])
def test_loss_reference_is_autograd_of_the_oracle(gamma, weighted):
    B, V, P, W = 2, 400, 31, 12
    rng, proj, mask, ids, off, rec, arg, seg = mesh(2 + int(gamma) + weighted, B, V, P, W)
    lab = rng.integers(0, 32, (B, W, W))
    lab[0, 0, :3] = [-1, 32, 255]                               # outside the classes: no loss, no gradient
    cw = o.FOCAL_CLASS_WEIGHTS[:32] if weighted else None
    dloss = rng.normal(0, 1, (B, W * W))
    y = (lab.reshape(B, -1, 1) == np.arange(32)).astype(np.float64)
    p = torch.tensor(proj, requires_grad=True)
    loss = to.softmax_focal_loss(to.projects_to_seg(p, torch.tensor(mask), W, ids, off), torch.tensor(y), gamma,
                                 None if cw is None else torch.tensor(cw))
    (loss * torch.tensor(dloss)).sum().backward()
    stats = so.make_stats(so.scores_of(arg, rec, W), lab, cw, gamma, arg[..., 0] == 1, dtype=np.float64)
    ref = so.seg_loss_bwd_ref(dloss, stats, arg, rec, V, W, labels=lab)
    close(ref.dproj, p.grad.numpy())
    # the float32 stats the kernels read carry the label's bits and agree to rounding
    st32 = so.make_stats(so.scores_of(arg, rec, W), lab, cw, gamma, arg[..., 0] == 1)
    assert np.array_equal(st32.view(np.int32)[..., 3], lab.reshape(B, -1))
    r32 = so.seg_loss_bwd_ref(dloss, st32, arg, rec, V, W)
    assert np.abs(r32.dproj - ref.dproj).max() <= 1e-6 * np.abs(ref.dproj).max()
    # |g_c| <= 2 |dloss| k, what the deterministic form's scale relies on
    assert (np.abs(ref.dproj) <= ref.mag + 1e-300).all()


def one_record(u, v, m, W=8):
    rec = np.zeros((1, 2, 4), np.float32)
    rec[0, 0] = (u, v, m * m, 0)                               # vertex 0 (its bits are those of 0.0f)
    arg = np.full((1, W, W, 32), -1, np.int16)
    arg[..., 0] = 0
    return rec, arg


def test_known_answers():
    W = 8
    rec, arg = one_record(5.0, 3.0, 1.0)
    arg[0, 2, 2, 7] = 0                                         # output row 2 = grid row 5: du = 3, dv = -2
    dseg = np.zeros((1, W, W, 32))
    dseg[0, 2, 2, 7], dseg[0, 2, 2, 0] = 1.5, 0.25
    d = np.sqrt(13.0)
    closed = so.seg_bwd_ref(dseg, arg, rec, 3, W, 32)
    assert np.allclose(closed.dproj[0, 0], [-1.5 * np.exp(-d) / d * 3, -1.5 * np.exp(-d) / d * -2, 0], rtol=1e-14)
    assert not closed.dproj[0, 1:].any() and closed.nterm[0, 0].tolist() == [1, 1, 0]
    assert np.allclose(closed.magx, closed.mag * d)
    arg[0, 2, 2, 0] = 1                                         # gate open: the background's cotangent is subtracted
    opened = so.seg_bwd_ref(dseg, arg, rec, 3, W, 32)
    assert np.allclose(opened.dproj, closed.dproj * (1.25 / 1.5), rtol=1e-14)
    # weight 500: x = m d
    rec5, _ = one_record(2.1, 5.0, 500.0)
    w5 = so.seg_bwd_ref(dseg, arg, rec5, 3, W, 32)
    du5 = np.float64(np.float32(2.1)) - 2.0
    assert np.allclose(w5.dproj[0, 0, :2], [-1.25 * np.exp(-500 * du5) * 500, 0], rtol=1e-12, atol=0)
    assert np.allclose(w5.magx, w5.mag * 500 * du5)
    # a pixel exactly on its record contributes exactly nothing, in both forms
    rec0, _ = one_record(2.0, 5.0, 1.0)
    z = so.seg_bwd_ref(dseg, arg, rec0, 3, W, 32)
    assert not z.dproj.any() and not z.mag.any() and not z.nterm.any()
    st = np.zeros((1, W * W, 4), np.float32)
    st[0, :, :3] = (0.01, 0.002, 0.3)
    st.view(np.int32)[0, :, 3] = 7
    zl = so.seg_loss_bwd_ref(np.ones((1, W * W)), st, arg, rec0, 3, W)
    assert not zl.dproj.any()
    # the loss form by hand: g = c1 - c2 exp(score)
    ls = so.seg_loss_bwd_ref(np.full((1, W * W), 2.0), st, arg, rec, 3, W)
    s = np.exp(-d)
    g = 2.0 * (np.float32(0.3) - np.float64(np.float32(0.002))) - 2.0 * np.float64(np.float32(0.01)) * np.exp(s)
    assert np.allclose(ls.dproj[0, 0, :2], [-g * s / d * 3, -g * s / d * -2], rtol=1e-14)
    st.view(np.int32)[0, :, 3] = 8                              # another label: c1 loses its k
    ls8 = so.seg_loss_bwd_ref(np.full((1, W * W), 2.0), st, arg, rec, 3, W)
    g8 = 2.0 * (0.0 - np.float64(np.float32(0.002))) - 2.0 * np.float64(np.float32(0.01)) * np.exp(s)
    assert np.allclose(ls8.dproj[0, 0, :2], [-g8 * s / d * 3, -g8 * s / d * -2], rtol=1e-14)


def fake_rec(rng, B, W, ids, off, VP, visible=0.5):
    """Record lists laid out as the binning kernel leaves them (csrc/raster_common.h): the far-reaching records
    part-major, each part padded to a multiple of 4 with +inf sentinels, the local records behind, the header last."""
    P, K = len(off) - 1, len(ids)
    S = ((K + 3 * P + 3) // 4 * 4) + (K + 3) // 4 * 4 + 4
    rec = np.zeros((B, S, 4), np.float32)
    ri = rec.view(np.int32)
    for n in range(B):
        proj = rng.uniform(-4.0, W + 4.0, (VP, 2)).astype(np.float32)
        vis = rng.random(VP) < visible
        s, near = 0, []
        for p in range(P):
            for v in ids[off[p]:off[p + 1]]:
                if vis[v]:
                    rec[n, s, :3] = (proj[v, 0], proj[v, 1], 1.0)
                    ri[n, s, 3] = v
                    s += 1
                else:
                    c, r = np.rint(proj[v])
                    if 0 <= c < W and 0 <= r < W and 500.0 * np.hypot(*(proj[v] - (c, r))) < 104.0:
                        near.append(v)
            while s % 4:
                rec[n, s, :3] = (np.inf, np.inf, 1.0)
                ri[n, s, 3] = -1
                s += 1
        far = s
        for v in near:
            rec[n, s, :3] = (proj[v, 0], proj[v, 1], 250000.0)
            ri[n, s, 3] = v
            s += 1
        ri[n, S - 1] = (s, 0, far, -1)
    return rec


def runs_of(row):
    """(value, start, length) of the runs of a 1-D array."""
    edge = np.flatnonzero(np.diff(row)) + 1
    start = np.concatenate([[0], edge])
    return [(int(row[a]), int(a), int(b - a)) for a, b in zip(start, np.concatenate([edge, [len(row)]]))]


@pytest.mark.parametrize("W,P", [(48, 31), (8, 31), (50, 31), (24, 5)])
def test_synthesised_arg_contains_every_pattern(W, P):
    rng = np.random.default_rng(W + P)
    ids, off = so.random_table(rng, P)
    pv = so.part_of_vertex(ids, off, so.VP_SMALL)
    B, C = 3, P + 1
    rec = fake_rec(rng, B, W, ids, off, so.VP_SMALL)
    arg, nulls = so.synth_arg(rng, rec, pv, W, C)
    valid, part, local, nslots = so.slot_tables(rec, pv)
    assert arg.dtype == np.int16 and arg.shape == (B, W, W, 32)
    assert set(np.unique(arg[..., 0])) == {0, 1}
    live = arg[..., 1:C]
    n, ro, c, k = np.nonzero(live >= 0)
    assert valid[n, live[n, ro, c, k]].all()                       # never a sentinel, the header or an unused slot
    assert (part[n, live[n, ro, c, k]] == k).mean() > 0.8           # mostly the channel's own part ...
    assert local[n, live[n, ro, c, k]].any()                        # ... and local records
    x = so._pairs(arg, rec, W, C)["x"]
    assert not ((x > so.X_LIVE) & (x < so.X_DEAD)).any() and (x >= so.X_DEAD).any()
    seen = set()
    for nn in range(B):
        for r in range(W):
            for ch in range(1, C):
                rs = runs_of(arg[nn, r, :, ch])
                if len(rs) == 1:
                    seen.add("all -1" if rs[0][0] < 0 else "whole row")
                for (v, a, ln), nxt in zip(rs, rs[1:] + [None]):
                    if v < 0:
                        seen.add("stretch of -1") if ln > 1 else None
                        continue
                    if ln == 1:
                        seen.add("run of 1")
                    if a <= 3 and a + ln >= min(W, 13):
                        seen.add("crosses every batch boundary")
                    later = [w for w, _, _ in rs[rs.index((v, a, ln)) + 2:]]
                    if v in later:
                        seen.add("returns after a gap")
    want = {"all -1", "whole row", "run of 1", "stretch of -1", "crosses every batch boundary", "returns after a gap"}
    assert seen >= want, want - seen
    # the two pixels that must add exactly nothing
    (n0, r0, c0, ch0), (n1, r1, c1, ch1) = nulls
    p = so._pairs(arg[n0:n0 + 1], rec[n0:n0 + 1], W, C)
    at = (p["ro"] == r0) & (p["c"] == c0) & (p["ch"] == ch0)
    assert at.sum() == 1 and p["w"][at][0] == 0.0 and p["du"][at][0] == 0.0 and p["dv"][at][0] == 0.0
    assert (arg[n0, r0, :, ch0] >= 0).sum() == 1
    p = so._pairs(arg[n1:n1 + 1], rec[n1:n1 + 1], W, C)
    at = (p["ro"] == r1) & (p["c"] == c1) & (p["ch"] == ch1)
    assert at.sum() == 1 and p["x"][at][0] > 104.0
    if C < 32:
        assert (arg[..., C:] >= 0).any()


def test_multi_window_rows_mix_the_windows():
    """All 6 890 vertices visible: more than one window of slots; kind-5 rows draw from every window, and the slots
    around the window's edge are named."""
    from ilps_amd.smpl_model import load_part_tables
    rng = np.random.default_rng(5)
    ids, off = load_part_tables(1)
    pv = so.part_of_vertex(ids, off, 6890)
    W = 48
    rec = fake_rec(rng, 1, W, np.asarray(ids), np.asarray(off), 6890, visible=1.1)
    valid, part, local, nslots = so.slot_tables(rec, pv)
    assert nslots[0] > so.SB_SLOTS
    arg, _ = so.synth_arg(rng, rec, pv, W, 32, multi=(0,))
    live = arg[0, :, :, 1:]
    wins = [{int(s) // so.SB_SLOTS for s in live[r, :, ch] if s >= 0} for r in range(W) for ch in range(31)]
    assert max(len(w) for w in wins) == (int(nslots[0]) + so.SB_SLOTS - 1) // so.SB_SLOTS
    for s in (so.SB_SLOTS - 1, so.SB_SLOTS, so.SB_SLOTS + 1):
        assert not valid[0, s] or (live == s).any()
