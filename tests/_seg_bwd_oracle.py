"""The segmentation backward as one operation, restated in NumPy float64, and the builder of its test cases.

    (dseg | dloss + stats, arg, rec) -> dproj

`arg` (the rasteriser's arg-min slots, channel 0 = the clip's gate) is an INPUT here: the reference reads the very slots
the kernel reads, so there are no arg-min ties between fp32 and float64 and nothing to set aside.  For every pixel (row
ro, column c) and channel ch = 1 .. C - 1 with a slot s = arg[n, ro, c, ch] >= 0, rec[n, s] = (u, v, m^2, vertex) and

    fr = W - 1 - ro,  du = u - c,  dv = v - fr,  d = sqrt(du^2 + dv^2),  x = m d,  score = exp(-x)
    dproj[n, vertex, 0:2] += -g score m / d (du, dv)            (exactly 0 at d == 0),    dproj[..., 2] = 0

with g = dseg[ch] - (gate ? dseg[0] : 0) (seg_bwd_ref) or, with the loss head fused in, g = c1 - c2 exp(score), c1 =
dloss ((label == ch ? stats.z : 0) - stats.y), c2 = dloss stats.x (seg_loss_bwd_ref; csrc/seg_bwd.hip above
seg_bwd_batch_loss).  Nothing here imports the package's kernels; only build_case() calls one, the
PRODUCER of the record lists (ops._seg_bin), so that header, padding sentinels and one slot per vertex are right by
construction.

Run as a script it prints one sha256 of the deterministic dproj per case of HASH_CASES, plain and loss: what
tests/test_gpu_seg_bwd_forms.py compares between the pipelined row walk and SMPLR_SEGBWD_PIPE=0 (the library reads that
variable once, so each setting is a process of its own).

The range of x the cases use.  A float32 score below the smallest normal number, x > 87.3, is outside what the kernel's
documented accuracy covers: v_exp_f32 has no denormal results, and the rasteriser's stages treat a pair as dead from x =
104 on (csrc/seg_bin.hip), while float64 keeps exp(-x) > 0.  The builder therefore keeps every live pair either at x <=
X_LIVE = 80 or at x >= X_DEAD = 300, where |g| m exp(-x) is below the smallest float32 subnormal for any |g| m < 2^280:
the first kind is compared under the bar, the second must add exactly nothing.
"""
import hashlib
import os
import sys

import numpy as np

F = np.float64
SB_SLOTS = 4096          # record slots per window of the kernel's accumulators (csrc/common.h)
SB_NWIN = 5              # windows the partial buffer holds
X_LIVE, X_DEAD = 80.0, 300.0
VP_SMALL, K_SMALL = 601, 580   # the custom tables: 601 is prime (the dproj zeroing's share never divides), 21 vertices unlisted


class Ref:
    """dproj and, per vertex component, mag = sum |term|, magx = sum |term| x, nterm = the number of non-zero terms;
    npair = the number of pairs with d > 0 and x < X_DEAD, whatever their g: where it is 0 float32 has nothing to add."""

    def __init__(self, B, VP):
        self.dproj, self.mag, self.magx = (np.zeros((B, VP, 3), F) for _ in range(3))
        self.nterm, self.npair = np.zeros((B, VP, 3), F), np.zeros((B, VP, 3), F)


def _pairs(arg, rec, W, C, n0=0):
    """The live (pixel, channel) pairs of arg (b, W, W, 32) against rec (b, S, 4) float32 -> dict of flat arrays."""
    a = np.asarray(arg)[..., 1:C].astype(np.int64)
    n, ro, c, k = np.nonzero(a >= 0)
    s = a[n, ro, c, k]
    rec = np.ascontiguousarray(rec, np.float32)
    r = rec[n, s].astype(F)
    vert = rec.view(np.int32)[n, s, 3].astype(np.int64)
    du, dv = r[:, 0] - c, r[:, 1] - (W - 1 - ro)
    d, m = np.sqrt(du * du + dv * dv), np.sqrt(r[:, 2])
    x = m * d
    score = np.exp(-x)
    w = np.where(d > 0, score * m / np.where(d > 0, d, 1.0), 0.0)
    return dict(n=n + n0, ro=ro, c=c, ch=k + 1, slot=s, vert=vert, du=du, dv=dv, x=x, score=score, w=w)


def _chunks(B, W, C):
    step = max(1, int(4e6) // max(1, W * W * (C - 1)))
    return [(lo, min(B, lo + step)) for lo in range(0, B, step)]


def _add(ref, p, g, gabs, VP):
    assert p["vert"].size == 0 or (p["vert"].min() >= 0 and p["vert"].max() < VP), "arg names a slot without a vertex"
    B = ref.dproj.shape[0]
    idx = p["n"] * VP + p["vert"]
    for j, dd in enumerate((p["du"], p["dv"])):
        term = -g * p["w"] * dd
        at = gabs * p["w"] * np.abs(dd)
        pair = ((p["w"] * np.abs(dd) > 0) & (p["x"] < X_DEAD)).astype(F)
        for dst, val in ((ref.dproj, term), (ref.mag, at), (ref.magx, at * p["x"]), (ref.nterm, (term != 0).astype(F)),
                         (ref.npair, pair)):
            dst[..., j] += np.bincount(idx, val, B * VP).reshape(B, VP)


def seg_bwd_ref(dseg, arg, rec, VP, W, C):
    """dseg (B, W, W, C), arg (B, W, W, 32) int, rec (B, S, 4) float32 -> Ref."""
    dseg, arg = np.asarray(dseg, F), np.asarray(arg)
    B = arg.shape[0]
    ref = Ref(B, VP)
    for lo, hi in _chunks(B, W, C):
        p = _pairs(arg[lo:hi], rec[lo:hi], W, C, lo)
        n, ro, c = p["n"], p["ro"], p["c"]
        g = dseg[n, ro, c, p["ch"]] - np.where(arg[n, ro, c, 0] == 1, dseg[n, ro, c, 0], 0.0)
        _add(ref, p, g, np.abs(g), VP)
    return ref


def seg_loss_bwd_ref(dloss, stats, arg, rec, VP, W, C=32, labels=None):
    """dloss (B, W*W), stats (B, W*W, 4) = (k / sum exp | k x the background's share | k | label bits), as the
    rasteriser's loss epilogue leaves them (float32; `labels` (B, W*W) replaces the bits where stats is float64)."""
    arg = np.asarray(arg)
    B = arg.shape[0]
    if labels is None:
        labels = np.ascontiguousarray(stats, np.float32).view(np.int32)[..., 3]
    labels = np.asarray(labels).reshape(B, W * W)
    dloss, stats = np.asarray(dloss, F).reshape(B, W * W), np.asarray(stats, F).reshape(B, W * W, 4)
    ref = Ref(B, VP)
    for lo, hi in _chunks(B, W, C):
        p = _pairs(arg[lo:hi], rec[lo:hi], W, C, lo)
        n, px = p["n"], p["ro"] * W + p["c"]
        dl, st = dloss[n, px], stats[n, px]
        c1 = dl * (np.where(labels[n, px] == p["ch"], st[:, 2], 0.0) - st[:, 1])
        c2 = dl * st[:, 0]
        es = np.exp(p["score"])
        _add(ref, p, c1 - c2 * es, np.abs(c1) + np.abs(c2) * es, VP)       # (g is a difference: its parts' sizes)
    return ref


def scores_of(arg, rec, W, C=32):
    """The float64 scores of a case's own (arg, rec) -> (B, W, W, 32): channel 0 = 1 - clip(sum of the parts, 0, 1)."""
    arg = np.asarray(arg)
    B = arg.shape[0]
    s = np.zeros((B, W, W, 32), F)
    for lo, hi in _chunks(B, W, C):
        p = _pairs(arg[lo:hi], rec[lo:hi], W, C, lo)
        s[p["n"], p["ro"], p["c"], p["ch"]] = p["score"]
    s[..., 0] = 1.0 - np.clip(s[..., 1:].sum(-1), 0.0, 1.0)
    return s


def make_stats(scores, labels, class_w, gamma, gate, dtype=np.float32):
    """What the loss epilogue leaves per pixel, from a real softmax over the 32 scores (the deterministic form's bound
    |g_c| <= 2 |dloss| k relies on that): (k / sum exp, k (delta_0t - softmax_0) gate, k, label), k = q_t softmax_t
    with q_t = d loss / d softmax_t of the focal loss; a label outside the classes gives k = 0.  -> (B, W*W, 4), rounded
    to `dtype`; float32 carries the label's bits in column 3 as the kernel reads them, float64 the label as a number."""
    B = scores.shape[0]
    s = np.asarray(scores, F).reshape(B, -1, 32)
    lab = np.asarray(labels).reshape(B, -1).astype(np.int64)
    gate = np.asarray(gate).reshape(B, -1).astype(bool)
    e = np.exp(s)
    den = e.sum(-1)
    inside = (lab >= 0) & (lab < 32)
    lc = np.where(inside, lab, 0)
    smt = np.take_along_axis(e, lc[..., None], 2)[..., 0] / den
    wt = 1.0 if class_w is None else np.asarray(class_w, F)[lc]
    dpow = gamma * (1 - smt) ** (gamma - 1) if gamma > 0 else 0.0
    q = wt * (dpow * np.log(smt) - (1 - smt) ** gamma / smt)
    k = np.where(inside, q * smt, 0.0)
    share = np.where(gate, (lab == 0) - e[..., 0] / den, 0.0)
    st = np.stack([k / den, k * share, k, lab.astype(F)], -1).astype(dtype)
    if dtype == np.float32:
        st[..., 3] = lab.astype(np.int32).view(np.float32)
    return st


def bar(ref, unit):
    """The bound on |got - want| per vertex component (derivation: tests/test_gpu_seg_bwd_forms.py)."""
    return 2.0 ** -23 * (8 * ref.mag + 6 * ref.magx) + 2.0 ** -24 * ref.nterm * ref.mag + unit


# ---------------------------------------------------------------------------------------------------------------------
# cases

def random_table(rng, P, VP=VP_SMALL, K=K_SMALL):
    """A part table over VP vertices: K of them in P non-empty parts, the rest in none -> (ids, off)."""
    ids = rng.permutation(VP)[:K]
    cuts = np.sort(rng.choice(np.arange(1, K), P - 1, replace=False))
    return ids.astype(np.int64), np.concatenate([[0], cuts, [K]]).astype(np.int64)


def part_of_vertex(ids, off, VP):
    pv = np.full(VP, -1, np.int64)
    pv[np.asarray(ids, np.int64)] = np.repeat(np.arange(len(off) - 1), np.diff(np.asarray(off, np.int64)))
    return pv


def slot_tables(rec, pv):
    """rec (B, S, 4) float32 as the binning kernel leaves it -> valid (B, S): slots that hold a vertex, part (B, S),
    local (B, S): the nearest-pixel records behind the far-reaching list, nslots (B,)."""
    ri = np.ascontiguousarray(rec, np.float32).view(np.int32)
    S = rec.shape[1]
    nslots, far = ri[:, S - 1, 0], ri[:, S - 1, 2]
    sl = np.arange(S)[None]
    valid = (sl < nslots[:, None]) & (ri[..., 3] >= 0)
    part = np.where(valid, pv[np.clip(ri[..., 3], 0, len(pv) - 1)], -1)
    valid &= part >= 0
    return valid, part, valid & (sl >= far[:, None]), nslots


def canonical(rec, W):
    """The local records of each mesh sorted by (pixel, vertex): the binning kernel places the records of one pixel in
    the order its threads arrive (an LDS cursor), so two of its runs can number them differently - any order within a
    pixel is a valid list, and this one makes a case the same in every process (the hashes of main())."""
    ri = rec.view(np.int32)
    S = rec.shape[1]
    for n in range(rec.shape[0]):
        nsl, far = int(ri[n, S - 1, 0]), int(ri[n, S - 1, 2])
        loc = rec[n, far:nsl].copy()
        pix = np.rint(loc[:, 1]).astype(np.int64) * W + np.rint(loc[:, 0]).astype(np.int64)
        rec[n, far:nsl] = loc[np.lexsort((loc.view(np.int32)[:, 3], pix))]
    return rec


def _padded(lists):
    m = max(1, max(len(l) for l in lists))
    out = np.zeros((len(lists), m), np.int64)
    for i, l in enumerate(lists):
        out[i, :len(l)] = l
    return out, np.array([len(l) for l in lists], np.int64)


# kinds of a lane's row: all -1 | one run | runs of one pixel | one run over pixels 2 .. 13 (every batch boundary of the
# walks: 3-4, 5-6, 7-8, 11-12) | a random mix | (multi-window meshes) slots of any part, hence of every window
KIND_P = (0.1, 0.1, 0.15, 0.15, 0.5)


def synth_arg(rng, rec, pv, W, C, multi=()):
    """arg (B, W, W, 32) int16, synthesised per (row, channel) as runs of slots of the channel's own part and of the local
    records; channel 0 a random 0 / 1 gate; channels >= C random slots (the kernel masks them).  Edits rec in place for
    the d == 0 pixel of mesh 0.  -> arg, nulls: the (n, ro, c, ch) of the d == 0 pixel and of an underflowed pair."""
    B, S = rec.shape[:2]
    valid, part, local, nslots = slot_tables(rec, pv)
    # the d == 0 pixel: a far-reaching record of mesh 0 moved onto a pixel centre
    far0 = np.flatnonzero(valid[0] & ~local[0] & (part[0] + 1 < C))
    s0 = int(far0[len(far0) // 2])
    ro0, c0, ch0 = W // 3, W // 2, int(part[0, s0]) + 1
    rec[0, s0, 0], rec[0, s0, 1] = c0, W - 1 - ro0

    cand, cnt = [], []
    for n in range(B):
        rows = [np.flatnonzero(part[n] == p) for p in range(C - 1)]
        t, c = _padded(rows)
        cand.append(t), cnt.append(c)
    M = max(t.shape[1] for t in cand)
    cand = np.stack([np.pad(t, ((0, 0), (0, M - t.shape[1]))) for t in cand])           # (B, C-1, M)
    cnt = np.stack(cnt)                                                                 # (B, C-1)
    loc, lcnt = _padded([np.flatnonzero(local[n]) for n in range(B)])
    allv, vcnt = _padded([np.flatnonzero(valid[n]) for n in range(B)])

    shape = (B, W, C - 1, W)                                                            # mesh, row, channel, column
    kind = rng.choice(len(KIND_P), size=shape[:3], p=KIND_P)
    for n in multi:
        kind[n] = np.where(rng.random(shape[1:3]) < 0.25, 5, kind[n])
    new = rng.random(shape) < 0.3
    new[kind == 2] = True
    new[kind == 1] = False
    k3 = kind == 3
    new[k3, 3:14] = False
    new[k3, 2:3] = True
    new[k3, 14:15] = True
    new[..., 0] = True
    run = np.cumsum(new, -1) - 1
    pick = rng.random(shape)
    back = rng.random(shape) < 0.25                                                     # the slot of two runs ago returns
    pick[..., 2:] = np.where(back[..., 2:], pick[..., :-2], pick[..., 2:])
    empty = rng.random(shape) < 0.25
    empty[..., 0] &= kind != 1
    use_loc = rng.random(shape) < 0.1
    pick, empty, use_loc = (np.take_along_axis(v, run, -1) for v in (pick, empty, use_loc))
    nn, _, cc, _ = np.indices(shape, sparse=True)

    def index(count):                            # a run's draw as an index into a list of `count` slots
        return np.minimum((pick * count).astype(np.int64), np.maximum(count - 1, 0))

    own_cnt = cnt[:, None, :, None]
    slot = np.where(own_cnt > 0, cand[nn, cc, index(own_cnt)], -1)
    lc = lcnt[:, None, None, None]
    slot = np.where(use_loc & (lc > 0), loc[nn, index(lc)], slot)
    vc = vcnt[:, None, None, None]
    slot = np.where((kind == 5)[..., None] & (vc > 0), allv[nn, index(vc)], slot)
    slot = np.where(empty | (kind == 0)[..., None], -1, slot)
    arg = np.full((B, W, W, 32), -1, np.int64)
    arg[..., 1:C] = slot.transpose(0, 1, 3, 2)

    # every record with a pixel centre in reach names that pixel in its part's channel (7 in 10 do): the term that
    # dominates its vertex' sum sits at ONE known pixel, so a pixel taken for its neighbour cannot hide behind the bar
    n, s = np.nonzero(valid)
    c, r = np.rint(rec[n, s, 0]).astype(np.int64), np.rint(rec[n, s, 1]).astype(np.int64)
    ok = (c >= 0) & (c < W) & (r >= 0) & (r < W) & (part[n, s] + 1 < C) & (rng.random(len(n)) < 0.7)
    arg[n[ok], W - 1 - r[ok], c[ok], part[n, s][ok] + 1] = s[ok]
    # multi-window meshes: the slots just below and at the multiples of the window, three pixels each
    for n in multi:
        for j, s in enumerate(b for b in (SB_SLOTS - 1, SB_SLOTS, SB_SLOTS + 1, 2 * SB_SLOTS - 1, 2 * SB_SLOTS) if
                              b < S and valid[n, b]):
            arg[n, (7 * j + 3) % W, (5 * j + 1) % W:(5 * j + 1) % W + 3, part[n, s] + 1] = s
    # x in (X_LIVE, X_DEAD) is neither compared nor dead (module docstring)
    for lo, hi in _chunks(B, W, C):
        p = _pairs(arg[lo:hi], rec[lo:hi], W, C, lo)
        out = (p["x"] > X_LIVE) & (p["x"] < X_DEAD)
        arg[p["n"][out], p["ro"][out], p["c"][out], p["ch"][out]] = -1
    # the d == 0 pixel, alone in its lane's row: with or without it the lane's runs end at the same places
    arg[0, ro0, :, ch0] = -1
    arg[0, ro0, c0, ch0] = s0
    nulls = [(0, ro0, c0, ch0)]
    # an underflowed pair: a local record (m = 500) three pixels from its own
    for n in range(B):
        ls = [s for s in np.flatnonzero(local[n]) if part[n, s] + 1 < C and (n, part[n, s] + 1) != (0, ch0)]
        if ls:
            s1 = int(ls[len(ls) // 2])
            ro1, c1 = W - 1 - int(np.rint(rec[n, s1, 1])), (int(np.rint(rec[n, s1, 0])) + 3) % W
            arg[n, ro1, c1, part[n, s1] + 1] = s1
            nulls.append((n, ro1, c1, int(part[n, s1]) + 1))
            break
    arg[..., 0] = rng.integers(0, 2, (B, W, W))
    if C < 32:
        arg[..., C:] = rng.integers(-1, int(nslots.min()), (B, W, W, 32 - C))
    return arg.astype(np.int16), nulls


def cotangent(rng, shape):
    """normal(0, 1) with a handful of entries scaled by 2^+-20."""
    g = rng.normal(0, 1, shape)
    flat = g.reshape(-1)
    at = rng.choice(flat.size, 6, replace=False)
    flat[at] *= np.array([2.0 ** 20, 2.0 ** -20] * 3)
    return g.astype(np.float32)


class Case:
    pass


def build_case(W, B, table="p31", multi=(), seed=0):
    """One case on the current HIP device: record lists from the binning kernel, everything else synthesised.
    table: "p31" / "p17" / "p5" (601 vertices) or "real" (the 6 890-vertex table; meshes in `multi` all visible: more
    than 4 096 used slots)."""
    import torch
    from ilps_amd import ops
    from ilps_amd.smpl_model import load_part_tables
    dev = torch.device("cuda")
    rng = np.random.default_rng(seed)
    k = Case()
    k.W, k.B, k.multi = W, B, tuple(multi)
    if table == "real":
        ids, off = load_part_tables(1)
        k.VP = 6890
        k.pt = ops.get_part_table(1, dev, 6890)
    else:
        k.VP = VP_SMALL
        ids, off = random_table(rng, int(table[1:]))
        k.pt = ops.build_part_table(ids, off, 1, k.VP, dev)
    k.C = k.pt.P + 1
    proj = rng.uniform(-4.0, W + 4.0, (B, k.VP, 3)).astype(np.float32)
    mask = np.where(rng.random((B, k.VP)) < (0.5 if table != "real" else 0.15), 1.0, 500.0).astype(np.float32)
    for n in multi:
        mask[n] = 1.0
    S = int(ops._lib.load().smplr_seg_slots(k.pt.P, k.pt.K))
    rec = torch.zeros((B, S, 4), dtype=torch.float32, device=dev)
    ops._seg_bin(torch.as_tensor(proj).to(dev), torch.as_tensor(mask).to(dev), W, k.pt, rec=rec)
    k.rec = canonical(rec.cpu().numpy(), W)
    pv = part_of_vertex(ids, off, k.VP)
    k.arg, k.nulls = synth_arg(rng, k.rec, pv, W, k.C, k.multi)
    k.nslots = slot_tables(k.rec, pv)[3]
    k.dseg = cotangent(rng, (B, W, W, k.C))
    if k.C == 32:
        k.dloss = cotangent(rng, (B, W * W))
        lab = rng.integers(0, 32, (B, W, W))
        lab.reshape(-1)[rng.choice(lab.size, 5, replace=False)] = [-1, 32, 255, -7, 1 << 20]
        k.labels = lab
        k.class_w = rng.uniform(0.3, 2.0, 32)
        k.stats = make_stats(scores_of(k.arg, k.rec, W), lab, k.class_w, 2.0, k.arg[..., 0] == 1)
    k.dev = {}
    return k


def on_dev(k, name, value=None):
    """The case's array `name` on the device (cached), or `value` uploaded."""
    import torch
    if value is not None:
        return torch.as_tensor(np.ascontiguousarray(value)).to("cuda")
    if name not in k.dev:
        k.dev[name] = torch.as_tensor(np.ascontiguousarray(getattr(k, name))).to("cuda")
    return k.dev[name]


def run_case(k, loss, det, merge=True, arg=None, scale=None, sel=None):
    """The HIP backward of case k -> dproj (B, VP, 3) on the device (merge=False: (partials, nsplit)).  arg: another
    arg tensor; scale: the cotangent's factor; sel: a slice / index array of meshes."""
    from ilps_amd import ops
    pick = (lambda v: v) if sel is None else (lambda v: v[sel].contiguous())
    a, rec = pick(on_dev(k, "arg") if arg is None else on_dev(k, None, arg)), pick(on_dev(k, "rec"))
    cot = on_dev(k, "dloss" if loss else "dseg")
    cot = pick(cot if scale is None else cot * scale)
    if loss:
        return ops._seg_loss_bwd(cot, pick(on_dev(k, "stats")), a, rec, k.VP, k.W, k.pt, merge=merge, deterministic=det)
    return ops._seg_bwd(cot, a, rec, k.VP, k.W, k.pt, merge=merge, deterministic=det)


# the cases whose deterministic dproj the script hashes: both pipelined widths, the 8-row and the tall launch
HASH_CASES = [(48, 2), (48, 128), (64, 2), (64, 64)]


def main():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if root not in sys.path:
        sys.path.insert(0, root)
    import ilps_amd  # noqa: F401  (alias of the hyphenated package directory)
    import torch
    for W, B in HASH_CASES:
        k = build_case(W, B, seed=W * 1000 + B)
        for loss in (False, True):
            d = run_case(k, loss, True)
            torch.cuda.synchronize()
            print("W=%d B=%d %s %s" % (W, B, "loss" if loss else "plain", hashlib.sha256(d.cpu().numpy().tobytes()).hexdigest()))


if __name__ == "__main__":
    main()
