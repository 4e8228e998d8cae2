"""Seeded problems for the label-map distance tests (CPU and GPU): every case the issue names in one generator."""
import numpy as np

import _labeldist_oracle as orc


def problem(B, V, W, C, seed=0, ties=True, weights=True):
    """-> dict of verts (B, V, 3), cam (B, 4), vweight (B, V) or None float32, labels (B, W, W) int32, vclass (V,) int32.
      * vclass: with V >= 600 and C >= 3 one class of exactly 256 and one of exactly 257 vertices, scattered over the
        indices; the rest random in -1 .. C (so -1, 0 and C - no part - occur).
      * labels: coherent 4 x 4 blocks of random classes, two in five of them class 1 or 2; pixels of -1, C and 255 (don't care); the highest class removed from
        every image (its vertices find nothing); the last row of a batch of 3 all background.
      * vweight: 0 and NaN entries; in row 0 every vertex of class 1 has weight 0 when C > 2 (its pixels find nothing).
      * cam = (2, 4, 0.5 + b, 1): with `ties` half of the vertices sit at X = k / 4, Y = m / 8 from a small set, so their
        projections are integer or half-integer points - equidistant pixels - and several vertices share a point; the others
        are random, some far outside the image."""
    rng = np.random.default_rng(1000 * seed + 131 * B + 17 * V + 3 * W + C)
    if V >= 600 and C >= 3:
        rest = rng.integers(1, C + 1, V - 513)                        # (-1, 0 or 3 .. C: classes 1 and 2 keep their counts)
        vclass = np.concatenate([np.full(256, 1), np.full(257, 2), np.where(rest < 3, rest - 2, rest)])
    else:
        vclass = rng.integers(-1, C + 1, V)
        vclass[0] = 1
    vclass = vclass[rng.permutation(V)].astype(np.int32)
    nb = (W + 3) // 4
    blocks = rng.integers(0, C, (B, nb, nb))
    blocks = np.where(rng.uniform(size=blocks.shape) < 0.4, rng.integers(1, min(C, 3), blocks.shape), blocks)   # (the large classes)
    labels = np.stack([np.kron(bl, np.ones((4, 4), np.int64))[:W, :W] for bl in blocks])
    if C > 2:
        labels[labels == C - 1] = 0
    for val in (-1, C, 255):
        labels[rng.uniform(size=labels.shape) < 0.03] = val
    if B == 3:
        labels[2][(labels[2] >= 0) & (labels[2] < C)] = 0
    cam = np.stack([np.full(B, 2.0), np.full(B, 4.0), 0.5 + np.arange(B), np.ones(B)], 1).astype(np.float32)
    X = rng.uniform(-0.25 * W, 0.75 * W, (B, V))
    Y = rng.uniform(-0.125 * W, 0.375 * W, (B, V))
    if ties:
        grid = rng.uniform(size=(B, V)) < 0.5
        X = np.where(grid, rng.integers(0, max(2, min(2 * W, 12)), (B, V)) / 4.0, X)
        Y = np.where(grid, rng.integers(0, max(2, min(2 * W, 12)), (B, V)) / 8.0, Y)
    verts = np.stack([X, Y, rng.normal(size=(B, V))], 2).astype(np.float32)
    vweight = None
    if weights:
        vweight = rng.uniform(0.2, 1.0, (B, V)).astype(np.float32)
        u = rng.uniform(size=(B, V))
        vweight[u < 0.08] = 0.0
        vweight[u > 0.95] = np.nan
        if C > 2:
            vweight[0, vclass == 1] = 0.0
    return dict(verts=verts, cam=cam, vweight=vweight, labels=labels.astype(np.int32), vclass=vclass, C=C, W=W)


def reference(p, sigma=None, slack=0.5, flip_rows=True, g_v=None, g_p=None):
    """The oracle over the rows of a problem -> (list of forward dicts, list of gradient dicts or None)."""
    B = len(p["verts"])
    fw = [orc.forward(p["verts"][b], p["cam"][b], p["labels"][b], p["vclass"], p["C"],
                      None if p["vweight"] is None else p["vweight"][b], sigma, slack, flip_rows) for b in range(B)]
    if g_v is None and g_p is None:
        return fw, None
    gr = [orc.grads(fw[b], p["verts"][b], p["cam"][b], None if g_v is None else g_v[b], None if g_p is None else g_p[b])
          if fw[b]["status"] == 0 else None for b in range(B)]
    return fw, gr


def compare(got, fw, gr=None, grads=None, rows=None):
    """got: dict of numpy arrays by the op's names (e_m2i, e_i2m, near_pix, near_vert, d2_v, d2_p, proj, status) against the
    oracle's rows: indices and status exactly, floats to the bar (Inf and NaN in the same places).  grads = (dverts, dcam).
    -> the worst ratio of error to bar."""
    worst = 0.0

    def floats(name, a, ref, T, b):
        nonlocal worst
        a, ref = np.asarray(a, np.float64).reshape(-1), np.asarray(ref, np.float64).reshape(-1)
        fin = np.isfinite(ref)
        assert np.array_equal(np.isnan(a), np.isnan(ref)), "%s row %d: NaN elsewhere" % (name, b)
        assert np.array_equal(a[~fin & ~np.isnan(ref)], ref[~fin & ~np.isnan(ref)]), "%s row %d: Inf elsewhere" % (name, b)
        ok, ratio = orc.within(a[fin], ref[fin], np.asarray(T, np.float64).reshape(-1)[fin])
        worst = max(worst, ratio)
        assert ok, "%s row %d: %.3g times the bar" % (name, b, ratio)
    for b in (range(len(fw)) if rows is None else rows):
        f = fw[b]
        assert int(got["status"][b]) == f["status"], "status row %d" % b
        for name in ("near_pix", "near_vert"):
            if got.get(name) is not None:
                want = f[name] if f["status"] == 0 else np.full_like(f[name], -1)
                assert np.array_equal(np.asarray(got[name][b]).reshape(-1), want), "%s row %d" % (name, b)
        for name in ("e_m2i", "e_i2m", "d2_v", "d2_p", "proj"):
            if got.get(name) is not None:
                floats(name, got[name][b], f[name], f["T_" + name], b)
        if grads is not None:
            dverts, dcam = grads
            if f["status"] != 0:
                assert np.isnan(np.asarray(dverts[b])).all() and np.isnan(np.asarray(dcam[b])).all(), "gradient row %d" % b
            else:
                floats("dverts", dverts[b], gr[b]["dverts"], gr[b]["T_dverts"], b)
                floats("dcam", dcam[b], gr[b]["dcam"], gr[b]["T_dcam"], b)
    return worst
