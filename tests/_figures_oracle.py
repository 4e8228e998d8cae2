"""NumPy restatement of the figure rules (ilps_amd.figures / csrc/figure.hip), independent of both implementations: int64
and np.float32 arithmetic, a plain loop over the vertices in painter's order with the disc as an offset mask, a plain
loop over the channels for the arg-max.  Also the inputs the CPU and the GPU tests share."""
import numpy as np

CLAMP = np.float32(1048576.0)


def default_lut():
    from ilps_amd.render import default_palette
    return (default_palette().astype(np.float32) * np.float32(255.0)).astype(np.uint8)


def argmax_nan_high(scores):
    """(..., C) -> (...) int64: NaN above every number, the first NaN wins, ties to the lower channel."""
    s = np.asarray(scores, np.float32)
    best_v = s[..., 0].copy()
    best_i = np.zeros(s.shape[:-1], np.int64)
    for c in range(1, s.shape[-1]):
        v = s[..., c]
        with np.errstate(invalid="ignore"):
            beats = np.where(np.isnan(best_v), False, np.isnan(v) | (v > best_v))
        best_v = np.where(beats, v, best_v)
        best_i = np.where(beats, c, best_i)
    return best_i


def seg_colour(x, H, W, lut=None, bad=(0, 0, 0), background=None, alpha_q=128):
    """x: (B, h, w, C) float scores or (B, h, w) integer labels -> (B, H, W, 3) uint8."""
    x = np.asarray(x)
    lab = argmax_nan_high(x) if x.dtype.kind == "f" else x.astype(np.int64)
    lut = default_lut() if lut is None else np.asarray(lut, np.uint8)
    B, h, w = lab.shape
    out = np.empty((B, H, W, 3), np.uint8)
    for i in range(H):
        for j in range(W):
            l = lab[:, (i * h) // H, (j * w) // W]
            for b in range(B):
                col = lut[l[b]].astype(np.int64) if 0 <= l[b] < len(lut) else np.asarray(bad, np.int64)
                if background is not None:
                    bg = background[b, i, j].astype(np.int64)
                    col = (alpha_q * col + (256 - alpha_q) * bg + 128) >> 8 if l[b] != 0 else bg
                out[b, i, j] = col
    return out


def disc_mask(r):
    d = np.arange(-r, r + 1, dtype=np.int64)
    return d[:, None] ** 2 + d[None, :] ** 2 <= r * r                      # [dy + r, dx + r]


def centre(s, u, v, H):
    """The rounded centre of one vertex: fp32 product, clamp to +-2^20, round half to even."""
    su = np.clip(np.float32(s) * np.float32(u), -CLAMP, CLAMP)
    sv = np.clip(np.float32(s) * np.float32(v), -CLAMP, CLAMP)
    return int(np.rint(su)), (H - 1) - int(np.rint(sv))


def scatter_vertex(proj, H, W, s, r, order, keep=None):
    """(B, V, 3) -> (B, H, W) int32 winner per pixel, -1 for none.  Vertices are painted in increasing index: in index
    order every one overwrites what is there; in depth order only a strictly larger z does (ties stay with the lower
    index)."""
    proj = np.asarray(proj, np.float32)
    B, V, _ = proj.shape
    win = np.full((B, H, W), -1, np.int32)
    zbuf = np.full((B, H, W), -np.inf, np.float32)
    disc = disc_mask(r)
    for b in range(B):
        for k in range(V):
            u, v, z = proj[b, k]
            if keep is not None and keep[b, k] == 0:
                continue
            if not (np.isfinite(u) and np.isfinite(v)) or (order == "depth" and not np.isfinite(z)):
                continue
            with np.errstate(over="ignore"):
                cx, cy = centre(s, u, v, H)
            i0, i1, j0, j1 = max(cy - r, 0), min(cy + r, H - 1), max(cx - r, 0), min(cx + r, W - 1)
            if i0 > i1 or j0 > j1:
                continue
            m = disc[i0 - cy + r:i1 - cy + r + 1, j0 - cx + r:j1 - cx + r + 1]
            if order == "depth":
                zs = zbuf[b, i0:i1 + 1, j0:j1 + 1]
                m = m & ((win[b, i0:i1 + 1, j0:j1 + 1] < 0) | (z > zs))
                zs[m] = z
            win[b, i0:i1 + 1, j0:j1 + 1][m] = k
    return win


def scatter_rgb(win, colours=None, colour=(31, 119, 180), image=None, alpha_q=230, canvas=(255, 255, 255)):
    """The picture of a winner map: colours[winner] or `colour` where covered, the image over the canvas elsewhere."""
    B, H, W = win.shape
    cv = np.asarray(canvas, np.int64)
    if image is not None:
        under = ((alpha_q * image.astype(np.int64) + (256 - alpha_q) * cv + 128) >> 8).astype(np.uint8)
    else:
        under = np.broadcast_to(cv.astype(np.uint8), (B, H, W, 3))
    top = colours[np.maximum(win, 0)] if colours is not None else np.broadcast_to(np.asarray(colour, np.uint8), (B, H, W, 3))
    return np.where((win >= 0)[..., None], top, under).astype(np.uint8)


# ---- shared inputs --------------------------------------------------------------------------------------------------------------
def seg_scores(B, h, w, C, seed):
    """Scores on a coarse grid of values (exact ties everywhere) with NaN in one and in several channels and +-inf."""
    rng = np.random.default_rng(seed)
    s = (rng.integers(-3, 4, (B, h, w, C)) * 0.5).astype(np.float32)
    flat = s.reshape(-1, C)
    n = flat.shape[0]
    for k, row in enumerate(rng.permutation(n)[:max(1, n // 3)]):
        kind = k % 6
        if kind == 0:
            flat[row, rng.integers(0, C)] = np.nan
        elif kind == 1:
            flat[row, rng.choice(C, size=min(C, 3), replace=False)] = np.nan
        elif kind == 2:
            flat[row, rng.integers(0, C)] = np.inf
        elif kind == 3:
            flat[row, rng.integers(0, C)] = -np.inf
        elif kind == 4:
            flat[row] = -np.inf
        else:
            flat[row] = flat[row, 0]                                     # every channel equal
    return s


def seg_labels(B, h, w, K, seed):
    """An integer map over [-1, K]: both out-of-table values occur."""
    rng = np.random.default_rng(seed)
    l = rng.integers(-1, K + 1, (B, h, w)).astype(np.int32)
    l.reshape(-1)[:2] = (-1, K)
    return l


def random_image(B, H, W, seed):
    return np.random.default_rng(seed).integers(0, 256, (B, H, W, 3)).astype(np.uint8)


def scatter_proj(B, V, H, W, r, s, seed):
    """(B, V, 3) float32 projections whose scaled centres spread over the image and a margin of r + 2 around it, with
    planted vertices (as many as V allows, in a seed-dependent rotation): on and next to columns and rows 63 / 64,
    outside the image by less and by more than r, a pile on one pixel with equal z, s u exactly at .5, non-finite and
    huge u, NaN z."""
    rng = np.random.default_rng(seed)
    m = r + 2
    p = np.empty((B, V, 3), np.float32)
    p[..., 0] = rng.uniform(-m, W + m, (B, V)) / s
    p[..., 1] = rng.uniform(-m, H + m, (B, V)) / s
    p[..., 2] = rng.integers(-4, 5, (B, V)) * 0.25                        # few depths: ties between distant indices
    f = lambda x: np.float32(x) / np.float32(s)
    px, py = min(W - 1, 20), min(H - 1, 11)
    planted = [(f(63), f(H - 1 - 63), 0.5), (f(64), f(H - 1 - 64), 0.5), (f(62), f(H - 1 - 64), 0.25),
               (f(65), f(H - 1 - 63), 0.75), (f(63), f(5), -0.0), (f(5), f(H - 1 - 64), 0.0),
               (f(-r), f(3), 1.0), (f(-r - 1), f(4), 1.0), (f(W - 1 + r), f(2), 1.0), (f(W + r), f(2), 1.0),
               (f(3), f(-r), 1.0), (f(3), f(H - 1 + r), 1.0), (f(3), f(H + r + 3), 1.0), (f(-r + 1 if r else 0), f(H - 1), 2.0),
               (f(px), f(py), 0.5), (f(px), f(py), 0.5), (f(px), f(py), 0.5), (f(px), f(py), 0.5), (f(px), f(py), 0.25),
               (f(px), f(py), 0.5), (f(10.5), f(7.5), 0.3), (f(11.5), f(8.5), 0.3), (f(12.5), f(6.5), 0.3),
               (np.nan, f(3), 9.0), (f(3), np.nan, 9.0), (np.inf, f(3), 9.0), (f(3), -np.inf, 9.0), (1e30, f(3), 9.0),
               (f(3), -1e30, 9.0), (f(7), f(7), np.nan), (f(8), f(9), np.inf), (f(9), f(8), -np.inf), (f(7), f(7), -3.0)]
    for b in range(B):
        rot = (seed + 5 * b) % len(planted)
        slots = rng.permutation(V)[:len(planted)]
        for k, slot in enumerate(slots):
            p[b, slot] = planted[(rot + k) % len(planted)]
    return p


def scatter_keep(B, V, seed):
    """(B, V) uint8 with zeros among ones; mesh 0 keeps nothing when there is more than one mesh."""
    k = (np.random.default_rng(seed).random((B, V)) < 0.8).astype(np.uint8)
    if B > 1:
        k[0] = 0
    return k


def vertex_colours(V, seed):
    return np.random.default_rng(seed).integers(0, 256, (V, 3)).astype(np.uint8)


# ---- the cases of the issue, run against any device (tests/test_figures_cpu.py: "cpu", tests/test_gpu_figures.py: the GPU) ---
SEG_SRC = ((1, 1), (48, 48), (5, 7))
SEG_OUT = ((1, 1), (48, 48), (63, 65), (100, 37))
SEG_C = (2, 32)
ALPHAS_Q = (0, 128, 256)
SC_B = (1, 3)
SC_V = (1, 255, 257, 6890)
SC_HW = ((1, 1), (63, 63), (64, 64), (65, 65), (96, 130))
SC_R = (0, 1, 3, 16)


def check_seg_colour(device, hw, HW):
    """Scores at both channel counts and an integer map, plain and over a background at every alpha, at one source and
    one picture size: the bytes of the oracle."""
    import torch
    from ilps_amd import figures
    (h, w), (H, W) = hw, HW
    B = 2
    bg = random_image(B, H, W, 11 + H)
    tbg = torch.from_numpy(bg).to(device)
    for C in SEG_C:
        s = seg_scores(B, h, w, C, 100 * h + C)
        ts = torch.from_numpy(s).to(device)
        lut = default_lut()[:C] if C == 2 else None                        # (a table shorter than the default one too)
        want = seg_colour(s, H, W, lut=lut)
        got = figures.seg_colour(ts, (W, H), lut=None if lut is None else torch.from_numpy(lut))
        assert got.dtype == torch.uint8 and got.device.type == torch.device(device).type
        assert np.array_equal(got.cpu().numpy(), want), ("scores", hw, HW, C)
        for aq in ALPHAS_Q:
            want = seg_colour(s, H, W, lut=lut, background=bg, alpha_q=aq)
            got = figures.seg_colour(ts, (W, H), lut=None if lut is None else torch.from_numpy(lut), background=tbg,
                                     alpha=aq / 256.0)
            assert np.array_equal(got.cpu().numpy(), want), ("scores over background", hw, HW, C, aq)
    K = 7
    lut = vertex_colours(K, 5)
    l = seg_labels(B, h, w, K, 3 + w)
    tl = torch.from_numpy(l).to(device)
    want = seg_colour(l, H, W, lut=lut, bad=(250, 1, 2))
    got = figures.seg_colour(tl, (W, H), lut=torch.from_numpy(lut), bad_colour=(250, 1, 2))
    assert np.array_equal(got.cpu().numpy(), want), ("labels", hw, HW)
    got = figures.seg_colour(tl.to(torch.int64), (W, H), lut=torch.from_numpy(lut), bad_colour=(250, 1, 2))
    assert np.array_equal(got.cpu().numpy(), want), ("int64 labels", hw, HW)
    for aq in ALPHAS_Q:
        want = seg_colour(l, H, W, lut=lut, bad=(250, 1, 2), background=bg, alpha_q=aq)
        got = figures.seg_colour(tl, (W, H), lut=torch.from_numpy(lut), bad_colour=(250, 1, 2), background=tbg, alpha=aq / 256.0)
        assert np.array_equal(got.cpu().numpy(), want), ("labels over background", hw, HW, aq)


def check_scatter(device, HW, r, Bs=SC_B, Vs=SC_V, s=2.0, run=None):
    """Every B and V of the issue at one picture size and radius, in both orders: vertex and rgb are the oracle's.  The
    options rotate over the combinations: keep, per-vertex colours, an image under the discs.  run: another way to make
    the call (the torch op), with `figures.scatter_points`' signature."""
    import torch
    from ilps_amd import figures
    H, W = HW
    run = figures.scatter_points if run is None else run
    n = 0
    for B in Bs:
        for V in Vs:
            n += 1
            seed = 1000 * H + 10 * r + n
            p = scatter_proj(B, V, H, W, r, s, seed)
            keep = scatter_keep(B, V, seed) if n % 2 == 0 else None
            cols = vertex_colours(V, seed) if n % 3 != 0 else None
            img = random_image(B, H, W, seed) if n % 4 < 2 else None
            tp = torch.from_numpy(p).to(device)
            kw = dict(keep=None if keep is None else torch.from_numpy(keep).to(device),
                      colours=None if cols is None else torch.from_numpy(cols).to(device),
                      image=None if img is None else torch.from_numpy(img).to(device))
            for order in ("index", "depth"):
                want_v = scatter_vertex(p, H, W, s, r, order, keep)
                want_rgb = scatter_rgb(want_v, cols, (9, 8, 7), img, 230, (255, 250, 245))
                rgb, vert = run(tp, (W, H), s, radius=r, order=order, colour=(9, 8, 7), canvas=(255, 250, 245),
                                return_vertex=True, **kw)
                tag = (B, V, HW, r, order)
                assert vert.dtype == torch.int32 and rgb.dtype == torch.uint8
                assert np.array_equal(vert.cpu().numpy(), want_v), tag + ("%d winners differ" % int(
                    (vert.cpu().numpy() != want_v).sum()),)
                assert np.array_equal(rgb.cpu().numpy(), want_rgb), tag
