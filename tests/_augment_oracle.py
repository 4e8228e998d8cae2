"""NumPy restatement of the data generator's semantics, in two precisions:

* float64: the definition (`dtype=np.float64`) - Keras 2.1's `apply_transform` with `order=0, mode='nearest'` on
  the coordinates of the fp32-rounded matrix;
* float32: the kernel's arithmetic operation for operation (`dtype=np.float32`): sr = (m00 r + m01 c) + m02 in
  that order, NumPy multiplying and adding in separate steps (no FMA), then floor(s + 0.5) and the clamp in fp32.

Test infrastructure only; nothing here is imported by the package."""
import numpy as np

REF_DRAWS = dict(rotation_range=10., width_shift_range=0.05, height_shift_range=0.05, shear_range=0.15, zoom_range=0.15,
                 horizontal_flip=False)                                   # train.py:96-109
WIDE_DRAWS = dict(rotation_range=40., width_shift_range=0.2, height_shift_range=0.2, shear_range=0.2, zoom_range=0.2,
                  horizontal_flip=True)                                   # train_autoencoder.py:82-89


def draws(rng, B, rotation_range=0., width_shift_range=0., height_shift_range=0., shear_range=0., zoom_range=0.,
          horizontal_flip=False):
    """One set of draws per sample from a NumPy generator (the tests' own source of draws)."""
    u = lambda a: rng.uniform(-a, a, B)
    return {"theta": u(rotation_range), "tx": u(height_shift_range), "ty": u(width_shift_range), "shear": u(shear_range),
            "zx": rng.uniform(1 - zoom_range, 1 + zoom_range, B), "zy": rng.uniform(1 - zoom_range, 1 + zoom_range, B),
            "flip": (rng.uniform(size=B) < 0.5).astype(np.float64) * float(horizontal_flip)}


def matrix_from_draws(d, h, w, shear_in_degrees=False):
    """(B, 2, 3) float64: C R T S Z C^-1 [F] as 3 x 3 products, the way Keras composes them."""
    B = len(d["theta"])
    out = np.zeros((B, 2, 3))
    for i in range(B):
        th = np.deg2rad(d["theta"][i])
        sh = np.deg2rad(d["shear"][i]) if shear_in_degrees else d["shear"][i]
        R = np.array([[np.cos(th), -np.sin(th), 0], [np.sin(th), np.cos(th), 0], [0, 0, 1]])
        T = np.array([[1, 0, d["tx"][i] * h], [0, 1, d["ty"][i] * w], [0, 0, 1]])
        S = np.array([[1, -np.sin(sh), 0], [0, np.cos(sh), 0], [0, 0, 1]])
        Z = np.diag([d["zx"][i], d["zy"][i], 1.0])
        C = np.array([[1, 0, h / 2 + 0.5], [0, 1, w / 2 + 0.5], [0, 0, 1]])
        Ci = np.array([[1, 0, -(h / 2 + 0.5)], [0, 1, -(w / 2 + 0.5)], [0, 0, 1]])
        M = C @ R @ T @ S @ Z @ Ci
        if d["flip"][i] > 0:
            M = M @ np.array([[1, 0, 0], [0, -1, w - 1], [0, 0, 1]])
        out[i] = M[:2]
    return out


def coords(M, h, w, dtype):
    """Source coordinates (sr, sc), each (h, w), of one 2 x 3 matrix in `dtype` arithmetic, in the defined order."""
    m = np.asarray(M, np.float32).astype(dtype)
    r = np.arange(h, dtype=dtype)[:, None]
    c = np.arange(w, dtype=dtype)[None, :]
    with np.errstate(all="ignore"):
        sr = (m[0, 0] * r + m[0, 1] * c) + m[0, 2]
        sc = (m[1, 0] * r + m[1, 1] * c) + m[1, 2]
    return sr.astype(dtype), sc.astype(dtype)


def clamp(x, hi):
    """[0, hi] in floating point; NaN -> 0, infinities to the ends."""
    with np.errstate(all="ignore"):
        x = np.where(x >= 0, x, 0).astype(x.dtype)
        return np.where(x > hi, x.dtype.type(hi), x)


def nearest_index(s, n):
    with np.errstate(all="ignore"):
        f = np.floor(s + s.dtype.type(0.5))
    return clamp(f, n - 1).astype(np.int64)


def pool_index(i, n, S):
    """Index on the n-sized grid -> index in a plane stored with S entries: floor((i + 0.5) S / n) in integers."""
    return ((2 * i + 1) * S) // (2 * n)


def warp_nearest(plane, M, h, w, dtype=np.float32):
    """plane (Hs, Ws[, C]) -> (h, w[, C]): the texels the nearest mode selects."""
    sr, sc = coords(M, h, w, dtype)
    ir, ic = nearest_index(sr, h), nearest_index(sc, w)
    return plane[pool_index(ir, h, plane.shape[0]), pool_index(ic, w, plane.shape[1])]


def warp_bilinear(plane, M, dtype=np.float32):
    """plane (h, w[, C]) -> (h, w[, C]) in `dtype`, before the rescale."""
    h, w = plane.shape[:2]
    sr, sc = coords(M, h, w, dtype)
    cr, cc = clamp(sr, h - 1), clamp(sc, w - 1)
    r0f, c0f = np.floor(cr), np.floor(cc)
    ar, ac = (cr - r0f).astype(dtype), (cc - c0f).astype(dtype)
    r0, c0 = r0f.astype(np.int64), c0f.astype(np.int64)
    r1, c1 = np.minimum(r0 + 1, h - 1), np.minimum(c0 + 1, w - 1)
    if plane.ndim == 3:
        ar, ac = ar[..., None], ac[..., None]
    p = plane.astype(dtype)
    one = dtype(1)
    top = (one - ac) * p[r0, c0] + ac * p[r0, c1]
    bot = (one - ac) * p[r1, c0] + ac * p[r1, c1]
    return ((one - ar) * top + ar * bot).astype(dtype)


def _rows(pool, B, index):
    N = pool.shape[0]
    idx = np.arange(B) if index is None else np.asarray(index, np.int64)
    return np.clip(idx, 0, N - 1)


def warp_images(pool, mats, hw, index=None, rescale=1 / 255., interpolation="nearest", dtype=np.float32):
    """pool (N, Hs, Ws[, C]) uint8 -> (B, C, H, W).  nearest: `dtype` is the precision of the coordinates that select
    the texel; the value is float32(texel) * float32(rescale), the one fp32 multiply of the definition, in float32
    whatever `dtype`.  bilinear: coordinates, interpolation and the rescale all in `dtype`."""
    h, w = hw
    mats = np.asarray(mats, np.float32)
    if pool.ndim == 3:
        pool = pool[..., None]
    nearest = interpolation == "nearest"
    out = np.empty((len(mats), pool.shape[3], h, w), np.float32 if nearest else dtype)
    for b, n in enumerate(_rows(pool, len(mats), index)):
        if nearest:
            t = warp_nearest(pool[n], mats[b], h, w, dtype).astype(np.float32) * np.float32(rescale)
        else:
            t = warp_bilinear(pool[n], mats[b], dtype) * dtype(rescale)
        out[b] = t.transpose(2, 0, 1)
    return out


def warp_labels(pool, mats, hw, index=None, binarize=False, dtype=np.float32):
    """pool (N, hs, ws) uint8 -> (B, h, w) int32."""
    h, w = hw
    mats = np.asarray(mats, np.float32)
    out = np.empty((len(mats), h, w), np.int32)
    for b, n in enumerate(_rows(pool, len(mats), index)):
        t = warp_nearest(pool[n], mats[b], h, w, dtype).astype(np.int32)
        out[b] = (t > 0) if binarize else t
    return out


def near_tie(mats, hw, delta):
    """(B, h, w) bool: the float64 coordinate puts sr + 0.5 or sc + 0.5 within delta of an integer - the only pixels
    where fp32 arithmetic may select another texel than the float64 definition."""
    h, w = hw
    out = np.zeros((len(mats), h, w), bool)
    for b, M in enumerate(np.asarray(mats, np.float32)):
        sr, sc = coords(M, h, w, np.float64)
        for s in (sr, sc):
            t = s + 0.5
            out[b] |= np.abs(t - np.rint(t)) <= delta
    return out


def delta_for(size):
    """Three fp32 roundings of terms up to 2 max(h, w): <= 1.5 ulp(2 max(h, w)); 2e-4 up to 256, 4e-4 up to 512."""
    if size <= 256:
        return 2e-4
    if size <= 512:
        return 4e-4
    raise ValueError("no bound derived above 512")
