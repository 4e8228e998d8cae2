"""The edge detector's definition (include/smplraster.h, ilps_amd/edges.py) in NumPy int64: loops over taps with clamped
index arrays, float quantisation in np.float32 step by step, hysteresis by an explicit stack flood.  Nothing here is shared
with the code under test."""
import numpy as np

FORMS = ("GREY_U8", "RGB_U8", "RGB_F32_HWC", "RGB_F32_CHW")


def quantize(c, scale=255.0):
    """clamp(floorf(c * scale + 0.5f), 0, 255): one fp32 multiply, one fp32 add; NaN -> 0, +inf -> 255, -inf -> 0."""
    with np.errstate(all="ignore"):
        p = (np.asarray(c, np.float32) * np.float32(scale)).astype(np.float32)
        v = np.floor((p + np.float32(0.5)).astype(np.float32))
    out = np.zeros(v.shape, np.int64)
    big = v >= 255                                                      # (a NaN fails both tests)
    mid = (v > 0) & ~big
    out[big] = 255
    out[mid] = v[mid].astype(np.int64)
    return out


def grey(img, form, scale=255.0, bgr=False):
    """One image of the given form -> (H, W) int64 in 0..255."""
    img = np.asarray(img)
    if form == "GREY_U8":
        return img.astype(np.int64)
    if form == "RGB_F32_CHW":
        img = np.moveaxis(img, 0, -1)
    ch = img.astype(np.int64) if form == "RGB_U8" else quantize(img, scale)
    r, g, b = (ch[..., 2], ch[..., 1], ch[..., 0]) if bgr else (ch[..., 0], ch[..., 1], ch[..., 2])
    return (4899 * r + 9617 * g + 1868 * b + 8192) >> 14


def _at(a, ys, xs):
    H, W = a.shape
    return a[np.clip(ys, 0, H - 1)[:, None], np.clip(xs, 0, W - 1)[None, :]]


def blur5(g):
    H, W = g.shape
    ys, xs = np.arange(H), np.arange(W)
    w = (1, 4, 6, 4, 1)
    acc = np.zeros((H, W), np.int64)
    for i in range(5):
        for j in range(5):
            acc += w[i] * w[j] * _at(g, ys + i - 2, xs + j - 2)
    return (acc + 128) >> 8


def sobel(g):
    H, W = g.shape
    ys, xs = np.arange(H), np.arange(W)
    t = lambda dy, dx: _at(g, ys + dy, xs + dx)
    gx = (t(-1, 1) + 2 * t(0, 1) + t(1, 1)) - (t(-1, -1) + 2 * t(0, -1) + t(1, -1))
    gy = (t(1, -1) + 2 * t(1, 0) + t(1, 1)) - (t(-1, -1) + 2 * t(-1, 0) + t(-1, 1))
    return gx, gy


def classes_of_grey(g, low, high, blur=True, l2=True):
    """(H, W) int64 grey -> (H, W) uint8 classes, pixel by pixel."""
    H, W = g.shape
    if not 0 <= low <= high <= 2047:
        return np.zeros((H, W), np.uint8)
    if blur:
        g = blur5(g)
    gx, gy = sobel(g)
    m = gx * gx + gy * gy if l2 else np.abs(gx) + np.abs(gy)
    tl, th = (low * low, high * high) if l2 else (low, high)
    mp = np.zeros((H + 2, W + 2), np.int64)                              # m outside the image is 0
    mp[1:-1, 1:-1] = m
    out = np.zeros((H, W), np.uint8)
    for y in range(H):
        for x in range(W):
            v = int(m[y, x])
            if v <= tl:
                continue
            ax, ay = abs(int(gx[y, x])), abs(int(gy[y, x]))
            T = 13573 * ax
            M = lambda dy, dx: int(mp[y + 1 + dy, x + 1 + dx])
            if (ay << 15) < T:
                keep = v > M(0, -1) and v >= M(0, 1)
            elif (ay << 15) > T + (ax << 16):
                keep = v > M(-1, 0) and v >= M(1, 0)
            else:
                s = -1 if (int(gx[y, x]) ^ int(gy[y, x])) < 0 else 1
                keep = v > M(-1, -s) and v > M(1, s)
            if keep:
                out[y, x] = 2 if v > th else 1
    return out


def link(cls, value=1):
    """(H, W) classes -> (H, W) uint8 edges: a stack flood from every pixel of class >= 2 through pixels of class >= 1."""
    cls = np.asarray(cls)
    H, W = cls.shape
    seen = np.zeros((H, W), bool)
    stack = [(int(y), int(x)) for y, x in zip(*np.nonzero(cls >= 2))]
    for y, x in stack:
        seen[y, x] = True
    while stack:
        y, x = stack.pop()
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                yy, xx = y + dy, x + dx
                if 0 <= yy < H and 0 <= xx < W and not seen[yy, xx] and cls[yy, xx] >= 1:
                    seen[yy, xx] = True
                    stack.append((yy, xx))
    return (seen * value).astype(np.uint8)


def classes(src, form, low=None, high=None, blur=True, l2=True, scale=255.0, bgr=False, thr=None):
    """A batch -> (classes (B, H, W) uint8, status (B,) int32); thr (B, 2) rows replace the scalars."""
    src = np.asarray(src)
    B = src.shape[0]
    out, status = [], np.zeros(B, np.int32)
    for b in range(B):
        lo, hi = (low, high) if thr is None else (int(thr[b][0]), int(thr[b][1]))
        status[b] = 0 if 0 <= lo <= hi <= 2047 else 1
        out.append(classes_of_grey(grey(src[b], form, scale, bgr), lo, hi, blur, l2))
    shape = (0,) + (src.shape[2:] if form == "RGB_F32_CHW" else src.shape[1:3])
    return (np.stack(out) if B else np.zeros(shape, np.uint8)), status


def canny(src, form, value=1, **kw):
    cls, status = classes(src, form, **kw)
    return (np.stack([link(c, value) for c in cls]) if len(cls) else cls), status


# ---- hand-built class maps for the link kernel ----------------------------------------------------------------------------
def boustrophedon(H, W):
    """Full even rows of weak pixels, joined alternately at the right and the left end by one pixel of the odd row between
    them, one strong pixel at the path's start (0, 0).  -> (class map, number of pixels on the path)."""
    c = np.zeros((H, W), np.uint8)
    c[0::2] = 1
    for k, y in enumerate(range(1, H - 1, 2)):
        c[y, W - 1 if k % 2 == 0 else 0] = 1
    c[0, 0] = 2
    return c, int((c > 0).sum())


def staircase(H, W):
    c = np.zeros((H, W), np.uint8)
    for i in range(min(H, W)):
        c[i, i] = 1
    c[min(H, W) - 1, min(H, W) - 1] = 2
    return c
