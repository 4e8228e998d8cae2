"""NumPy restatement of INTEGRATION.md section 4e (input preprocessing), in int64: `pad_image`, cv2's INTER_LINEAR
geometry as exact rationals num / D, the quantised form floor((2 num + D) / (2 D)), both nearest rules, and the packing of
ragged images into (data, desc).  This file is the tests' definition; nothing here is taken from the code under test."""
import numpy as np


def pad_geometry(h, w, pad=True):
    if not pad:
        return h, w, 0, 0
    if w < h:
        b = (h - w) // 2
        return h, w + 2 * b, 0, b
    b = (w - h) // 2
    return h + 2 * b, w, b, 0


def padded_plane(img, pad=True):
    """(h, w) or (h, w, C) uint8 -> the zero-padded plane (Hp, Wp, C) int64."""
    img = np.asarray(img)
    if img.ndim == 2:
        img = img[..., None]
    h, w, C = img.shape
    Hp, Wp, top, left = pad_geometry(h, w, pad)
    out = np.zeros((Hp, Wp, C), np.int64)
    out[top:top + h, left:left + w] = img
    return out


def linear_axis(n_out, S):
    """-> (s0, s1, r, d) int64 arrays of n_out entries: source indices, the numerator of s1's weight, d = 2 n_out."""
    i = np.arange(n_out, dtype=np.int64)
    n = (2 * i + 1) * S - n_out
    d = 2 * n_out
    s = n // d                                  # floor division
    r = n - s * d
    neg = n < 0
    s = np.where(neg, 0, s)
    r = np.where(neg, 0, r)
    hi = s >= S - 1
    s = np.where(hi, S - 1, s)
    r = np.where(hi, 0, r)
    return s, np.minimum(s + 1, S - 1), r, d


def bilinear_num(plane, H, W):
    """plane (Hp, Wp, C) int64 -> (num (H, W, C) int64, D)."""
    Hp, Wp, _ = plane.shape
    y0, y1, ry, dy = linear_axis(H, Hp)
    x0, x1, rx, dx = linear_axis(W, Wp)
    rx_, ry_ = rx[None, :, None], ry[:, None, None]
    p00, p01 = plane[y0][:, x0], plane[y0][:, x1]
    p10, p11 = plane[y1][:, x0], plane[y1][:, x1]
    num = (dy - ry_) * ((dx - rx_) * p00 + rx_ * p01) + ry_ * ((dx - rx_) * p10 + rx_ * p11)
    return num, dx * dy


def nearest_index(n_out, S, rule="cv2"):
    i = np.arange(n_out, dtype=np.int64)
    if rule == "cv2":
        return np.minimum((i * S) // n_out, S - 1)
    if rule == "pil":
        return ((2 * i + 1) * S) // (2 * n_out)
    raise ValueError(rule)


def nearest_plane(plane, H, W, rule="cv2"):
    Hp, Wp, _ = plane.shape
    return plane[nearest_index(H, Hp, rule)][:, nearest_index(W, Wp, rule)]


def load_image(img, out_hw, pad=False, interpolation="linear", swap_rb=False, rescale=1 / 255., quantize=True,
               nearest_rule="cv2"):
    """One image -> (C, H, W) float32, as the definition writes it; quantize=False returns float64 (num / D) * rescale
    with rescale rounded to float32 first (the value the kernel's result is compared with)."""
    H, W = out_hw
    plane = padded_plane(img, pad)
    if swap_rb:
        plane = plane[..., ::-1]
    rs = np.float32(1.0 if rescale is None else rescale)
    if interpolation == "nearest":
        q = nearest_plane(plane, H, W, nearest_rule)
        return (q.astype(np.float32) * rs).transpose(2, 0, 1)
    num, D = bilinear_num(plane, H, W)
    if quantize:
        q = (2 * num + D) // (2 * D)
        return (q.astype(np.float32) * rs).transpose(2, 0, 1)
    return (num.astype(np.float64) / np.float64(D) * np.float64(rs)).transpose(2, 0, 1)


def quantized_levels(img, out_hw, pad=False):
    num, D = bilinear_num(padded_plane(img, pad), *out_hw)
    return (2 * num + D) // (2 * D)


def load_label(mask, out_hw, pad=False, nearest_rule="cv2", binarize=False):
    q = nearest_plane(padded_plane(mask, pad), out_hw[0], out_hw[1], nearest_rule)[..., 0]
    return (q > 0).astype(np.int32) if binarize else q.astype(np.int32)


def pack(arrays):
    """list of uint8 arrays -> (data (bytes,) uint8, desc (N, 4) int64), images back to back, pitch = w C."""
    desc, chunks, off = [], [], 0
    for a in arrays:
        a = np.asarray(a)
        C = 1 if a.ndim == 2 else a.shape[2]
        h, w = a.shape[:2]
        desc.append((off, w * C, h, w))
        chunks.append(np.ascontiguousarray(a).reshape(-1))
        off += h * w * C
    return np.concatenate(chunks), np.asarray(desc, np.int64)
