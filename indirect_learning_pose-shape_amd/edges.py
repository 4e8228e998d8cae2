"""Canny edge maps on the device: the "edge image + joint heatmaps" proxy of the synthetic-training papers that follow
"Synthetic Training for Accurate 3D Human Pose and Shape Estimation" (same author), computed from the renderer's rgb at
training time and from a photograph at test time.  Beyond the reference, which has no edge detector.

    edges = canny_edges(render_mesh(...)["rgb"], low=60, high=120)                  # (B, H, W) uint8, 0 / 1
    x = edge_proxy_inputs(load_images(...), joints, low=60, high=120)               # (B, 1 + J, H, W) fp32: photographs
    batches = SyntheticBatches(..., seg="edges", edge=dict(low=60, high=120))       # the training loop's inputs

Two launches of csrc/edges.hip (`edge_classes`, `link_edges`), no host synchronisation, capturable in a graph.  Exact integer
arithmetic: the result equals tests/_edges_oracle.py bit for bit.  The formulation follows cv2.Canny's (aperture 3,
fixed-point direction test, asymmetric ties); no bit-equality with cv2 is claimed - the text below is the contract
(include/smplraster.h has the same text).

Per image, independently of every other image in the batch:

Grey.  g (H, W) in 0..255 from one of four source forms: "GREY_U8" (B, H, W) uint8; "RGB_U8" (B, H, W, 3) uint8;
  "RGB_F32_HWC" (B, H, W, 3) fp32 (`render_mesh`'s rgb); "RGB_F32_CHW" (B, 3, H, W) fp32 (`load_images`' output).
  A float channel c is first quantised: q = clamp(floorf(c * scale + 0.5f), 0, 255) - one fp32 multiply, then one fp32 add,
  no FMA; NaN gives 0, +inf 255, -inf 0.  scale defaults to 255; with `load_images`' default rescale = 1 / 255 this returns
  the original byte exactly.  Colour to grey: g = (4899 R + 9617 G + 1868 B + 8192) >> 14.  bgr swaps which channel is R.
Blur (optional).  5 x 5 binomial, w = [1 4 6 4 1], indices clamped to the image (replicate border):
  g' = (sum_ij w_i w_j g + 128) >> 8.
Gradient.  3 x 3 Sobel on g', replicate border: gx = (right column weighted 1 2 1) - (left column), gy = (row below) -
  (row above).  l2 False: m = |gx| + |gy|, and a pixel counts against a threshold t iff m > t.  l2 True: m = gx^2 + gy^2, iff
  m > t^2.  Everything fits int32.
Thresholds.  Integers 0 <= low <= high <= 2047, as scalars or per image as a (B, 2) int32 device tensor `thr` (random
  thresholds are an augmentation).  A row whose pair violates the range yields an all-zero map for that row and status 1 in
  the optional (B,) int32 status; other rows are unaffected.
Non-maximum suppression.  m outside the image is 0.  ax = |gx|, ay = |gy|, T = 13573 ax.
  If (ay << 15) < T: keep iff m > m[y][x-1] and m >= m[y][x+1].
  Else if (ay << 15) > T + (ax << 16): keep iff m > m[y-1][x] and m >= m[y+1][x].
  Else s = -1 if (gx ^ gy) < 0 else 1: keep iff m > m[y-1][x-s] and m > m[y+1][x+s].
Class.  2 (strong): kept and over high; 1 (weak): kept and over low; 0: everything else.
Link (hysteresis).  A pixel is an edge iff its class is >= 1 and an 8-connected path of pixels of class >= 1 joins it to a
  pixel of class >= 2.  In a class map handed in from outside any value >= 2 is strong.  Output uint8: `value` (1..255) on
  edges, 0 elsewhere.  The exact transitive closure: no iteration cap truncates it.
Limits.  1 <= H, W <= 512; B >= 0 (B = 0 is a no-op).

Device tensors run the kernels; CPU tensors run `canny_edges_torch`, the plain-torch restatement, which on device tensors
is the stock composition the kernels are timed against (tools/edges_time.py).  The maps are not differentiable."""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

from . import _lib
from ._lib import check, ptr, stream

FORMS = {"GREY_U8": 0, "RGB_U8": 1, "RGB_F32_HWC": 2, "RGB_F32_CHW": 3}        # SMPLR_EDGE_* of include/smplraster.h
MAX_SIDE, MAX_THRESHOLD = 512, 2047


def infer_form(src):
    """The source form of a tensor by dtype and shape; a float (B, 3, H, 3) is taken as RGB_F32_HWC."""
    if isinstance(src, torch.Tensor):
        if src.dtype == torch.uint8 and src.dim() == 3:
            return "GREY_U8"
        if src.dtype == torch.uint8 and src.dim() == 4 and src.shape[3] == 3:
            return "RGB_U8"
        if src.dtype == torch.float32 and src.dim() == 4 and src.shape[3] == 3:
            return "RGB_F32_HWC"
        if src.dtype == torch.float32 and src.dim() == 4 and src.shape[1] == 3:
            return "RGB_F32_CHW"
    raise ValueError("src must be (B, H, W) uint8, (B, H, W, 3) uint8 or float32, or (B, 3, H, W) float32")


def _source(src, form):
    """-> (form name, B, H, W) of a checked source."""
    if not isinstance(src, torch.Tensor):
        raise ValueError("src must be a torch.Tensor")
    if form is None:
        form = infer_form(src)
    if form not in FORMS:
        raise ValueError("form must be one of %s, got %r" % (", ".join(map(repr, FORMS)), form))
    f = FORMS[form]
    want = torch.uint8 if f <= 1 else torch.float32
    ok = src.dtype == want and src.dim() == (3 if f == 0 else 4) and (f == 0 or src.shape[1 if f == 3 else 3] == 3)
    if not ok:
        raise ValueError("a %s source is %s %s, got %s %s" % (form, {0: "(B, H, W)", 1: "(B, H, W, 3)", 2: "(B, H, W, 3)",
                                                                     3: "(B, 3, H, W)"}[f], want, tuple(src.shape), src.dtype))
    B, H, W = int(src.shape[0]), int(src.shape[2 if f == 3 else 1]), int(src.shape[3 if f == 3 else 2])
    if not (1 <= H <= MAX_SIDE and 1 <= W <= MAX_SIDE):
        raise ValueError("images must be 1..%d on a side, got %d x %d" % (MAX_SIDE, H, W))
    return form, B, H, W


def _thresholds(low, high, thr, B, dev):
    """-> (low, high, thr): the scalars checked, or thr (B, 2) int32 on the source's device."""
    if thr is not None:
        if low is not None or high is not None:
            raise ValueError("give low and high, or thr, not both")
        if not isinstance(thr, torch.Tensor) or tuple(thr.shape) != (B, 2) or thr.dtype != torch.int32:
            raise ValueError("thr must be a (B, 2) int32 tensor of (low, high) rows")
        if thr.device != dev:
            raise ValueError("thr lives on %s, src on %s" % (thr.device, dev))
        return 0, 0, thr.contiguous()
    if low is None or high is None:
        raise ValueError("low and high (or thr) are required")
    if int(low) != low or int(high) != high:
        raise ValueError("low and high are integers (float thresholds are out of scope), got %r, %r" % (low, high))
    low, high = int(low), int(high)
    if not 0 <= low <= high <= MAX_THRESHOLD:
        raise ValueError("thresholds must satisfy 0 <= low <= high <= %d, got %d, %d" % (MAX_THRESHOLD, low, high))
    return low, high, None


def _scale(scale):
    scale = float(scale)
    if not math.isfinite(scale):
        raise ValueError("scale must be finite, got %r" % scale)
    return scale


def _value(value):
    if int(value) != value or not 1 <= int(value) <= 255:
        raise ValueError("value must be an integer in 1..255, got %r" % (value,))
    return int(value)


def _class_map(classes):
    if not isinstance(classes, torch.Tensor) or classes.dim() != 3 or classes.dtype != torch.uint8:
        raise ValueError("classes must be a (B, H, W) uint8 tensor")
    B, H, W = (int(s) for s in classes.shape)
    if not (1 <= H <= MAX_SIDE and 1 <= W <= MAX_SIDE):
        raise ValueError("class maps must be 1..%d on a side, got %d x %d" % (MAX_SIDE, H, W))
    return B, H, W


# ---- the plain-torch restatement ------------------------------------------------------------------------------------------
def quantize_torch(c, scale=255.0):
    """A float tensor's bytes: clamp(floor(c * scale + 0.5), 0, 255) in fp32, NaN -> 0.  -> int32."""
    v = torch.floor(c.to(torch.float32) * torch.tensor(scale, dtype=torch.float32, device=c.device) + 0.5)
    zero = torch.zeros((), dtype=torch.float32, device=c.device)
    v = torch.where(v >= 255.0, torch.full_like(zero, 255.0), torch.where(v > 0.0, v, zero))
    return v.to(torch.int32)


def _pad_replicate(t, p):
    # (replication padding has no integer form: 0..255 pass through fp32 unchanged)
    return F.pad(t.to(torch.float32)[:, None], (p, p, p, p), mode="replicate")[:, 0].to(torch.int32)


def grey_torch(src, form=None, scale=255.0, bgr=False):
    """The definition's grey image, (B, H, W) int32."""
    form, B, H, W = _source(src, form)
    f = FORMS[form]
    if f == 0:
        return src.to(torch.int32)
    ch = src.unbind(1 if f == 3 else 3)
    ch = [c.to(torch.int32) for c in ch] if f == 1 else [quantize_torch(c, scale) for c in ch]
    r, g, b = (ch[2], ch[1], ch[0]) if bgr else ch
    return (4899 * r + 9617 * g + 1868 * b + 8192) >> 14


def edge_classes_torch(src, *, form=None, low=None, high=None, blur=True, l2=True, scale=255.0, bgr=False, thr=None,
                       return_status=False):
    """`edge_classes` in plain torch on any device: integer tensors and `F.pad(mode="replicate")`."""
    form, B, H, W = _source(src, form)
    low, high, thr = _thresholds(low, high, thr, B, src.device)
    g = grey_torch(src, form, _scale(scale), bgr)
    if blur:
        p = _pad_replicate(g, 2)
        h = p[:, :, 0:W] + 4 * p[:, :, 1:W + 1] + 6 * p[:, :, 2:W + 2] + 4 * p[:, :, 3:W + 3] + p[:, :, 4:W + 4]
        g = (h[:, 0:H] + 4 * h[:, 1:H + 1] + 6 * h[:, 2:H + 2] + 4 * h[:, 3:H + 3] + h[:, 4:H + 4] + 128) >> 8
    p = _pad_replicate(g, 1)
    gx = (p[:, 0:H, 2:] + 2 * p[:, 1:H + 1, 2:] + p[:, 2:, 2:]) - (p[:, 0:H, 0:W] + 2 * p[:, 1:H + 1, 0:W] + p[:, 2:, 0:W])
    gy = (p[:, 2:, 0:W] + 2 * p[:, 2:, 1:W + 1] + p[:, 2:, 2:]) - (p[:, 0:H, 0:W] + 2 * p[:, 0:H, 1:W + 1] + p[:, 0:H, 2:])
    ax, ay = gx.abs(), gy.abs()
    m = gx * gx + gy * gy if l2 else ax + ay
    q = F.pad(m, (1, 1, 1, 1))                                              # m outside the image is 0
    left, right, up, down = q[:, 1:H + 1, 0:W], q[:, 1:H + 1, 2:], q[:, 0:H, 1:W + 1], q[:, 2:, 1:W + 1]
    ul, ur, dl, dr = q[:, 0:H, 0:W], q[:, 0:H, 2:], q[:, 2:, 0:W], q[:, 2:, 2:]
    T = 13573 * ax
    horizontal = (ay << 15) < T
    vertical = (ay << 15) > T + (ax << 16)
    keep = torch.where(horizontal, (m > left) & (m >= right),
                       torch.where(vertical, (m > up) & (m >= down),
                                   torch.where((gx ^ gy) < 0, (m > ur) & (m > dl), (m > ul) & (m > dr))))
    if thr is None:
        thr = torch.tensor([[low, high]], dtype=torch.int32, device=src.device).expand(B, 2)
    lo, hi = thr[:, 0, None, None], thr[:, 1, None, None]
    valid = (lo >= 0) & (lo <= hi) & (hi <= MAX_THRESHOLD)
    lo, hi = lo.clamp(0, MAX_THRESHOLD), hi.clamp(0, MAX_THRESHOLD)
    if l2:
        lo, hi = lo * lo, hi * hi
    classes = ((keep & valid).to(torch.uint8) * ((m > lo).to(torch.uint8) + (m > hi).to(torch.uint8))).contiguous()
    return (classes, (~valid).reshape(B).to(torch.int32)) if return_status else classes


def link_edges_torch(classes, value=1):
    """`link_edges` in plain torch: one ring of 3 x 3 dilation inside the weak set per pass, until `.any()` (a host
    synchronisation per pass) says nothing changed."""
    _class_map(classes)
    value = _value(value)
    weak, e = classes >= 1, classes >= 2
    while True:
        n = (F.max_pool2d(e.to(torch.float32)[:, None], 3, 1, 1)[:, 0] > 0) & weak
        if not bool((n != e).any()):
            break
        e = n
    return (e.to(torch.uint8) * value).contiguous()


def canny_edges_torch(src, *, form=None, low=None, high=None, blur=True, l2=True, scale=255.0, bgr=False, thr=None, value=1,
                      return_status=False):
    """The module's definition in plain torch, on any device: some forty element-wise and padding passes and a hysteresis
    loop that asks the host whether anything changed.  The CPU path of `edge_classes`, `link_edges` and `canny_edges`, and
    on the HIP device the baseline the kernels are timed against."""
    res = edge_classes_torch(src, form=form, low=low, high=high, blur=blur, l2=l2, scale=scale, bgr=bgr, thr=thr,
                             return_status=return_status)
    if return_status:
        return link_edges_torch(res[0], value), res[1]
    return link_edges_torch(res, value)


# ---- the kernels --------------------------------------------------------------------------------------------------------------
@_lib.on_device
def _classify(src, f, B, H, W, scale, bgr, blur, l2, low, high, thr, classes, status):
    check(_lib.load().smplr_edge_classify(ptr(src), f, B, H, W, scale, int(bool(bgr)), int(bool(blur)), int(bool(l2)), low, high,
                                          ptr(thr), ptr(classes), ptr(status), stream()), "smplr_edge_classify")


@_lib.on_device
def _link(classes, B, H, W, value, edges):
    check(_lib.load().smplr_edge_link(ptr(classes), B, H, W, value, ptr(edges), stream()), "smplr_edge_link")


def edge_classes(src, *, form=None, low=None, high=None, blur=True, l2=True, scale=255.0, bgr=False, thr=None,
                 return_status=False):
    """src (see the module's source forms; without `form` it is inferred from dtype and shape, `infer_form`) -> the class
    map (B, H, W) uint8: 0 none, 1 weak, 2 strong.  low, high: integers 0 <= low <= high <= 2047, or thr (B, 2) int32 on
    the device in their place.  return_status: also the (B,) int32 status (1: the row's thresholds were out of range and
    its map is zero).  A non-contiguous source is made contiguous.  One launch, no host synchronisation; CPU tensors run
    `edge_classes_torch`."""
    form, B, H, W = _source(src, form)
    low, high, thr = _thresholds(low, high, thr, B, src.device)
    scale = _scale(scale)
    if not src.is_cuda:
        kw = dict(low=low, high=high) if thr is None else dict(thr=thr)
        return edge_classes_torch(src, form=form, blur=blur, l2=l2, scale=scale, bgr=bgr, return_status=return_status, **kw)
    classes = torch.empty((B, H, W), dtype=torch.uint8, device=src.device)
    status = torch.empty((B,), dtype=torch.int32, device=src.device) if return_status else None
    if B:
        _classify(src.contiguous(), FORMS[form], B, H, W, scale, bgr, blur, l2, low, high, thr, classes, status)
    return (classes, status) if return_status else classes


def link_edges(classes, value=1, out=None):
    """classes (B, H, W) uint8 (`edge_classes`', or any map: >= 2 strong, 1 weak) -> edges (B, H, W) uint8, `value` on
    every weak-or-strong pixel that an 8-connected path of such pixels joins to a strong one, 0 elsewhere.  out: write
    into this contiguous uint8 tensor.  One launch, one workgroup per image, no host synchronisation; CPU tensors run
    `link_edges_torch`."""
    B, H, W = _class_map(classes)
    value = _value(value)
    if out is not None:
        if not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or tuple(out.shape) != (B, H, W) or \
                not out.is_contiguous() or out.device != classes.device:
            raise ValueError("out must be a contiguous uint8 tensor of shape %s on classes' device" % ((B, H, W),))
    if not classes.is_cuda:
        res = link_edges_torch(classes, value)
        return res if out is None else out.copy_(res)
    if out is None:
        out = torch.empty((B, H, W), dtype=torch.uint8, device=classes.device)
    if B:
        _link(classes.contiguous(), B, H, W, value, out)
    return out


def canny_edges(src, *, form=None, low=None, high=None, blur=True, l2=True, scale=255.0, bgr=False, thr=None, value=1,
                return_status=False, out=None):
    """`edge_classes` then `link_edges`: src -> edges (B, H, W) uint8 (and the status with return_status)."""
    res = edge_classes(src, form=form, low=low, high=high, blur=blur, l2=l2, scale=scale, bgr=bgr, thr=thr,
                       return_status=return_status)
    if return_status:
        return link_edges(res[0], value, out), res[1]
    return link_edges(res, value, out)


def edge_proxy_inputs(images, joints=None, keep=None, boxes=None, *, sigma=4.0, **canny):
    """The edge proxy of a batch of pictures: images (any source form) -> (B, 1 + J, H, W) fp32, channel 0 the edge map
    (0 / 1, zeroed inside `boxes`), then one Gaussian heatmap per joint (joints (B, J, 2) in pixels, keep (B, J) uint8), as
    `synthetic.proxy_inputs`.  canny: `canny_edges`' keywords (low and high, or thr, at least).  Three launches: classify,
    link, and the proxy kernel for the edge channel, the heat channels and the boxes together.  The test-time path for
    photographs (`preprocess.load_images`) and a 2D detector's joints."""
    from .synthetic import proxy_inputs
    if canny.get("value", 1) != 1 or canny.get("return_status") or canny.get("out") is not None:
        raise ValueError("edge_proxy_inputs takes canny_edges' keywords except value, return_status and out")
    edges = canny_edges(images, **canny)
    return proxy_inputs(edges, joints, keep, None, boxes, num_parts=1, seg="silhouette", sigma=sigma)
