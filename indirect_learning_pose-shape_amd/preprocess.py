"""Input preprocessing on the device: the reference's `load_input_img` (predict.py:17-25, evaluate.py:13-19,
evaluate3d.py:13-19), `load_input_seg` (predict_autoencoder.py:17-24, evaluate_autoencoder.py:13-20),
`preprocessing.pad_image`, the ground-truth resize of evaluate.py:96-100 and the webcam crop of
predict_realtime.py:52-58, over ragged uint8 images that live in one device buffer.

    imgs = RaggedImages.from_arrays(decoded_bgr_images, dev)        # every file its own height and width
    gts = RaggedImages.from_arrays(decoded_masks, dev)
    evaluate_iou_and_acc(net, decoder, EvalBatches(imgs, gts, 32, 256, 48, pad=True, swap_rb=True))
    for images in EvalBatches(imgs, None, 1, 256, 48):
        predict_batch(net, decoder, images)

One launch of `csrc/preprocess.hip` per batch pads, resizes, reorders and rescales into the (B, C, H, W) fp32 tensor the
encoder takes, another makes the (B, h, w) int32 ground-truth maps; no host traffic and no host synchronisation per batch.
The semantics (cv2's bilinear geometry in exact integers, both nearest rules, `pad_image` with its odd case, and where
cv2 itself is not imitated) are INTEGRATION.md section 4e; `tests/_preprocess_oracle.py` is their NumPy form.  There is no
CPU path for the resize: CPU tensors raise.  File decoding stays the caller's."""
from __future__ import annotations

import numpy as np
import torch

from . import _gather, _lib
from ._gather import MAX_OUT, _out_hw
from ._lib import check, ptr, stream

IMAGE_BILINEAR, IMAGE_NEAREST, LABEL, LABEL_BINARY = 0, 1, 2, 3      # SMPLR_RESIZE_* modes of include/smplraster.h
PAD, SWAP_RB, QUANTIZE, PIL_RULE = 1, 2, 4, 8                        # ... and flags
MAX_SIDE = 8192


def pad_geometry(h, w, pad=True):
    """(Hp, Wp, top, left) of `pad_image` (preprocessing.py:6-23) for an h x w image: w < h puts b = (h - w) // 2 zero
    columns on either side, otherwise b = (w - h) // 2 zero rows above and below.  With an odd difference the plane stays
    one short of square (101 x 40 -> 101 x 100), as the reference's does.  pad=False: the image itself."""
    h, w = int(h), int(w)
    if h < 1 or w < 1:
        raise ValueError("an image has at least one row and one column")
    if not pad:
        return h, w, 0, 0
    if w < h:
        b = (h - w) // 2
        return h, w + 2 * b, 0, b
    b = (w - h) // 2
    return h + 2 * b, w, b, 0


def validate_descriptors(desc, data_bytes, channels):
    """The kernel's check of every row (byte offset, pitch, h, w), on the host: offset >= 0, sides 1..8192,
    pitch >= w C, offset + (h - 1) pitch + w C <= data_bytes.  Raises ValueError naming the first row that fails."""
    desc = np.asarray(desc, np.int64).reshape(-1, 4)
    C = int(channels)
    for i, (off, pitch, h, w) in enumerate(desc.tolist()):
        if off < 0:
            raise ValueError("descriptor %d: negative offset %d" % (i, off))
        if not (1 <= h <= MAX_SIDE and 1 <= w <= MAX_SIDE):
            raise ValueError("descriptor %d: sides %d x %d outside 1..%d" % (i, h, w, MAX_SIDE))
        if pitch < w * C:
            raise ValueError("descriptor %d: pitch %d below w * C = %d" % (i, pitch, w * C))
        if off + (h - 1) * pitch + w * C > data_bytes:
            raise ValueError("descriptor %d: the view ends at byte %d of %d" % (i, off + (h - 1) * pitch + w * C, data_bytes))
    return desc


class RaggedImages:
    """N uint8 images of their own heights and widths in one flat buffer: `data` (bytes,) uint8 and `desc` (N, 4) int64
    on one device - per image the byte offset of its first pixel, its row pitch in bytes, h and w - with a copy of the
    descriptors on the host (`desc_host`, a NumPy array; validated there once).  Pixels are HWC with `channels` in
    {1, 3} for the whole set.  Crops are new descriptors over the same buffer."""

    def __init__(self, data, desc_host, channels, desc=None):
        if not isinstance(data, torch.Tensor) or data.dtype != torch.uint8 or data.dim() != 1 or not data.is_contiguous():
            raise ValueError("data must be a flat contiguous uint8 tensor")
        if int(channels) not in (1, 3):
            raise ValueError("channels must be 1 or 3")
        self.data, self.channels = data, int(channels)
        self.desc_host = validate_descriptors(desc_host, int(data.numel()), self.channels)
        if len(self.desc_host) < 1:
            raise ValueError("RaggedImages needs at least one image")
        self.desc = torch.from_numpy(self.desc_host.copy()).to(data.device) if desc is None else desc

    @classmethod
    def from_arrays(cls, arrays, device):
        """list of (h, w) or (h, w, C) uint8 arrays (NumPy or CPU tensors), C the same for all -> one packed upload: the
        descriptor table and the pixels travel in one buffer, images back to back with pitch = w C."""
        arrs = [a.numpy() if isinstance(a, torch.Tensor) else np.asarray(a) for a in arrays]
        if not arrs:
            raise ValueError("from_arrays needs at least one image")
        C = None
        for i, a in enumerate(arrs):
            if a.dtype != np.uint8 or a.ndim not in (2, 3):
                raise ValueError("image %d must be a (h, w) or (h, w, C) uint8 array" % i)
            c = 1 if a.ndim == 2 else int(a.shape[2])
            if c not in (1, 3) or (C is not None and c != C):
                raise ValueError("image %d has %d channels (1 or 3, the same for every image)" % (i, c))
            C = c
        N = len(arrs)
        desc = np.zeros((N, 4), np.int64)
        off = 0
        for i, a in enumerate(arrs):
            h, w = int(a.shape[0]), int(a.shape[1])
            desc[i] = (off, w * C, h, w)
            off += h * w * C
        validate_descriptors(desc, off, C)
        head = N * 32
        buf = np.empty(head + off, np.uint8)
        buf[:head] = desc.view(np.uint8).reshape(-1)
        for a, (o, _, h, w) in zip(arrs, desc.tolist()):
            buf[head + o:head + o + h * w * C] = np.ascontiguousarray(a).reshape(-1)
        dev_buf = torch.from_numpy(buf).to(device)
        return cls(dev_buf[head:], desc, C, desc=dev_buf[:head].view(torch.int64).view(N, 4))

    @classmethod
    def from_dense(cls, tensor):
        """(N, H, W) or (N, H, W, C) uint8 tensor, contiguous -> equal-sized images over the tensor's own memory (no
        copy)."""
        if not isinstance(tensor, torch.Tensor) or tensor.dtype != torch.uint8 or tensor.dim() not in (3, 4):
            raise ValueError("from_dense takes a (N, H, W) or (N, H, W, C) uint8 tensor")
        if not tensor.is_contiguous():
            raise ValueError("from_dense takes a contiguous tensor (it does not copy)")
        N, H, W = (int(s) for s in tensor.shape[:3])
        C = int(tensor.shape[3]) if tensor.dim() == 4 else 1
        desc = np.empty((N, 4), np.int64)
        desc[:, 0] = np.arange(N, dtype=np.int64) * (H * W * C)
        desc[:, 1], desc[:, 2], desc[:, 3] = W * C, H, W
        return cls(tensor.view(-1), desc, C)

    def __len__(self):
        return int(self.desc_host.shape[0])

    @property
    def device(self):
        return self.data.device

    @property
    def sizes(self):
        """[(h, w)] per image."""
        return [(int(h), int(w)) for h, w in self.desc_host[:, 2:4].tolist()]

    def crop(self, rects):
        """rects: one (top, left, height, width) for every image or a list of one per image -> a RaggedImages of the
        views, over the same buffer: a larger offset, a smaller h and w, the same pitch.  A rectangle has to lie inside
        its image."""
        N = len(self)
        if len(rects) == 4 and all(isinstance(v, (int, np.integer)) for v in rects):
            rects = [tuple(rects)] * N
        if len(rects) != N:
            raise ValueError("crop takes one rectangle or one per image (%d)" % N)
        desc = self.desc_host.copy()
        for i, (t, l, hh, ww) in enumerate(rects):
            off, pitch, h, w = self.desc_host[i].tolist()
            t, l, hh, ww = int(t), int(l), int(hh), int(ww)
            if t < 0 or l < 0 or hh < 1 or ww < 1 or t + hh > h or l + ww > w:
                raise ValueError("crop %d: (%d, %d, %d, %d) leaves the %d x %d image" % (i, t, l, hh, ww, h, w))
            desc[i] = (off + t * pitch + l * self.channels, pitch, hh, ww)
        return RaggedImages(self.data, desc, self.channels)

    def center_crop_width(self, lo=0.25, hi=0.75):
        """Columns int(lo w) : int(hi w) of every image (predict_realtime.py:54)."""
        rects = []
        for h, w in self.sizes:
            a, b = int(lo * w), int(hi * w)
            rects.append((0, a, h, b - a))
        return self.crop(rects)


@_lib.on_device
def _resize(data, ragged, index, out, shape, dtype, mode, flags, rescale):
    _lib.require_cuda(data, "the image buffer", torch.uint8)
    dev = data.device
    desc = ragged.desc
    if not desc.is_cuda or desc.device != dev:
        raise RuntimeError("desc lives on %s, data on %s" % (desc.device, dev))
    if index is not None:
        index = _gather._index(index, None, dev, "the images")
    B = len(ragged) if index is None else int(index.shape[0])
    shape = (B,) + shape
    out = _gather._out(out, shape, dtype, dev, "the images'")
    if B == 0:
        return out
    check(_lib.load().smplr_resize_pad(ptr(data), int(data.numel()), ptr(desc), len(ragged), ragged.channels, ptr(index),
                                       int(index is not None and index.dtype == torch.int64), B, shape[-2], shape[-1],
                                       mode, flags, float(rescale), ptr(out), stream()),
          "smplr_resize_pad")
    return out


def _ragged(ragged, label):
    if not isinstance(ragged, RaggedImages):
        raise TypeError("expected a RaggedImages (RaggedImages.from_arrays / from_dense)")
    if label and ragged.channels != 1:
        raise ValueError("label maps have one channel, these images %d" % ragged.channels)
    return ragged


def _rule(nearest_rule):
    if nearest_rule not in ("cv2", "pil"):
        raise ValueError("nearest_rule must be 'cv2' or 'pil'")
    return PIL_RULE if nearest_rule == "pil" else 0


def load_images(ragged, out_hw, index=None, pad=False, interpolation="linear", swap_rb=False, rescale=1 / 255.,
                quantize=True, nearest_rule="cv2", out=None):
    """`load_input_img` / `load_input_seg` for a batch: rows index[b] of `ragged` (int32 / int64, default every image in
    order, repeats allowed; values are clamped to the table by the kernel, not checked here) -> (B, C, H, W) fp32 NCHW.
    pad: `pad_image` first.  interpolation "linear" (cv2.INTER_LINEAR's geometry in exact integers; quantize=True rounds
    to the uint8 level cv2.resize returns, half up, before the multiply; False keeps the exact weighted mean) or
    "nearest" (nearest_rule "cv2": (i S) // W, or "pil": ((2 i + 1) S) // (2 W)).  swap_rb: the reference's
    `[..., ::-1]` for buffers decoded as BGR.  rescale: 1 / 255., or 1 / (num_classes - 1) for `load_input_seg`; None
    multiplies by 1.  out: write into this tensor (a captured graph's static input).  No host sync."""
    if interpolation not in ("linear", "nearest"):
        raise ValueError("interpolation must be 'linear' or 'nearest'")
    flags = _rule(nearest_rule)
    ragged = _ragged(ragged, False)
    H, W = _out_hw(out_hw)
    if swap_rb and ragged.channels != 3:
        raise ValueError("swap_rb needs 3-channel images")
    flags |= (PAD if pad else 0) | (SWAP_RB if swap_rb else 0) | (QUANTIZE if quantize else 0)
    return _resize(ragged.data, ragged, index, out, (ragged.channels, H, W), torch.float32,
                   IMAGE_BILINEAR if interpolation == "linear" else IMAGE_NEAREST, flags, 1.0 if rescale is None else rescale)


def load_labels(ragged, out_hw, index=None, pad=False, nearest_rule="cv2", binarize=False, out=None):
    """`cv2.resize(mask, ..., INTER_NEAREST)` (evaluate.py:96-100) for a batch of 1-channel masks -> (B, h, w) int32: the
    nearest texel's value, unchanged, or `texel > 0` with binarize.  Other arguments as `load_images`."""
    flags = _rule(nearest_rule) | (PAD if pad else 0)
    ragged = _ragged(ragged, True)
    H, W = _out_hw(out_hw)
    return _resize(ragged.data, ragged, index, out, (H, W), torch.int32, LABEL_BINARY if binarize else LABEL, flags, 1.0)


class EvalBatches:
    """An iterable of (images, gt_maps) in file order, the last batch short, no shuffle: the `batches` argument of
    `evaluation.evaluate_iou_and_acc`.  images: RaggedImages of the photographs -> (B, C, H, W) fp32 at input_wh through
    `load_images` (pad, interpolation, swap_rb, rescale, quantize, nearest_rule); masks: RaggedImages of the 1-channel
    part masks -> (B, h, w) int32 at output_wh through `load_labels` (pad, nearest_rule, binarize).  masks=None yields
    the images alone (for `inference.predict_batch`).  `EvalBatches.autoencoder(masks, ...)` is the autoencoder's pair:
    the `load_input_seg` image and the ground-truth map, both from one mask set.  Can be iterated more than once."""

    def __init__(self, images, masks, batch_size, input_wh, output_wh, pad=False, interpolation="linear", swap_rb=False,
                 rescale=1 / 255., quantize=True, nearest_rule="cv2", binarize=False):
        self.images = _ragged(images, False)
        self.masks = None if masks is None else _ragged(masks, True)
        if self.masks is not None and (len(self.masks) != len(self.images) or self.masks.device != self.images.device):
            raise ValueError("images and masks must hold the same samples on one device")
        if int(batch_size) < 1:
            raise ValueError("batch_size must be positive")
        self.batch_size = int(batch_size)
        self.input_hw = _out_hw(input_wh)
        self.output_hw = None if output_wh is None else _out_hw(output_wh)
        if self.masks is not None and self.output_hw is None:
            raise ValueError("output_wh is needed for the ground-truth maps")
        self.image_args = dict(pad=bool(pad), interpolation=interpolation, swap_rb=bool(swap_rb), rescale=rescale,
                               quantize=bool(quantize), nearest_rule=nearest_rule)
        self.label_args = dict(pad=bool(pad), nearest_rule=nearest_rule, binarize=bool(binarize))

    @classmethod
    def autoencoder(cls, masks, batch_size, input_wh, output_wh, num_classes=32, pad=False, nearest_rule="cv2"):
        """(load_input_seg(mask) (B, 1, H, W) = nearest resize * 1 / (num_classes - 1), gt_map (B, h, w)) from one mask
        set (predict_autoencoder.py:17-24, evaluate_autoencoder.py:94-96)."""
        return cls(masks, masks, batch_size, input_wh, output_wh, pad=pad, interpolation="nearest",
                   rescale=1.0 / (int(num_classes) - 1), nearest_rule=nearest_rule)

    def __len__(self):
        return (len(self.images) + self.batch_size - 1) // self.batch_size

    def __iter__(self):
        N = len(self.images)
        for start in range(0, N, self.batch_size):
            idx = torch.arange(start, min(start + self.batch_size, N), device=self.images.device)
            images = load_images(self.images, self.input_hw, idx, **self.image_args)
            if self.masks is None:
                yield images
            else:
                yield images, load_labels(self.masks, self.output_hw, idx, **self.label_args)
