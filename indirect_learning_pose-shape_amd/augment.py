"""Device-side data generators: the reference's Keras `ImageDataGenerator` pairs (train.py:96-143,
train_stage2_silhouette.py:127-177, train_autoencoder.py:82-127) over a uint8 pool that lives in HBM.

    gen = ImageDataGenerator(rotation_range=10, width_shift_range=0.05, height_shift_range=0.05, shear_range=0.15,
                             zoom_range=0.15, fill_mode='nearest', rescale=1 / 255.)
    batches = DeviceBatches(images_u8, masks_u8, 128, 256, 48, gen)          # (N,256,256,3) / (N,h,w) uint8 on the device
    fit(trainer, batches, trials, steps_per_trial)

One set of random draws per sample gives one 2 x 3 matrix per output size (what seeding the reference's image and mask
generators alike buys it); `csrc/augment.hip` gathers the encoder's (B, 3, H, W) fp32 input and the loss head's
(B, w, w) int32 class map straight out of the pool.  No host traffic and no host synchronisation per batch.  The
semantics (Keras 2.1's `random_transform` + `apply_transform` restated, and where they deviate) are INTEGRATION.md
section 4d; `tests/_augment_oracle.py` is their NumPy form.  There is no CPU path for the warp: CPU tensors raise.
The matrix builder, the draws and the batch index stream are plain torch and run on any device."""
from __future__ import annotations

import math

import torch

from . import _gather, _lib
from ._gather import MAX_OUT, _hw, _out_hw
from ._lib import check, ptr, stream

IMAGE_NEAREST, IMAGE_BILINEAR, LABEL, LABEL_BINARY = 0, 1, 2, 3      # SMPLR_WARP_* of include/smplraster.h
MAX_POOL = 8192
DRAW_KEYS = ("theta", "tx", "ty", "shear", "zx", "zy", "flip")


def _zoom_bounds(zoom_range):
    if isinstance(zoom_range, (tuple, list)):
        if len(zoom_range) != 2:
            raise ValueError("zoom_range is a float or (lower, upper)")
        return float(zoom_range[0]), float(zoom_range[1])
    return 1.0 - float(zoom_range), 1.0 + float(zoom_range)


def random_draws(B, generator=None, rotation_range=0., width_shift_range=0., height_shift_range=0., shear_range=0.,
                 zoom_range=0., horizontal_flip=False, device=None, uniform=None):
    """One set of draws per sample, as `ImageDataGenerator.random_transform` makes them: dict of (B,) float64 tensors
    theta ~ U(-rotation_range, +) in degrees, tx ~ U(-height_shift_range, +) and ty ~ U(-width_shift_range, +) as
    fractions of the plane, shear ~ U(-shear_range, +), zx, zy ~ U(1 - zoom_range, 1 + zoom_range) independently
    (or zoom_range = (lo, hi)), flip ~ Bernoulli(0.5) as 0 / 1 iff horizontal_flip.  They come from `generator` on
    its device (or `device`), not from Keras' NumPy stream.  uniform: a (7, B) tensor of U[0, 1) numbers to use
    instead of drawing (rows in the order of DRAW_KEYS) - a static input for a captured graph.  No host sync."""
    if uniform is None:
        dev = torch.device(device) if device is not None else (generator.device if generator is not None else torch.device("cpu"))
        uniform = torch.rand((7, int(B)), dtype=torch.float64, device=dev, generator=generator)
    elif tuple(uniform.shape) != (7, int(B)):
        raise ValueError("uniform must be (7, B)")
    u = uniform.to(torch.float64)
    lo, hi = _zoom_bounds(zoom_range)
    sym = lambda row, a: (2.0 * u[row] - 1.0) * float(a)
    return {"theta": sym(0, rotation_range), "tx": sym(1, height_shift_range), "ty": sym(2, width_shift_range),
            "shear": sym(3, shear_range), "zx": lo + u[4] * (hi - lo), "zy": lo + u[5] * (hi - lo),
            "flip": ((u[6] < 0.5) & bool(horizontal_flip)).to(torch.float64)}


def affine_matrices(draws, size, shear_in_degrees=False):
    """draws (dict of (B,) tensors, see `random_draws`; missing keys are neutral) -> (B, 2, 3) fp32 matrices for an
    h x w plane, output -> input in (row, column) index space: M = C R T S Z C^-1, C the translation by
    (h / 2 + 0.5, w / 2 + 0.5) (Keras' `transform_matrix_offset_center`), T shifting by (tx h, ty w), a flip folded in
    as M F with F: c -> w - 1 - c.  Formed in float64 on the draws' device, rounded to fp32 once; no host sync.
    shear is in radians (Keras 2.1) unless shear_in_degrees."""
    h, w = _hw(size)
    ref = next(iter(draws.values()))
    get = lambda k, d: draws[k].to(torch.float64) if k in draws else torch.full_like(ref, d, dtype=torch.float64)
    th = get("theta", 0.) * (math.pi / 180.0)
    sh = get("shear", 0.)
    if shear_in_degrees:
        sh = sh * (math.pi / 180.0)
    tx, ty = get("tx", 0.) * h, get("ty", 0.) * w
    zx, zy = get("zx", 1.), get("zy", 1.)
    c, s, cs, ss = torch.cos(th), torch.sin(th), torch.cos(sh), torch.sin(sh)
    ox, oy = h / 2.0 + 0.5, w / 2.0 + 0.5
    a00, a01, a02 = c * zx, -(c * ss + s * cs) * zy, c * tx - s * ty          # A = R T S Z
    a10, a11, a12 = s * zx, (c * cs - s * ss) * zy, s * tx + c * ty
    m02 = ((a02 + ox) - a00 * ox) - a01 * oy                                   # C A C^-1
    m12 = ((a12 + oy) - a10 * ox) - a11 * oy
    if "flip" in draws:
        f = draws["flip"] > 0
        m02, a01 = torch.where(f, m02 + a01 * (w - 1), m02), torch.where(f, -a01, a01)
        m12, a11 = torch.where(f, m12 + a11 * (w - 1), m12), torch.where(f, -a11, a11)
    m = torch.stack([a00, a01, m02, a10, a11, m12], dim=-1) + 0.0              # (-0 -> +0)
    return m.to(torch.float32).reshape(-1, 2, 3)


def _pool(pool, name, label):
    pool = _lib.require_cuda(pool, name, torch.uint8)
    if label and pool.dim() == 4 and pool.shape[3] == 1:
        pool = pool.reshape(pool.shape[:3])
    if label and pool.dim() != 3:
        raise ValueError("%s must be (N, hs, ws) or (N, hs, ws, 1) uint8" % name)
    if not label and not (pool.dim() == 3 or (pool.dim() == 4 and pool.shape[3] in (1, 3))):
        raise ValueError("%s must be (N, Hs, Ws, 3), (N, Hs, Ws, 1) or (N, Hs, Ws) uint8" % name)
    if pool.shape[0] < 1 or not (1 <= pool.shape[1] <= MAX_POOL and 1 <= pool.shape[2] <= MAX_POOL):
        raise ValueError("%s needs N >= 1 and planes of 1..%d on a side" % (name, MAX_POOL))
    return pool


@_lib.on_device
def _warp(pool, matrices, index, out, shape, dtype, mode, rescale):
    dev = pool.device
    matrices = _lib.require_cuda(matrices, "matrices")
    if matrices.dim() != 3 or tuple(matrices.shape[1:]) != (2, 3):
        raise ValueError("matrices must be (B, 2, 3)")
    B = int(matrices.shape[0])
    if matrices.device != dev:
        raise RuntimeError("matrices live on %s, the pool on %s" % (matrices.device, dev))
    if index is not None:
        index = _gather._index(index, B, dev, "the pool")
    shape = (B,) + shape
    out = _gather._out(out, shape, dtype, dev, "the pool's")
    if B == 0:
        return out
    C = int(pool.shape[3]) if pool.dim() == 4 else 1
    check(_lib.load().smplr_affine_warp(ptr(pool), int(pool.shape[0]), int(pool.shape[1]), int(pool.shape[2]), C,
                                        ptr(matrices), ptr(index), int(index is not None and index.dtype == torch.int64),
                                        B, shape[-2], shape[-1], mode, float(rescale), ptr(out), stream()),
          "smplr_affine_warp")
    return out


def warp_images(pool, matrices, out_hw, index=None, rescale=1 / 255., interpolation="nearest", out=None):
    """pool (N, Hs, Ws, 3) uint8 NHWC on the HIP device (or (N, Hs, Ws[, 1]) grayscale) -> (B, 3 | 1, H, W) fp32 NCHW =
    float(texel) * rescale, sample b warped by matrices[b] (see `affine_matrices`) out of pool row index[b] (int32 /
    int64, default 0..B-1, repeats allowed; values are clamped to the pool by the kernel, not checked here).
    interpolation "nearest" (Keras 2.1's order 0, edge replicate; the pool may be stored at another size than out_hw
    and is then read through PIL's NEAREST resize) or "bilinear" (pool size = out_hw).  out: write into this tensor
    (a captured graph replays into it).  No host sync."""
    if interpolation not in ("nearest", "bilinear"):
        raise ValueError("interpolation must be 'nearest' or 'bilinear'")
    pool = _pool(pool, "pool", False)
    H, W = _out_hw(out_hw)
    if interpolation == "bilinear" and (int(pool.shape[1]), int(pool.shape[2])) != (H, W):
        raise ValueError("bilinear needs pool size = out_hw")
    C = int(pool.shape[3]) if pool.dim() == 4 else 1
    return _warp(pool, matrices, index, out, (C, H, W), torch.float32,
                 IMAGE_NEAREST if interpolation == "nearest" else IMAGE_BILINEAR, 1.0 if rescale is None else rescale)


def warp_labels(pool, matrices, out_hw, index=None, binarize=False, out=None):
    """pool (N, hs, ws) or (N, hs, ws, 1) uint8 on the HIP device -> (B, h, w) int32: the nearest texel's value,
    unchanged (what `classlab` makes of a part mask), or `texel > 0` with binarize (the silhouette head's labels).
    Other arguments as `warp_images`."""
    pool = _pool(pool, "pool", True)
    H, W = _out_hw(out_hw)
    return _warp(pool, matrices, index, out, (H, W), torch.int32, LABEL_BINARY if binarize else LABEL, 1.0)


class ImageDataGenerator:
    """The reference's `keras.preprocessing.image.ImageDataGenerator(...)` keyword set, as far as it uses it
    (train.py:96-109, train_stage2_silhouette.py:127-133, train_autoencoder.py:82-89): holds the ranges;
    `DeviceBatches` draws from them.  `fill_mode` other than 'nearest' and every other Keras option raise
    NotImplementedError by name."""

    def __init__(self, rotation_range=0, width_shift_range=0, height_shift_range=0, shear_range=0, zoom_range=0,
                 horizontal_flip=False, rescale=None, fill_mode='nearest', **unsupported):
        for k in unsupported:
            raise NotImplementedError("ImageDataGenerator option %r is not implemented (rotation_range, "
                                      "width_shift_range, height_shift_range, shear_range, zoom_range, horizontal_flip, "
                                      "rescale and fill_mode='nearest' are)" % k)
        if fill_mode != 'nearest':
            raise NotImplementedError("ImageDataGenerator fill_mode=%r is not implemented (only 'nearest')" % (fill_mode,))
        self.rotation_range = float(rotation_range)
        self.width_shift_range = float(width_shift_range)
        self.height_shift_range = float(height_shift_range)
        self.shear_range = float(shear_range)
        self.zoom_range = _zoom_bounds(zoom_range)
        self.horizontal_flip = bool(horizontal_flip)
        self.rescale = rescale
        self.fill_mode = fill_mode

    def ranges(self):
        return {"rotation_range": self.rotation_range, "width_shift_range": self.width_shift_range,
                "height_shift_range": self.height_shift_range, "shear_range": self.shear_range,
                "zoom_range": self.zoom_range, "horizontal_flip": self.horizontal_flip}

    def random_draws(self, B, generator=None, device=None, uniform=None):
        return random_draws(B, generator, device=device, uniform=uniform, **self.ranges())


class BatchIndexer:
    """The row order of Keras' batch iterator as an endless stream of (batch_size,) int64 index tensors on
    `device`: one `torch.randperm(N)` per epoch (0..N-1 in order without shuffle); nothing is dropped - a batch
    that the epoch's rest cannot fill takes its tail from the next epoch's permutation, so every window of N
    consecutive indices starting at an epoch boundary visits each row once.  No host sync."""

    def __init__(self, N, batch_size, shuffle=True, generator=None, device=None):
        if N < 1 or batch_size < 1:
            raise ValueError("N and batch_size must be positive")
        self.N, self.batch_size, self.shuffle, self.generator = int(N), int(batch_size), bool(shuffle), generator
        self.device = torch.device(device) if device is not None else (generator.device if generator is not None
                                                                        else torch.device("cpu"))
        self.epochs = 0
        self._rest = torch.empty(0, dtype=torch.int64, device=self.device)

    def _epoch(self):
        self.epochs += 1
        if self.shuffle:
            return torch.randperm(self.N, generator=self.generator, device=self.device)
        return torch.arange(self.N, device=self.device)

    def __iter__(self):
        return self

    def __next__(self):
        parts, have = [self._rest], int(self._rest.numel())
        while have < self.batch_size:
            parts.append(self._epoch())
            have += self.N
        buf = torch.cat(parts) if len(parts) > 1 else parts[0]
        self._rest = buf[self.batch_size:]
        return buf[:self.batch_size]


class DeviceBatches:
    """An endless iterator of (images, labels) or, with silh_wh, (images, labels, silh_labels) for
    `training.fit(trainer, batches, ...)`: images (B, 3, H, H) fp32 and labels (B, w, w) int32 (silh_labels
    (B, s, s) int32 = label > 0), contiguous, on the pools' device - what `SegTrainer.step` takes with no copy or cast.

    images_pool (N, Hs, Ws, 3) uint8 and labels_pool (N, hs, ws[, 1]) uint8 live on the HIP device (the decoded
    files; any stored size: `flow_from_directory`'s NEAREST resize to target_size is folded into the gather).
    image_args: an `ImageDataGenerator` or the dict of its keywords; one set of draws per sample warps the image and
    its label maps alike.  Rows are shuffled per epoch with `torch.randperm` on the device, nothing is dropped (see
    `BatchIndexer`).  generator: a `torch.Generator` on the device (default: a new one seeded with `seed`).
    binarize: labels = label > 0 (a pool of 0 / 255 silhouette masks, train_stage2_silhouette.py:138-140, for
    `trainer.step(images, None, labels)`).  interpolation: of the images, "nearest" (Keras 2.1) or "bilinear"."""

    def __init__(self, images_pool, labels_pool, batch_size, input_wh, output_wh, image_args, silh_wh=None, shuffle=True,
                 seed=1, generator=None, interpolation="nearest", binarize=False):
        self.images_pool = _pool(images_pool, "images_pool", False)
        self.labels_pool = _pool(labels_pool, "labels_pool", True)
        if self.labels_pool.shape[0] != self.images_pool.shape[0] or self.labels_pool.device != self.images_pool.device:
            raise ValueError("images_pool and labels_pool must hold the same samples on one device")
        self.args = image_args if isinstance(image_args, ImageDataGenerator) else ImageDataGenerator(**dict(image_args))
        self.batch_size = int(batch_size)
        self.input_hw, self.output_hw = _out_hw(input_wh), _out_hw(output_wh)
        self.silh_hw = None if silh_wh is None else _out_hw(silh_wh)
        self.interpolation, self.binarize = interpolation, bool(binarize)
        dev = self.images_pool.device
        if generator is None:
            generator = torch.Generator(device=dev)
            generator.manual_seed(int(seed))
        self.generator = generator
        self.indexer = BatchIndexer(int(self.images_pool.shape[0]), self.batch_size, shuffle, generator, dev)

    def __iter__(self):
        return self

    def __next__(self):
        idx = next(self.indexer)
        draws = self.args.random_draws(self.batch_size, self.generator)
        images = warp_images(self.images_pool, affine_matrices(draws, self.input_hw), self.input_hw, idx,
                             self.args.rescale, self.interpolation)
        labels = warp_labels(self.labels_pool, affine_matrices(draws, self.output_hw), self.output_hw, idx, self.binarize)
        if self.silh_hw is None:
            return images, labels
        silh = warp_labels(self.labels_pool, affine_matrices(draws, self.silh_hw), self.silh_hw, idx, binarize=True)
        return images, labels, silh
