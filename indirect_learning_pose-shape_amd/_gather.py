"""What the fronts of the per-sample gather kernels share (augment.py over csrc/augment.hip, preprocess.py over
csrc/preprocess.hip): sizes, the `index` operand and the `out` tensor.  Private; the checks raise what the fronts document."""
from __future__ import annotations

import torch

from . import _lib

MAX_OUT = 4096


def _hw(size):
    if isinstance(size, (tuple, list)):
        if len(size) != 2:
            raise ValueError("a size is H or (H, W)")
        return int(size[0]), int(size[1])
    return int(size), int(size)


def _out_hw(out_hw):
    H, W = _hw(out_hw)
    if not (1 <= H <= MAX_OUT and 1 <= W <= MAX_OUT):
        raise ValueError("out_hw must be 1..%d on a side" % MAX_OUT)
    return H, W


def _index(index, length, dev, noun):
    """index -> an int32 / int64 (B,) tensor on dev; length: the B it has to have, or None for any.  noun: what else
    lives on dev ("the pool" / "the images")."""
    if not isinstance(index, torch.Tensor) or index.dtype not in (torch.int32, torch.int64):
        raise TypeError("index must be an int32 or int64 tensor")
    index = _lib.require_cuda(index, "index", index.dtype)
    if index.dim() != 1 or (length is not None and int(index.shape[0]) != length):
        raise ValueError("index must be (B,)" + ("" if length is None else " = (%d,)" % length))
    if index.device != dev:
        raise RuntimeError("index lives on %s, %s on %s" % (index.device, noun, dev))
    return index


def _out(out, shape, dtype, dev, noun):
    """A new tensor, or the caller's after its checks.  noun: whose device ("the pool's" / "the images'")."""
    if out is None:
        return torch.empty(shape, dtype=dtype, device=dev)
    if not isinstance(out, torch.Tensor) or not out.is_cuda or out.device != dev:
        raise RuntimeError("out must live on %s device" % noun)
    if out.dtype != dtype or tuple(out.shape) != shape or not out.is_contiguous():
        raise ValueError("out must be a contiguous %s tensor of shape %s" % (dtype, shape))
    return out
