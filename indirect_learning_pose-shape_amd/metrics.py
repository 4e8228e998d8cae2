"""Segmentation metrics of the reference: per-part IoU and pixel accuracy (evaluate.py:22-127,
evaluate_autoencoder.py:23-117) and Keras' per-step `metrics=['accuracy']` (train.py:207-215,
train_autoencoder.py:178-183, train_stage2_silhouette.py:228-234).

Everything is a function of one confusion matrix `counts` (C + 1, C) int64: row = ground-truth label (row C: a label
outside [0, C)), column = the arg-max of the scores.  Then, as evaluate.py defines them over classes 1..C-1:
    I_k = counts[k, k],  U_k = rowsum_k + colsum_k - counts[k, k],  mean IoU = mean(I / U),
    accuracy = trace / sum   (sum counts every pixel, invalid labels included: evaluate.py's W*W*num_images).
CUDA tensors are counted by the HIP kernel (csrc/metrics.hip, smplr_seg_confusion) or inside the rasteriser's loss
epilogue (DecoderOpts.confusion); CPU tensors by torch (`bincount`) with the same arg-max order: NaN above every number,
ties to the lower channel (torch.argmax / np.argmax).
"""
from __future__ import annotations

import numpy as np
import torch
import torch.distributed as dist

from . import _lib
from ._lib import check, ptr, stream


@_lib.on_device
def seg_confusion(scores, labels, conf, pred=None):
    """conf (C + 1, C) int64 on the device += the (label, arg-max) counts of scores (..., C) fp32 - or of an integer
    prediction map `pred` (then scores is None).  labels: one integer per pixel.  The HIP path only."""
    C = conf.shape[1]
    if conf.dtype != torch.int64 or conf.dim() != 2 or conf.shape[0] != C + 1 or not 2 <= C <= 32 or not conf.is_cuda:
        raise RuntimeError("conf must be a (C + 1, C) int64 device tensor with 2 <= C <= 32")
    if not conf.is_contiguous():
        raise RuntimeError("conf must be contiguous (the kernel adds into it in place)")
    # (every operand on the device the launch runs on: a tensor of another GPU would be read through a foreign pointer)
    for name, tt in (("scores", scores), ("pred", pred), ("labels", labels)):
        if tt is not None and tt.device != conf.device:
            raise RuntimeError("%s lives on %s, the counts on %s" % (name, tt.device, conf.device))
    if scores is not None:
        scores = _lib.require_cuda(scores, "scores")
        if scores.shape[-1] != C:
            raise RuntimeError("scores have %d channels, the counts %d classes" % (scores.shape[-1], C))
        npix = scores.numel() // C
    else:
        pred = _lib.require_cuda(pred.to(torch.int32), "pred", torch.int32)
        npix = pred.numel()
    if labels.numel() != npix:
        raise RuntimeError("labels hold %d entries for %d pixels" % (labels.numel(), npix))
    labels = _lib.require_cuda(labels.to(torch.int32), "labels", torch.int32)
    check(_lib.load().smplr_seg_confusion(ptr(scores), ptr(pred), ptr(labels), npix, C, ptr(conf), None, stream()),
          "smplr_seg_confusion")
    return conf


def _argmax_cpu(scores):
    """torch.argmax over the last axis with NaN above every number (the first NaN wins)."""
    nan = torch.isnan(scores)
    am = scores.argmax(dim=-1)
    if bool(nan.any()):
        has = nan.any(dim=-1)
        am = torch.where(has, nan.to(torch.int8).argmax(dim=-1), am)
    return am


class SegConfusion:
    """Accumulated (label, prediction) counts over any number of batches.

        m = SegConfusion(32, device)
        m.update(out["seg"], labels)            # or the decoder's fused form: DecoderOpts.confusion = m.counts
        m.mean_iou(), m.pixel_accuracy()        # evaluate.py's numbers
    """

    def __init__(self, num_classes=32, device=None):
        self.num_classes = C = int(num_classes)
        if not 2 <= C <= 32:
            raise ValueError("num_classes must be in 2..32 (got %d)" % C)
        self.device = torch.device(device) if device is not None else torch.device("cpu")
        self.counts = torch.zeros((C + 1, C), dtype=torch.int64, device=self.device)

    def reset(self):
        self.counts.zero_()
        return self

    def _add(self, pred, labels):
        """CPU path: bincount of row * C + column."""
        C = self.num_classes
        lab = labels.reshape(-1).to(torch.int64)
        pr = pred.reshape(-1).to(torch.int64)
        if lab.numel() != pr.numel():
            raise RuntimeError("labels hold %d entries for %d pixels" % (lab.numel(), pr.numel()))
        row = torch.where((lab >= 0) & (lab < C), lab, torch.full_like(lab, C))
        ok = (pr >= 0) & (pr < C)
        idx = (row * C + pr)[ok]
        self.counts += torch.bincount(idx.cpu(), minlength=(C + 1) * C).reshape(C + 1, C).to(self.counts.device)

    def update(self, scores, labels):
        """scores (..., C) raw scores (the arg-max is taken over them as they are, as predict.py does), labels one
        integer per pixel (the same layout without the channel axis)."""
        if scores.shape[-1] != self.num_classes:
            raise RuntimeError("scores have %d channels, SegConfusion counts %d classes"
                               % (scores.shape[-1], self.num_classes))
        if self.counts.is_cuda:
            seg_confusion(scores.detach().float(), labels, self.counts)
        else:
            self._add(_argmax_cpu(scores.detach().cpu().float()), labels.cpu())
        return self

    def update_maps(self, pred, labels):
        """pred: an integer prediction map (a prediction outside [0, C) is not counted), labels: the same shape."""
        if self.counts.is_cuda:
            seg_confusion(None, labels, self.counts, pred=pred)
        else:
            self._add(pred.cpu(), labels.cpu())
        return self

    # ---- the numbers (float64 numpy, as evaluate.py computes them) --------------------------------------------------
    def _np(self):
        return self.counts.cpu().numpy().astype(np.float64)

    def intersections(self):
        """I_k for classes 1..C-1 (background excluded)."""
        c = self._np()
        return np.diagonal(c[:self.num_classes])[1:].copy()

    def unions(self):
        """U_k = |gt == k| + |pred == k| - I_k for classes 1..C-1."""
        c = self._np()
        d = np.diagonal(c[:self.num_classes])
        return (c[:self.num_classes].sum(axis=1) + c.sum(axis=0) - d)[1:]

    def iou(self):
        """I_k / U_k per class 1..C-1 (NaN for a class in neither map: take np.nanmean if that is what you want)."""
        with np.errstate(invalid="ignore", divide="ignore"):
            return self.intersections() / self.unions()

    def mean_iou(self):
        """np.mean(I / U), the reference's plain mean: NaN when a class never occurs."""
        return float(np.mean(self.iou()))

    def correct(self):
        return int(torch.diagonal(self.counts[:self.num_classes]).sum())

    def total(self):
        return int(self.counts.sum())

    def pixel_accuracy(self):
        """correct / every counted pixel (evaluate.py: correct / (W * W * num_images))."""
        t = self.total()
        return self.correct() / t if t else float("nan")

    def all_reduce(self, group=None):
        """Sum the counts over the ranks of `group` (int64 SUM: every rank ends with the same matrix)."""
        if dist.is_available() and dist.is_initialized():
            dist.all_reduce(self.counts, op=dist.ReduceOp.SUM, group=group)
        return self


# ---- the reference's helpers, by name (evaluate.py:22-60), on label maps -----------------------------------------------
def compute_intersection_and_union(ground_truth, predict, num_classes):
    """evaluate.py:22-47: -> (intersections, unions) float64 arrays over classes 1..num_classes-1."""
    C = int(num_classes)
    gt = np.asarray(ground_truth).reshape(-1).astype(np.int64)
    pr = np.asarray(predict).reshape(-1).astype(np.int64)
    I = np.array([np.sum((gt == k) & (pr == k)) for k in range(1, C)], dtype=np.float64)
    U = np.array([np.sum((gt == k) | (pr == k)) for k in range(1, C)], dtype=np.float64)
    return I, U


def count_correct_predicts(ground_truth, predict):
    """evaluate.py:50-59: number of pixels where the maps agree (float, as there)."""
    return float(np.sum(np.equal(np.asarray(ground_truth), np.asarray(predict))))
