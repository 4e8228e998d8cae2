"""Evaluation of the reference (`evaluate.py:59-127`, `evaluate_autoencoder.py:23-117`, `evaluate3d.py:32-65`) without its file, `cv2` and
printing I/O: per-part IoU over classes 1..31 and pixel accuracy of the arg-max part map against ground-truth maps, in the
style of `inference.predict_batch`.  With a decoder built with a fused loss (`SMPLDecoder(..., loss=softmax_focal_loss(..))`)
the counting runs inside the rasteriser's loss epilogue and the (N, W, W, 32) scores are never written; a decoder without
one writes them and the confusion kernel counts them."""
from __future__ import annotations

import torch

from .metrics import SegConfusion


@torch.no_grad()
def evaluate_iou_and_acc(smpl_model, decoder, batches, num_classes=32):
    """batches: an iterable of (images (N,3,H,W) or (N,H,W,3), gt_maps (N,W,W) integer part maps laid out as the
    decoder's output) already on the HIP device.  -> dict(ious (num_classes - 1,) float64 = I / U per part,
    mean_iou = their plain mean (NaN when a part occurs in neither map, as np.mean in evaluate.py), accuracy = correct /
    pixels, counts (num_classes + 1, num_classes) int64 on the device, intersections, unions, correct, total = pixels
    counted (evaluate.py's W * W * num_images))."""
    m = None
    was_training = smpl_model.training
    smpl_model.eval()
    try:
        for images, gt in batches:
            if m is None:
                m = SegConfusion(num_classes, images.device)
            decoder(smpl_model(images), gt, confusion=m)
    finally:
        smpl_model.train(was_training)
    if m is None:
        raise ValueError("evaluate_iou_and_acc: no batches")
    return {"ious": m.iou(), "mean_iou": m.mean_iou(), "accuracy": m.pixel_accuracy(), "counts": m.counts,
            "intersections": m.intersections(), "unions": m.unions(), "correct": m.correct(), "total": m.total()}


@torch.no_grad()
def evaluate_pose_param_mse(smpl_model, batches):
    """`evaluate3d.py:32-65`: batches: an iterable of (images, gt_pose (N, 72) axis-angle pose parameters) on the model's
    device.  -> the mean of (gt_pose[:, 3:] - smpl[:, 7:76])^2 over all samples and the 69 parameters without the global
    rotation, as a float (accumulated in float64)."""
    total, count = None, 0
    was_training = smpl_model.training
    smpl_model.eval()
    try:
        for images, gt_pose in batches:
            smpl = smpl_model(images)
            gt = torch.as_tensor(gt_pose, device=smpl.device)
            if gt.dim() != 2 or gt.shape[1] != 72 or gt.shape[0] != smpl.shape[0]:
                raise ValueError("gt_pose must be (N, 72) with N = the batch's images")
            err = (gt[:, 3:].to(torch.float64) - smpl[:, 7:76].to(torch.float64)).square().sum()
            total = err if total is None else total + err
            count += int(smpl.shape[0]) * 69
    finally:
        smpl_model.train(was_training)
    if total is None:
        raise ValueError("evaluate_pose_param_mse: no batches")
    return float(total) / count
