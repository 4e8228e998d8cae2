"""Predict step of the reference (`predict.py:80-126`) without its file and plotting I/O: one forward of the
encoder + regressor + HIP decoder per batch of images, returning what `predict` hands to its visualiser -
vertices, projected vertices, raw 32-channel scores and their arg-max part map (`predict.py:106-118`)."""
from __future__ import annotations

import torch

from .training import regress


@torch.no_grad()
def predict_batch(smpl_model, decoder, images, amp=None, samples=None, generator=None):
    """images (N,3,H,W) or (N,H,W,3) on the HIP device -> dict(smpl (N,86), verts (N,6890,3),
    projects (N,V',3), segs (N,W,W,32) raw scores, seg_maps (N,W,W) int64 = argmax over channels).
    amp = "bf16": the encoder + regressor run under torch.autocast(bfloat16) (`training.amp_dtype`); the 86-vector and
    everything the decoder makes of it stay fp32.  amp = None: fp32 throughout.
    samples = S >= 1 (an `SMPLRegressor(probabilistic=True)` only; default None: nothing below happens): S bodies per image
    are drawn from the predicted Gaussian with `generator` (sample 0 the mean) and skinned as N S more rows; the result gains
    verts_mean (N,6890,3) and verts_rms (N,6890), `prob.sample_spread` of them: the per-vertex uncertainty map."""
    was_training = smpl_model.training
    smpl_model.eval()
    try:
        param = regress(smpl_model, images, amp)               # (amp = None: smpl_model(images) itself)
        out = dict(decoder(param), smpl=param)                 # what FullModel(smpl_model, decoder, "all") returns
        spread = None
        if samples is not None:
            from .keras_smpl.batch_smpl import SMPLLayer
            from .prob import sample_spread
            S = int(samples)
            with torch.no_grad():
                eps = torch.randn((param.shape[0], S, smpl_model.nout), generator=generator, device=param.device)
                layer = SMPLLayer(decoder._model, num_cam=decoder.num_cam)
                layer._consts, layer._consts_device = decoder.constants(param.device), param.device
                spread = sample_spread(layer(smpl_model.sample(eps, mean_first=True)), S)
    finally:
        smpl_model.train(was_training)
    res = {"smpl": out["smpl"], "verts": out["verts"], "projects": out["projects"], "segs": out["seg"],
           "seg_maps": out["seg"].argmax(dim=-1)}
    if spread is not None:
        res["verts_mean"], res["verts_rms"] = spread
    return res


def refine_predictions(smpl_model, fitter, images, labels, **fit_kw):
    """The encoder's prediction refined against label maps (ground truth or another network's segmentation): one
    forward of `smpl_model` on images, then `fitter.fit(labels, init=prediction, **fit_kw)` (`fitting.ParamFitter`).
    -> dict(smpl (N, 86): the network's parameters, refined (N, 86): the best iterate of each row, loss (N,): its loss,
    result: the whole `fitting.FitResult`).  The best iterate includes step 0, so `refined` is never worse than `smpl`
    under the fitter's loss.  Every keyword of `fit` passes through, so `group_size=G, tie=..., smooth=...` refine G
    consecutive images as views or frames of one body (the predictions' tied columns start at the group's mean), and
    `ld_weight=` reaches a fitter built with `label_distance=...`: the term that still pulls when the prediction lies many
    pixels from its labels."""
    was_training = smpl_model.training
    smpl_model.eval()
    try:
        with torch.no_grad():
            pred = smpl_model(images)
    finally:
        smpl_model.train(was_training)
    result = fitter.fit(labels, init=pred, **fit_kw)
    return {"smpl": pred, "refined": result.x, "loss": result.loss, "result": result}


class GraphedPredictor:
    """`predict_batch` for a fixed image shape replayed from ONE captured HIP graph: at batch 1 the eager forward
    is bound by ~500 host-side kernel launches (6.7 ms per image), the graph by the kernels themselves.
    `predictor(images)` copies the images into the static input and returns views of the static outputs
    (valid until the next call).  `predictor.input` is that static input: whatever writes into it in place
    (`preprocess.load_images(frame, 256, ..., out=predictor.input)`) followed by `predictor.replay()` is the per-frame
    path of predict_realtime.py:52-64 without the copy.  amp: as `predict_batch` takes it (the autocast is captured)."""

    def __init__(self, smpl_model, decoder, example_images, warmup=3, amp=None):
        self.smpl_model, self.decoder, self.amp = smpl_model, decoder, amp
        self._in = example_images.detach().clone()
        was_training = smpl_model.training
        smpl_model.eval()
        try:
            side = torch.cuda.Stream(device=self._in.device)
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side), torch.no_grad():
                for _ in range(max(1, warmup)):                    # MIOpen picks its solvers outside the capture
                    predict_batch(smpl_model, decoder, self._in, amp)
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            self._graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self._graph), torch.no_grad():
                self._out = predict_batch(smpl_model, decoder, self._in, amp)
        finally:
            smpl_model.train(was_training)

    @property
    def input(self):
        """The captured graph's static input tensor, shaped as the example images."""
        return self._in

    def replay(self):
        """Replay the graph on what `input` holds now -> the static outputs (valid until the next replay)."""
        self._graph.replay()
        return self._out

    def __call__(self, images):
        if images.shape != self._in.shape:
            raise RuntimeError("GraphedPredictor was captured for images of shape %s, got %s"
                               % (tuple(self._in.shape), tuple(images.shape)))
        self._in.copy_(images)
        self._graph.replay()
        return self._out
