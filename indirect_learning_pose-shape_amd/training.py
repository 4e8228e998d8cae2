"""Train-step structure of the reference (train.py:179-242, train_stage2_silhouette.py:226-270) on the
MI355X path: forward (encoder + regressor on stock torch ops, decoder on the HIP kernels), focal
loss, backward, Adam(lr=1e-4).  Data parallelism replaces `keras.utils.multi_gpu_model`
(train.py:205-210): one process per GPU, `DistributedDataParallel` over RCCL (backend "nccl"),
gradients of the encoder/regressor all-reduced in ~25 MiB buckets overlapped with backward; the
decoder has no parameters and exchanges nothing.  BatchNorm stays local per rank
(statistics AND running buffers: `broadcast_buffers=False`), as Keras towers normalise per tower.
`with_silhouette` adds the silhouette cross-entropy of train_stage2_silhouette.py:226-229 to the same step - the
reference alternates two separately compiled models over one shared encoder; here both heads come out of one
decoder pass and one backward - at its own resolution `silh_wh` (`silhs_output_wh`, :72-86)."""
from __future__ import annotations

import os

import torch
import torch.distributed as dist
from torch import nn

from .decoder import SMPLDecoder
from .focal_loss import softmax_focal_loss
from .model import SMPLRegressor


def configure_conv_backend():
    """OPT-IN (`SMPLR_CONV_BACKEND=find`): MIOpen find mode with torch's full workspace (`cudnn.benchmark = True`,
    MIOPEN_FIND_MODE=FAST unless set) for the encoder's stock-torch convolutions.  Not the default: on a fresh box (no
    user database, no cached kernels) the first train step then spends MINUTES compiling and timing candidate solvers -
    `tools/conv_backend_ab.sh` on an MI355X: default 28.9 s for the whole run of 8 steps at 26.07 ms per step and no
    workspace warning; find mode silent for over 420 s (killed).  The `GemmFwdRest ... IsEnoughWorkspace` lines a
    `bench.py` run prints (8 of them) come from the batch-1 predict leg's first convolution: immediate mode EVALUATES
    that solver against the workspace torch sized for the solution it picked and logs that it does not fit; the step
    above, at 128 images, prints none."""
    os.environ.setdefault("MIOPEN_FIND_MODE", "FAST")
    torch.backends.cudnn.benchmark = True


def amp_dtype(amp):
    """The `amp` option of SegTrainer, inference.predict_batch and inference.GraphedPredictor -> the autocast dtype:
    None (fp32 throughout, the default) or torch.bfloat16 for "bf16" / torch.bfloat16.  Anything else is a ValueError;
    fp16 in particular needs loss scaling, which is not offered."""
    if amp is None:
        return None
    if amp is torch.bfloat16 or (isinstance(amp, str) and amp == "bf16"):
        return torch.bfloat16
    if amp is torch.float16 or (isinstance(amp, str) and amp.lower() in ("fp16", "float16", "half")):
        raise ValueError("amp=%r: fp16 needs loss scaling and no loss scaling is offered; use amp='bf16'" % (amp,))
    raise ValueError("amp must be None, 'bf16' or torch.bfloat16 (got %r)" % (amp,))


def regress(net, images, amp):
    """net(images) -> the (N, 86) vector in fp32.  With amp, that forward alone runs under torch.autocast(device type,
    bfloat16) and the vector is `.float()`ed on the way out; amp = None is net(images) itself."""
    dt = amp_dtype(amp)
    if dt is None:
        return net(images)
    with torch.autocast(images.device.type, dtype=dt):
        param = net(images)
    return param.float()


class SegTrainer:
    """One optimiser step = `segs_model.fit` on one batch with the focal loss (train.py:207-242).
    amp = "bf16" (or torch.bfloat16): mixed precision for the encoder + regressor - that forward alone runs under
    torch.autocast(bfloat16), where the convolutions and linears take bf16 and the package's batch-norm / PReLU kernels
    stream bf16 activations; the 86-vector comes out as fp32, and decoder, loss heads, backward's accumulation into the
    parameters, Adam, the DDP buckets and the checkpoints are the fp32 ones of amp = None (bf16 has fp32's exponent: no
    GradScaler).  amp = None, the default, is the fp32 step unchanged."""

    def __init__(self, smpl_path=None, input_wh=256, output_wh=48, encoder_architecture="enet", use_IEF=True,
                 weight_classes=True, gamma=2.0, lr=1e-4, device=None, ddp=False, bucket_mb=25,
                 with_silhouette=False, silh_wh=None, fused_loss=True, fused_silh_loss=False, amp=None, in_channels=3,
                 pose_repr="axis_angle", probabilistic=False, init_sigma=0.1):
        amp_dtype(amp)                                                # (ValueError before anything is built)
        if amp is not None and os.environ.get("SMPLR_ENCODER_LAYOUT", "").lower() == "channels_last":
            # that layout runs torch's own BatchNorm2d (the package's kernels read NCHW planes), and torch 2.10 / ROCm 7.0's
            # training-mode batch norm is not safe on a bf16 channels_last tensor: it ends the process
            raise ValueError("amp and SMPLR_ENCODER_LAYOUT=channels_last do not go together")
        self.amp = amp
        if fused_silh_loss and not with_silhouette:
            raise ValueError("fused_silh_loss needs with_silhouette=True")
        self.device = (torch.device(device) if device is not None
                       else torch.device("cuda", torch.cuda.current_device()))
        if self.device.type == "cuda" and os.environ.get("SMPLR_CONV_BACKEND", "default") == "find":
            configure_conv_backend()
        self.output_wh = output_wh
        self.in_channels = int(in_channels)                           # (3: images; synthetic.SyntheticBatches.in_channels)
        self.smpl_model = SMPLRegressor(output_wh, encoder_architecture, use_IEF, in_channels=self.in_channels,
                                        pose_repr=pose_repr, probabilistic=probabilistic,
                                        init_sigma=init_sigma).to(self.device)    # ("rot6d": rot6d.py; still (N, 86) out)
        # OPT-IN (`SMPLR_ENCODER_LAYOUT=channels_last`): the encoder's weights and activations in NHWC, the layout
        # MIOpen's implicit-GEMM convolution solvers work in (the default NCHW tensors are transposed around them:
        # `batched_transpose_32x32_dword` in the train step's kernel trace).  The package's fused batch-norm / PReLU
        # kernels read NCHW planes, so this layout runs the stock modules for them.  Measured before being made a default:
        # tools/train_layout_ab.py.
        self.channels_last = os.environ.get("SMPLR_ENCODER_LAYOUT", "").lower() == "channels_last"
        if self.channels_last:
            self.smpl_model = self.smpl_model.to(memory_format=torch.channels_last)
        self.loss_fn = softmax_focal_loss(gamma, weight_classes)      # softmax + focal loss, one HIP kernel
        self.silh_loss_fn = softmax_focal_loss(0.0, False)            # softmax + categorical CE
        # the train pass consumes losses only: verts / projects / mask are not written out, and with an integer class
        # map the segmentation loss runs inside the rasteriser (no (B,W,W,32) score or gradient tensor in memory)
        # fused_silh_loss (opt-in): the silhouette cross-entropy, its gradient and the accuracy counts run around the
        # silhouette rasteriser too (SMPLDecoder(silh_loss=...)), in the joint step and in the silhouette-only step
        self.fused_silh_loss = bool(fused_silh_loss)
        silh_head = self.silh_loss_fn if fused_silh_loss else None
        self.decoder = SMPLDecoder(smpl_path, img_wh=output_wh, with_silhouette=with_silhouette, silh_wh=silh_wh,
                                   outputs=(), loss=self.loss_fn if fused_loss else None, silh_loss=silh_head)
        self.with_silhouette = with_silhouette
        # what the reference's monitor step reads every 10 trials (train.py:245-300: `verts_model` / `projects_model` /
        # `segs_model` predictions of the monitor images): verts, projects, mask and the raw scores - the train
        # decoder above writes none of them.  Same constants, no second upload; `on_trial_end(trial, trainer)` hooks
        # use `trainer.monitor(images)`.
        self.monitor_decoder = SMPLDecoder(smpl_path, img_wh=output_wh, with_silhouette=with_silhouette,
                                           silh_wh=silh_wh).share_constants(self.decoder)
        # the silhouette-only pass of the reference's alternating schedule (train_stage2_silhouette.py:262-270)
        self.silh_decoder = (SMPLDecoder(smpl_path, img_wh=output_wh, heads=("silhouette",), silh_wh=silh_wh, outputs=(),
                                         silh_loss=silh_head)
                             .share_constants(self.decoder)) if with_silhouette else None
        self.net = self.smpl_model
        if ddp:
            self.net = nn.parallel.DistributedDataParallel(
                self.smpl_model, device_ids=[self.device.index] if self.device.type == "cuda" else None,
                bucket_cap_mb=bucket_mb, gradient_as_bucket_view=True, broadcast_buffers=False)
        self.opt = torch.optim.Adam(self.smpl_model.parameters(), lr=lr)       # train.py:179

    def step(self, images, labels, silh_labels=None, metrics=None, _marks=None):
        """images (N,C,H,W) or (N,H,W,C), C = in_channels (3 by default); labels (N,W,W) integer class map or (N,W*W,32) one-hot, or None for the
        silhouette-only step of the alternating schedule (then silh_labels is required).
        metrics: Keras' metrics=['accuracy'] (train.py:207-215, train_stage2_silhouette.py:228-234) - a
        `metrics.SegConfusion(32, device)` for the seg head, or a pair (seg, silhouette) of which either may be None,
        the silhouette one a SegConfusion(2, device); each pixel's (label, arg-max) is added to it (for the seg head
        inside the rasteriser's loss epilogue when the loss is fused), no host sync.
        Returns the mean loss (a 0-d tensor; no host sync).  (`_marks`: see `step_timed`.)"""
        mark = (lambda k: None) if _marks is None else _marks
        param = self._regress(images, mark, _marks is not None)
        loss = self.param_loss(param, labels, silh_labels, metrics)
        return self._update(loss, mark)

    def _regress(self, images, mark, hook):
        """The frame's first half: zero_grad and the regressor's forward -> param (N, 86)."""
        mark("start")
        self.opt.zero_grad(set_to_none=True)
        if self.channels_last and images.dim() == 4 and images.shape[1] == self.in_channels:
            images = images.contiguous(memory_format=torch.channels_last)
        param = regress(self.net, images, self.amp)
        mark("encoder_fwd")
        if hook and param.requires_grad:
            param.register_hook(lambda g: (mark("decoder_bwd"), g)[1])     # fires between the decoder's and the encoder's backward
        return param

    def _update(self, loss, mark):
        """The frame's second half: backward and Adam -> the detached loss."""
        mark("decoder_fwd")
        loss.backward()
        mark("backward")
        self.opt.step()
        mark("optimizer")
        return loss.detach()

    def param_loss(self, param, labels, silh_labels=None, metrics=None):
        """The step's loss from the regressed `param` (N, 86): the decoder, the focal loss and, with silhouette labels, the
        silhouette cross-entropy, as `step` describes them -> the mean loss (0-d, differentiable in param)."""
        seg_m, silh_m = metrics if isinstance(metrics, (tuple, list)) else (metrics, None)
        as_map = lambda t: t if t.dtype in (torch.int64, torch.int32, torch.int16, torch.uint8) else t.argmax(dim=-1)
        if labels is None:
            # `silhouettes_model.fit` (train_stage2_silhouette.py:226-234, the 150 silhouette steps of :262-270):
            # the silhouette head alone - no mask, no binning, no 31-part rasteriser
            if self.silh_decoder is None or silh_labels is None:
                raise RuntimeError("a step without labels is the silhouette-only step: needs with_silhouette and silh_labels")
            if self.fused_silh_loss:
                loss = self.silh_decoder(param, silh_labels=as_map(silh_labels), silh_confusion=silh_m)["silh_loss"].mean()
            else:
                out = self.silh_decoder(param)
                loss = self.silh_loss_fn(silh_labels, out["silhouette"]).mean()
                if silh_m is not None:
                    silh_m.update(out["silhouette"], as_map(silh_labels))
        else:
            is_map = labels.dtype in (torch.int64, torch.int32, torch.int16, torch.uint8)
            fused_silh = self.fused_silh_loss and silh_labels is not None
            skw = dict(silh_labels=as_map(silh_labels), silh_confusion=silh_m) if fused_silh else {}
            if self.decoder.loss is not None and is_map:           # model.py:119-120 + focal_loss.py, in the rasteriser
                loss = self.decoder(param, labels, confusion=seg_m, **skw)
                out, loss = loss, loss["seg_loss"].mean()
            else:
                out = self.decoder(param, **skw)
                loss = self.loss_fn(labels, out["seg"]).mean()
                if seg_m is not None:
                    seg_m.update(out["seg"], as_map(labels))
            if fused_silh:
                loss = loss + out["silh_loss"].mean()
            elif self.with_silhouette and silh_labels is not None:  # train_stage2_silhouette.py:85-86,226-229
                loss = loss + self.silh_loss_fn(silh_labels, out["silhouette"]).mean()
                if silh_m is not None:
                    silh_m.update(out["silhouette"], as_map(silh_labels))
        return loss

    def step_timed(self, images, labels, silh_labels=None, **kw):
        """One `step` with HIP events between its sections -> dict(encoder_ms, decoder_ms, optimizer_ms, total_ms):
        encoder = regressor forward + its backward (under DDP that includes the all-reduce buckets it overlaps),
        decoder = decoder + loss forward and backward (up to the gradient of the 86-vector), optimizer = zero_grad +
        Adam.  Synchronises; a measurement aid for bench.py's train leg (train.py:179-242 is the step reproduced)."""
        ev = {}

        def mark(k):
            e = torch.cuda.Event(enable_timing=True)
            e.record(torch.cuda.current_stream(self.device))
            ev[k] = e
        self.step(images, labels, silh_labels, _marks=mark, **kw)          # (kw: what a subclass's step takes beyond these)
        torch.cuda.synchronize(self.device)
        dt = lambda a, b: ev[a].elapsed_time(ev[b])
        dec_bwd_end = "decoder_bwd" if "decoder_bwd" in ev else "backward"
        return {"encoder_ms": dt("start", "encoder_fwd") + dt(dec_bwd_end, "backward"),
                "decoder_ms": dt("encoder_fwd", "decoder_fwd") + dt("decoder_fwd", dec_bwd_end),
                "optimizer_ms": dt("backward", "optimizer"), "total_ms": dt("start", "optimizer")}

    @torch.no_grad()
    def monitor(self, images):
        """The monitor step's predictions (train.py:245-262) for a batch of images: dict(smpl (N,86), verts, projects,
        mask, seg (N,W,W,32) raw scores [, silhouette], J_transformed) from the full-output decoder.  `step()`'s own
        decoder returns losses only (outputs=()), so monitor hooks must not read `trainer.decoder(...)['verts']`."""
        was_training = self.smpl_model.training
        self.smpl_model.eval()
        try:
            param = regress(self.smpl_model, images, self.amp)
            out = dict(self.monitor_decoder(param))
        finally:
            self.smpl_model.train(was_training)
        out["smpl"] = param
        return out

    def state_dict(self):                                           # train.py:302-315 saves smpl_model only
        return self.smpl_model.state_dict()

    # ---- save / resume (train.py:181-193 `resume_from`, :300-315 `smpl_model.save`) -------------------------
    def save(self, path, trial=0):
        """The regressor's weights (what the reference saves), plus what a bit-exact resume of THIS trainer also
        needs and Keras' `model.save` would have kept: the Adam state, and the trial counter."""
        torch.save({"smpl_model": self.smpl_model.state_dict(), "optimizer": self.opt.state_dict(),
                    "trial": int(trial), "output_wh": int(self.output_wh)}, path)

    def resume(self, path):
        """-> the trial to continue from.  A file holding only a state dict (weights) is accepted too."""
        ck = torch.load(path, map_location=self.device)
        if "smpl_model" not in ck:
            self.smpl_model.load_state_dict(ck)
            return 0
        if int(ck.get("output_wh", self.output_wh)) != int(self.output_wh):
            raise RuntimeError("checkpoint was trained at %dx%d, this trainer renders %dx%d"
                               % (ck["output_wh"], ck["output_wh"], self.output_wh, self.output_wh))
        self.smpl_model.load_state_dict(ck["smpl_model"])
        self.opt.load_state_dict(ck["optimizer"])
        return int(ck.get("trial", -1)) + 1


class SupervisedTrainer(SegTrainer):
    """`SegTrainer` with the supervised 3D losses of `supervised.py` on the regressed parameters - how "Synthetic Training
    for Accurate 3D Human Pose and Shape Estimation" trains - for batches that know their truth
    (`synthetic.SyntheticBatches(..., truth=True)`).

    spec, root, cam_scale: `supervised_terms`' (spec None: no 3D joint term).  weights None: the five terms are weighted by
    learned homoscedastic uncertainties (`supervised.UncertaintyWeights`), whose log-variances join Adam's parameters and
    the checkpoints; a 5-tuple: fixed weights.  indirect_weight > 0 adds that many times `SegTrainer`'s loss (part
    rasteriser and, with silhouette labels, the silhouette head) whenever a step gets labels; with 0 (the default) no
    binning or rasteriser kernel is launched and labels may be None.  ddp=True needs fixed weights: the log-variances live
    outside the DDP module."""

    def __init__(self, *args, spec=None, root=-1, weights=None, indirect_weight=0.0, cam_scale=None, **kw):
        import inspect
        from .keras_smpl.batch_smpl import SMPLLayer
        from .supervised import UncertaintyWeights
        if weights is None and inspect.signature(SegTrainer.__init__).bind(self, *args, **kw).arguments.get("ddp", False):
            raise ValueError("ddp=True needs fixed weights=(w0, .., w4): the learned log-variances live outside the DDP module")
        super().__init__(*args, **kw)
        self.spec, self.root, self.indirect_weight = spec, int(root), float(indirect_weight)
        self.cam_scale = None if cam_scale is None else torch.tensor([float(c) for c in cam_scale], dtype=torch.float32,
                                                                     device=self.device)
        self.weights = UncertaintyWeights(fixed=weights).to(self.device)
        if self.weights.learned:
            self.opt.add_param_group({"params": [self.weights.s]})
        self.smpl_layer = SMPLLayer(self.decoder._model, num_cam=self.decoder.num_cam)      # (the decoder's model and constants)
        self.last_terms = None

    def step(self, images, labels=None, silh_labels=None, truth=None, metrics=None, _marks=None):
        """images, labels, silh_labels, metrics: `SegTrainer.step`'s (labels are read only with indirect_weight > 0); truth:
        dict(x (N, 86), verts (N, V, 3), J_transformed (N, 24, 3)) on the device.  Returns the mean loss (0-d, no host sync);
        `last_terms` then holds the batch means of the five terms, (5,), detached."""
        from .supervised import supervised_terms
        if truth is None:
            raise ValueError("SupervisedTrainer.step needs truth= (SyntheticBatches(..., truth=True) yields it)")
        mark = (lambda k: None) if _marks is None else _marks
        param = self._regress(images, mark, _marks is not None)
        layer = self.smpl_layer
        layer._consts, layer._consts_device = self.decoder.constants(param.device), param.device
        verts = layer(param)
        terms = supervised_terms(param, verts, layer.J_transformed, truth, self.spec, self.root, None, self.cam_scale,
                                 self.decoder.num_cam)
        loss = self.weights(terms).mean()
        if self.indirect_weight > 0 and labels is not None:
            loss = loss + self.indirect_weight * self.param_loss(param, labels, silh_labels, metrics)
        self.last_terms = terms.detach().mean(0)
        return self._update(loss, mark)

    def save(self, path, trial=0):
        """`SegTrainer.save` plus the log-variances under "uncertainty" (the Adam state covers them already)."""
        torch.save({"smpl_model": self.smpl_model.state_dict(), "optimizer": self.opt.state_dict(), "trial": int(trial),
                    "output_wh": int(self.output_wh), "uncertainty": self.weights.state_dict()}, path)

    def resume(self, path):
        """-> the trial to continue from.  A `SegTrainer` checkpoint (no "uncertainty") is accepted: its Adam state goes to
        the regressor's parameters and the log-variances start at 0."""
        ck = torch.load(path, map_location=self.device)
        has_s = "s" in ck.get("uncertainty", {})
        if "smpl_model" not in ck or has_s == self.weights.learned:
            if has_s:
                self.weights.load_state_dict(ck["uncertainty"])
            return super().resume(path)
        if has_s:
            raise RuntimeError("the checkpoint carries learned log-variances, this trainer has fixed weights")
        if int(ck.get("output_wh", self.output_wh)) != int(self.output_wh):
            raise RuntimeError("checkpoint was trained at %dx%d, this trainer renders %dx%d"
                               % (ck["output_wh"], ck["output_wh"], self.output_wh, self.output_wh))
        self.smpl_model.load_state_dict(ck["smpl_model"])
        own = torch.optim.Adam(self.smpl_model.parameters(), lr=self.opt.defaults["lr"])
        own.load_state_dict(ck["optimizer"])
        for p, st in own.state.items():
            self.opt.state[p] = st
        self.opt.param_groups[0].update({k: v for k, v in own.param_groups[0].items() if k != "params"})
        with torch.no_grad():
            self.weights.s.zero_()
        self.opt.state.pop(self.weights.s, None)
        return int(ck.get("trial", -1)) + 1


class ProbabilisticTrainer(SupervisedTrainer):
    """`SupervisedTrainer` on a regressor that predicts a Gaussian per regressed column (`SMPLRegressor(probabilistic=True)`,
    prob.py) - how "Probabilistic 3D Human Shape and Pose Estimation from Multiple Unconstrained Images in the Wild" trains.

    A step's loss is `SupervisedTrainer`'s on the mean row, plus
      nll_weight     times the mean over rows and the two groups (pose, shape; the camera does not count) of `gaussian_nll`
                     against the truth's parameters - with pose_repr="rot6d" against `axis_angle_to_rot6d` of its pose;
      sample_weight  times the mean over the B S sampled bodies (`samples` = S per row, drawn through the reparameterisation
                     trick from `generator`, decoded as B S more rows) of `supervised_terms`' vertex and joint terms against
                     the repeated truth.
    generator: a torch.Generator on the trainer's device (default: a fresh one seeded with 0); its state goes into the
    checkpoints, the new layer's weights and Adam state with the regressor's."""

    def __init__(self, *args, samples=4, nll_weight=1.0, sample_weight=1.0, generator=None, init_sigma=0.1, **kw):
        if kw.pop("probabilistic", True) is not True:
            raise ValueError("ProbabilisticTrainer trains a probabilistic regressor")
        super().__init__(*args, probabilistic=True, init_sigma=init_sigma, **kw)
        self.samples, self.nll_weight, self.sample_weight = int(samples), float(nll_weight), float(sample_weight)
        if self.samples < 1:
            raise ValueError("samples must be positive")
        if generator is None:
            generator = torch.Generator(device=self.device)
            generator.manual_seed(0)
        self.generator = generator
        nc = self.decoder.num_cam
        npose = self.smpl_model.nout - nc - 10
        self.groups = (-1,) * nc + (0,) * npose + (1,) * 10
        self.last_nll = self.last_sample_terms = None

    def _target(self, x_t):
        """The truth's (N, 86) in the space the regressor works in."""
        if self.smpl_model.pose_repr != "rot6d":
            return x_t
        from .rot6d import axis_angle_to_rot6d
        nc, n = self.decoder.num_cam, int(x_t.shape[0])
        a = axis_angle_to_rot6d(x_t[:, nc:nc + 72].reshape(n, 24, 3)).reshape(n, 144)
        return torch.cat([x_t[:, :nc], a, x_t[:, nc + 72:]], 1)

    def step(self, images, labels=None, silh_labels=None, truth=None, metrics=None, _marks=None):
        """`SupervisedTrainer.step`'s arguments and result; afterwards `last_nll` (2,) holds the batch means of the pose and
        shape likelihoods and `last_sample_terms` (2,) those of the samples' vertex and joint terms, detached."""
        from .prob import gaussian_nll
        from .supervised import supervised_terms
        if truth is None:
            raise ValueError("ProbabilisticTrainer.step needs truth= (SyntheticBatches(..., truth=True) yields it)")
        mark = (lambda k: None) if _marks is None else _marks
        param = self._regress(images, mark, _marks is not None)
        net, layer, nc = self.smpl_model, self.smpl_layer, self.decoder.num_cam
        layer._consts, layer._consts_device = self.decoder.constants(param.device), param.device
        verts = layer(param)
        terms = supervised_terms(param, verts, layer.J_transformed, truth, self.spec, self.root, None, self.cam_scale, nc)
        loss = self.weights(terms).mean()
        if self.indirect_weight > 0 and labels is not None:
            loss = loss + self.indirect_weight * self.param_loss(param, labels, silh_labels, metrics)
        self.last_terms = terms.detach().mean(0)
        nll = gaussian_nll(net.mean, net.log_var, self._target(truth["x"].detach().float()), self.groups)
        loss = loss + self.nll_weight * nll.mean()
        self.last_nll = nll.detach().mean(0)
        if self.sample_weight > 0:
            B, S = int(param.shape[0]), self.samples
            eps = torch.randn((B, S, net.nout), generator=self.generator, device=param.device)
            xs = net.sample(eps, mean_first=False)
            verts_s = layer(xs)
            truth_s = {k: v.repeat_interleave(S, 0) for k, v in truth.items() if k in ("x", "verts", "J_transformed")}
            row_w = torch.tensor([1.0, 1.0, 0.0, 0.0, 0.0], device=param.device).repeat(B * S, 1)
            terms_s = supervised_terms(xs, verts_s, layer.J_transformed, truth_s, self.spec, self.root, row_w, self.cam_scale, nc)
            loss = loss + self.sample_weight * terms_s[:, :2].sum(1).mean()
            self.last_sample_terms = terms_s.detach()[:, :2].mean(0)
        return self._update(loss, mark)

    def save(self, path, trial=0):
        """`SupervisedTrainer.save` plus the generator's state under "generator"."""
        torch.save({"smpl_model": self.smpl_model.state_dict(), "optimizer": self.opt.state_dict(), "trial": int(trial),
                    "output_wh": int(self.output_wh), "uncertainty": self.weights.state_dict(),
                    "generator": self.generator.get_state()}, path)

    def resume(self, path):
        """-> the trial to continue from; a checkpoint that carries a generator state restores it."""
        trial = super().resume(path)
        ck = torch.load(path, map_location="cpu")
        if isinstance(ck, dict) and ck.get("generator") is not None:
            self.generator.set_state(ck["generator"].cpu())
        return trial


def save_name(dataset, output_wh, use_IEF=True, scaledown=0.005, vertex_sampling=None, weight_classes=True, trial=0,
              encoder="resnet"):
    """The reference's checkpoint file name (train.py:302-313), with torch's extension."""
    name = "%s_%dx%d_%s" % (dataset, output_wh, output_wh, encoder)
    if use_IEF:
        name += "_ief"
    name += "_scaledown" + str(scaledown).replace(".", "")
    if vertex_sampling is not None:
        name += "_vs%d" % vertex_sampling
    if weight_classes:
        name += "_arms_weighted_2_bg_weighted_0point3_gamma2_multigpu"
    return name + "_%d.pt" % trial


def fit(trainer, batches, trials, steps_per_trial, save_dir=None, save_every=10, name_fn=None, start_trial=0,
        on_trial_end=None, metrics=None):
    """The loop of train.py:221-315: `trials` rounds of `steps_per_trial` optimiser steps (`fit_generator(...,
    steps_per_epoch, nb_epoch=1)`) over `batches` - an iterator of (images, labels[, silhouette labels]) already
    on the device, the data generators being the caller's (`augment.DeviceBatches` is the reference's
    `ImageDataGenerator` pair over a uint8 pool on the device and plugs in here unchanged) - and every `save_every` trials (on rank 0) the monitor
    hook `on_trial_end(trial, trainer)` (use `trainer.monitor(images)` for verts / projects / seg: the train decoder
    `trainer.decoder` writes losses only) and a checkpoint named like the reference's.  -> list of per-trial mean losses (python floats; the one
    host sync per trial).  metrics: what `step` takes (a SegConfusion, or a (seg, silhouette) pair), handed to every
    step and reset at the start of every trial - `on_trial_end` reads the trial's accuracy from it (Keras'
    metrics=['accuracy'])."""
    it = iter(batches)
    rank0 = (not dist.is_initialized()) or dist.get_rank() == 0
    history = []
    mlist = [m for m in (metrics if isinstance(metrics, (tuple, list)) else (metrics,)) if m is not None]
    for trial in range(start_trial, trials):
        total = None
        for m in mlist:
            m.reset()
        for _ in range(steps_per_trial):
            batch = next(it)
            loss = trainer.step(*batch, metrics=metrics) if metrics is not None else trainer.step(*batch)
            total = loss if total is None else total + loss
        history.append(float(total) / max(1, steps_per_trial))
        if trial % save_every == 0:
            if on_trial_end is not None and rank0:
                on_trial_end(trial, trainer)
            if save_dir is not None and rank0:
                os.makedirs(save_dir, exist_ok=True)
                fname = name_fn(trial) if name_fn is not None else "smpl_model_%d.pt" % trial
                trainer.save(os.path.join(save_dir, fname), trial)
    return history


def init_distributed():
    """Rank/world from torchrun's environment; RCCL over xGMI on GPUs, gloo on CPU."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world > 1 and not dist.is_initialized():
        if torch.cuda.is_available():
            torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")))
            dist.init_process_group("nccl", device_id=torch.device("cuda", torch.cuda.current_device()))
        else:
            dist.init_process_group("gloo")
    return int(os.environ.get("RANK", "0")), world
