"""Fitting SMPL parameters to label maps: per-sample Adam on the 86-vectors through the decoder and its fused loss.

The reference's `decoder_loss_debugging.py:103-125` (`train()`: a table of learnable 86-vectors, 1601 Adam steps through
decoder + focal loss) as a call, and the same loop as test-time refinement of an encoder's prediction:

    fitter = ParamFitter(smpl_path, img_wh=48)
    result = fitter.fit(labels)                                 # from the mean body; labels (B, 48, 48) integer part maps
    result = fitter.fit(labels, init=prediction, stages=[(30, column_scale(cam=20., pose=0., shape=0.)),
                                                         (200, column_scale(cam=0., shape=0.))])
    result.x, result.loss, result.step                          # best iterate per row, its loss, the step it was reached

One iteration is the decoder's forward (the loss head inside the rasteriser), its backward, and ONE more launch
(csrc/fit.hip, smplr_fit_step) that does everything else per row of x (B, P): the row's loss, the loss trace, the check
for non-finite values, the best iterate, the stop, and the Adam update.  No torch reduction, no optimiser object and no
host synchronisation in the loop; the state is device memory, so G iterations replay from one captured graph.

Semantics of one call for row b (the definition; tests/_fitting_oracle.py restates it in NumPy float64):
  1. L = mean(loss[b, :]) (+ silh_weight mean(silh_loss[b, :])).  Thread i of `THREADS` adds its strided share serially in
     fp32; a fixed tree combines the partial sums: the same bits on every launch and in any batch.
  2. history[calls[b], b] = L while calls[b] < H; calls[b] += 1.
  3. L or any g[b, :] not finite: bad[b] += 1, and nothing else of the row changes in this call.
  4. Else, a row with active[b]: L < best_loss[b] (strict) -> best_loss[b] = L, best_x[b, :] = x[b, :] (the iterate that
     produced L, before this call's update), best_step[b] = t[b], stall[b] = 0; otherwise stall[b] += 1.  With
     patience > 0 and stall[b] >= patience: active[b] = 0 and no update.
  5. A row still active: t += 1; g^ = grad_scale g; m = b1 m + (1 - b1) g^; v = b2 v + (1 - b2) g^ g^ (all P columns), and
       "keras": x -= lr col_scale[j] sqrt(1 - b2^t) / (1 - b1^t) m / (sqrt(v) + eps)     (Keras 2 `Adam`, eps = 1e-7)
       "torch": x -= lr col_scale[j] / (1 - b1^t) m / (sqrt(v) / sqrt(1 - b2^t) + eps)   (`torch.optim.Adam`)
     with both bias corrections in fp64.  x[b, j] keeps its bits where col_scale[j] = 0 or the new m is 0 (so: frozen
     columns, inactive and bad rows, and entries with g = m = v = 0).
Stages change col_scale only: step counts, moments and the best iterate run on across them.

Priors (SMPLify's regularisers; csrc/prior_device.h; tests/_prior_oracle.py restates them in NumPy float64).  A part map does
not determine bends in depth, twist about a limb's axis or the last shape components, so the data term can be paired with

    prior = PosePrior.from_pickle("gmm_08.pkl").with_angles(SMPLIFY_ANGLE_IDX, SMPLIFY_ANGLE_SCALE)
    result = fitter.fit(labels, init=prediction, stages=[(100, cs), (100, cs)], prior=prior,
                        prior_weights=[(4.04, 15.2, 1.0), (0.4, 1.5, 0.5)])         # one triple per stage: annealing
    E = prior_energy(x, prior.to(x.device), (1.0, 1.0, 1.0))                         # (B,), differentiable: a regulariser

For row b, with theta = x[num_cam : num_cam + 72], beta = x[num_cam + 72 :], theta' = theta[3:72] (the global rotation is free):
  pose   d_k = theta' - mean_k, y_k = A_k d_k, E_k = 1/2 |y_k|^2 + c_k over the K <= 16 components of a Gaussian mixture
         (A_k^T A_k = the inverse covariance); E_pose = the first minimum over k (max-mixture), gradient A_k*^T y_k*.
  angle  E_angle = sum_a exp(angle_scale[a] theta[angle_idx[a]]): A <= 16 terms that punish elbows and knees bent backwards.
  shape  E_shape = sum_i (beta_i - shape_mean_i)^2.
  E = w_pose E_pose + w_angle E_angle + w_shape E_shape; a term whose weight is exactly 0 is not evaluated.
Everything is fp64 on the fp32 operands in a fixed order and rounded to fp32 once per output, so a row's E and gradient are
the same bits on every launch and in any batch.  With a prior, `fit_step` makes ONE smplr_fit_step_prior launch instead of
smplr_fit_step: L = fp32(L_data + E), g + dE/dx (one fp32 addition) in place of g, steps 2 - 5 on these totals; a non-finite E
or gradient entry is a bad call.  The weights are a (3,) device tensor that `fit` rewrites at each stage boundary, so a
captured graph follows them.

Several views or frames of one body (csrc/fit.hip fit_group_kernel; tests/_fit_group_oracle.py restates it in NumPy float64):

    r = fitter.fit(labels, group_size=2, tie=("shape", "pose"))                      # front + side: one beta, one body pose
    r = fitter.fit(frames, group_size=8, tie=("shape",), smooth=smooth_weights(cam=0.1, global_rot=1.0, pose=1.0))   # a clip

Rows come in groups of G = group_size consecutive rows (B a multiple of G, 1 <= G <= 16); `tie` (P,) uint8 marks the columns
that are ONE unknown for a group, `smooth` (P,) fp32 >= 0 weighs a first-difference penalty between consecutive rows of a
group, per column (ignored where tie is set or the weight is 0).  ONE smplr_fit_step_group launch, one workgroup per group:
  a. L_r: every row's loss exactly as above (with a prior fp32(L_data + E_r)): the same bits.
  b. g_r[j]: the incoming gradient (+ dE_r/dx_j, one fp32 addition).
  c. E_s = sum_j smooth[j] sum_{r>=1} (x_r[j] - x_{r-1}[j])^2; s_r[j] = 2 smooth[j] ((x_r - x_{r-1})[r>0] - (x_{r+1} - x_r)[r<G-1]);
     fp64 on the fp32 operands in a fixed order, each rounded to fp32 once; g_r[j] += s_r[j] (one fp32 addition).  This is a
     penalty on differences of axis-angle (and camera, shape) entries, meant for neighbouring frames where they are small: it
     is no distance between rotations.
  d. L = fp32(sum_r L_r + E_s), rows in order.
  e. history[calls[b], b] = L_r, the row's own loss; calls[b] += 1 - every row.
  f. L or any g_r[j] of the group not finite: bad += 1 on every row of the group, nothing else of it changes.
  g. step 4's decisions once per group, on L, from t, stall, active, best_loss of the group's first row; written to all G rows
     alike; best_x[r] = x[r] for every row on a new best.
  h. an untied column of row r: step 5 with g_r[j] on the row's own m, v, x.  A tied column: step 5 with
     g = fp32(sum_r g_r[j]) (rows in order) on m, v, x of the group's first row, written to all G rows, so tied columns that
     start equal stay bit-equal (`fit` starts them at the group's mean).  Passed unequal, the first row's value wins wherever
     the column moves.
G = 1 without `smooth` is the plain call (and `fit_step` makes the plain launch then).  `FitState` keeps its layout: a group's
rows carry copies of the group's scalars.

Self-penetration (penetration.py, csrc/penetration.hip; SMPLify's fourth regulariser, the one that needs the mesh):

    fitter = ParamFitter(smpl_path, penetration=True)            # or a render.MeshTopology; ScanFitter(..., penetration=True)
    r = fitter.fit(labels, stages=[(100, cs), (100, cs)], pen_weight=[0.0, 50.0])   # one float, or one per stage

With E_b = pen_weight mean_V(e[b, :]), e = `self_penetration` of the iteration's vertices: E_b is added to every column of
the detached loss handed to `fit_step` (so the recorded loss, the best iterate and the patience stop see it), and its gradient
enters `torch.autograd.grad` through a preallocated cotangent pen_weight / V on e.  The weight lives in a device scalar and the
cotangent in a device tensor, both rewritten at stage boundaries, so a captured graph follows them.  `fit_step` and
csrc/fit.hip are untouched; without `penetration` a fitter runs exactly the launches it ran before.

2D keypoints (keypoints.py, csrc/keypoints.hip; detected image joints, SMPLify's data term):

    fitter = ParamFitter(smpl_path, keypoints=KeypointSpec.from_model(model), kp_sigma=3.0)
    r = fitter.fit(labels, keypoints=(target, conf), stages=[(100, cs), (100, cs)], kp_weight=[1.0, 0.1])
    r = KeypointFitter(smpl_path, sigma=3.0).fit(target, conf, steps=200)      # the keypoint term as the only data term

kp_weight mean_K(e[b, :]), e = `keypoint_energy` of the iteration's vertices (and posed joints) under cam = x[:, :4], joins the
loss and the one `torch.autograd.grad` call exactly as the self-penetration term does, through a cotangent kp_weight / K;
targets are in the decoder's pixel frame.  Without `keypoints` a fitter runs exactly the launches it ran before.

Label-map distances (labeldist.py, csrc/labeldist.hip; the one data term that pulls from far away and needs only the labels):

    fitter = LabelDistanceFitter(smpl_path, label_distance=True, ld_sigma=8.0) # or "visible", or a LabelDistanceSpec; a ParamFitter
    r = fitter.fit(labels, stages=[(100, cs), (100, cs)], ld_weight=[1.0, 0.1])

ld_weight mean(e[b, :]), e = `label_distance` of the iteration's vertices under cam = x[:, :4] against the fit's own labels -
every vertex to the nearest pixel of its part beside every labelled pixel to the nearest vertex of its part - is the third
side term, after penetration and keypoints, through a cotangent ld_weight / (V + W W).  The labels are sorted by class once
per fit, outside any captured graph.  `ParamFitter` itself keeps its signatures and runs exactly the launches it ran before.

Dense surface correspondences (surface.py, csrc/surface.hip; IUV pixels or markers that each name a face and barycentric weights):

    fitter = with_surface(ParamFitter)(smpl_path, surface=topo, sc_sigma=3.0)  # also LabelDistanceFitter, KeypointFitter, ScanFitter
    r = fitter.fit(labels, surface=SurfaceTargets(topo, face, bary, target, conf), stages=[(100, cs), (100, cs)], sc_weight=[1.0, 0.1])
    r = SurfaceFitter(smpl_path, sigma=3.0).fit(targets, steps=200)            # the surface term as the only data term

sc_weight mean_N(e[b, :]), e = `surface_energy` of the iteration's vertices against the fit's `SurfaceTargets` - under cam =
x[:, :4] with image targets (D = 2), in the vertices' own frame with 3D targets (D = 3; `ScanFitter` takes these only) - is the
fourth side term, after label distance, through a cotangent sc_weight / N.  The targets are sorted by face once, when they are
built, outside any captured graph.  `with_surface(cls)` is a class of its own for the reason `LabelDistanceFitter` is one: the
four fitters' constructors, `fit` and `losses` keep their signatures, and they run exactly the launches they ran before.

Per-row L-BFGS (csrc/lbfgs.hip, smplr_lbfgs_step; tests/_lbfgs_oracle.py restates it in NumPy float64).  The keypoint, scan and
prior terms are smooth least-squares-like energies that a quasi-Newton method minimises in far fewer evaluations than Adam:

    r = KeypointFitter(smpl_path, sigma=3.0).fit(target, conf, steps=60, mode="lbfgs")
    r = fitter.fit(labels, stages=[(40, cs0), (40, cs1)], mode=Lbfgs(memory=8, c1=1e-4, max_ls=10, tol_grad=0.0, lr=1.0), graph=True)

`mode` picks the update rule of `ParamFitter`, `LabelDistanceFitter`, `ScanFitter` and `KeypointFitter`: Adam's two forms, or
"lbfgs" / an `Lbfgs` record - a limited-memory BFGS with a backtracking Armijo line search, written as a state machine that
advances by exactly ONE function evaluation per launch, in `fit_step`'s place: the iteration (forward, one `autograd.grad`,
side terms, one launch), stages, graph capture, history, best iterate and patience stay as they are, and every row has its own
memory, direction, step length and line-search state.  `steps` and stage counts are evaluations; the record's `lr` is the first
trial step (fit's `lr`, `beta1`, `beta2`, `eps` are Adam's and ignored); a stage boundary also calls `state.restart()` - column
scales and weights change the objective, so the memory and f0 are void.  group_size > 1, tie with groups, or smooth raise
ValueError.  `LbfgsState` = `FitState` without m, v, plus x0, g0 (B, P) the accepted iterate and its scaled gradient, f0 (B,) its
loss, d (B, P) the direction, gd = g0 . d, alpha the step length, ls rejections in this line search, pairs (B,) int32 pairs ever
stored (ring slot pairs % M), phase (B,) uint8 (0: the next evaluation starts a search from x; 1: x is a trial point), S, Y
(B, M, P) the memory, 1 <= M <= 16.  state.x is always the point the next forward evaluates.  One call, for row b:
  1. L exactly as `fit_step`'s step 1 (+ prior): the same device functions, the same bits.
  2. history[calls[b], b] = L while calls[b] < H; calls[b] += 1.
  3. g^_j = c_j (grad_scale g_j), c = col_scale: two fp32 products.  The method works in z = x / c, so column scales are a
     diagonal preconditioner and c_j = 0 freezes column j.
  4. L or any g_j not finite: bad[b] += 1; in phase 0 nothing else of the row changes; in phase 1 an active row takes the call as
     a rejected trial (8), without 6.
  5. An inactive row: nothing else changes.
  6. `fit_step`'s step 4 on the evaluated point: L < best_loss (strict) -> best_loss, best_x = x, best_step = t, stall = 0,
     otherwise stall += 1; patience > 0 and stall >= patience: active = 0 and nothing below happens.
  7. Accept in phase 0, or when L <= f0 + c1 alpha gd (fp64 on the four fp32 values).  Then, in this order: (7.1, phase 1)
     s_j = fp32(alpha d_j), y_j = g^_j - g0_j; y . s > 1e-10 (the rule of `torch.optim.LBFGS`): the pair goes to slot pairs % M and
     pairs += 1; t += 1 either way.  (7.2) x0 = x, f0 = L, g0 = g^.  (7.3) max_j |g^_j| <= tol_grad: active = 0, stop here.  (7.4) the
     two-loop recursion in fp64 over the k = min(pairs, M) newest pairs, rho_i = 1 / (y_i . s_i) from the stored vectors, scaled by
     (y . s) / (y . y) of the newest pair between the loops; d = fp32(-q), gd = fp32(g^ . d).  (7.5) k > 0 and not gd < 0: pairs = 0.
     (7.6) k = 0 or pairs = 0: d = -g^, gd = fp32(-g^ . g^), alpha = fp32(lr min(1, 1 / |g^|_1)); otherwise alpha = lr.  (7.7) ls = 0,
     phase = 1.
  8. Reject: ls += 1.  ls > max_ls: with pairs > 0 the memory is forgotten and the search restarts along steepest descent from x0
     (pairs = 0, d = -g0, gd = fp32(-g0 . g0), alpha = fp32(lr min(1, 1 / |g0|_1)), ls = 0); with pairs = 0 already the line search
     has failed at fp32 resolution: active = 0.  Otherwise alpha = fp32(alpha / 2).
  9. An active row: x_j = x0_j + (alpha c_j) d_j, three fp32 operations; not stored where c_j = 0.
Dot products are fp64 on the fp32 operands, combined by the loss's fixed tree; every stored value is rounded to fp32 once.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, fields, replace
from typing import Optional

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr, stream

THREADS = 256                  # threads of a row's workgroup (csrc/fit.hip FT_T) = the widest row
MODES = ("keras", "torch")
KERAS_EPS = 1e-7               # keras.backend.epsilon(): Adam(epsilon=None) of Keras 2
POSE_DIM = 69                  # theta[3:72]: what the pose prior sees (csrc/prior_device.h PR_D)
MAX_COMPONENTS = 16            # PR_KMAX
MAX_ANGLES = 16                # PR_AMAX
# SMPLify's four bending terms: both elbows and both knees (theta indices), exp(+theta[55]), exp(-theta[58]), exp(-theta[12]),
# exp(-theta[15])
SMPLIFY_ANGLE_IDX = (55, 58, 12, 15)
SMPLIFY_ANGLE_SCALE = (1.0, -1.0, -1.0, -1.0)
MAX_GROUP = 16                 # rows of a group (csrc/fit.hip FT_GMAX)
TIE_NAMES = ("cam", "global_rot", "pose", "shape")
MAX_MEMORY = 16                # pairs of a row's L-BFGS memory (csrc/lbfgs.hip LB_MMAX)


@dataclass
class FitState:
    """The per-row state smplr_fit_step reads and writes: x, m, v, best_x (B, P) fp32; t (updates done), calls, stall
    (calls since the best), bad (calls with a non-finite loss or gradient), best_step (B) int32; active (B) uint8;
    best_loss (B) fp32."""
    x: torch.Tensor
    m: torch.Tensor
    v: torch.Tensor
    best_x: torch.Tensor
    t: torch.Tensor
    calls: torch.Tensor
    stall: torch.Tensor
    bad: torch.Tensor
    best_step: torch.Tensor
    active: torch.Tensor
    best_loss: torch.Tensor

    @classmethod
    def new(cls, x0):
        """x0 (B, P) -> a fresh state around a float32 copy of it: m = v = 0, t = calls = stall = bad = best_step = 0,
        active = 1, best_loss = +inf, best_x = x0."""
        if not isinstance(x0, torch.Tensor):
            x0 = torch.as_tensor(np.asarray(x0))
        if x0.dim() != 2 or not 1 <= x0.shape[1] <= THREADS:
            raise ValueError("x0 must be (B, P) with 1 <= P <= %d, got %s" % (THREADS, tuple(x0.shape)))
        x = x0.detach().to(torch.float32).clone().contiguous()
        B = x.shape[0]
        zi = lambda: torch.zeros(B, dtype=torch.int32, device=x.device)
        return cls(x=x, m=torch.zeros_like(x), v=torch.zeros_like(x), best_x=x.clone(), t=zi(), calls=zi(), stall=zi(),
                   bad=zi(), best_step=zi(), active=torch.ones(B, dtype=torch.uint8, device=x.device),
                   best_loss=torch.full((B,), float("inf"), dtype=torch.float32, device=x.device))

    def clone(self):
        return FitState(**{f.name: getattr(self, f.name).clone() for f in fields(self)})


@dataclass(frozen=True)
class Lbfgs:
    """`fit(mode=Lbfgs(...))`: per-row L-BFGS in Adam's place ("lbfgs" = the defaults).  memory: pairs kept per row, 1..16;
    c1: the Armijo constant, in (0, 1); max_ls: halvings of a line search before the memory is dropped (then: before the row
    stops); tol_grad: a row stops when max_j |g^_j| <= tol_grad; lr: the first trial step of a search, > 0."""
    memory: int = 8
    c1: float = 1e-4
    max_ls: int = 10
    tol_grad: float = 0.0
    lr: float = 1.0

    def __post_init__(self):
        check_memory(self.memory)
        if isinstance(self.max_ls, bool) or not isinstance(self.max_ls, (int, np.integer)) or self.max_ls < 0:
            raise ValueError("max_ls must be an integer >= 0, got %r" % (self.max_ls,))
        if not (0.0 < float(self.c1) < 1.0):
            raise ValueError("c1 must lie in (0, 1), got %r" % (self.c1,))
        if not (math.isfinite(float(self.tol_grad)) and float(self.tol_grad) >= 0.0):
            raise ValueError("tol_grad must be finite and >= 0, got %r" % (self.tol_grad,))
        if not (math.isfinite(float(self.lr)) and float(self.lr) > 0.0):
            raise ValueError("lr must be finite and > 0, got %r" % (self.lr,))


def check_memory(memory):
    if isinstance(memory, bool) or not isinstance(memory, (int, np.integer)) or not 1 <= memory <= MAX_MEMORY:
        raise ValueError("memory must be an integer in 1..%d, got %r" % (MAX_MEMORY, memory))
    return int(memory)


def check_mode(mode, lbfgs=True):
    """`fit`'s mode -> None for Adam's two forms, an `Lbfgs` record for "lbfgs" or a record; anything else: ValueError."""
    if isinstance(mode, Lbfgs):
        opt = mode
    elif isinstance(mode, str) and mode == "lbfgs":
        opt = Lbfgs()
    elif isinstance(mode, str) and mode in MODES:
        return None
    else:
        raise ValueError("mode %r is none of %s%s" % (mode, MODES, ", \"lbfgs\" or an Lbfgs record" if lbfgs else ""))
    if not lbfgs:
        raise ValueError("mode %r: this loop runs Adam only, mode is one of %s" % (mode, MODES))
    return opt


@dataclass
class LbfgsState:
    """The per-row state smplr_lbfgs_step reads and writes: every field of `FitState` but m and v, with the same meaning, and
    x0, g0, d (B, P) fp32; f0, gd, alpha (B,) fp32; ls, pairs (B,) int32; phase (B,) uint8; S, Y (B, M, P) fp32 (the module's
    semantics).  x is always the point the next forward evaluates."""
    x: torch.Tensor
    best_x: torch.Tensor
    t: torch.Tensor
    calls: torch.Tensor
    stall: torch.Tensor
    bad: torch.Tensor
    best_step: torch.Tensor
    active: torch.Tensor
    best_loss: torch.Tensor
    x0: torch.Tensor
    g0: torch.Tensor
    f0: torch.Tensor
    d: torch.Tensor
    gd: torch.Tensor
    alpha: torch.Tensor
    ls: torch.Tensor
    pairs: torch.Tensor
    phase: torch.Tensor
    S: torch.Tensor
    Y: torch.Tensor

    @classmethod
    def new(cls, x0, memory=8):
        """x0 (B, P) -> a fresh state around a float32 copy of it: phase = 0, an empty memory of `memory` pairs, every counter 0,
        active = 1, best_loss = +inf, best_x = x0 = x."""
        M = check_memory(memory)
        base = FitState.new(x0)
        x = base.x
        B, P = int(x.shape[0]), int(x.shape[1])
        zf = lambda: torch.zeros(B, dtype=torch.float32, device=x.device)
        zi = lambda: torch.zeros(B, dtype=torch.int32, device=x.device)
        return cls(x=x, best_x=base.best_x, t=base.t, calls=base.calls, stall=base.stall, bad=base.bad, best_step=base.best_step,
                   active=base.active, best_loss=base.best_loss, x0=x.clone(), g0=torch.zeros_like(x), f0=zf(), d=torch.zeros_like(x),
                   gd=zf(), alpha=zf(), ls=zi(), pairs=zi(), phase=torch.zeros(B, dtype=torch.uint8, device=x.device),
                   S=torch.zeros((B, M, P), dtype=torch.float32, device=x.device),
                   Y=torch.zeros((B, M, P), dtype=torch.float32, device=x.device))

    @property
    def memory(self):
        return int(self.S.shape[1])

    def clone(self):
        return LbfgsState(**{f.name: getattr(self, f.name).clone() for f in fields(self)})

    def restart(self):
        """The objective has changed (column scales, weights): rows at a trial point go back to their accepted iterate, and every
        row forgets its memory and starts a new search with its next evaluation - x <- x0 where phase = 1; pairs = ls = 0,
        phase = 0.  Counters and the best iterate run on.  In place, on the tensors' device, no host synchronisation."""
        self.x.copy_(torch.where((self.phase != 0)[:, None], self.x0, self.x))
        self.pairs.zero_()
        self.ls.zero_()
        self.phase.zero_()
        return self


def column_scale(cam=1.0, pose=1.0, shape=1.0, num_cam=4):
    """(P,) float32 per-column learning-rate multipliers for x = [cam (num_cam) | pose (72) | shape (10)]: camera columns are
    in pixels, pose in radians, shape in standard deviations.  0 freezes a block."""
    num_cam = int(num_cam)
    if num_cam < 0 or num_cam + 82 > THREADS:
        raise ValueError("num_cam must lie in 0..%d, got %r" % (THREADS - 82, num_cam))
    s = torch.empty(num_cam + 82, dtype=torch.float32)
    s[:num_cam], s[num_cam:num_cam + 72], s[num_cam + 72:] = float(cam), float(pose), float(shape)
    if not bool(torch.isfinite(s).all()) or bool((s < 0).any()):
        raise ValueError("column scales must be finite and >= 0, got cam=%r pose=%r shape=%r" % (cam, pose, shape))
    return s


def _blocks(num_cam):
    """Column ranges of x = [cam | global_rot (theta[0:3]) | pose (theta[3:72]) | shape] for `num_cam` camera columns."""
    num_cam = int(num_cam)
    if num_cam < 0 or num_cam + 82 > THREADS:
        raise ValueError("num_cam must lie in 0..%d, got %r" % (THREADS - 82, num_cam))
    return {"cam": (0, num_cam), "global_rot": (num_cam, num_cam + 3), "pose": (num_cam + 3, num_cam + 72),
            "shape": (num_cam + 72, num_cam + 82)}


def tie_mask(shape=True, pose=False, global_rot=False, cam=False, num_cam=4):
    """(P,) uint8 mask of the columns that are one unknown for a whole group of rows (`fit(group_size=...)`): 1 on the
    blocks named.  pose = theta[3:72] (the body pose), global_rot = theta[0:3]; a sibling of `column_scale`."""
    blocks = _blocks(num_cam)
    tie = torch.zeros(int(num_cam) + 82, dtype=torch.uint8)
    for name, on in (("shape", shape), ("pose", pose), ("global_rot", global_rot), ("cam", cam)):
        if not isinstance(on, (bool, np.bool_)):
            raise ValueError("%s must be True or False, got %r" % (name, on))
        if on:
            lo, hi = blocks[name]
            tie[lo:hi] = 1
    return tie


def smooth_weights(cam=0.0, global_rot=0.0, pose=0.0, shape=0.0, num_cam=4):
    """(P,) float32 weights of the first-difference penalty between consecutive rows of a group, per column block; each
    finite and >= 0 (0: no penalty).  On the rotation columns it weighs differences of axis-angle entries: meant for
    neighbouring frames."""
    blocks = _blocks(num_cam)
    s = torch.empty(int(num_cam) + 82, dtype=torch.float32)
    for name, w in (("cam", cam), ("global_rot", global_rot), ("pose", pose), ("shape", shape)):
        w = float(w)
        if not math.isfinite(w) or w < 0 or w > float(np.finfo(np.float32).max):
            raise ValueError("smoothing weights must be finite and >= 0, got %s=%r" % (name, w))
        lo, hi = blocks[name]
        s[lo:hi] = w
    return s


def check_tie(tie, P, num_cam=4):
    """Block names ("cam", "global_rot", "pose", "shape") or a (P,) mask -> a (P,) uint8 CPU tensor of 0 / 1."""
    if isinstance(tie, str):
        tie = (tie,)
    if isinstance(tie, (tuple, list)) and all(isinstance(n, str) for n in tie):
        for n in tie:
            if n not in TIE_NAMES:
                raise ValueError("tie names %r; the blocks are %s" % (n, TIE_NAMES))
        m = tie_mask(**{n: n in tie for n in TIE_NAMES}, num_cam=num_cam)
    else:
        a = np.asarray(tie.detach().cpu() if isinstance(tie, torch.Tensor) else tie)
        if a.shape != (P,) or not (a.dtype == np.bool_ or np.issubdtype(a.dtype, np.integer)) or not np.isin(a, (0, 1)).all():
            raise ValueError("tie must be block names or a (%d,) mask of 0 / 1, got %r" % (P, tie))
        m = torch.as_tensor(a.astype(np.uint8))
    if tuple(m.shape) != (P,):
        raise ValueError("tie covers %d columns, x has %d" % (m.shape[0], P))
    return m.contiguous()


def check_smooth(smooth, P):
    """A (P,) array of weights -> a (P,) float32 CPU tensor; each finite and >= 0."""
    a = np.asarray(smooth.detach().cpu() if isinstance(smooth, torch.Tensor) else smooth, dtype=np.float64)
    if a.shape != (P,):
        raise ValueError("smooth must be (%d,), got %s" % (P, a.shape))
    s = torch.as_tensor(a).to(torch.float32).contiguous()
    if not bool(torch.isfinite(s).all()) or bool((s < 0).any()):
        raise ValueError("smoothing weights must be finite and >= 0")
    return s


def check_group(B, group_size):
    G = int(group_size)
    if not 1 <= G <= MAX_GROUP:
        raise ValueError("group_size must lie in 1..%d, got %r" % (MAX_GROUP, group_size))
    if B % G:
        raise ValueError("%d rows are no multiple of group_size = %d" % (B, G))
    return G


def check_stages(stages, P, steps=None):
    """A stage list [(steps, column_scale), ...] -> [(int steps, (P,) float32 CPU tensor), ...]; None -> one stage of
    `steps` with every column at 1."""
    if stages is None:
        if steps is None:
            raise ValueError("either steps or stages is needed")
        stages = [(steps, torch.ones(P))]
    out = []
    for i, st in enumerate(stages):
        if not isinstance(st, (tuple, list)) or len(st) != 2:
            raise ValueError("stage %d must be (steps, column_scale), got %r" % (i, st))
        n, cs = int(st[0]), torch.as_tensor(st[1], dtype=torch.float32).detach().cpu().contiguous()
        if n < 0:
            raise ValueError("stage %d has %d steps" % (i, n))
        if tuple(cs.shape) != (P,):
            raise ValueError("stage %d: column_scale must be (%d,), got %s" % (i, P, tuple(cs.shape)))
        if not bool(torch.isfinite(cs).all()) or bool((cs < 0).any()):
            raise ValueError("stage %d: column scales must be finite and >= 0" % i)
        out.append((n, cs))
    return out

def _f32(a, shape, name):
    t = torch.as_tensor(np.asarray(a.detach().cpu() if isinstance(a, torch.Tensor) else a, dtype=np.float64))
    if tuple(t.shape) != tuple(shape):
        raise ValueError("%s must be %s, got %s" % (name, tuple(shape), tuple(t.shape)))
    t = t.to(torch.float32).contiguous()
    if not bool(torch.isfinite(t).all()):
        raise ValueError("%s holds values that are not finite in float32" % name)
    return t


def check_prior_weights(w, name="prior_weights"):
    """(w_pose, w_angle, w_shape) -> a (3,) float32 CPU tensor; each finite and >= 0."""
    t = torch.as_tensor(np.asarray(w.detach().cpu() if isinstance(w, torch.Tensor) else w, dtype=np.float64))
    if tuple(t.shape) != (3,):
        raise ValueError("%s must be (w_pose, w_angle, w_shape), got %r" % (name, w))
    t = t.to(torch.float32)
    if not bool(torch.isfinite(t).all()) or bool((t < 0).any()):
        raise ValueError("%s must be finite and >= 0, got %r" % (name, w))
    return t


def mixture_terms(covs, mix_weights):
    """covs (K, D, D), mix_weights (K,) -> float64 (factor (K, D, D), offset (K,)): factor[k] = the upper Cholesky factor of
    inv(covs[k]), so factor[k]^T factor[k] covs[k] = I; offset[k] = -log w_k + 1/2 (logdet covs[k] - min_j logdet covs[j]) with
    the weights normalised to sum 1 (so offset >= 0)."""
    covs = np.asarray(covs, np.float64)
    w = np.asarray(mix_weights, np.float64)
    K = covs.shape[0]
    factor = np.empty_like(covs)
    logdet = np.empty(K)
    for k in range(K):
        try:
            prec = np.linalg.inv(covs[k])
            factor[k] = np.linalg.cholesky(0.5 * (prec + prec.T)).T
        except np.linalg.LinAlgError as e:
            raise ValueError("covariance %d is not positive definite: %s" % (k, e)) from None
        sign, logdet[k] = np.linalg.slogdet(covs[k])
        if sign <= 0:
            raise ValueError("covariance %d is not positive definite" % k)
    return factor, np.maximum(-np.log(w / w.sum()) + 0.5 * (logdet - logdet.min()), 0.0)


@dataclass
class PosePrior:
    """The priors' data as fp32 tensors (built on the CPU and validated there; `.to(device)` for the kernels):
    mean (K, 69), factor (K, 69, 69) dense row-major A_k with A_k^T A_k = inverse covariance, offset (K,) c_k >= 0,
    angle_idx (A,) int32 in 0..71 with angle_scale (A,), shape_mean (10,); 1 <= K <= 16, 0 <= A <= 16."""
    mean: torch.Tensor
    factor: torch.Tensor
    offset: torch.Tensor
    angle_idx: torch.Tensor = None
    angle_scale: torch.Tensor = None
    shape_mean: torch.Tensor = None

    def __post_init__(self):
        # (always: tensors that live on a device are validated through a CPU copy, and the prior built is on the CPU;
        # only `.to()` makes a device copy, of fields that passed here)
        K = int(np.shape(self.mean)[0]) if np.ndim(self.mean) == 2 else -1
        if not 1 <= K <= MAX_COMPONENTS:
            raise ValueError("mean must be (K, %d) with 1 <= K <= %d, got %s" % (POSE_DIM, MAX_COMPONENTS, tuple(np.shape(self.mean))))
        self.mean = _f32(self.mean, (K, POSE_DIM), "mean")
        self.factor = _f32(self.factor, (K, POSE_DIM, POSE_DIM), "factor")
        self.offset = _f32(self.offset, (K,), "offset")
        if bool((self.offset < 0).any()):
            raise ValueError("offset must be >= 0")
        idx = np.asarray([] if self.angle_idx is None else
                         (self.angle_idx.detach().cpu() if isinstance(self.angle_idx, torch.Tensor) else self.angle_idx))
        A = idx.size
        if idx.ndim != 1 or A > MAX_ANGLES:
            raise ValueError("angle_idx must be (A,) with A <= %d, got shape %s" % (MAX_ANGLES, idx.shape))
        if A and (not np.array_equal(idx, np.round(idx)) or idx.min() < 0 or idx.max() > 71):
            raise ValueError("angle_idx must hold integers in 0..71, got %s" % idx.tolist())
        self.angle_idx = torch.as_tensor(idx.astype(np.int32)).contiguous()
        self.angle_scale = _f32([] if self.angle_scale is None else self.angle_scale, (A,), "angle_scale")
        self.shape_mean = _f32(np.zeros(10) if self.shape_mean is None else self.shape_mean, (10,), "shape_mean")

    @property
    def K(self):
        return int(self.mean.shape[0])

    @property
    def A(self):
        return int(self.angle_idx.shape[0])

    @property
    def device(self):
        return self.mean.device

    def to(self, device):
        """A copy of the validated fields on `device` (not validated again: no host synchronisation)."""
        p = object.__new__(PosePrior)
        for f in fields(self):
            setattr(p, f.name, getattr(self, f.name).to(device))
        return p

    def cpu(self):
        return self if not self.mean.is_cuda else self.to("cpu")

    def with_angles(self, idx=SMPLIFY_ANGLE_IDX, scale=SMPLIFY_ANGLE_SCALE):
        """The same prior with angle terms exp(scale[a] theta[idx[a]]); idx in 0..71 (theta's own numbering)."""
        return replace(self.cpu(), angle_idx=list(idx), angle_scale=list(scale))

    def with_shape_mean(self, shape_mean):
        return replace(self.cpu(), shape_mean=shape_mean)

    # ---- constructors -------------------------------------------------------------------------------------------------
    @classmethod
    def mixture(cls, means, covs, mix_weights):
        """A Gaussian mixture over theta[3:72]: means (K, 69), covs (K, 69, 69) symmetric positive definite, mix_weights (K,)
        > 0.  A_k = the upper Cholesky factor of inv(cov_k) in float64 (A_k^T A_k = inv(cov_k));
        c_k = -log w_k + 1/2 (logdet cov_k - min_j logdet cov_j) >= -log w_k.  The (2 pi)^(D/2) constant is left out: it moves
        neither the arg-min nor the gradient, and E stays on the data term's scale."""
        means = np.asarray(means, np.float64)
        covs = np.asarray(covs, np.float64)
        w = np.asarray(mix_weights, np.float64)
        K = means.shape[0] if means.ndim == 2 else -1
        if not 1 <= K <= MAX_COMPONENTS or means.shape != (K, POSE_DIM) or covs.shape != (K, POSE_DIM, POSE_DIM) or w.shape != (K,):
            raise ValueError("means (K, 69), covs (K, 69, 69), mix_weights (K,) with 1 <= K <= %d; got %s, %s, %s"
                             % (MAX_COMPONENTS, means.shape, covs.shape, w.shape))
        if not (np.isfinite(means).all() and np.isfinite(covs).all() and np.isfinite(w).all()) or (w <= 0).any():
            raise ValueError("means, covs and mix_weights must be finite, the weights > 0")
        factor, offset = mixture_terms(covs, w)
        return cls(mean=means, factor=factor, offset=offset)

    @classmethod
    def gaussian(cls, mean69, cov):
        return cls.mixture(np.asarray(mean69, np.float64)[None], np.asarray(cov, np.float64)[None], [1.0])

    @classmethod
    def from_samples(cls, theta69, shrink=0.1):
        """One Gaussian from poses theta69 (N, 69): the sample mean and the covariance shrunk towards its own diagonal mean,
        (1 - shrink) S + shrink tr(S) / 69 I (N may be smaller than 69)."""
        t = np.asarray(theta69, np.float64)
        if t.ndim != 2 or t.shape[1] != POSE_DIM or t.shape[0] < 2 or not 0.0 < shrink <= 1.0:
            raise ValueError("theta69 must be (N >= 2, 69) and 0 < shrink <= 1")
        S = np.cov(t, rowvar=False)
        return cls.gaussian(t.mean(0), (1.0 - shrink) * S + shrink * np.trace(S) / POSE_DIM * np.eye(POSE_DIM))

    @classmethod
    def mean_pose(cls, sigma=0.5):
        """Isotropic, sigma radians about the mean pose of data/mean_params.npz."""
        from .smpl_model import load_mean_params
        if not (math.isfinite(sigma) and sigma > 0):
            raise ValueError("sigma must be > 0")
        pose, shape = load_mean_params()
        return cls(mean=pose[None, 3:], factor=(np.eye(POSE_DIM) / sigma)[None], offset=[0.0], shape_mean=np.zeros(10))

    @classmethod
    def from_pickle(cls, path):
        """SMPLify's `gmm_08.pkl` layout: a (Python 2) pickle of {'means' (K, 69), 'covars' (K, 69, 69), 'weights' (K,)}, read
        by a restricted unpickler that refuses every global outside numpy's array reconstruction."""
        from .smpl_pkl import load_numpy_pickle
        dd = load_numpy_pickle(path)
        if not isinstance(dd, dict) or not all(k in dd for k in ("means", "covars", "weights")):
            raise ValueError("%s: not a dict with 'means', 'covars' and 'weights'" % path)
        return cls.mixture(dd["means"], dd["covars"], dd["weights"])


def check_prior_layout(prior):
    """What the kernels take on trust, checked without reading a value (no host synchronisation; any device): every field a
    contiguous tensor of its dtype, mean (K, 69), factor (K, 69, 69), offset (K,) with 1 <= K <= 16, angle_idx and
    angle_scale (A,) with A <= 16, shape_mean (10,).  The launchers get raw pointers and cannot see any of it."""
    if not isinstance(prior, PosePrior):
        raise TypeError("prior must be a PosePrior")
    mean = prior.mean
    K = int(mean.shape[0]) if isinstance(mean, torch.Tensor) and mean.dim() == 2 else -1
    idx = prior.angle_idx
    A = int(idx.shape[0]) if isinstance(idx, torch.Tensor) and idx.dim() == 1 else -1
    if not 1 <= K <= MAX_COMPONENTS or not 0 <= A <= MAX_ANGLES:
        raise RuntimeError("prior.mean must be a (K, %d) tensor with 1 <= K <= %d and prior.angle_idx an (A,) tensor with A <= %d"
                           % (POSE_DIM, MAX_COMPONENTS, MAX_ANGLES))
    want = {"mean": (K, POSE_DIM), "factor": (K, POSE_DIM, POSE_DIM), "offset": (K,), "angle_idx": (A,), "angle_scale": (A,),
            "shape_mean": (10,)}
    for name, shape in want.items():
        a = getattr(prior, name)
        dtype = torch.int32 if name == "angle_idx" else torch.float32
        if not isinstance(a, torch.Tensor) or tuple(a.shape) != shape or a.dtype != dtype or not a.is_contiguous():
            raise RuntimeError("prior.%s must be a contiguous %s tensor of shape %s, got %s"
                               % (name, dtype, shape, "%s %s" % (a.dtype, tuple(a.shape)) if isinstance(a, torch.Tensor) else type(a)))
    return prior


def _prior_operands(prior, weights, x):
    """Checked operands of a prior launch on x's device: (prior, weights (3,) fp32 device tensor)."""
    check_prior_layout(prior)
    for f in fields(prior):
        a = getattr(prior, f.name)
        if a.device != x.device:
            raise RuntimeError("prior.%s lives on %s, x on %s: use prior.to(device)" % (f.name, a.device, x.device))
        _lib.require_cuda(a, "prior." + f.name, torch.int32 if f.name == "angle_idx" else torch.float32)
    if isinstance(weights, torch.Tensor) and weights.is_cuda:
        if tuple(weights.shape) != (3,) or weights.device != x.device:
            raise RuntimeError("prior weights must be a (3,) tensor on %s" % x.device)
        w = _lib.require_cuda(weights, "prior_weights")
    else:
        w = check_prior_weights((1.0, 1.0, 1.0) if weights is None else weights).to(x.device)
    return prior, w


def _prior_args(prior, w, num_cam):
    """The ten arguments every launcher takes from num_cam to weights, of `_prior_operands`' pair (the caller holds on to w
    until it has launched); prior None: no prior, all NULL and 0."""
    if prior is None:
        return (int(num_cam), None, None, None, None, None, None, 0, 0, None)
    return (int(num_cam), ptr(prior.mean), ptr(prior.factor), ptr(prior.offset), ptr(prior.angle_idx) if prior.A else None,
            ptr(prior.angle_scale) if prior.A else None, ptr(prior.shape_mean), prior.K, prior.A, ptr(w))


@_lib.on_device
def prior_terms(x, prior, weights=None, num_cam=4, with_grad=True):
    """One smplr_prior_energy launch: x (B, num_cam + 82) -> dict(energy (B, 4) = E_pose, E_angle, E_shape unweighted and the
    weighted E; comp (B,) int32 = the winning component; grad (B, P) = dE/dx or None)."""
    x = _lib.require_cuda(x.detach(), "x")
    if x.dim() != 2 or x.shape[1] != int(num_cam) + 82:
        raise RuntimeError("x must be (B, num_cam + 82) with num_cam = %d, got %s" % (num_cam, tuple(x.shape)))
    prior, w = _prior_operands(prior, weights, x)
    B, P = int(x.shape[0]), int(x.shape[1])
    energy = torch.empty((B, 4), dtype=torch.float32, device=x.device)
    comp = torch.empty((B,), dtype=torch.int32, device=x.device)
    grad = torch.empty((B, P), dtype=torch.float32, device=x.device) if with_grad else None
    check(_lib.load().smplr_prior_energy(ptr(x), B, P, *_prior_args(prior, w, num_cam), ptr(energy), ptr(comp), ptr(grad), stream()),
          "smplr_prior_energy")
    return {"energy": energy, "comp": comp, "grad": grad}


class _PriorEnergy(torch.autograd.Function):
    """-> E (B,), energy (B, 4), comp (B,), grad (B, P) of one launch; only E is differentiable."""

    @staticmethod
    def forward(ctx, x, prior, weights, num_cam):
        out = prior_terms(x, prior, weights, num_cam, with_grad=True)
        ctx.save_for_backward(out["grad"])
        ctx.mark_non_differentiable(out["energy"], out["comp"], out["grad"])
        return out["energy"][:, 3].clone(), out["energy"], out["comp"], out["grad"]

    @staticmethod
    def backward(ctx, upstream, *_):
        (grad,) = ctx.saved_tensors
        return upstream[:, None] * grad, None, None, None


def prior_energy(x, prior, weights=None, num_cam=4, return_terms=False):
    """E (B,) of the rows of x (B, num_cam + 82), differentiable in x: forward is one smplr_prior_energy launch that also
    saves dE/dx, backward is upstream[:, None] * dE/dx.  weights = (w_pose, w_angle, w_shape) (None: ones) or a (3,) device
    tensor.  return_terms=True -> (E, dict(energy (B, 4), comp (B,), grad (B, P))): the breakdown of the same launch (constants
    to autograd; E stays differentiable)."""
    E, energy, comp, grad = _PriorEnergy.apply(x, prior, weights, num_cam)
    return (E, {"energy": energy, "comp": comp, "grad": grad}) if return_terms else E


@_lib.on_device
def fit_step(state, grad, loss, silh_loss=None, silh_weight=1.0, col_scale=None, history=None, lr=1e-3, beta1=0.9,
             beta2=0.999, eps=KERAS_EPS, grad_scale=1.0, mode="keras", patience=0, prior=None, prior_weights=None, num_cam=4,
             group_size=1, tie=None, smooth=None):
    """One smplr_fit_step launch on `state` (in place; see the module's semantics).  grad (B, P): the gradient of
    sum_b L_b; loss (B, N) and silh_loss (B, Ns): per-pixel losses as `SMPLDecoder(loss=...)` returns them; col_scale (P,)
    (None: ones); history (H, B) or None.  HIP tensors only.  With prior (a `PosePrior` on the device) the launch is
    smplr_fit_step_prior: the prior's E joins L and its gradient joins grad inside the kernel; prior_weights = a triple or
    a (3,) device tensor (None: ones); P = num_cam + 82.  group_size = G > 1 or a `smooth`: ONE smplr_fit_step_group launch over
    groups of G consecutive rows (the module's semantics a - h), with or without a prior; tie (P,) uint8 and smooth (P,) fp32
    are device tensors (tie None: nothing tied), checked for shape, dtype and device only - no value is read.  group_size = 1
    without `smooth` makes the plain launch."""
    if mode not in MODES:
        raise ValueError("mode %r is none of %s" % (mode, MODES))
    rc = _lib.require_cuda
    if not state.x.is_contiguous():
        raise RuntimeError("x must be contiguous (it is updated in place)")
    x = rc(state.x, "x")
    B, P = int(x.shape[0]), int(x.shape[1])
    same = {"grad": grad, "m": state.m, "v": state.v, "best_x": state.best_x}
    ints = {"t": state.t, "calls": state.calls, "stall": state.stall, "bad": state.bad, "best_step": state.best_step}
    for name, a in same.items():
        if tuple(a.shape) != (B, P) or not a.is_contiguous():
            raise RuntimeError("%s must be a contiguous (%d, %d) tensor, got %s" % (name, B, P, tuple(a.shape)))
        rc(a, name)
    for name, a in ints.items():
        if tuple(a.shape) != (B,):
            raise RuntimeError("%s must be (%d,), got %s" % (name, B, tuple(a.shape)))
        rc(a, name, torch.int32)
    if tuple(state.active.shape) != (B,) or tuple(state.best_loss.shape) != (B,):
        raise RuntimeError("active and best_loss must be (%d,)" % B)
    rc(state.active, "active", torch.uint8)
    rc(state.best_loss, "best_loss")
    if loss.dim() != 2 or loss.shape[0] != B or loss.shape[1] < 1 or not loss.is_contiguous():
        raise RuntimeError("loss must be a contiguous (%d, N) tensor, got %s" % (B, tuple(loss.shape)))
    rc(loss, "loss")
    Ns = 0
    if silh_loss is not None:
        if silh_loss.dim() != 2 or silh_loss.shape[0] != B or silh_loss.shape[1] < 1 or not silh_loss.is_contiguous():
            raise RuntimeError("silh_loss must be a contiguous (%d, Ns) tensor, got %s" % (B, tuple(silh_loss.shape)))
        rc(silh_loss, "silh_loss")
        Ns = int(silh_loss.shape[1])
    if col_scale is None:
        col_scale = torch.ones(P, dtype=torch.float32, device=x.device)
    if tuple(col_scale.shape) != (P,) or not col_scale.is_contiguous():
        raise RuntimeError("col_scale must be a contiguous (%d,) tensor, got %s" % (P, tuple(col_scale.shape)))
    rc(col_scale, "col_scale")
    H = 0
    if history is not None:
        if history.dim() != 2 or history.shape[1] != B or not history.is_contiguous():
            raise RuntimeError("history must be a contiguous (H, %d) tensor, got %s" % (B, tuple(history.shape)))
        rc(history, "history")
        H = int(history.shape[0])
    for name, a in list(same.items()) + list(ints.items()) + [("active", state.active), ("best_loss", state.best_loss),
                                                               ("loss", loss), ("silh_loss", silh_loss),
                                                               ("col_scale", col_scale), ("history", history)]:
        if a is not None and a.device != x.device:
            raise RuntimeError("%s lives on %s, x on %s" % (name, a.device, x.device))
    grouped = int(group_size) != 1 or smooth is not None
    if grouped:
        G = check_group(B, group_size)
        if tie is None:
            tie = torch.zeros(P, dtype=torch.uint8, device=x.device)
        for name, a, dt in (("tie", tie, torch.uint8), ("smooth", smooth, torch.float32)):
            if a is None:
                continue
            if not isinstance(a, torch.Tensor) or tuple(a.shape) != (P,) or not a.is_contiguous():
                raise RuntimeError("%s must be a contiguous (%d,) tensor" % (name, P))
            rc(a, name, dt)
            if a.device != x.device:
                raise RuntimeError("%s lives on %s, x on %s" % (name, a.device, x.device))
    w = None
    if prior is not None:
        prior, w = _prior_operands(prior, prior_weights, x)
    elif prior_weights is not None:
        raise ValueError("prior_weights without a prior")
    # what every launcher starts with: smplr_fit_step's own arguments up to the stream
    common = (ptr(x), ptr(grad), ptr(state.m), ptr(state.v), ptr(state.t), ptr(state.calls), ptr(state.stall), ptr(state.bad),
              ptr(state.best_step), ptr(state.active), ptr(state.best_loss), ptr(state.best_x), ptr(loss), int(loss.shape[1]),
              ptr(silh_loss), Ns, float(silh_weight), ptr(col_scale), ptr(history) if H else None, H, B, P, float(lr), float(beta1),
              float(beta2), float(eps), float(grad_scale), MODES.index(mode), int(patience))
    lib = _lib.load()
    if grouped:
        check(lib.smplr_fit_step_group(*common, *_prior_args(prior, w, num_cam), G, ptr(tie), ptr(smooth), stream()),
              "smplr_fit_step_group")
    elif prior is not None:
        check(lib.smplr_fit_step_prior(*common, *_prior_args(prior, w, num_cam), stream()), "smplr_fit_step_prior")
    else:
        check(lib.smplr_fit_step(*common, stream()), "smplr_fit_step")
    return state


@_lib.on_device
def lbfgs_step(state, grad, loss, silh_loss=None, silh_weight=1.0, col_scale=None, history=None, lr=1.0, c1=1e-4, max_ls=10,
               tol_grad=0.0, grad_scale=1.0, patience=0, prior=None, prior_weights=None, num_cam=4):
    """One smplr_lbfgs_step launch on `state` (an `LbfgsState`, in place; see the module's semantics): ONE function evaluation
    of every row's own L-BFGS with a backtracking Armijo line search.  grad, loss, silh_loss, col_scale, history, grad_scale,
    patience, prior, prior_weights and num_cam as `fit_step` takes them (with a prior the launch is smplr_lbfgs_step_prior);
    HIP tensors only."""
    rc = _lib.require_cuda
    if not isinstance(state, LbfgsState):
        raise TypeError("state must be an LbfgsState")
    if not state.x.is_contiguous():
        raise RuntimeError("x must be contiguous (it is updated in place)")
    x = rc(state.x, "x")
    B, P = int(x.shape[0]), int(x.shape[1])
    same = {"grad": grad, "best_x": state.best_x, "x0": state.x0, "g0": state.g0, "d": state.d}
    ints = {"t": state.t, "calls": state.calls, "stall": state.stall, "bad": state.bad, "best_step": state.best_step,
            "ls": state.ls, "pairs": state.pairs}
    flts = {"best_loss": state.best_loss, "f0": state.f0, "gd": state.gd, "alpha": state.alpha}
    byts = {"active": state.active, "phase": state.phase}
    for name, a in same.items():
        if tuple(a.shape) != (B, P) or not a.is_contiguous():
            raise RuntimeError("%s must be a contiguous (%d, %d) tensor, got %s" % (name, B, P, tuple(a.shape)))
        rc(a, name)
    for group, dt in ((ints, torch.int32), (flts, torch.float32), (byts, torch.uint8)):
        for name, a in group.items():
            if tuple(a.shape) != (B,):
                raise RuntimeError("%s must be (%d,), got %s" % (name, B, tuple(a.shape)))
            rc(a, name, dt)
    M = int(state.S.shape[1]) if state.S.dim() == 3 else -1
    if not 1 <= M <= MAX_MEMORY:
        raise RuntimeError("S must be (B, M, P) with 1 <= M <= %d, got %s" % (MAX_MEMORY, tuple(state.S.shape)))
    mem = {"S": state.S, "Y": state.Y}
    for name, a in mem.items():
        if tuple(a.shape) != (B, M, P) or not a.is_contiguous():
            raise RuntimeError("%s must be a contiguous (%d, %d, %d) tensor, got %s" % (name, B, M, P, tuple(a.shape)))
        rc(a, name)
    if loss.dim() != 2 or loss.shape[0] != B or loss.shape[1] < 1 or not loss.is_contiguous():
        raise RuntimeError("loss must be a contiguous (%d, N) tensor, got %s" % (B, tuple(loss.shape)))
    rc(loss, "loss")
    Ns = 0
    if silh_loss is not None:
        if silh_loss.dim() != 2 or silh_loss.shape[0] != B or silh_loss.shape[1] < 1 or not silh_loss.is_contiguous():
            raise RuntimeError("silh_loss must be a contiguous (%d, Ns) tensor, got %s" % (B, tuple(silh_loss.shape)))
        rc(silh_loss, "silh_loss")
        Ns = int(silh_loss.shape[1])
    if col_scale is None:
        col_scale = torch.ones(P, dtype=torch.float32, device=x.device)
    if tuple(col_scale.shape) != (P,) or not col_scale.is_contiguous():
        raise RuntimeError("col_scale must be a contiguous (%d,) tensor, got %s" % (P, tuple(col_scale.shape)))
    rc(col_scale, "col_scale")
    H = 0
    if history is not None:
        if history.dim() != 2 or history.shape[1] != B or not history.is_contiguous():
            raise RuntimeError("history must be a contiguous (H, %d) tensor, got %s" % (B, tuple(history.shape)))
        rc(history, "history")
        H = int(history.shape[0])
    for name, a in (list(same.items()) + list(ints.items()) + list(flts.items()) + list(byts.items()) + list(mem.items()) +
                    [("loss", loss), ("silh_loss", silh_loss), ("col_scale", col_scale), ("history", history)]):
        if a is not None and a.device != x.device:
            raise RuntimeError("%s lives on %s, x on %s" % (name, a.device, x.device))
    w = None
    if prior is not None:
        prior, w = _prior_operands(prior, prior_weights, x)
    elif prior_weights is not None:
        raise ValueError("prior_weights without a prior")
    common = (ptr(x), ptr(grad), ptr(state.x0), ptr(state.g0), ptr(state.d), ptr(state.S), ptr(state.Y), ptr(state.f0), ptr(state.gd),
              ptr(state.alpha), ptr(state.ls), ptr(state.pairs), ptr(state.phase), ptr(state.t), ptr(state.calls), ptr(state.stall),
              ptr(state.bad), ptr(state.best_step), ptr(state.active), ptr(state.best_loss), ptr(state.best_x), ptr(loss),
              int(loss.shape[1]), ptr(silh_loss), Ns, float(silh_weight), ptr(col_scale), ptr(history) if H else None, H, B, P, M,
              float(lr), float(c1), int(max_ls), float(tol_grad), float(grad_scale), int(patience))
    lib = _lib.load()
    if prior is not None:
        check(lib.smplr_lbfgs_step_prior(*common, *_prior_args(prior, w, num_cam), stream()), "smplr_lbfgs_step_prior")
    else:
        check(lib.smplr_lbfgs_step(*common, stream()), "smplr_lbfgs_step")
    return state


@dataclass
class FitResult:
    """x (B, P): the best iterate of each row; loss (B,): its loss; step (B,) int32: the update count it was reached at;
    final_x (B, P): where the row stood at the end; nonfinite (B,) int32: calls that met a non-finite loss or gradient (and
    changed nothing); active (B,) bool: rows the patience rule had not stopped; history (steps run, B) fp32 loss trace or
    None; steps: iterations run (fewer than asked for when `check_every` found every row stopped); state: the whole
    `FitState` the loop ended with (moments and counters included); group_size: rows per group - with groups, loss, step and
    active are the group's, repeated on each of its rows (history holds every row's own loss).  `optimizer` (a property, read
    off the state): "adam", or "lbfgs" - then state is an `LbfgsState`, steps are evaluations, step counts accepted steps and
    final_x is the last ACCEPTED iterate state.x0 (state.x may be a trial point)."""
    x: torch.Tensor
    loss: torch.Tensor
    step: torch.Tensor
    final_x: torch.Tensor
    nonfinite: torch.Tensor
    active: torch.Tensor
    history: Optional[torch.Tensor]
    steps: int
    state: Optional[FitState] = None
    group_size: int = 1

    @property
    def optimizer(self):
        return "lbfgs" if isinstance(self.state, LbfgsState) else "adam"


def _stage_prior_weights(prior, prior_weights, stage_list):
    """`fit`'s prior_weights (None, one triple, or a list of one triple per stage) -> one (3,) CPU tensor per stage; None
    without a prior."""
    if prior is None:
        if prior_weights is not None:
            raise ValueError("prior_weights without a prior")
        return None
    pw = (1.0, 1.0, 1.0) if prior_weights is None else prior_weights
    per_stage = isinstance(pw, (list, tuple)) and len(pw) > 0 and all(np.ndim(w) == 1 for w in pw)
    if per_stage and len(pw) != len(stage_list):
        raise ValueError("prior_weights lists %d triples for %d stages" % (len(pw), len(stage_list)))
    return [check_prior_weights(w) for w in (pw if per_stage else [pw] * len(stage_list))]


def _stage_weights(weight, stage_list, name):
    """A scalar weight of `fit` - pen_weight, kp_weight, lap_weight, edge_weight, offset_weight - (None: 1, one float, or a
    list of one float per stage) -> one float per stage; `name` is the argument's, for the messages."""
    pw = 1.0 if weight is None else weight
    per_stage = isinstance(pw, (list, tuple))
    if per_stage and len(pw) != len(stage_list):
        raise ValueError("%s lists %d weights for %d stages" % (name, len(pw), len(stage_list)))
    out = [float(w) for w in (pw if per_stage else [pw] * len(stage_list))]
    if any(not math.isfinite(w) or w < 0 or w > float(np.finfo(np.float32).max) for w in out):
        raise ValueError("%s must be finite and >= 0, got %r" % (name, weight))
    return out


# the loop's arguments: what every `fit` of `_Fitter`'s family hands on to `_Fitter._fit` by name
_LOOP_ARGS = ("steps", "lr", "mode", "stages", "patience", "grad_scale", "graph", "check_every", "history", "beta1", "beta2", "eps",
             "graph_steps", "prior", "prior_weights", "group_size", "tie", "smooth")


def _fit_args(given, lbfgs=False):
    """What every `fit` starts with, on its own locals(): the mode check - so it is the first error a bad call raises - and
    the loop's arguments among them, by name.  lbfgs: the loop also takes mode = "lbfgs" or an `Lbfgs` record."""
    check_mode(given["mode"], lbfgs)
    return {k: given[k] for k in _LOOP_ARGS if k in given}


def _capture(body, scratch, real, k, dev):
    """body(*scratch) 3 times on a side stream (the warm-up, on scratch state), a synchronise, then body(*real) k times
    captured into one graph -> its replay.  The capture runs nothing: the real state is still the start's."""
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            body(*scratch)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g_ = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g_):
        for _ in range(k):
            body(*real)
    return g_.replay


def _run_stages(stage_list, set_stage, one, replay=None, G=1, check_every=0, any_active=None):
    """The stages one after the other -> iterations run.  set_stage(i) at every stage boundary, outside any captured graph
    (it rewrites the device tensors a graph reads: column scales and weights); then the stage's iterations, replay() - G of
    them - while at least G are left, else one().  check_every = k > 0: any_active() is read whenever the count passes a
    multiple of k, and the loop ends when it says no."""
    done, stopped = 0, False
    for si, (n, _) in enumerate(stage_list):
        set_stage(si)
        left = n
        while left > 0 and not stopped:
            if replay is not None and left >= G:
                replay()
                k = G
            else:
                one()
                k = 1
            left -= k
            if check_every > 0 and (done + k) // check_every > done // check_every:
                stopped = not any_active()
            done += k
        if stopped:
            break
    return done


class _SideTerm:
    """A weighted side term w mean_n(e[b, :]) of a fitter, built by its constructor: `name` of its weight argument (the word
    in its messages too), its column count n, energy(x, verts, joints, data) -> e (B, n) differentiable, on what the forward
    produced, and check(data, B, dev) -> the term's own data on the device (None: the term has none).  `begin` makes the
    copy one fit works with: w (1,) and cot (B, n) device tensors - the weight in the loss and the cotangent w / n of e, so a
    captured graph follows both - one weight per stage, and the data.  width(data) -> n, for a term whose column count is its
    data's (then n is None until `begin`)."""

    skip_zero = False          # True: a fit (or `losses`) whose weights for the term are 0 in every stage runs without it

    def __init__(self, name, n, energy, check=None, width=None):
        self.name, self.n, self.energy, self.check, self.width = name, None if n is None else int(n), energy, check, width

    @staticmethod
    def live(sides):
        """[(term, its weight per stage, data)] without the `skip_zero` terms whose weights are all 0: those are not
        evaluated at all, so the fit takes the launches - and gives the bits - of a fitter built without them."""
        return [(t, ws, d) for t, ws, d in sides if not (t.skip_zero and not any(ws))]

    def begin(self, stages, B, dev, data=None):
        """-> the term for one fit over B rows on dev, at its first stage's weight; stages: `_stage_weights`' list."""
        t = _SideTerm(self.name, self.n, self.energy)
        t.stages, t.data = stages, self.check(data, B, dev) if self.check is not None else None
        if self.width is not None:
            t.n = int(self.width(t.data))
        t.w = torch.zeros(1, dtype=torch.float32, device=dev)
        t.cot = torch.zeros((B, t.n), dtype=torch.float32, device=dev)
        t.set(0)
        return t

    def set(self, stage):
        """The weight of a stage into the device scalar and the cotangent (outside any captured graph)."""
        self.w.fill_(self.stages[stage])
        self.cot.fill_(self.stages[stage] / self.n)

    def join(self, e, loss):
        """-> loss.detach() + w mean_n(e) on every column: three stock launches (mean, product, sum)."""
        return loss.detach() + (self.w * e.detach().mean(1))[:, None]


class _Fitter:
    """What `ParamFitter`, `ScanFitter`, `KeypointFitter` and `SurfaceFitter` share: the iteration, `losses`, the loop.  A fitter adds its data
    term - `_forward(x, data)` and `_cotangents(B, dev, data)` - and sets num_cam and P."""
    pen_topo = None            # a render.MeshTopology when the fitter was built with `penetration`
    pen_collide = None         # its part-pair table (None: `penetration.part_collision_table(topo, 1)`)
    kp_spec = None             # a keypoints.KeypointSpec when the fitter was built with `keypoints`
    kp_sigma = None            # the robust function's sigma in pixels (None: rho(s) = s)
    ld_spec = None             # a labeldist.LabelDistanceSpec when the fitter was built with `label_distance`
    sc_topo = None             # a render.MeshTopology when the fitter was built with `surface`
    sc_sigma = None            # the robust function's sigma, in the targets' unit (None: rho(s) = s)
    sc_dims = (2, 3)           # the target dimensions the fitter takes (`ScanFitter`: 3 only)
    _sc_options = (None, None) # surface, sc_sigma of the constructor (`with_surface` sets them; a plain fitter has no term)
    _sc_call = (None, None)    # surface=, sc_weight= of the `fit` / `losses` call in progress (`with_surface`)
    _pen = _kp = _ld = _sc = None   # their `_SideTerm`s; a fitter's side terms come in this order: penetration, keypoints,
                                    # label distance, then surface correspondences

    def _layer_init(self, smpl_path, four_columns):
        """A fitter over an `SMPLLayer` (given, or built from a path or a model): layer, num_cam - which must be 4, else a
        ValueError of `four_columns` - and P."""
        from .keras_smpl.batch_smpl import SMPLLayer
        self.layer = smpl_path if isinstance(smpl_path, SMPLLayer) else SMPLLayer(smpl_path)
        self.num_cam = self.layer.num_cam
        if self.num_cam != 4:
            raise ValueError(four_columns)
        self.P = self.num_cam + 82

    def _pen_init(self, penetration, model, collide=None):
        """`penetration` of a fitter's constructor: None / False (no term), True (the faces of `model`) or a MeshTopology."""
        if penetration is None or penetration is False:
            return
        from .penetration import check_collide, self_penetration
        from .render import MeshTopology
        if penetration is True:
            if getattr(model, "faces", None) is None:
                raise ValueError("this SMPL model carries no faces: pass penetration=MeshTopology(faces, num_verts)")
            penetration = MeshTopology(model.faces, model.num_verts)
        if not all(hasattr(penetration, a) for a in ("faces", "vf_off", "vf_face", "vertex_part", "num_verts", "on")):
            raise TypeError("penetration must be True or a render.MeshTopology")
        if penetration.num_verts != model.num_verts:
            raise ValueError("the topology has %d vertices, the model %d" % (penetration.num_verts, model.num_verts))
        self.pen_topo, self.pen_collide = penetration, check_collide(collide, penetration)
        self._pen = _SideTerm("pen_weight", penetration.num_verts,
                              lambda x, verts, joints, data: self_penetration(verts, self.pen_topo, self.pen_collide))

    def _kp_init(self, keypoints, model, sigma=None):
        """`keypoints` of a fitter's constructor: None (no term) or a KeypointSpec over the model's vertices.  The term is
        `keypoint_energy` of the iteration's vertices (and posed joints) under cam = x[:, :4]."""
        from .keypoints import KeypointSpec, check_sigma, keypoint_energy
        check_sigma(sigma)
        if keypoints is None:
            if sigma is not None:
                raise ValueError("kp_sigma goes with a fitter built with keypoints=...")
            return
        if not isinstance(keypoints, KeypointSpec):
            raise TypeError("keypoints must be a keypoints.KeypointSpec")
        if keypoints.num_verts != model.num_verts:
            raise ValueError("the keypoint spec has %d vertices, the model %d" % (keypoints.num_verts, model.num_verts))
        if self.num_cam != 4:
            raise ValueError("the keypoint term projects with four camera columns")
        self.kp_spec, self.kp_sigma = keypoints, sigma

        def energy(x, verts, joints, data):
            return keypoint_energy(verts, x[:, :4], self.kp_spec, data[0], data[1], self.kp_sigma,
                                   joints if self.kp_spec.with_joints else None)
        self._kp = _SideTerm("kp_weight", keypoints.K, energy, self._kp_data)

    def _kp_data(self, keypoints, B, dev):
        """`fit`'s / `losses`' keypoints=(target (B, K, 2), conf (B, K)) -> both as fp32 device tensors."""
        if not isinstance(keypoints, (tuple, list)) or len(keypoints) != 2:
            raise ValueError("keypoints must be (target (B, K, 2), conf (B, K))")
        K = self.kp_spec.K
        target, conf = (torch.as_tensor(a) for a in keypoints)
        if tuple(target.shape) != (B, K, 2) or tuple(conf.shape) != (B, K):
            raise ValueError("keypoints must be (target (%d, %d, 2), conf (%d, %d)), got %s and %s"
                             % (B, K, B, K, tuple(target.shape), tuple(conf.shape)))
        return (target.detach().to(device=dev, dtype=torch.float32).contiguous(),
                conf.detach().to(device=dev, dtype=torch.float32).contiguous())

    def _sc_init(self, surface, model, sigma=None):
        """`surface` of a fitter's constructor: None (no term) or a MeshTopology over the model's vertices.  The term is
        `surface.surface_energy` of the iteration's vertices against the fit's `SurfaceTargets`: under cam = x[:, :4] with
        image targets (D = 2), in the vertices' own frame with 3D targets (cam is not used).  Its column count is the data's N:
        the term is sc_weight mean_N(e), padding included.  With sc_weight = 0 in every stage the term is left out of the fit
        altogether (`_SideTerm.live`): a cotangent on the vertices, even a zero one, would send the decoder's backward down
        its per-vertex skinning path, whose sums round in another order than the record-driven one."""
        from .keypoints import check_sigma
        from .surface import surface_energy
        check_sigma(sigma)
        if surface is None:
            if sigma is not None:
                raise ValueError("sc_sigma goes with a fitter built with surface=...")
            return
        if not all(hasattr(surface, a) for a in ("faces", "num_verts", "num_faces", "on")):
            raise TypeError("surface must be a render.MeshTopology")
        if surface.num_verts != model.num_verts:
            raise ValueError("the surface topology has %d vertices, the model %d" % (surface.num_verts, model.num_verts))
        if self.num_cam != 4:
            raise ValueError("the surface term projects with four camera columns")
        self.sc_topo, self.sc_sigma = surface, sigma

        def energy(x, verts, joints, data):
            return surface_energy(verts, x[:, :4] if data.D == 2 else None, data, self.sc_sigma)
        self._sc = _SideTerm("sc_weight", None, energy, self._sc_data, lambda data: data.N)
        self._sc.skip_zero = True

    def _sc_data(self, surface, B, dev):
        """`fit`'s / `losses`' surface=SurfaceTargets: B rows on the fit's device, over the fitter's topology."""
        from .surface import SurfaceTargets
        if not isinstance(surface, SurfaceTargets):
            raise TypeError("surface must be a surface.SurfaceTargets")
        if surface.B != B:
            raise ValueError("the surface targets have %d rows, the fit %d" % (surface.B, B))
        if surface.D not in self.sc_dims:
            raise ValueError("this fitter takes surface targets with D in %s, got D = %d" % (self.sc_dims, surface.D))
        if surface.topo is not self.sc_topo and not np.array_equal(surface.topo.faces, self.sc_topo.faces):
            raise ValueError("the surface targets were built over another topology than the fitter's")
        if torch.device(surface.device) != torch.device(dev):
            raise RuntimeError("the surface targets live on %s, the fit on %s" % (surface.device, dev))
        return surface

    def _check_sides(self, pen_weight=None, keypoints=None, kp_weight=None, ld_weight=None, labels=None):
        """The pairing rules, before anything touches a device: a weight only with its term, keypoint or surface data only
        with a spec and a spec only with data -> [(term, its weight argument, its data)] of the terms the fitter has, in their
        order.  The label-distance term's data are the fit's own `labels`; the surface term's data and weight are the
        call's `surface=` and `sc_weight=`, which `with_surface`'s `fit` and `losses` hold in `_sc_call` for the call."""
        surface, sc_weight = self._sc_call
        if self._pen is None and pen_weight is not None:
            raise ValueError("pen_weight goes with a fitter built with penetration=...")
        if self._kp is None:
            if keypoints is not None or kp_weight is not None:
                raise ValueError("keypoints and kp_weight go with a fitter built with keypoints=...")
        elif keypoints is None:
            raise ValueError("this fitter was built with keypoints=...: pass keypoints=(target, conf)")
        if self._ld is None and ld_weight is not None:
            raise ValueError("ld_weight goes with a LabelDistanceFitter built with label_distance=...")
        if self._sc is None:
            if surface is not None or sc_weight is not None:
                raise ValueError("surface and sc_weight go with a fitter built with surface=...")
        elif surface is None:
            raise ValueError("this fitter was built with surface=...: pass surface=SurfaceTargets")
        return [(t, w, d) for t, w, d in ((self._pen, pen_weight, None), (self._kp, kp_weight, keypoints),
                                          (self._ld, ld_weight, labels), (self._sc, sc_weight, surface)) if t is not None]

    def _initial(self, B, init, device, default):
        """`initial`: a (B, P) tensor as it is, anything else from default(); then the move to the device."""
        if isinstance(init, torch.Tensor):
            if tuple(init.shape) != (B, self.P):
                raise ValueError("init must be (%d, %d), got %s" % (B, self.P, tuple(init.shape)))
            x0 = init.detach().to(torch.float32)
        else:
            x0 = default()
        return x0.to(device) if device is not None else x0

    def _prior_kw(self, prior, weights, dev):
        """fit_step's prior arguments: the prior on the device and a (3,) device tensor of weights; {} without a prior."""
        if prior is None:
            if weights is not None:
                raise ValueError("prior_weights without a prior")
            return {}
        if not isinstance(prior, PosePrior):
            raise TypeError("prior must be a PosePrior")
        return dict(prior=prior.to(dev), prior_weights=check_prior_weights((1.0, 1.0, 1.0) if weights is None else weights).to(dev),
                    num_cam=self.num_cam)

    def _compose(self, x, data, sides):
        """The forward of one iteration, and of `losses`: the fitter's `_forward(x, data)` -> (its data terms, the second
        term's weight, verts, posed joints or None), then the side terms on those.  -> (terms, loss, silh_loss, silh_weight):
        every term in the order `autograd.grad` takes them, and what `fit_step` gets.  The bits depend on these rules:
          - terms: the data terms first - [seg_loss, silh_loss?] of `ParamFitter`, [p2m, m2p] or the one direction present of
            `ScanFitter` (p2m scaled by N / counts inside `terms()`), [e] of `KeypointFitter` or `SurfaceFitter` - then penetration,
            keypoints, label distance and surface correspondences: autograd accumulates into x in that order.
          - loss: the first data term detached, then + w_pen mean_V, then + w_kp mean_K, + w_ld mean and + w_sc mean_N, each onto every column; silh_loss:
            the second data term where there is one (with `ScanFitter` the m2p terms, silh_weight = m2p_weight, only when both
            directions are on; with one direction the weight is 1.0).  Both contiguous."""
        terms, silh_weight, verts, joints = self._forward(x, data)
        loss = terms[0].detach()
        silh_loss = terms[1].detach().contiguous() if len(terms) == 2 else None
        for s in sides:
            e = s.energy(x, verts, joints, s.data)
            terms, loss = terms + [e], s.join(e, loss)
        return terms, loss.contiguous(), silh_loss, silh_weight

    def _iteration(self, state, data, sides, cots, cs, hist, kw):
        """One iteration on `state`: `_compose` on x, ONE `torch.autograd.grad` over all terms with their constant
        cotangents cots (the data terms', then each side term's `cot`, in `_compose`'s order), one `fit_step` - or, on an
        `LbfgsState`, one `lbfgs_step` in its place (kw: that function's)."""
        x = state.x.detach().requires_grad_(True)                 # (shares x's memory: the kernel updates it in place)
        terms, loss, silh_loss, silh_weight = self._compose(x, data, sides)
        (g,) = torch.autograd.grad(terms, [x], grad_outputs=cots)
        step = lbfgs_step if isinstance(state, LbfgsState) else fit_step
        step(state, g.contiguous(), loss, silh_loss, silh_weight, cs, hist, **kw)

    def _losses(self, x, data, prior, prior_weights, sides):
        """`losses` behind a fitter's own look at its inputs: `_compose` - the forward `fit` iterates - without a gradient,
        reduced to (B,) by the kernel of the loop: a call with a zero gradient on a scratch state that records one row of
        history.  sides: `_check_sides`' list; each term joins at its weight (None: 1)."""
        x = _lib.require_cuda(x.detach(), "x")
        with torch.no_grad(), torch.cuda.device(x.device):
            B = int(x.shape[0])
            sides = [t.begin(ws, B, x.device, d) for t, ws, d in
                     _SideTerm.live([(t, _stage_weights(w, [None], t.name), d) for t, w, d in sides])]
            _, loss, silh_loss, silh_weight = self._compose(x, data, sides)
            hist = torch.empty((1, B), dtype=torch.float32, device=x.device)
            fit_step(FitState.new(x), torch.zeros_like(x), loss, silh_loss, silh_weight, None, hist,
                     **self._prior_kw(prior, prior_weights, x.device))
            return hist[0]

    def _fit(self, B, dev, start, check_data, sides, *, steps, lr, mode, stages, patience, grad_scale, graph, check_every, history,
             beta1, beta2, eps, graph_steps, prior, prior_weights, group_size, tie, smooth):
        """The rest of `fit` behind a fitter's own look at its inputs (the `_LOOP_ARGS` by name; B rows on device dev): the
        checks of groups, stages and weights, the start from start() (tied columns set to their group's mean), the state,
        the stages with their column scales, prior weights and side-term weights, graph capture and replay, the stop on
        `check_every`.  check_data() -> the fitter's checked data, called between the groups' checks and the stages':
        whatever the fitter checks of its data there; sides: `_check_sides`' list."""
        P = self.P
        opt = check_mode(mode)                                    # an `Lbfgs` record, or None: Adam
        grp = check_group(B, group_size)
        grouped = grp != 1 or smooth is not None
        if opt is not None and grouped:
            raise ValueError("mode \"lbfgs\" fits every row on its own: group_size > 1, tie and smooth need Adam's modes")
        tie_m = check_tie(tie, P, self.num_cam) if grouped else None
        smooth_w = check_smooth(smooth, P) if smooth is not None else None
        data = check_data()
        stage_list = check_stages(stages, P, steps)
        stage_w = _stage_prior_weights(prior, prior_weights, stage_list)
        sides = _SideTerm.live([(t, _stage_weights(w, stage_list, t.name), d) for t, w, d in sides])
        if opt is None:
            kw = dict(lr=float(lr), beta1=float(beta1), beta2=float(beta2), eps=float(eps), grad_scale=float(grad_scale),
                      mode=mode, patience=int(patience))
        else:
            kw = dict(lr=float(opt.lr), c1=float(opt.c1), max_ls=int(opt.max_ls), tol_grad=float(opt.tol_grad),
                      grad_scale=float(grad_scale), patience=int(patience))
        total = sum(n for n, _ in stage_list)
        G = max(1, int(graph_steps))
        with torch.cuda.device(dev):
            x0 = start()
            if grouped:
                tie_m = tie_m.to(dev)
                if grp > 1:                                           # a group starts with one value in every tied column
                    mean = x0.reshape(B // grp, grp, P).mean(1, keepdim=True).expand(-1, grp, -1).reshape(B, P)
                    x0 = torch.where(tie_m.bool(), mean, x0)
            state = FitState.new(x0) if opt is None else LbfgsState.new(x0, opt.memory)
            hist = torch.full((total, B), float("nan"), dtype=torch.float32, device=dev) if history and total else None
            cs = torch.ones(P, dtype=torch.float32, device=dev)
            scales = [c.to(dev) for _, c in stage_list]
            if grouped:
                kw.update(group_size=grp, tie=tie_m, smooth=smooth_w.to(dev) if smooth_w is not None else None)
            if prior is not None:
                kw.update(self._prior_kw(prior, stage_w[0], dev))     # (the (3,) tensor is rewritten at each stage boundary)
                stage_w = [w.to(dev) for w in stage_w]
            sides = [t.begin(ws, B, dev, d) for t, ws, d in sides]
            cots = self._cotangents(B, dev, data) + [s.cot for s in sides]

            def one(st, h):
                self._iteration(st, data, sides, cots, cs, h, kw)

            def set_stage(si):
                cs.copy_(scales[si])
                if prior is not None:
                    kw["prior_weights"].copy_(stage_w[si])
                for s in sides:
                    s.set(si)
                if opt is not None:                                   # (the objective changes: the memory and f0 are void)
                    state.restart()
            replay = None
            if graph and B > 0 and any(n >= G for n, _ in stage_list):
                replay = _capture(one, (state.clone(), None), (state, hist), G, dev)
            done = _run_stages(stage_list, set_stage, lambda: one(state, hist), replay, G, int(check_every) if B > 0 else 0,
                               lambda: bool(state.active.any()))
            torch.cuda.synchronize()
        return FitResult(x=state.best_x, loss=state.best_loss, step=state.best_step, final_x=state.x if opt is None else state.x0,
                         nonfinite=state.bad,
                         active=state.active.bool(), history=hist[:done] if hist is not None else None, steps=done,
                         state=state, group_size=grp)


class ParamFitter(_Fitter):
    """Owns an `SMPLDecoder(outputs=(), loss=softmax_focal_loss(gamma, weight_classes)[, silh_loss=...])` and fits its
    input to label maps.  The defaults are those of decoder_loss_debugging.py:117-118: focal loss with gamma = 5, no class
    weights; `fit`'s are Keras' Adam (lr 1e-3, eps 1e-7)."""
    _ld_options = (None, None, 0.5, ("m2i", "i2m"))    # label_distance, ld_sigma, ld_slack, ld_directions: no third side term

    def __init__(self, smpl_path=None, img_wh=48, gamma=5.0, weight_classes=False, with_silhouette=False, silh_wh=None,
                 silh_weight=1.0, vertex_sampling=None, deterministic=False, penetration=None, collide=None, keypoints=None,
                 kp_sigma=None):
        from .decoder import SMPLDecoder
        from .focal_loss import softmax_focal_loss
        self.img_wh = int(img_wh)
        self.with_silhouette = bool(with_silhouette)
        self.silh_weight = float(silh_weight)
        with_pen = penetration is not None and penetration is not False
        if with_pen and vertex_sampling not in (None, 1):
            raise ValueError("penetration needs every vertex: vertex_sampling must be None or 1, got %r" % (vertex_sampling,))
        if keypoints is not None and vertex_sampling not in (None, 1):
            raise ValueError("keypoints need every vertex: vertex_sampling must be None or 1, got %r" % (vertex_sampling,))
        label_distance, ld_sigma, ld_slack, ld_directions = self._ld_options     # (`LabelDistanceFitter` sets them)
        with_ld = label_distance is not None and label_distance is not False
        if with_ld and vertex_sampling not in (None, 1):
            raise ValueError("label_distance needs every vertex: vertex_sampling must be None or 1, got %r" % (vertex_sampling,))
        surface, sc_sigma = self._sc_options                                      # (`with_surface` sets them)
        if surface is not None and vertex_sampling not in (None, 1):
            raise ValueError("surface needs every vertex: vertex_sampling must be None or 1, got %r" % (vertex_sampling,))
        outputs = ("verts",) if with_pen or keypoints is not None or with_ld or surface is not None else ()
        if with_ld and isinstance(label_distance, str) and label_distance == "visible":
            outputs += ("mask",)
        # (streams=1: one chain of launches, so a captured graph has no parallel branches)
        self.decoder = SMPLDecoder(smpl_path, img_wh=self.img_wh, vertex_sampling=vertex_sampling,
                                   with_silhouette=self.with_silhouette, silh_wh=silh_wh, streams=1,
                                   deterministic=deterministic, outputs=outputs,
                                   loss=softmax_focal_loss(gamma, weight_classes),
                                   silh_loss=softmax_focal_loss(0.0, False) if self.with_silhouette else None)
        self._pen_init(penetration, self.decoder._model, collide)
        self.num_cam = self.decoder.num_cam
        self.P = self.num_cam + 82
        self.silh_wh = self.decoder.silh_wh
        self._kp_init(keypoints, self.decoder._model, kp_sigma)
        self._ld_init(label_distance, ld_sigma, ld_slack, ld_directions)
        self._sc_init(surface, self.decoder._model, sc_sigma)

    def _ld_init(self, label_distance, sigma, slack, directions):
        """`label_distance` of `LabelDistanceFitter`'s constructor: None / False (no term), True (`LabelDistanceSpec.from_parts` of the decoder's
        part table), "visible" (that, with vweight = (the decoder's mask == 1), detached) or a LabelDistanceSpec.  The term
        is `labeldist.label_distance` of the iteration's vertices under cam = x[:, :4] against the fit's own labels: e =
        the directions in use side by side, (B, V + W W) for both."""
        from .labeldist import LabelDistanceSpec, LabelTargets, check_directions, check_slack, label_distance as ld_energy
        from .keypoints import check_sigma
        from .smpl_model import load_part_tables
        check_sigma(sigma)
        if label_distance is None or label_distance is False:
            if sigma is not None:
                raise ValueError("ld_sigma goes with a fitter built with label_distance=...")
            return
        V, W = self.decoder._model.num_verts, self.img_wh
        visible = isinstance(label_distance, str) and label_distance == "visible"
        if label_distance is True or visible:
            label_distance = LabelDistanceSpec.from_parts(load_part_tables(1), V)
        if not isinstance(label_distance, LabelDistanceSpec):
            raise TypeError("label_distance must be True, \"visible\" or a labeldist.LabelDistanceSpec")
        if label_distance.num_verts != V:
            raise ValueError("the label-distance spec has %d vertices, the model %d" % (label_distance.num_verts, V))
        if self.num_cam != 4:
            raise ValueError("the label-distance term projects with four camera columns")
        dirs, slack = check_directions(directions), check_slack(slack)
        self.ld_spec, self.ld_sigma, self.ld_slack, self.ld_directions, self.ld_visible = label_distance, sigma, slack, dirs, visible
        n = (V if "m2i" in dirs else 0) + (W * W if "i2m" in dirs else 0)

        def energy(x, verts, joints, data):
            targets, mask = data
            e = ld_energy(verts, x[:, :4], self.ld_spec, targets, (mask[0] == 1).to(torch.float32) if visible else None,
                          self.ld_sigma, self.ld_slack, dirs)
            e = e if isinstance(e, tuple) else (e,)
            return torch.cat([t.reshape(t.shape[0], -1) for t in e], 1)

        def check(labels, B, dev):
            # (the prep launch: once per fit, outside any captured graph; mask: the cell `_forward` fills every iteration)
            return LabelTargets(self._labels(labels, B, W, "labels"), self.ld_spec.num_classes), self._ld_mask
        self._ld_mask = [None]
        self._ld = _SideTerm("ld_weight", n, energy, check)

    # ---- inputs -------------------------------------------------------------------------------------------------------
    def initial(self, B, init=None, generator=None, device=None):
        """(B, P) float32 start: None = `smpl_model.mean86(img_wh)` per row; "reference" = that plus Keras' Embedding
        initialiser uniform(-0.05, 0.05) drawn from `generator` (decoder_loss_debugging.py:75-77); a (B, P) tensor as it is
        (an encoder's prediction)."""
        from .smpl_model import mean86

        def default():
            if self.num_cam != 4:
                raise ValueError("the mean parameters have 4 camera columns")
            mean = torch.as_tensor(mean86(self.img_wh), dtype=torch.float32).repeat(B, 1)
            if init is None:
                return mean
            if init == "reference":
                return mean + (torch.rand(B, self.P, generator=generator) * 0.1 - 0.05)
            raise ValueError("init must be None, 'reference' or a (B, %d) tensor, got %r" % (self.P, init))
        return self._initial(B, init, device, default)

    def _labels(self, labels, B, W, name):
        if not isinstance(labels, torch.Tensor) or labels.is_floating_point() or labels.numel() != B * W * W:
            raise ValueError("%s must be an integer map of %d x %d x %d entries" % (name, B, W, W))
        return _lib.require_cuda(labels.to(torch.int32).reshape(B, W, W), name, torch.int32)

    def _data(self, labels, silh_labels, B):
        """-> (labels (B, W, W), silh_labels (B, Ws, Ws) or None) int32 on the device; silh_labels go with the silhouette."""
        labels = self._labels(labels, B, self.img_wh, "labels")
        if (silh_labels is not None) != self.with_silhouette:
            raise ValueError("silh_labels go with ParamFitter(with_silhouette=True), and only with it")
        return labels, self._labels(silh_labels, B, self.silh_wh, "silh_labels") if silh_labels is not None else None

    # ---- one iteration ------------------------------------------------------------------------------------------------
    def _forward(self, x, data):
        out = self.decoder(x, data[0], silh_labels=data[1])
        terms = [out["seg_loss"]] if data[1] is None else [out["seg_loss"], out["silh_loss"]]
        if self._ld is not None and self.ld_visible:
            self._ld_mask[0] = out["mask"].detach()
        return terms, self.silh_weight, out.get("verts"), out.get("J_transformed")

    def _cotangents(self, B, dev, data):
        N, Ns = self.img_wh * self.img_wh, self.silh_wh * self.silh_wh
        gout = torch.full((B, N), 1.0 / N, dtype=torch.float32, device=dev)
        return [gout] if data[1] is None else [gout, torch.full((B, Ns), self.silh_weight / Ns, dtype=torch.float32, device=dev)]

    def losses(self, x, labels, silh_labels=None, prior=None, prior_weights=None, pen_weight=None, keypoints=None,
               kp_weight=None):
        """Per-row loss (B,) fp32 of parameters x (B, P) against the labels: one gradient-free decoder forward reduced by
        the kernel of the loop (a call with a zero gradient on a scratch state), so the bits are those `fit` would record
        for x in its history.  With a prior its weighted energy E is part of the loss, as in `fit`; so is the
        self-penetration term of a fitter built with `penetration` (pen_weight None: 1) and the keypoint term of one built
        with `keypoints` (keypoints = (target, conf), kp_weight None: 1)."""
        return self._losses_maps(x, labels, silh_labels, prior, prior_weights, pen_weight, keypoints, kp_weight)

    def _losses_maps(self, x, labels, silh_labels=None, prior=None, prior_weights=None, pen_weight=None, keypoints=None,
                     kp_weight=None, ld_weight=None):
        """`losses`, with the weight of the label-distance term that only `LabelDistanceFitter.losses` takes."""
        sides = self._check_sides(pen_weight, keypoints, kp_weight, ld_weight, labels)
        return self._losses(x, self._data(labels, silh_labels, int(x.shape[0])), prior, prior_weights, sides)

    # ---- the loop -----------------------------------------------------------------------------------------------------
    def fit(self, labels, init=None, steps=1601, lr=1e-3, mode="keras", stages=None, silh_labels=None, patience=0,
            grad_scale=1.0, graph=False, check_every=0, history=False, beta1=0.9, beta2=0.999, eps=KERAS_EPS,
            graph_steps=4, generator=None, prior=None, prior_weights=None, group_size=1, tie=("shape",), smooth=None,
            pen_weight=None, keypoints=None, kp_weight=None):
        """labels (B, W, W) integer part maps on the HIP device -> FitResult.

        steps: iterations (decoder_loss_debugging.py:123 runs 1601), or stages = [(steps, column_scale), ...] run one after
        the other; silh_labels (B, Ws, Ws) with `with_silhouette=True`; patience: a row stops after that many calls in a row
        without a new best (0: never); grad_scale = 1 / B reproduces Keras' batch-mean loss (decoder_loss_debugging.py:125,
        batch_size = num_indices); graph=True replays `graph_steps` iterations per launch of one captured HIP graph;
        check_every = k > 0 reads `active.any()` every k iterations (the loop's only host synchronisation) and stops when
        no row is active; history=True records every call's loss per row; prior: a `PosePrior` whose energy joins every row's
        loss inside the same launch, with prior_weights = (w_pose, w_angle, w_shape) (None: ones) or a list of one triple
        per stage (SMPLify's annealing).

        mode: "keras" or "torch" - Adam's two forms - or "lbfgs" / an `Lbfgs(memory, c1, max_ls, tol_grad, lr)` record: per-row
        L-BFGS with a backtracking line search, one `lbfgs_step` launch per evaluation in `fit_step`'s place (the module's
        semantics).  Then steps and stage counts are evaluations, the record's lr is the first trial step (lr, beta1, beta2 and
        eps here are Adam's and ignored), every stage boundary restarts the searches, final_x is the last accepted iterate,
        and groups or smooth raise ValueError.

        group_size = G > 1: rows kG .. kG + G - 1 of labels are views or frames of ONE body (B a multiple of G).  tie: the
        column blocks that are one unknown per group - names among "cam", "global_rot", "pose", "shape", or a (P,) mask of
        0 / 1 (`tie_mask`); the start's tied columns are replaced by their mean over the group (also with init=prediction), so
        they are equal within a group and stay bit-equal.  smooth: (P,) weights (`smooth_weights`) of a first-difference
        penalty between consecutive rows of a group, for clips.  Still one launch per iteration after the decoder's backward,
        and graph=True replays as before (tie and smooth are static device tensors).  loss, step and active of the result are
        the group's, repeated per row.  With group_size = 1 and no smooth, tie has no effect.

        pen_weight (a fitter built with `penetration` only; None: 1): the weight of the self-penetration term
        pen_weight mean_V(e), one float or a list of one per stage.

        keypoints = (target (B, K, 2), conf (B, K)) and kp_weight (a fitter built with `keypoints` only; kp_weight None: 1):
        detected 2D joints in the decoder's pixel frame; the term kp_weight mean_K(e), e = `keypoints.keypoint_energy`, joins
        every column of the loss and the one `torch.autograd.grad` call, as the self-penetration term does."""
        return self._fit_maps(locals())

    def _fit_maps(self, given, ld_weight=None):
        """`fit` on its own arguments by name (`given`), with the weight of the label-distance term that only
        `LabelDistanceFitter.fit` takes."""
        loop = _fit_args(given, lbfgs=True)
        labels, init, generator, silh_labels = (given[k] for k in ("labels", "init", "generator", "silh_labels"))
        sides = self._check_sides(given["pen_weight"], given["keypoints"], given["kp_weight"], ld_weight, labels)
        if not isinstance(labels, torch.Tensor) or labels.dim() != 3:
            raise ValueError("labels must be a (B, W, W) integer tensor")
        B, dev = int(labels.shape[0]), labels.device
        return self._fit(B, dev, lambda: self.initial(B, init, generator, dev), lambda: self._data(labels, silh_labels, B), sides,
                         **loop)


class LabelDistanceFitter(ParamFitter):
    """`ParamFitter` with the label-distance term (labeldist.py) as a third side term, after penetration and keypoints: every
    vertex to the nearest pixel of its part beside every labelled pixel to the nearest vertex of its part, against the fit's
    own labels - the term that pulls from far away, where the focal loss of the soft scores says nothing.  A class of its
    own because `ParamFitter`'s constructor, `fit` and `losses` keep the signatures their callers rely on; every other
    argument of those three passes through by name.

    label_distance: True (`LabelDistanceSpec.from_parts` of the decoder's part table), "visible" (that, with vweight = (the
    decoder's mask == 1), detached, the decoder built with "mask" among its outputs), a LabelDistanceSpec, or None / False
    (no term: a plain `ParamFitter`).  ld_sigma (pixels; None: rho(s) = s), ld_slack (px^2) and ld_directions as
    `labeldist.label_distance` takes them.  vertex_sampling must be None or 1.
    fit(labels, ld_weight=None, ...) and losses(x, labels, ld_weight=None, ...): ld_weight (None: 1, one float, or one per
    stage) times mean(e) joins every column of the loss and the one `torch.autograd.grad` call through a cotangent
    ld_weight / n, n = V + W W for both directions, cam = x[:, :4].  The labels are sorted by class once per fit, before the
    loop: the prep launch stays outside any captured graph."""

    def __init__(self, smpl_path=None, label_distance=True, ld_sigma=None, ld_slack=0.5, ld_directions=("m2i", "i2m"),
                 **param_fitter):
        self._ld_options = (label_distance, ld_sigma, ld_slack, ld_directions)
        super().__init__(smpl_path, **param_fitter)

    def losses(self, x, labels, ld_weight=None, **losses_kw):
        return self._losses_maps(x, labels, ld_weight=ld_weight, **losses_kw)

    def fit(self, labels, ld_weight=None, **fit_kw):
        import inspect
        given = inspect.signature(ParamFitter.fit).bind(self, labels, **fit_kw)    # (an unknown name: TypeError, as `fit` gives)
        given.apply_defaults()
        return self._fit_maps(dict(given.arguments), ld_weight)


def robust_rho(d2, sigma):
    """Geman-McClure on squared distances: rho(d2) = sigma^2 d2 / (sigma^2 + d2) - d2 for small residuals, sigma^2 for
    outliers (points of a scan that belong to no part of the body)."""
    s2 = float(sigma) ** 2
    return s2 * d2 / (s2 + d2)


class ScanFitter(_Fitter):
    """`ParamFitter`'s loop with `SMPLLayer -> s verts + t -> scan.surface_distance` in place of decoder + rasteriser: fits
    x (B, 86) to point clouds without correspondences.  Columns 4..85 are pose and shape; the four columns the image fit
    uses for the camera hold (s, t_x, t_y, t_z), the similarity that places the body in the scan's frame (`SMPLLayer`
    ignores them).  Row b's data term is

        L_b = sum_n rho(d2[b, n]) / counts[b]  +  m2p_weight sum_i rho(vd2[b, i]) / V

    (rho = `robust_rho` with `sigma`, the identity when sigma is None), handed to `fit_step` as per-term losses: `loss` = the
    p2m terms scaled by N / counts[b] (fit_step takes the mean over all N columns; the columns beyond counts[b] are 0),
    `silh_loss` = the m2p terms with `silh_weight` = m2p_weight; the gradient comes from constant cotangents 1 / N and
    m2p_weight / V.  A row without a usable point has an infinite m2p term and counts as a bad call (nothing changes).
    Every launch of an iteration reproduces its bits, so two fits from the same start agree bit for bit.

        fitter = ScanFitter(smpl_path, topo)                        # topo: a render.MeshTopology of the model's faces
        r = fitter.fit(points, counts, init=x0, steps=200, lr=0.02, mode="torch", prior=prior, prior_weights=(1, 1, 1))
    """

    sc_dims = (3,)             # (markers in the scan's frame; the four leading columns are no camera)

    def __init__(self, smpl_path=None, topo=None, m2p_weight=1.0, sigma=None, directions=("p2m", "m2p"), penetration=None,
                 collide=None):
        from .render import MeshTopology
        self._layer_init(smpl_path, "ScanFitter keeps (s, t_x, t_y, t_z) in four leading columns")
        if topo is None:
            faces = self.layer._model.faces
            if faces is None:
                raise ValueError("this SMPL model carries no faces: pass topo=MeshTopology(faces, num_verts)")
            topo = MeshTopology(faces, self.layer._model.num_verts)
        if topo.num_verts != self.layer._model.num_verts:
            raise ValueError("the topology has %d vertices, the model %d" % (topo.num_verts, self.layer._model.num_verts))
        self.topo = topo
        self.directions = (directions,) if isinstance(directions, str) else tuple(directions)
        if not self.directions or any(d not in ("p2m", "m2p") for d in self.directions):
            raise ValueError("directions must name \"p2m\" and / or \"m2p\"")
        self.m2p_weight = float(m2p_weight)
        if sigma is not None and not (math.isfinite(sigma) and sigma > 0):
            raise ValueError("sigma must be > 0 (or None: no robust function)")
        self.sigma = sigma
        # (penetration=True: the fitter's own topology - the verts the term sees are the ones the scan distances see)
        self._pen_init(self.topo if penetration is True else penetration, self.layer._model, collide)
        # (surface=True: the fitter's own topology; the targets are 3D points in the scan's frame, against `place(x)`)
        self._sc_init(self.topo if self._sc_options[0] is True else self._sc_options[0], self.layer._model, self._sc_options[1])

    def initial(self, B, init=None, device=None):
        """(B, 86) float32 start: None = scale 1, no shift, the mean pose and shape; a (B, 86) tensor as it is."""
        from .smpl_model import mean86

        def default():
            if init is not None:
                raise ValueError("init must be None or a (B, %d) tensor, got %r" % (self.P, init))
            row = mean86(1.0)
            row[:4] = (1.0, 0.0, 0.0, 0.0)
            return torch.as_tensor(row, dtype=torch.float32).repeat(B, 1)
        return self._initial(B, init, device, default)

    def place(self, x, offsets=None):
        """x (B, 86) -> the body in the scan's frame: x[:, 0] SMPLLayer(x) + x[:, 1:4]; differentiable.  offsets (B, V, 3):
        SMPL+D offsets, handed to the layer (differentiable in them as well)."""
        if offsets is None:
            return x[:, 0, None, None] * self.layer(x) + x[:, None, 1:4]
        return x[:, 0, None, None] * self.layer(x, offsets) + x[:, None, 1:4]

    def terms(self, x, points, counts=None, verts=None, offsets=None):
        """-> (p2m terms (B, N) scaled by N / counts or None, m2p terms (B, V) or None, the op's dict): what `fit_step`
        gets as `loss` and `silh_loss`; differentiable in x.  verts: `place(x)` when the caller has it already; offsets go
        to `place` when it has not."""
        from .scan import surface_distance
        out = surface_distance(self.place(x, offsets) if verts is None else verts, self.topo, points, counts, self.directions)
        rho = (lambda d: d) if self.sigma is None else (lambda d: robust_rho(d, self.sigma))
        N = int(points.shape[1])
        p2m = m2p = None
        if "d2" in out:
            p2m = rho(out["d2"])
            if counts is not None:
                p2m = p2m * (float(N) / counts.to(torch.float32).clamp(min=1.0))[:, None]
        if "vd2" in out:
            m2p = rho(out["vd2"])
        return p2m, m2p, out

    def _forward(self, x, data):
        verts = self.place(x)
        p2m, m2p, _ = self.terms(x, data[0], data[1], verts)
        terms = [t for t in (p2m, m2p) if t is not None]
        return terms, self.m2p_weight if len(terms) == 2 else 1.0, verts, None

    def _cotangents(self, B, dev, data):
        N, V = int(data[0].shape[1]), self.topo.num_verts
        gout = torch.full((B, N), 1.0 / N, dtype=torch.float32, device=dev) if "p2m" in self.directions else None
        sgout = torch.full((B, V), 1.0 / V, dtype=torch.float32, device=dev) if "m2p" in self.directions else None
        if gout is not None and sgout is not None:
            sgout = sgout * self.m2p_weight
        return [c for c in (gout, sgout) if c is not None]

    def _points(self, points, counts):
        if not isinstance(points, torch.Tensor) or points.dim() != 3 or points.shape[2] != 3 or points.shape[1] < 1:
            raise ValueError("points must be a (B, N, 3) tensor with N >= 1")
        points = _lib.require_cuda(points.detach(), "points")
        B, N = int(points.shape[0]), int(points.shape[1])
        if counts is not None:
            c = torch.as_tensor(counts)
            if tuple(c.shape) != (B,) or c.is_floating_point():
                raise ValueError("counts must be (%d,) integers" % B)
            if not c.is_cuda and B and (int(c.min()) < 0 or int(c.max()) > N):
                raise ValueError("counts must lie in 0 .. %d" % N)
            counts = c.to(device=points.device, dtype=torch.int32).contiguous()
        return points, counts

    def losses(self, x, points, counts=None, prior=None, prior_weights=None, pen_weight=None):
        """Per-row loss (B,) of parameters x against the scans, reduced by the kernel of the loop (a call with a zero
        gradient on a scratch state): the bits `fit` would record for x in its history (the self-penetration term of a
        fitter built with `penetration` included, pen_weight None: 1)."""
        return self._losses(x, self._points(points, counts), prior, prior_weights, self._check_sides(pen_weight))

    def fit(self, points, counts=None, init=None, steps=200, lr=1e-2, mode="torch", stages=None, patience=0, grad_scale=1.0,
            graph=False, check_every=0, history=False, beta1=0.9, beta2=0.999, eps=KERAS_EPS, graph_steps=4, prior=None,
            prior_weights=None, group_size=1, tie=("shape",), smooth=None, pen_weight=None):
        """points (B, N, 3) fp32 on the HIP device, counts (B,) or None -> FitResult.  Everything else as `ParamFitter.fit`:
        steps or stages = [(steps, column_scale), ...] (`column_scale(cam=...)` scales the (s, t) columns), patience,
        grad_scale, graph / graph_steps, check_every, history, prior and prior_weights (one triple or one per stage),
        group_size / tie / smooth for several scans of one body (tie="cam" would tie the placement as well), pen_weight with
        a fitter built with `penetration`."""
        loop = _fit_args(locals(), lbfgs=True)
        sides = self._check_sides(pen_weight)
        data = self._points(points, counts)
        B, dev = int(data[0].shape[0]), data[0].device
        return self._fit(B, dev, lambda: self.initial(B, init, dev), lambda: data, sides, **loop)


class KeypointFitter(_Fitter):
    """`ScanFitter`'s shape with detected 2D joints as the only data term: `SMPLLayer -> keypoints.keypoint_energy` with
    cam = x[:, :4], the decoder's camera columns, so targets are in the pixel frame of a decoder at `img_wh`.  Row b's data
    term is mean_K(e[b, :]), e = conf rho(d2) per joint (rho = `robust_rho` with `sigma` in pixels, the identity when sigma is
    None), handed to `fit_step` as per-term losses with the constant cotangent 1 / K.  A row whose status is NONFINITE has a
    NaN loss and gradient and counts as a bad call (nothing changes).  Every launch of an iteration reproduces its bits, so
    two fits from the same start agree bit for bit.

        fitter = KeypointFitter(smpl_path, sigma=3.0)               # spec: the model's cocoplus joints
        r = fitter.fit(target, conf, steps=200, lr=0.02, prior=prior, prior_weights=(1, 1, 1))
    """

    def __init__(self, smpl_path=None, spec=None, sigma=None, img_wh=48, penetration=None, collide=None):
        from .keypoints import KeypointSpec, check_sigma
        self._layer_init(smpl_path, "KeypointFitter projects with four camera columns")
        self.img_wh = int(img_wh)
        if spec is None:
            spec = KeypointSpec.from_model(self.layer)
        if not isinstance(spec, KeypointSpec):
            raise TypeError("spec must be a keypoints.KeypointSpec")
        if spec.num_verts != self.layer._model.num_verts:
            raise ValueError("the keypoint spec has %d vertices, the model %d" % (spec.num_verts, self.layer._model.num_verts))
        check_sigma(sigma)
        self.spec, self.sigma = spec, sigma
        self._pen_init(penetration, self.layer._model, collide)
        self._sc_init(self._sc_options[0], self.layer._model, self._sc_options[1])

    def initial(self, B, init=None, device=None):
        """(B, 86) float32 start: None = `smpl_model.mean86(img_wh)` per row; a (B, 86) tensor as it is."""
        from .smpl_model import mean86

        def default():
            if init is not None:
                raise ValueError("init must be None or a (B, %d) tensor, got %r" % (self.P, init))
            return torch.as_tensor(mean86(self.img_wh), dtype=torch.float32).repeat(B, 1)
        return self._initial(B, init, device, default)

    def terms(self, x, target, conf):
        """-> (e (B, K) differentiable in x, the op's details, verts): what `fit_step` gets as `loss`."""
        from .keypoints import keypoint_energy
        verts = self.layer(x)
        jtr = self.layer.J_transformed if self.spec.with_joints else None
        e, det = keypoint_energy(verts, x[:, :4], self.spec, target, conf, self.sigma, jtr, return_details=True)
        return e, det, verts

    def _forward(self, x, data):
        e, _, verts = self.terms(x, *data)
        return [e], 1.0, verts, None

    def _cotangents(self, B, dev, data):
        return [torch.full((B, self.spec.K), 1.0 / self.spec.K, dtype=torch.float32, device=dev)]

    def _data(self, target, conf):
        K = self.spec.K
        if not isinstance(target, torch.Tensor) or target.dim() != 3 or tuple(target.shape[1:]) != (K, 2):
            raise ValueError("target must be a (B, %d, 2) tensor" % K)
        B = int(target.shape[0])
        if not isinstance(conf, torch.Tensor) or tuple(conf.shape) != (B, K):
            raise ValueError("conf must be a (%d, %d) tensor" % (B, K))
        target = _lib.require_cuda(target.detach().to(torch.float32), "target")
        conf = _lib.require_cuda(conf.detach().to(torch.float32), "conf")
        if conf.device != target.device:
            raise RuntimeError("conf lives on %s, target on %s" % (conf.device, target.device))
        return target, conf

    def losses(self, x, target, conf, prior=None, prior_weights=None, pen_weight=None):
        """Per-row loss (B,) of parameters x against the detections, reduced by the kernel of the loop (a call with a zero
        gradient on a scratch state): the bits `fit` would record for x in its history."""
        return self._losses(x, self._data(target, conf), prior, prior_weights, self._check_sides(pen_weight))

    def fit(self, target, conf, init=None, steps=200, lr=1e-2, mode="torch", stages=None, patience=0, grad_scale=1.0,
            graph=False, check_every=0, history=False, beta1=0.9, beta2=0.999, eps=KERAS_EPS, graph_steps=4, prior=None,
            prior_weights=None, group_size=1, tie=("shape",), smooth=None, pen_weight=None):
        """target (B, K, 2) and conf (B, K) fp32 on the HIP device -> FitResult.  Everything else as `ParamFitter.fit`: steps or
        stages = [(steps, column_scale), ...], patience, grad_scale, graph / graph_steps, check_every, history, prior and
        prior_weights (one triple or one per stage), group_size / tie / smooth for several views or frames of one body,
        pen_weight with a fitter built with `penetration`."""
        loop = _fit_args(locals(), lbfgs=True)
        sides = self._check_sides(pen_weight)
        data = self._data(target, conf)
        B, dev = int(data[0].shape[0]), data[0].device
        return self._fit(B, dev, lambda: self.initial(B, init, dev), lambda: data, sides, **loop)


class _WithSurface:
    """The dense surface-correspondence term on a fitter class: constructor arguments surface= (a render.MeshTopology over
    the model's vertices; `ScanFitter` also takes True: its own topology) and sc_sigma= (None: rho(s) = s), and on `fit` and
    `losses` surface= (a `surface.SurfaceTargets` of B rows) and sc_weight= (None: 1, one float, or one per stage).  Every
    other argument passes through to the fitter's own method; the pairing rules are `_check_sides`'."""

    def __init__(self, *args, surface=None, sc_sigma=None, **kw):
        self._sc_options = (surface, sc_sigma)
        super().__init__(*args, **kw)

    def _sc_during(self, call, args, kw, surface, sc_weight):
        self._sc_call = (surface, sc_weight)
        try:
            return call(*args, **kw)
        finally:
            self._sc_call = (None, None)

    def fit(self, *args, surface=None, sc_weight=None, **kw):
        return self._sc_during(super().fit, args, kw, surface, sc_weight)

    def losses(self, *args, surface=None, sc_weight=None, **kw):
        return self._sc_during(super().losses, args, kw, surface, sc_weight)


_with_surface = {}


def with_surface(fitter_class):
    """`ParamFitter`, `LabelDistanceFitter`, `KeypointFitter` or `ScanFitter` -> that fitter with the dense
    surface-correspondence term as its fourth side term (`_WithSurface`: surface=, sc_sigma= at construction, surface=,
    sc_weight= on `fit` and `losses`).  A class of its own, as `LabelDistanceFitter` is, because the four fitters' constructors,
    `fit` and `losses` keep the signatures their callers rely on.  `ScanFitter` takes 3D targets only; the others image targets
    under cam = x[:, :4] or 3D targets in the vertices' own frame.

        fitter = with_surface(ParamFitter)(smpl_path, surface=topo, sc_sigma=3.0)
        r = fitter.fit(labels, surface=SurfaceTargets(topo, face, bary, target, conf), sc_weight=[1.0, 0.1], stages=...)
    """
    if not (isinstance(fitter_class, type) and issubclass(fitter_class, _Fitter)) or issubclass(fitter_class, (SurfaceFitter, _WithSurface)):
        raise TypeError("with_surface takes ParamFitter, LabelDistanceFitter, KeypointFitter or ScanFitter")
    if fitter_class not in _with_surface:
        _with_surface[fitter_class] = type("Surface" + fitter_class.__name__, (_WithSurface, fitter_class), {"__doc__": _WithSurface.__doc__})
    return _with_surface[fitter_class]


class SurfaceFitter(_Fitter):
    """`KeypointFitter`'s shape with dense surface correspondences as the only data term: `SMPLLayer ->
    surface.surface_energy`.  With image targets (D = 2) cam = x[:, :4], the decoder's camera columns, so targets are in the
    pixel frame of a decoder at `img_wh`; with 3D targets (D = 3) the vertices are compared in the layer's own frame and the
    four camera columns get no gradient.  Row b's data term is mean_N(e[b, :]) over all N columns (padding counts as 0), e =
    conf rho(d2) per correspondence (rho = `robust_rho` with `sigma`, the identity when sigma is None), handed to `fit_step`
    as per-term losses with the constant cotangent 1 / N.  A row whose status is NONFINITE has a NaN loss and gradient and
    counts as a bad call (nothing changes).  Every launch of an iteration reproduces its bits, so two fits from the same
    start agree bit for bit.

        fitter = SurfaceFitter(smpl_path, sigma=3.0)                # topo: the model's faces
        r = fitter.fit(SurfaceTargets(fitter.topo, face, bary, target), steps=200, lr=0.02)
    """

    def __init__(self, smpl_path=None, topo=None, sigma=None, img_wh=48, penetration=None, collide=None):
        from .keypoints import check_sigma
        from .render import MeshTopology
        self._layer_init(smpl_path, "SurfaceFitter projects with four camera columns")
        self.img_wh = int(img_wh)
        if topo is None:
            faces = self.layer._model.faces
            if faces is None:
                raise ValueError("this SMPL model carries no faces: pass topo=MeshTopology(faces, num_verts)")
            topo = MeshTopology(faces, self.layer._model.num_verts)
        if not all(hasattr(topo, a) for a in ("faces", "num_verts", "num_faces", "on")):
            raise TypeError("topo must be a render.MeshTopology")
        if topo.num_verts != self.layer._model.num_verts:
            raise ValueError("the topology has %d vertices, the model %d" % (topo.num_verts, self.layer._model.num_verts))
        check_sigma(sigma)
        self.topo, self.sigma = topo, sigma
        self.sc_topo = topo                                       # (what `_sc_data` checks the targets against)
        self._pen_init(self.topo if penetration is True else penetration, self.layer._model, collide)

    def initial(self, B, init=None, device=None):
        """(B, 86) float32 start: None = `smpl_model.mean86(img_wh)` per row; a (B, 86) tensor as it is."""
        from .smpl_model import mean86

        def default():
            if init is not None:
                raise ValueError("init must be None or a (B, %d) tensor, got %r" % (self.P, init))
            return torch.as_tensor(mean86(self.img_wh), dtype=torch.float32).repeat(B, 1)
        return self._initial(B, init, device, default)

    def terms(self, x, targets):
        """-> (e (B, N) differentiable in x, the op's details, verts): what `fit_step` gets as `loss`."""
        from .surface import surface_energy
        verts = self.layer(x)
        e, det = surface_energy(verts, x[:, :4] if targets.D == 2 else None, targets, self.sigma, return_details=True)
        return e, det, verts

    def _forward(self, x, data):
        e, _, verts = self.terms(x, data)
        return [e], 1.0, verts, None

    def _cotangents(self, B, dev, data):
        return [torch.full((B, data.N), 1.0 / data.N, dtype=torch.float32, device=dev)]

    def _data(self, targets):
        from .surface import SurfaceTargets
        if not isinstance(targets, SurfaceTargets):
            raise TypeError("targets must be a surface.SurfaceTargets")
        if not targets.face.is_cuda:
            raise RuntimeError("the targets must live on a HIP device (got %s); this framework has no CPU path" % targets.device)
        return self._sc_data(targets, targets.B, targets.device)

    def losses(self, x, targets, prior=None, prior_weights=None, pen_weight=None):
        """Per-row loss (B,) of parameters x against the correspondences, reduced by the kernel of the loop (a call with a
        zero gradient on a scratch state): the bits `fit` would record for x in its history."""
        return self._losses(x, self._data(targets), prior, prior_weights, self._check_sides(pen_weight))

    def fit(self, targets, init=None, steps=200, lr=1e-2, mode="torch", stages=None, patience=0, grad_scale=1.0, graph=False,
            check_every=0, history=False, beta1=0.9, beta2=0.999, eps=KERAS_EPS, graph_steps=4, prior=None, prior_weights=None,
            group_size=1, tie=("shape",), smooth=None, pen_weight=None):
        """targets: a `surface.SurfaceTargets` on the HIP device -> FitResult.  Everything else as `ParamFitter.fit`: steps or
        stages = [(steps, column_scale), ...], patience, grad_scale, graph / graph_steps, check_every, history, prior and
        prior_weights (one triple or one per stage), group_size / tie / smooth for several views or frames of one body,
        pen_weight with a fitter built with `penetration`."""
        loop = _fit_args(locals(), lbfgs=True)
        sides = self._check_sides(pen_weight)
        data = self._data(targets)
        return self._fit(data.B, data.device, lambda: self.initial(data.B, init, data.device), lambda: data, sides, **loop)


# ---- SMPL+D registration: free vertex offsets under mesh regularisers --------------------------------------------------
def offset_step(D, grad, m, v, t, bad, loss, lr=1e-3, beta1=0.9, beta2=0.999, eps=KERAS_EPS, mode="torch"):
    """One smplr_offset_step launch (in place): Adam over the rows of D (B, V, 3) with the row's own step count t (B,) int32,
    in `fit_step`'s keras or torch form.  grad, m, v: D's shape; loss (B,): a row whose loss is not finite is a bad call -
    bad[b] += 1 and nothing else of the row changes.  HIP tensors only."""
    if mode not in MODES:
        raise ValueError("mode %r is none of %s" % (mode, MODES))
    rc = _lib.require_cuda
    if not D.is_contiguous():
        raise RuntimeError("D must be contiguous (it is updated in place)")
    rc(D, "D")
    B = int(D.shape[0])
    n = int(D.numel() // B) if B else int(np.prod(D.shape[1:]))
    if D.dim() < 2 or n < 1:
        raise RuntimeError("D must be (B, ...) with at least one entry per row, got %s" % (tuple(D.shape),))
    for name, a in (("grad", grad), ("m", m), ("v", v)):
        if tuple(a.shape) != tuple(D.shape) or not a.is_contiguous():
            raise RuntimeError("%s must be a contiguous %s tensor, got %s" % (name, tuple(D.shape), tuple(a.shape)))
        rc(a, name)
    for name, a in (("t", t), ("bad", bad)):
        if tuple(a.shape) != (B,):
            raise RuntimeError("%s must be (%d,), got %s" % (name, B, tuple(a.shape)))
        rc(a, name, torch.int32)
    if tuple(loss.shape) != (B,) or not loss.is_contiguous():
        raise RuntimeError("loss must be a contiguous (%d,) tensor, got %s" % (B, tuple(loss.shape)))
    rc(loss, "loss")
    for name, a in (("grad", grad), ("m", m), ("v", v), ("t", t), ("bad", bad), ("loss", loss)):
        if a.device != D.device:
            raise RuntimeError("%s lives on %s, D on %s" % (name, a.device, D.device))
    with torch.cuda.device(D.device):
        check(_lib.load().smplr_offset_step(ptr(D), ptr(grad), ptr(m), ptr(v), ptr(t), ptr(bad), ptr(loss), float(lr), float(beta1),
                                            float(beta2), float(eps), MODES.index(mode), B, n, stream()), "smplr_offset_step")
    return D


@dataclass
class OffsetFitResult:
    """offsets (B, V, 3): D at the end; x (B, 86): the parameters at the end (the start, unless fit_params); history
    (steps, B) fp32 per-row loss trace or None; bad (B,) int32: iterations that met a non-finite loss (and changed nothing of
    D); steps: iterations run; t (B,) int32: D's update count; state: the `FitState` of x with fit_params, else None."""
    offsets: torch.Tensor
    x: torch.Tensor
    history: Optional[torch.Tensor]
    bad: torch.Tensor
    steps: int
    t: torch.Tensor
    state: Optional[FitState] = None


class OffsetFitter:
    """SMPL+D registration behind a `ScanFitter`: free per-vertex offsets D (B, V, 3) move the surface onto the scan, held
    together by the regularisers of a `meshreg.MeshRegSpec`.  Row b's loss is

        L_b = [ScanFitter's data terms of place(x, D)] + lap_weight E_lap + edge_weight E_edge + offset_weight mean_i |D_i|^2

    with (E_lap, E_edge) = `mesh_regularisers(v_template + D, spec)`: the regulariser sees the UNPOSED mesh in the template's
    frame - the frame a spec built on v_template was measured in (E_lap with lap_ref = L(ref) is not invariant under a
    rotation of the mesh, so the posed surface would be penalised for its pose), and there E_lap is mean |L(D)|^2.  An
    iteration is place, the terms, one `autograd.grad` with respect to D (and x with fit_params), `fit_step` on x (with
    fit_params) and `offset_step` on D; every launch reproduces its bits, so two fits from the same start agree bit for bit.
    penetration=True adds the scan fitter's self-penetration term (it must have been built with one).

        reg = OffsetFitter(scan_fitter, MeshRegSpec(scan_fitter.topo, model.v_template, "cotangent"))
        r = reg.fit(points, counts, x=fit.x, steps=200, lr=1e-3, lap_weight=1e4, edge_weight=1.0, offset_weight=1.0)
    """

    def __init__(self, scan_fitter, spec, penetration=None):
        from .meshreg import MeshRegSpec
        if not isinstance(scan_fitter, ScanFitter):
            raise TypeError("scan_fitter must be a ScanFitter")
        if not isinstance(spec, MeshRegSpec):
            raise TypeError("spec must be a meshreg.MeshRegSpec")
        if spec.num_verts != scan_fitter.topo.num_verts:
            raise ValueError("the spec has %d vertices, the fitter's topology %d" % (spec.num_verts, scan_fitter.topo.num_verts))
        if penetration not in (None, False, True):
            raise TypeError("penetration must be None, False or True (the scan fitter's own term)")
        if penetration and scan_fitter.pen_topo is None:
            raise ValueError("penetration=True needs a ScanFitter built with penetration=...")
        self.scan, self.spec, self.penetration = scan_fitter, spec, bool(penetration)
        self.V = spec.num_verts
        self._template = {}

    def template(self, device):
        """v_template (1, V, 3) fp32 on `device`: the frame the regulariser works in."""
        device = torch.device(device)
        t = self._template.get(device)
        if t is None:
            t = torch.as_tensor(np.asarray(self.scan.layer._model.v_template), dtype=torch.float32).reshape(1, self.V, 3).to(device)
            self._template[device] = t
        return t

    def row_loss(self, x, D, points, counts, wts, pen_w=None):
        """-> L (B,), differentiable in x and D: the composition `fit` iterates.  wts (3,) device tensor = (lap_weight,
        edge_weight, offset_weight); pen_w (1,) device tensor with the penetration term."""
        from .meshreg import mesh_regularisers
        sf = self.scan
        verts = sf.place(x, D)
        p2m, m2p, _ = sf.terms(x, points, counts, verts)
        L = None
        if p2m is not None:
            L = p2m.sum(1) / float(p2m.shape[1])
        if m2p is not None:
            d = m2p.sum(1) / float(m2p.shape[1])
            L = d if L is None else L + sf.m2p_weight * d
        reg = mesh_regularisers(self.template(D.device) + D, self.spec, return_terms=True)
        L = L + wts[0] * reg[:, 0] + wts[1] * reg[:, 1] + wts[2] * ((D * D).sum((1, 2)) / float(self.V))
        if pen_w is not None:
            from .penetration import self_penetration
            L = L + pen_w * self_penetration(verts, sf.pen_topo, sf.pen_collide).mean(1)
        return L

    def _iteration(self, var, data, wts, pen_w, hist, it, kw, xkw=None):
        """One iteration on var = (D, m, v, t, bad, state) - the real state or a scratch copy - against data = (points,
        counts).  hist (steps, B) with its row counter `it` (1,) on the device, or None; kw: `offset_step`'s; xkw: `fit_step`'s
        with the column scales under "col_scale" when x moves too (fit_params), else None."""
        D, m, v, t, bad, state = var
        x = state.x.detach().requires_grad_(True) if xkw is not None else state.x
        Dg = D.detach().requires_grad_(True)                      # (shares D's memory: the kernel updates it in place)
        L = self.row_loss(x, Dg, data[0], data[1], wts, pen_w)
        grads = torch.autograd.grad(L.sum(), [Dg, x] if xkw is not None else [Dg])
        Ld = L.detach().contiguous()
        if hist is not None:
            hist.index_copy_(0, it, Ld[None])
            it.add_(1)
        if xkw is not None:
            fit_step(state, grads[1].contiguous(), Ld[:, None].contiguous(), **xkw)
        offset_step(D, grads[0].contiguous(), m, v, t, bad, Ld, **kw)

    def fit(self, points, counts, x, steps=200, lr=1e-3, lap_weight=1.0, edge_weight=1.0, offset_weight=0.0, stages=None,
            fit_params=False, history=False, graph=False, offsets=None, mode="torch", beta1=0.9, beta2=0.999, eps=KERAS_EPS,
            x_lr=None, pen_weight=None):
        """points (B, N, 3) fp32 on the HIP device, counts (B,) or None, x (B, 86) the parameters a `ScanFitter.fit` ended
        with -> OffsetFitResult.  steps, or stages = [(steps, column_scale), ...] as `ScanFitter.fit` takes them (the column
        scales act on x, with fit_params); lap_weight, edge_weight, offset_weight (and pen_weight with penetration=True): one
        float or a list of one per stage.  offsets: the start (None: zeros).  fit_params: x moves too, through `fit_step`
        with x_lr (None: lr).  graph: one iteration is captured once and replayed."""
        _fit_args(locals())                                       # (for its mode check: this loop names its own arguments)
        sf = self.scan
        data = sf._points(points, counts)
        B, dev = int(data[0].shape[0]), data[0].device
        if not isinstance(x, torch.Tensor) or tuple(x.shape) != (B, sf.P):
            raise ValueError("x must be a (%d, %d) tensor" % (B, sf.P))
        stage_list = check_stages(stages, sf.P, steps)
        names = ("lap_weight", "edge_weight", "offset_weight")
        per = [_stage_weights(w, stage_list, n) for w, n in zip((lap_weight, edge_weight, offset_weight), names)]
        if self.penetration:
            pen_stages = _stage_weights(pen_weight, stage_list, "pen_weight")
        elif pen_weight is not None:
            raise ValueError("pen_weight goes with OffsetFitter(..., penetration=True)")
        total = sum(n for n, _ in stage_list)
        kw = dict(lr=float(lr), beta1=float(beta1), beta2=float(beta2), eps=float(eps), mode=mode)
        with torch.cuda.device(dev):
            x0 = _lib.require_cuda(x.detach().to(dev), "x").clone()
            if offsets is None:
                D = torch.zeros((B, self.V, 3), dtype=torch.float32, device=dev)
            else:
                if tuple(offsets.shape) != (B, self.V, 3):
                    raise ValueError("offsets must be (%d, %d, 3), got %s" % (B, self.V, tuple(offsets.shape)))
                D = _lib.require_cuda(offsets.detach().to(dev), "offsets").clone()
            zi = lambda: torch.zeros(B, dtype=torch.int32, device=dev)
            var = (D, torch.zeros_like(D), torch.zeros_like(D), zi(), zi(), FitState.new(x0))
            wts = torch.zeros(3, dtype=torch.float32, device=dev)
            pen_w = torch.zeros(1, dtype=torch.float32, device=dev) if self.penetration else None
            hist = torch.full((total, B), float("nan"), dtype=torch.float32, device=dev) if history and total else None
            it = torch.zeros(1, dtype=torch.long, device=dev)
            cs = torch.ones(sf.P, dtype=torch.float32, device=dev)
            xkw = dict(kw, lr=float(lr if x_lr is None else x_lr), grad_scale=1.0, patience=0, col_scale=cs) if fit_params else None

            def set_stage(si):
                wts.copy_(torch.tensor([p[si] for p in per], dtype=torch.float32))
                cs.copy_(stage_list[si][1].to(dev))
                if pen_w is not None:
                    pen_w.fill_(pen_stages[si])

            def one(var_, h, i):
                self._iteration(var_, data, wts, pen_w, h, i, kw, xkw)
            replay = None
            if total:
                set_stage(0)
            if graph and B > 0 and total > 0:
                replay = _capture(one, (tuple(a.clone() for a in var), None, None), (var, hist, it), 1, dev)
            done = _run_stages(stage_list, set_stage, lambda: one(var, hist, it), replay)
            torch.cuda.synchronize()
        D, _, _, t, bad, state = var
        return OffsetFitResult(offsets=D, x=state.x, history=hist, bad=bad, steps=done, t=t, state=state if fit_params else None)
