"""2D keypoints, differentiable: detected image joints as a data term - what every SMPL fitting pipeline starts from.
Beyond the reference, which compares label maps only.

    spec = KeypointSpec.from_model(layer, "cocoplus")              # 19 joints as sparse combinations of the 6 890 vertices
    e = keypoint_energy(verts, x[:, :4], spec, target, conf, sigma=3.0)             # (B, K) fp32
    e, det = keypoint_energy(verts, cam, spec, target, conf, return_details=True)   # det: joints, proj, d2, status

Definitions.
  Sources   verts (B, V, 3) fp32, optionally followed by J_transformed (B, 24, 3): source i < V is vertex i, source V + j is
            posed joint j - allowed only when the spec was built `with_joints` and `joints=` is given.
  Spec      `KeypointSpec(regressor, num_verts, with_joints=False)`: regressor (K, S) dense or scipy-sparse, S = V or V + 24,
            stored as CSR over joints - off (K + 1) int32, idx (nnz) int32 increasing within a row, w (nnz) fp32 with exact
            zeros dropped - and as its transpose, source-major: t_off (S + 1), t_joint (increasing within a source), t_w.
            1 <= K <= 64, nnz <= 2^24; non-finite weights are refused, and so are indices >= V without with_joints.
  Joints    J[b, k] = sum over row k of w source[b, idx]; an empty row gives 0.
  Camera    cam (B, 4) = (k_u, k_v, u0, v0), the decoder's four columns; p[b, k] = (u0 + k_u J_x, v0 + k_v J_y), the
            convention of `orthographic_project`.
  Energy    target (B, K, 2) fp32 in that camera's pixel frame, conf (B, K) fp32.  Joint k of row b counts iff conf > 0 (a NaN
            conf does not count).  r = p - t, d2 = r_u^2 + r_v^2, e = conf rho(d2) with rho(s) = sigma^2 s / (sigma^2 + s)
            (`fitting.robust_rho`, Geman-McClure; sigma=None: rho(s) = s).  A joint that does not count has e = 0 and no
            gradient whatever its target holds (a select, not a product: a NaN target under conf = 0 is harmless); its d2, proj
            and joints entries are still what the formulas give.
  Status    status (B,) int32 = NONFINITE (1) when a coordinate of a source that a counted joint uses is NaN / Inf, or a cam
            column is, or a counted joint's target is: that row's e, d2, proj, joints and gradient rows are NaN; other rows
            are untouched.  A NaN in a source no counted joint uses does not matter.
  Gradient  with cotangent g (B, K) on e: q = g conf rho'(d2) 2 r, rho'(s) = sigma^4 / (sigma^2 + s)^2 (or 1); dJ = (q_u k_u,
            q_v k_v, 0); dsource[i] = sum_k w_ki dJ_k, written for every source (exact zeros where no joint uses it);
            dcam = (sum_k q_u J_x, sum_k q_v J_y, sum_k q_u, sum_k q_v).  None for target or conf.
  Rounding  all products and sums in fp64 on the fp32 inputs, in an order the launch geometry alone fixes - never B or other
            rows; every output is rounded to fp32 once.
Device tensors run csrc/keypoints.hip: one forward launch (smplr_kp_fwd) and one backward launch (smplr_kp_bwd), no atomics,
the same bits in every run and whatever else is in the batch.  CPU tensors run `keypoint_energy_torch`, a float64 torch
restatement; on device tensors that function is the stock composition the kernels are timed against.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr, stream
from ._mesh_common import check_verts, nan_rows

NONFINITE = 1          # SMPLR_KP_NONFINITE
MAX_JOINTS = 64
MAX_NNZ = 1 << 24
NUM_POSED = 24         # rows of J_transformed
KEYS = ("joints", "proj", "d2", "status")


class KeypointSpec:
    """K joints as sparse combinations of V vertices (and, `with_joints`, of the 24 posed joints): see the module's
    definitions.  Everything is checked here, once, on the host - the kernels trust the arrays.  Attributes: K, num_verts,
    S, nnz, with_joints; off, idx, w, t_off, t_joint, t_w (numpy)."""

    def __init__(self, regressor, num_verts, with_joints=False):
        V = int(num_verts)
        if V < 1 or V > (1 << 24):
            raise ValueError("num_verts must lie in 1 .. 2^24, got %r" % (num_verts,))
        if hasattr(regressor, "toarray") and not isinstance(regressor, np.ndarray):
            regressor = regressor.toarray()                      # (scipy-sparse: K <= 64 rows, the dense form is small)
        if isinstance(regressor, torch.Tensor):
            regressor = regressor.detach().cpu().numpy()
        R = np.asarray(regressor)
        if R.ndim != 2:
            raise ValueError("regressor must be a (K, S) array, got shape %s" % (R.shape,))
        K, S_in = int(R.shape[0]), int(R.shape[1])
        if K < 1 or K > MAX_JOINTS:
            raise ValueError("1 <= K <= %d joints, got K = %d" % (MAX_JOINTS, K))
        if S_in not in (V, V + NUM_POSED):
            raise ValueError("regressor has %d columns: neither num_verts = %d nor num_verts + %d" % (S_in, V, NUM_POSED))
        R = R.astype(np.float64)
        if not np.isfinite(R).all():
            raise ValueError("regressor holds non-finite weights")
        with np.errstate(over="ignore"):
            w32 = R.astype(np.float32)
        if not np.isfinite(w32).all():
            raise ValueError("regressor holds weights beyond float32")
        self.with_joints = bool(with_joints)
        if not self.with_joints and S_in > V and (w32[:, V:] != 0).any():
            raise ValueError("regressor uses joint sources (indices >= num_verts = %d) without with_joints=True" % V)
        S = V + NUM_POSED if self.with_joints else V
        full = np.zeros((K, S), np.float32)
        full[:, :min(S, S_in)] = w32[:, :min(S, S_in)]
        rows, cols = np.nonzero(full)                            # (row-major: columns increase within a row)
        if len(rows) > MAX_NNZ:
            raise ValueError("at most 2^24 non-zero weights, got %d" % len(rows))
        self.K, self.num_verts, self.S, self.nnz = K, V, S, int(len(rows))
        self.off = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=K))]).astype(np.int32)
        self.idx = cols.astype(np.int32)
        self.w = full[rows, cols].astype(np.float32)
        order = np.lexsort((rows, cols))                         # source-major, joints increasing within a source
        self.t_off = np.concatenate([[0], np.cumsum(np.bincount(cols, minlength=S))]).astype(np.int32)
        self.t_joint = rows[order].astype(np.int32)
        self.t_w = self.w[order]
        self._dev = {}

    # ---- constructors ---------------------------------------------------------------------------------------------------
    @classmethod
    def from_model(cls, model_or_layer, joint_type="cocoplus"):
        """The loaded `cocoplus_regressor` (19, V) of an `SMPLModelData`, or of the model behind an `SMPLLayer` /
        `SMPLDecoder`: all 19 rows ("cocoplus") or the first 14 ("lsp"), as `SMPLLayer.joints` takes them."""
        if joint_type not in ("cocoplus", "lsp"):
            raise ValueError("joint_type must be \"cocoplus\" or \"lsp\", got %r" % (joint_type,))
        model = getattr(model_or_layer, "_model", model_or_layer)
        reg = getattr(model, "cocoplus_regressor", None)
        if reg is None:
            raise ValueError("this SMPL model has no cocoplus_regressor")
        reg = np.asarray(reg, np.float64)
        return cls(reg[:14] if joint_type == "lsp" else reg, int(model.num_verts))

    @classmethod
    def smpl_joints(cls, num_verts=6890):
        """The identity on the 24 posed joints: K = 24, joint k = J_transformed[:, k] (every index >= V)."""
        R = np.zeros((NUM_POSED, int(num_verts) + NUM_POSED), np.float32)
        R[np.arange(NUM_POSED), int(num_verts) + np.arange(NUM_POSED)] = 1.0
        return cls(R, num_verts, with_joints=True)

    # ---- views ----------------------------------------------------------------------------------------------------------
    def dense(self):
        """(K, S) float32 numpy: the regressor as stored."""
        R = np.zeros((self.K, self.S), np.float32)
        R[np.repeat(np.arange(self.K), np.diff(self.off)), self.idx] = self.w
        return R

    def on(self, device):
        """dict of the six index / weight arrays as tensors on `device`, plus "dense" (K, S) float64 and "mask" (K, S)
        float64 of 0 / 1 for the torch path: uploaded once per device (no copy in later calls, so a call can be captured
        into a graph)."""
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        d = self._dev.get(device)
        if d is None:
            d = {n: torch.from_numpy(getattr(self, n)).to(device) for n in ("off", "idx", "w", "t_off", "t_joint", "t_w")}
            dense = torch.from_numpy(self.dense().astype(np.float64)).to(device)
            d["dense"], d["mask"] = dense, (dense != 0).to(torch.float64)
            self._dev[device] = d
        return d

    def to(self, device):
        """The spec itself, its device copies for `device` made and cached."""
        self.on(device)
        return self


def check_sigma(sigma):
    """None, or a finite float > 0 that float32 holds -> the float the kernels get (0.0: no robust function)."""
    if sigma is None:
        return 0.0
    s = float(sigma)
    if not (math.isfinite(s) and s > 0 and float(np.float32(s)) > 0 and math.isfinite(float(np.float32(s)))):
        raise ValueError("sigma must be > 0 (or None: no robust function), got %r" % (sigma,))
    return float(np.float32(s))


def _rho(s, s2):
    return s if s2 == 0.0 else (s2 * s) / (s2 + s)


def _drho(s, s2):
    return torch.ones_like(s) if s2 == 0.0 else (s2 * s2) / ((s2 + s) * (s2 + s))


def keypoint_energy_torch(verts, cam, spec, target, conf, sigma=None, joints=None):
    """The definitions in float64 torch on any device (the CPU path, and the stock composition the kernels are timed
    against): one dense einsum for the joints and element-wise launches for the rest; differentiable in verts, cam and joints
    by autograd (on rows whose status is 0).  -> dict of e, d2 (B, K), proj (B, K, 2), joints (B, K, 3), ws (B, K, 4) =
    (J_x, J_y, r_u, r_v), all float64, and status (B,) int32."""
    s2 = check_sigma(sigma) ** 2
    d = spec.on(verts.device)
    f64 = torch.float64
    src = verts if joints is None else torch.cat([verts, joints], 1)
    src = src.to(f64)
    fin = torch.isfinite(src).all(-1)                                                 # (B, S)
    zero = torch.zeros((), dtype=f64, device=src.device)
    nan = torch.full((), float("nan"), dtype=f64, device=src.device)
    R, M = d["dense"][:, :src.shape[1]], d["mask"][:, :src.shape[1]]
    J = torch.einsum("ks,bsc->bkc", R, torch.where(fin[..., None], src, zero))
    jbad = torch.einsum("ks,bs->bk", M, (~fin).to(f64)) > 0
    c = cam.to(f64)
    t = target.to(f64)
    counted = conf > 0
    p = torch.stack([c[:, 2, None] + c[:, 0, None] * J[..., 0], c[:, 3, None] + c[:, 1, None] * J[..., 1]], -1)
    r = p - t
    d2 = (r * r).sum(-1)
    rc = torch.where(counted[..., None], r, zero)                                     # (what the energy is made of)
    e = torch.where(counted, torch.where(counted, conf.to(f64), zero) * _rho((rc * rc).sum(-1), s2), zero)
    bad = ~torch.isfinite(c).all(1) | (counted & (jbad | ~torch.isfinite(t).all(-1))).any(1)
    b1, b2 = bad[:, None] | jbad, (bad[:, None] | jbad)[..., None]                    # (a joint of non-finite sources: NaN)
    return {"e": nan_rows(bad, e), "d2": torch.where(b1, nan, d2), "proj": torch.where(b2, nan, p),
            "joints": torch.where(b2, nan, J), "ws": torch.cat([J[..., :2], r], -1).detach(),
            "status": bad.to(torch.int32) * NONFINITE}


def _backward_torch(spec, cam, conf, ws, status, g, s2, num_sources):
    """The gradient definition in float64 torch -> (dsource (B, S, 3), dcam (B, 4)) float32, rounded once."""
    f64 = torch.float64
    d = spec.on(cam.device)
    zero = torch.zeros((), dtype=f64, device=cam.device)
    counted = conf > 0
    Jxy, r = ws[..., :2], ws[..., 2:]
    c = g.to(f64) * conf.to(f64) * _drho((r * r).sum(-1), s2)
    q = torch.where(counted[..., None], c[..., None] * (2.0 * r), zero)               # (B, K, 2)
    k = cam.to(f64)[:, None, :2]
    dJ = torch.cat([q * k, torch.zeros_like(q[..., :1])], -1)
    dsrc = torch.einsum("ks,bkc->bsc", d["dense"][:, :num_sources], dJ)
    dcam = torch.cat([(q * Jxy).sum(1), q.sum(1)], -1)
    bad = status != 0
    return nan_rows(bad, dsrc).to(torch.float32), nan_rows(bad, dcam).to(torch.float32)


class _KeypointFn(torch.autograd.Function):
    """verts, cam, joints (or None) -> e, d2, proj, joints, status.  Device tensors: smplr_kp_fwd forward, smplr_kp_bwd
    backward; CPU tensors: the float64 torch path."""

    @staticmethod
    def forward(ctx, verts, cam, jtr, spec, target, conf, sigma):
        ctx.set_materialize_grads(False)
        dev = verts.device
        B, V, K = int(verts.shape[0]), int(verts.shape[1]), spec.K
        if verts.is_cuda:
            d = spec.on(dev)
            f32 = dict(dtype=torch.float32, device=dev)
            e, d2 = torch.empty((B, K), **f32), torch.empty((B, K), **f32)
            proj, joints = torch.empty((B, K, 2), **f32), torch.empty((B, K, 3), **f32)
            status = torch.empty((B,), dtype=torch.int32, device=dev)
            ws = torch.empty((B, K, 4), dtype=torch.float64, device=dev)
            check(_lib.load().smplr_kp_fwd(ptr(verts), ptr(jtr), ptr(cam), ptr(d["off"]), ptr(d["idx"]) if spec.nnz else None,
                                           ptr(d["w"]) if spec.nnz else None, ptr(target), ptr(conf), B, V, K, spec.nnz, sigma,
                                           ptr(e), ptr(d2), ptr(proj), ptr(joints), ptr(status), ptr(ws), stream()),
                  "smplr_kp_fwd")
        else:
            with torch.no_grad():
                o = keypoint_energy_torch(verts, cam, spec, target, conf, sigma or None, jtr)
            e, d2, proj, joints = (o[n].to(torch.float32) for n in ("e", "d2", "proj", "joints"))
            status, ws = o["status"], o["ws"]
        ctx.dims = (B, V, K)
        ctx.spec, ctx.sigma, ctx.has_jtr = spec, sigma, jtr is not None
        ctx.save_for_backward(cam, conf, status, ws)
        ctx.mark_non_differentiable(d2, proj, joints, status)
        return e, d2, proj, joints, status

    @staticmethod
    def backward(ctx, g, *_):
        cam, conf, status, ws = ctx.saved_tensors
        B, V, K = ctx.dims
        spec = ctx.spec
        need_v, need_c, need_j = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.has_jtr and ctx.needs_input_grad[2]
        if g is None or not (need_v or need_c or need_j):
            return (None,) * 7
        g = g.to(torch.float32).contiguous()
        if not cam.is_cuda:
            S = V + (NUM_POSED if ctx.has_jtr else 0)
            dsrc, dcam = _backward_torch(spec, cam, conf, ws, status, g, ctx.sigma ** 2, S)
            return (dsrc[:, :V].contiguous() if need_v else None, dcam if need_c else None,
                    dsrc[:, V:].contiguous() if need_j else None, None, None, None, None)
        dev = cam.device
        d = spec.on(dev)
        dverts = torch.empty((B, V, 3), dtype=torch.float32, device=dev)
        djtr = torch.empty((B, NUM_POSED, 3), dtype=torch.float32, device=dev) if need_j else None
        dcam = torch.empty((B, 4), dtype=torch.float32, device=dev) if need_c else None
        with torch.cuda.device(dev):
            check(_lib.load().smplr_kp_bwd(ptr(cam), ptr(d["t_off"]), ptr(d["t_joint"]) if spec.nnz else None,
                                           ptr(d["t_w"]) if spec.nnz else None, ptr(conf), ptr(status), ptr(ws), ptr(g), B, V, K,
                                           spec.nnz, ctx.sigma, ptr(dverts), ptr(djtr), ptr(dcam), stream()), "smplr_kp_bwd")
        return dverts if need_v else None, dcam, djtr, None, None, None, None


@_lib.on_device
def _apply(verts, cam, jtr, spec, target, conf, sigma):
    return _KeypointFn.apply(verts, cam, jtr, spec, target, conf, sigma)


def keypoint_energy(verts, cam, spec, target, conf, sigma=None, joints=None, return_details=False):
    """verts (B, V, 3), cam (B, 4), target (B, K, 2), conf (B, K) fp32, spec a `KeypointSpec`, joints = J_transformed
    (B, 24, 3) exactly when the spec was built with_joints -> e (B, K) fp32, differentiable in verts, cam and joints; with
    return_details=True also dict(joints (B, K, 3), proj (B, K, 2), d2 (B, K) fp32, status (B,) int32), constants to
    autograd."""
    if not isinstance(spec, KeypointSpec):
        raise TypeError("spec must be a KeypointSpec")
    (B, V), K = check_verts(verts, spec=spec), spec.K
    if spec.with_joints != (joints is not None):
        raise ValueError("joints (J_transformed) go with a spec built with_joints=True, and only with it")
    shapes = [("cam", cam, (B, 4)), ("target", target, (B, K, 2)), ("conf", conf, (B, K))]
    if joints is not None:
        shapes.append(("joints", joints, (B, NUM_POSED, 3)))
    for name, t, shape in [("verts", verts, (B, V, 3))] + shapes:
        if not isinstance(t, torch.Tensor) or tuple(t.shape) != shape:
            raise ValueError("%s must be a %s tensor" % (name, shape))
        if t.dtype != torch.float32:
            raise RuntimeError("%s must be float32" % name)
        if t.device != verts.device:
            raise RuntimeError("%s lives on %s, verts on %s" % (name, t.device, verts.device))
    e, d2, proj, jts, status = _apply(verts.contiguous(), cam.contiguous(), None if joints is None else joints.contiguous(), spec,
                                      target.detach().contiguous(), conf.detach().contiguous(), check_sigma(sigma))
    return (e, dict(zip(KEYS, (jts, proj, d2, status)))) if return_details else e
