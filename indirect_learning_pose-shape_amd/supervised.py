"""Supervised 3D losses, differentiable: squared errors on vertices, sparse 3D joints, pose as rotation matrices, shape and
camera against known truth, weighted by learned homoscedastic uncertainties - how "Synthetic Training for Accurate 3D Human
Pose and Shape Estimation" trains, with no image loss.  Beyond the reference, whose only loss goes through the rasteriser.

    batches = SyntheticBatches(smpl_path, 128, 256, 48, truth=True)
    images, labels, _, truth = next(batches)                       # truth: x, verts, J_transformed as the sampler made them
    verts = layer(x); jtr = layer.J_transformed
    terms = supervised_terms(x, verts, jtr, truth, spec=KeypointSpec.smpl_joints(), root=0)         # (B, 5) fp32
    loss = UncertaintyWeights().to(dev)(terms).mean()

Definitions, per row b (TERM_NAMES gives the order).
  Operands  x (B, num_cam + 82) fp32 = [cam | theta (72) | beta (10)], the decoder's layout (its rows may be strided); verts
            (B, V, 3); jtr = J_transformed (B, 24, 3), used exactly when `spec` was built with_joints; truth: a dict with the
            same three under "x", "verts", "J_transformed".  Nothing of truth gets a gradient.
  Weights   row_w (B, 5) or None (ones).  Term t of row b counts iff row_w[b, t] > 0 (a NaN does not count); a term that does
            not count is 0 and gives no gradient whatever its targets hold, NaN included (a select, the `conf` rule of the
            keypoint term).  A term that counts is multiplied by its weight.
  verts     T0 = w_0 / V sum_i |v_i - v*_i|^2
  joints3d  T1 = w_1 / K sum_k |(J_k - J_root) - (J*_k - J*_root)|^2, J = spec's sparse joints of (verts, jtr), J* the same of
            truth; root = -1: not relative.  spec None (or K = 0): T1 = 0.
  pose      T2 = w_2 / 24 sum_j |R(theta_j) - R(theta*_j)|_F^2 with the package's Rodrigues exactly as
            oracle/np_oracle.batch_rodrigues states it: a = |theta + 1e-8|, r = theta / a, R = cos a I + (1 - cos a) r r^T +
            sin a [r]x.  Rotation matrices, not parameters: theta and theta (1 + 2 pi / |theta|) are the same pose.
  shape     T3 = w_3 / 10 sum (beta - beta*)^2
  cam       T4 = w_4 / num_cam sum_c (cam_scale_c (x_c - x*_c))^2; cam_scale None: ones.
  Status    status (B,) int32 = NONFINITE (1) when an operand of a counted term is NaN / Inf (T1: a coordinate of a source a
            joint uses): the row's five terms and its gradients are NaN; other rows are untouched.
  Rounding  all products and sums in fp64 on the fp32 operands, in an order V, K and the spec alone fix - never B or other
            rows; every output is rounded to fp32 once.
Device tensors only (csrc/supervised.hip: one forward launch, smplr_sup_fwd, and one backward launch, smplr_sup_bwd; no
atomics, the same bits in every run and whatever else is in the batch); a CPU tensor raises, like the rest of the package.
`supervised_terms_torch` is the same definition in plain torch at the inputs' dtype: the composition a user would otherwise
write, and what tools/supervised_time.py times the kernels against.
"""
from __future__ import annotations

import torch
from torch import nn

from . import _lib
from ._lib import check, ptr, stream
from ._mesh_common import check_verts
from .keypoints import NUM_POSED, KeypointSpec

NONFINITE = 1            # SMPLR_SUP_NONFINITE
WS_DOUBLES = 408         # SMPLR_SUP_WS_DOUBLES
MAX_CAM = 8
TERM_NAMES = ("verts", "joints3d", "pose", "shape", "cam")


def rodrigues(theta):
    """theta (..., 3) -> R (..., 3, 3) at theta's dtype, as oracle/np_oracle.batch_rodrigues: a = |theta + 1e-8|,
    r = theta / a, R = cos a I + (1 - cos a) r r^T + sin a [r]x."""
    a = ((theta + 1e-8) ** 2).sum(-1, keepdim=True).sqrt()
    r = theta / a
    c, s = torch.cos(a)[..., None], torch.sin(a)[..., None]
    rx, ry, rz = r[..., 0], r[..., 1], r[..., 2]
    z = torch.zeros_like(rx)
    skew = torch.stack([z, -rz, ry, rz, z, -rx, -ry, rx, z], -1).reshape(r.shape[:-1] + (3, 3))
    eye = torch.eye(3, dtype=theta.dtype, device=theta.device)
    return c * eye + (1 - c) * (r[..., :, None] * r[..., None, :]) + s * skew


def _truth(truth, use_j):
    if not isinstance(truth, dict) or "x" not in truth or "verts" not in truth:
        raise ValueError("truth must be a dict holding \"x\" and \"verts\" (and \"J_transformed\" for a spec with joint sources)")
    jt = truth.get("J_transformed") if use_j else None
    if use_j and jt is None:
        raise ValueError("the spec uses joint sources: truth needs \"J_transformed\"")
    return truth["x"], truth["verts"], jt


def _check(x, verts, jtr, truth, spec, root, row_w, cam_scale, num_cam):
    """Shapes and devices of a call -> (x_t, verts_t, jtr, jtr_t, K, cam_scale) with jtr None unless the spec uses it."""
    if spec is not None and not isinstance(spec, KeypointSpec):
        raise TypeError("spec must be a KeypointSpec or None")
    check_verts(verts)
    num_cam = int(num_cam)
    if not 0 <= num_cam <= MAX_CAM:
        raise ValueError("num_cam must lie in 0 .. %d, got %d" % (MAX_CAM, num_cam))
    B, V, K = int(verts.shape[0]), int(verts.shape[1]), 0 if spec is None else spec.K
    if spec is not None and V != spec.num_verts:
        raise ValueError("verts have %d vertices, the spec %d" % (V, spec.num_verts))
    if int(root) != -1 and not 0 <= int(root) < K:
        raise ValueError("root must lie in -1 .. K - 1 = %d, got %r" % (K - 1, root))
    use_j = spec is not None and spec.with_joints
    if use_j and jtr is None:
        raise ValueError("the spec uses joint sources: jtr (J_transformed) is required")
    x_t, verts_t, jtr_t = _truth(truth, use_j)
    jtr = jtr if use_j else None
    shapes = [("x", x, (B, num_cam + 82)), ("truth[\"x\"]", x_t, (B, num_cam + 82)), ("truth[\"verts\"]", verts_t, (B, V, 3))]
    if use_j:
        shapes += [("jtr", jtr, (B, NUM_POSED, 3)), ("truth[\"J_transformed\"]", jtr_t, (B, NUM_POSED, 3))]
    if row_w is not None:
        shapes.append(("row_w", row_w, (B, 5)))
    for name, t, shape in shapes:
        if not isinstance(t, torch.Tensor) or tuple(t.shape) != shape:
            raise ValueError("%s must be a %s tensor" % (name, shape))
        if t.device != verts.device:
            raise RuntimeError("%s lives on %s, verts on %s" % (name, t.device, verts.device))
    if cam_scale is not None and not isinstance(cam_scale, torch.Tensor):
        cam_scale = torch.tensor([float(c) for c in cam_scale], dtype=torch.float32, device=verts.device)
    if cam_scale is not None and (cam_scale.numel() != num_cam or cam_scale.device != verts.device):
        raise ValueError("cam_scale must hold num_cam = %d numbers on verts' device" % num_cam)
    return x_t, verts_t, jtr, jtr_t, K, cam_scale


def supervised_terms_torch(x, verts, jtr, truth, spec=None, root=-1, row_w=None, cam_scale=None, num_cam=4):
    """The module's definitions in plain torch at the inputs' dtype, on any device -> terms (B, 5): a dense einsum for the
    joints and a few dozen element-wise launches; differentiable in x, verts and jtr by autograd.  No status: a non-finite
    operand of a counted term simply spreads."""
    x_t, verts_t, jtr, jtr_t, K, cam_scale = _check(x, verts, jtr, truth, spec, root, row_w, cam_scale, num_cam)
    dt, dev, nc = verts.dtype, verts.device, int(num_cam)
    B, V = int(verts.shape[0]), int(verts.shape[1])
    x_t, verts_t = x_t.detach().to(dt), verts_t.detach().to(dt)
    zero = torch.zeros((), dtype=dt, device=dev)
    if row_w is None:
        on, wt = torch.ones((B, 5), dtype=torch.bool, device=dev), torch.ones((B, 5), dtype=dt, device=dev)
    else:
        on = row_w > 0
        wt = torch.where(on, row_w.to(dt), zero)
    sel = lambda t, d: torch.where(on[:, t].reshape((B,) + (1,) * (d.dim() - 1)), d, zero)      # (a select: no 0 * NaN)
    t0 = sel(0, verts - verts_t).square().sum((1, 2)) / V
    if K:
        src = verts if jtr is None else torch.cat([verts, jtr], 1)
        src_t = verts_t if jtr is None else torch.cat([verts_t, jtr_t.detach().to(dt)], 1)
        R = spec.on(dev)["dense"].to(dt)
        d = torch.einsum("ks,bsc->bkc", R, sel(1, src - src_t))
        if int(root) >= 0:
            d = d - d[:, int(root), None]
        t1 = d.square().sum((1, 2)) / K
    else:
        t1 = torch.zeros((B,), dtype=dt, device=dev)
    th, th_t = x[:, nc:nc + 72].reshape(B, 24, 3), x_t[:, nc:nc + 72].reshape(B, 24, 3)
    t2 = sel(2, rodrigues(th) - rodrigues(th_t)).square().sum((1, 2, 3)) / 24
    t3 = sel(3, x[:, nc + 72:nc + 82] - x_t[:, nc + 72:nc + 82]).square().sum(1) / 10
    if nc:
        cs = torch.ones((nc,), dtype=dt, device=dev) if cam_scale is None else cam_scale.to(dt)
        t4 = sel(4, cs * (x[:, :nc] - x_t[:, :nc])).square().sum(1) / nc
    else:
        t4 = torch.zeros((B,), dtype=dt, device=dev)
    return wt * torch.stack([t0, t1, t2, t3, t4], 1)


def _rows(x):
    """x (B, C) with unit column stride and rows at least C apart, as it is; anything else contiguous."""
    if x.dim() == 2 and x.stride(1) == 1 and (x.shape[0] <= 1 or x.stride(0) >= x.shape[1]):
        return x
    return x.contiguous()


def _on_hip(t, name):
    """`_lib.require_cuda` without its copy: a strided x stays where it is."""
    if not t.is_cuda:
        raise RuntimeError("%s must live on a HIP device (got %s); this framework has no CPU path" % (name, t.device))
    if t.dtype != torch.float32:
        raise RuntimeError("%s must be torch.float32 (got %s)" % (name, t.dtype))
    return t


class _SupervisedFn(torch.autograd.Function):
    """x, verts, jtr (or None) -> terms, status: smplr_sup_fwd forward, smplr_sup_bwd backward."""

    @staticmethod
    def forward(ctx, x, verts, jtr, x_t, verts_t, jtr_t, spec, root, row_w, cam_scale, num_cam):
        ctx.set_materialize_grads(False)
        dev = verts.device
        B, V = int(verts.shape[0]), int(verts.shape[1])
        K, nnz = (0, 0) if spec is None else (spec.K, spec.nnz)
        d = None if spec is None else spec.on(dev)
        stride = int(x.stride(0)) if B > 1 else int(x.shape[1])
        terms = torch.empty((B, 5), dtype=torch.float32, device=dev)
        status = torch.empty((B,), dtype=torch.int32, device=dev)
        ws = torch.empty((B, WS_DOUBLES), dtype=torch.float64, device=dev)
        csr = (ptr(d["off"]), ptr(d["idx"]), ptr(d["w"])) if nnz else (None, None, None)
        check(_lib.load().smplr_sup_fwd(ptr(x), ptr(x_t), stride, ptr(verts), ptr(verts_t), ptr(jtr), ptr(jtr_t), *csr, root,
                                        ptr(row_w), ptr(cam_scale), B, V, K, nnz, num_cam, ptr(terms), ptr(status), ptr(ws),
                                        stream()), "smplr_sup_fwd")
        ctx.dims = (B, V, K, nnz, stride, root, num_cam)
        ctx.spec, ctx.has_jtr = spec, jtr is not None
        ctx.save_for_backward(x, x_t, verts, verts_t, row_w, cam_scale, status, ws)
        ctx.mark_non_differentiable(status)
        return terms, status

    @staticmethod
    def backward(ctx, g, *_):
        x, x_t, verts, verts_t, row_w, cam_scale, status, ws = ctx.saved_tensors
        B, V, K, nnz, stride, root, num_cam = ctx.dims
        need_x, need_v, need_j = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.has_jtr and ctx.needs_input_grad[2]
        if g is None or not (need_x or need_v or need_j):
            return (None,) * 11
        g = g.to(torch.float32).contiguous()
        dev = verts.device
        d = None if ctx.spec is None else ctx.spec.on(dev)
        dverts = torch.empty((B, V, 3), dtype=torch.float32, device=dev)
        # (the transposed CSR of a spec with joint sources has V + 24 rows: djtr goes with it)
        djtr = torch.empty((B, NUM_POSED, 3), dtype=torch.float32, device=dev) if ctx.has_jtr else None
        dx = torch.empty((B, stride), dtype=torch.float32, device=dev)
        csr = (ptr(d["t_off"]), ptr(d["t_joint"]), ptr(d["t_w"])) if nnz else (None, None, None)
        with torch.cuda.device(dev):
            check(_lib.load().smplr_sup_bwd(ptr(x), ptr(x_t), stride, ptr(verts), ptr(verts_t), *csr, root, ptr(row_w),
                                            ptr(cam_scale), ptr(status), ptr(ws), ptr(g), B, V, K, nnz, num_cam, ptr(dverts),
                                            ptr(djtr), ptr(dx), stream()), "smplr_sup_bwd")
        return (dx[:, :x.shape[1]] if need_x else None, dverts if need_v else None, djtr if need_j else None) + (None,) * 8


@_lib.on_device
def _apply(x, verts, jtr, x_t, verts_t, jtr_t, spec, root, row_w, cam_scale, num_cam):
    return _SupervisedFn.apply(x, verts, jtr, x_t, verts_t, jtr_t, spec, root, row_w, cam_scale, num_cam)


def supervised_terms(x, verts, jtr, truth, spec=None, root=-1, row_w=None, cam_scale=None, num_cam=4, return_status=False):
    """x (B, num_cam + 82), verts (B, V, 3), jtr = J_transformed (B, 24, 3) or None, truth = dict(x, verts[, J_transformed]),
    all fp32 on one HIP device; spec a `KeypointSpec` or None; root in -1 .. K - 1; row_w (B, 5) or None; cam_scale (num_cam)
    numbers or None -> terms (B, 5) fp32 in TERM_NAMES' order, differentiable in x, verts and jtr; with return_status=True
    also status (B,) int32.  See the module's definitions."""
    x_t, verts_t, jtr, jtr_t, K, cam_scale = _check(x, verts, jtr, truth, spec, root, row_w, cam_scale, num_cam)
    req = _lib.require_cuda
    verts, verts_t = req(verts, "verts"), req(verts_t.detach(), "truth[\"verts\"]")
    x, x_t = _rows(_on_hip(x, "x")), _rows(_on_hip(x_t.detach(), "truth[\"x\"]"))
    if x.shape[0] > 1 and x.stride(0) != x_t.stride(0):                   # (the launch takes one row stride for both)
        x, x_t = x.contiguous(), x_t.contiguous()
    if jtr is not None:
        jtr, jtr_t = req(jtr, "jtr"), req(jtr_t.detach(), "truth[\"J_transformed\"]")
    if row_w is not None:
        row_w = req(row_w.detach(), "row_w")
    if int(num_cam) and cam_scale is None:
        cam_scale = torch.ones((int(num_cam),), dtype=torch.float32, device=verts.device)
    elif cam_scale is not None:
        cam_scale = req(cam_scale.detach(), "cam_scale")
    terms, status = _apply(x, verts, jtr, x_t, verts_t, jtr_t, spec, int(root), row_w, cam_scale, int(num_cam))
    return (terms, status) if return_status else terms


class UncertaintyWeights(nn.Module):
    """Homoscedastic uncertainty weighting of the five terms: forward(terms (B, 5), row_w=None) -> (B,)
    sum_t [row_w_t > 0] (exp(-s_t) T_t + s_t), s the five learned log-variances (a parameter, initialised to 0).
    fixed=(w0, .., w4): constant weights instead, sum_t [row_w_t > 0] w_t T_t, and no parameters."""

    def __init__(self, fixed=None):
        super().__init__()
        if fixed is None:
            self.s = nn.Parameter(torch.zeros(5))
        else:
            w = [float(v) for v in fixed]
            if len(w) != 5:
                raise ValueError("fixed weights: one per term of %s" % (TERM_NAMES,))
            self.s = None
            self.register_buffer("w", torch.tensor(w, dtype=torch.float32))

    @property
    def learned(self):
        return self.s is not None

    def forward(self, terms, row_w=None):
        each = torch.exp(-self.s) * terms + self.s if self.s is not None else self.w * terms
        if row_w is not None:
            each = torch.where(row_w > 0, each, torch.zeros((), dtype=each.dtype, device=each.device))
        return each.sum(1)
