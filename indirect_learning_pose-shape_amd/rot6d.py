"""A 6D rotation pose head: the continuous representation of Zhou et al. ("On the Continuity of Rotation Representations in
Neural Networks") in front of the decoder, which keeps its (B, num_cam + 82) layout [cam | theta | beta].  A regressor that
puts out 24 x 6 numbers instead of 24 axis-angle vectors trains through a seam-free chart of SO(3): the decoder applies
Rodrigues to theta again, so the composite rot6d -> theta -> R is the Gram-Schmidt map itself.  Beyond the reference.

    y = regressor(images)                         # (B, 158) = [cam (4) | 24 x 6 | beta (10)]
    x, status = params_from_rot6d(y, return_status=True)          # (B, 86) for SMPLDecoder / supervised_terms, (B,) int32
    y0 = mean_rot6d_row(48)                       # the mean pose in this layout: an IEF start state, an initialisation
    a_true = axis_angle_to_rot6d(theta_true)      # truth given as axis-angle; rotation-matrix truth: its first two columns

Definitions.
  Operand   y (B, num_cam + 154) fp32 = [cam (num_cam) | a (24 x 6) | beta (10)], 0 <= num_cam <= 8; its rows may be strided,
            the last dimension is contiguous.
  Result    x (B, num_cam + 82) fp32 = [cam | theta (72) | beta], status (B,) int32; cam and beta are bit copies.
  Joint j   the six numbers are a 3 x 2 row-major matrix, a1 its first column and a2 its second:
            b1 = a1 / |a1|, u = a2 - (b1 . a2) b1, b2 = u / |u|, b3 = b1 x b2, R = [b1 b2 b3] as columns.
  Logarithm the unit quaternion (w, v) of R by the largest of the four diagonal candidates (trace, R00, R11, R22: Shepperd's
            method, ties to the lowest index), flipped so that w >= 0 (at w == 0 it stays as the candidate gives it);
            phi = 2 atan2(|v|, w) in [0, pi], theta_j = phi v / |v|; |v| == 0 gives exactly 0.
  Status    NONFINITE (1): one of the joint's six numbers is NaN / Inf - that joint's theta and its six gradients are NaN.
            DEGENERATE (2): not (|a1| >= 1e-6 and |u| >= 1e-6), the six being finite - that joint's theta is 0 and its six
            gradients are 0.  Other joints of the row and other rows are untouched; status[b] is the OR over the row's joints.
  Gradient  dy = [dcam copy | da | dbeta copy], da the exact derivative of the above (at phi = pi the one-sided one): with
            g = dL/dtheta, g_w = (I + [theta]x / 2 + c(phi) [theta]x^2) g, c = 1 / phi^2 - cot(phi / 2) / (2 phi) (-> 1 / 12 as
            phi -> 0, 1 / pi^2 at pi), dL/dR = [g_w]x R / 2, then the Gram-Schmidt backward.
  Rounding  all arithmetic in fp64 on the fp32 operands; every output is rounded to fp32 once; no atomics; a row's bits never
            depend on B or on other rows.
Device tensors only (csrc/rot6d.hip: one forward launch, smplr_rot6d_fwd, and one backward launch, smplr_rot6d_bwd, which
recomputes R and every joint's flags from y: no workspace); a CPU tensor raises, like the rest of the package.
`params_from_rot6d_torch` is the same definition in plain torch at the input's dtype: the composition a user would otherwise
write (a cat, a Gram-Schmidt, a matrix logarithm under autograd), and what tools/rot6d_time.py times the kernels against.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr, stream
from .supervised import _on_hip, _rows, rodrigues

NONFINITE = 1            # SMPLR_ROT6D_NONFINITE
DEGENERATE = 2           # SMPLR_ROT6D_DEGENERATE
MAX_CAM = 8
EPS = 1e-6


def _num_cam(y, num_cam, cols, name="y"):
    num_cam = int(num_cam)
    if not 0 <= num_cam <= MAX_CAM:
        raise ValueError("num_cam must lie in 0 .. %d, got %d" % (MAX_CAM, num_cam))
    if not isinstance(y, torch.Tensor) or y.dim() != 2 or y.shape[1] != num_cam + cols:
        raise ValueError("%s must be a (B, num_cam + %d = %d) tensor" % (name, cols, num_cam + cols))
    return num_cam


def _rows32(t):
    """`supervised._rows`, and contiguous as well when the row stride would not fit the launchers' int."""
    t = _rows(t)
    return t.contiguous() if t.shape[0] > 1 and t.stride(0) > 2 ** 31 - 1 else t


def rot6d_to_matrix(a):
    """a (..., 6), a 3 x 2 row-major matrix per rotation -> R (..., 3, 3) = [b1 b2 b3] as columns, by Gram-Schmidt; plain
    torch at a's dtype, no guards: a zero |a1| or |u| divides."""
    m = a.reshape(a.shape[:-1] + (3, 2))
    a1, a2 = m[..., 0], m[..., 1]
    b1 = a1 / a1.square().sum(-1, keepdim=True).sqrt()
    u = a2 - (b1 * a2).sum(-1, keepdim=True) * b1
    b2 = u / u.square().sum(-1, keepdim=True).sqrt()
    return torch.stack([b1, b2, torch.linalg.cross(b1, b2)], -1)


def axis_angle_to_rot6d(theta):
    """theta (..., 3) -> a (..., 6): the first two columns of the package's Rodrigues (`supervised.rodrigues`), flattened
    row-major as 3 x 2.  Plain torch at theta's dtype: for means, truth and initialisation."""
    R = rodrigues(theta)
    return R[..., :, :2].reshape(theta.shape[:-1] + (6,))


def _log_matrix(R):
    """The module's logarithm in plain torch: R (..., 3, 3) -> theta (..., 3).  Every candidate of Shepperd's method is
    evaluated on a guarded square root (a select keeps the others' NaN out of autograd)."""
    r = lambda i, j: R[..., i, j]
    tr = r(0, 0) + r(1, 1) + r(2, 2)
    k = torch.stack([tr, r(0, 0), r(1, 1), r(2, 2)], -1).argmax(-1)
    one = torch.ones((), dtype=R.dtype, device=R.device)
    root = lambda i, s: 0.5 * torch.where(k == i, 1.0 + s, one).sqrt()
    d = (r(2, 1) - r(1, 2), r(0, 2) - r(2, 0), r(1, 0) - r(0, 1))
    s = (r(1, 2) + r(2, 1), r(0, 2) + r(2, 0), r(0, 1) + r(1, 0))              # (yz, xz, xy)
    w = root(0, tr); f = 0.25 / w
    q0 = torch.stack([w, d[0] * f, d[1] * f, d[2] * f], -1)
    x = root(1, r(0, 0) - r(1, 1) - r(2, 2)); f = 0.25 / x
    q1 = torch.stack([d[0] * f, x, s[2] * f, s[1] * f], -1)
    y = root(2, r(1, 1) - r(0, 0) - r(2, 2)); f = 0.25 / y
    q2 = torch.stack([d[1] * f, s[2] * f, y, s[0] * f], -1)
    z = root(3, r(2, 2) - r(0, 0) - r(1, 1)); f = 0.25 / z
    q3 = torch.stack([d[2] * f, s[1] * f, s[0] * f, z], -1)
    kk = k[..., None]
    q = torch.where(kk == 0, q0, torch.where(kk == 1, q1, torch.where(kk == 2, q2, q3)))
    q = torch.where(q[..., :1] < 0, -q, q)
    w, v = q[..., :1], q[..., 1:]
    n2 = v.square().sum(-1, keepdim=True)
    tiny = n2 < 1e-20                                  # (phi / |v| -> 2 / w there, to 1e-21 relative; exactly 0 at v = 0)
    nv = torch.where(tiny, one, n2).sqrt()
    return torch.where(tiny, 2.0 / w, 2.0 * torch.atan2(nv, w) / nv) * v


def params_from_rot6d_torch(y, num_cam=4):
    """The module's definitions in plain torch at y's dtype, on any device: y (B, num_cam + 154) -> x (B, num_cam + 82),
    differentiable by autograd - a few hundred element-wise launches forward and backward.  No status: a degenerate joint
    gives theta = 0 and no gradient, a non-finite number simply spreads over its joint."""
    nc = _num_cam(y, num_cam, 154)
    B = int(y.shape[0])
    a = y[:, nc:nc + 144].reshape(B, 24, 6)
    m = a.reshape(B, 24, 3, 2)
    a1, a2 = m[..., 0], m[..., 1]
    n1 = a1.square().sum(-1, keepdim=True).sqrt()
    ok1 = n1 >= EPS
    b1 = a1 / torch.where(ok1, n1, torch.ones_like(n1))
    u = a2 - (b1 * a2).sum(-1, keepdim=True) * b1
    nu = u.square().sum(-1, keepdim=True).sqrt()
    ok = ok1 & (nu >= EPS)
    degenerate = ~ok & torch.isfinite(a).all(-1, keepdim=True)
    eye = torch.tensor([1.0, 0.0, 0.0, 1.0, 0.0, 0.0], dtype=y.dtype, device=y.device)
    theta = _log_matrix(rot6d_to_matrix(torch.where(degenerate, eye, a)))
    theta = torch.where(degenerate, torch.zeros((), dtype=y.dtype, device=y.device), theta)
    return torch.cat([y[:, :nc], theta.reshape(B, 72), y[:, nc + 144:]], 1)


class _Rot6dFn(torch.autograd.Function):
    """y -> x, status: smplr_rot6d_fwd forward, smplr_rot6d_bwd backward."""

    @staticmethod
    def forward(ctx, y, num_cam):
        ctx.set_materialize_grads(False)                   # (no zero fill for the status' cotangent)
        B = int(y.shape[0])
        stride = int(y.stride(0)) if B > 1 else int(y.shape[1])
        x = torch.empty((B, num_cam + 82), dtype=torch.float32, device=y.device)
        status = torch.empty((B,), dtype=torch.int32, device=y.device)
        check(_lib.load().smplr_rot6d_fwd(ptr(y), stride, B, num_cam, ptr(x), ptr(status), stream()), "smplr_rot6d_fwd")
        ctx.dims = (B, stride, num_cam)
        ctx.save_for_backward(y, status)
        ctx.mark_non_differentiable(status)
        return x, status

    @staticmethod
    def backward(ctx, dx, *_):
        y, status = ctx.saved_tensors
        B, stride, num_cam = ctx.dims
        if dx is None or not ctx.needs_input_grad[0]:
            return None, None
        dx = _rows32(dx.to(torch.float32))
        dstride = int(dx.stride(0)) if B > 1 else int(dx.shape[1])
        dy = torch.empty((B, num_cam + 154), dtype=torch.float32, device=y.device)
        with torch.cuda.device(y.device):
            check(_lib.load().smplr_rot6d_bwd(ptr(y), stride, ptr(status), ptr(dx), dstride, B, num_cam, ptr(dy), stream()),
                  "smplr_rot6d_bwd")
        return dy, None


@_lib.on_device
def _apply(y, num_cam):
    return _Rot6dFn.apply(y, num_cam)


def params_from_rot6d(y, num_cam=4, return_status=False):
    """y (B, num_cam + 154) fp32 on a HIP device = [cam | 24 x 6 | beta] -> x (B, num_cam + 82) fp32 = [cam | theta | beta],
    differentiable in y; with return_status=True also status (B,) int32.  See the module's definitions."""
    nc = _num_cam(y, num_cam, 154)
    x, status = _apply(_rows32(_on_hip(y, "y")), nc)
    return (x, status) if return_status else x


_mean_cache = {}


def mean_rot6d_row(img_wh, device=None):
    """`smpl_model.mean86(img_wh)` with its theta replaced by `axis_angle_to_rot6d` of it, computed in float64 on the host
    -> (1, 158) fp32 = [W/2, W/2, W/2, W/1.6 | 24 x 6 | mean shape] on `device` (default: the CPU), cached per width and
    device like `set_cam_params._row`."""
    from .smpl_model import mean86
    key = (float(img_wh), str(device))
    if key not in _mean_cache:
        row = mean86(img_wh)
        a = axis_angle_to_rot6d(torch.as_tensor(row[4:76].reshape(24, 3), dtype=torch.float64)).numpy().reshape(144)
        row = torch.as_tensor(np.concatenate([row[:4], a, row[76:]]), dtype=torch.float32)
        _mean_cache[key] = (row if device is None else row.to(device)).unsqueeze(0)
    return _mean_cache[key]
