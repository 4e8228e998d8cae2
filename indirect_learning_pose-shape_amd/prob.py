"""A probabilistic head: independent Gaussians over the regressor's D-vector, as "Probabilistic 3D Human Shape and Pose
Estimation from Multiple Unconstrained Images in the Wild" predicts them - reparameterised samples, the negative
log-likelihood, the product of the Gaussians of several images of one person, and the statistics of sampled meshes.  Beyond
the reference, whose regressor gives a point estimate.

    net = SMPLRegressor(48, "enet", True, probabilistic=True)      # net(images) -> (B, 86); net.mean, net.log_var (B, D)
    eps = torch.randn((B, S, D), generator=g, device=dev)          # the caller draws: the kernels hold no random numbers
    x = gaussian_samples(net.mean, net.log_var, eps, stochastic=mask, mean_first=True)              # (B, S, D)
    verts = layer(x.view(B * S, D))                                # a row's samples are consecutive rows of the decoder
    mean, rms = sample_spread(verts, S)                            # (B, V, 3), (B, V): the per-vertex uncertainty map
    nll = gaussian_nll(net.mean, net.log_var, truth_x, groups)     # (B, G)
    mu_f, s_f = fuse_gaussians(mu, s, group_size=G)                # (B / G, D): G images of one person

Definitions.  s is a log-variance, sigma = exp(s / 2); D is the width of the space the regressor works in (1 <= D <= 256).
  Samples   mu, s (B, D), eps (B, S, D), stochastic (D,) flags or None (all ones).  Entry (b, i, d) is DRAWN iff stochastic[d]
            != 0 and not (mean_first and i == 0): x = fl32(mu + sigma eps).  Every other entry is a bit copy of mu, and its eps
            is never read.  Gradient: dmu[b, d] = sum_i g[b, i, d], ds[b, d] = sigma / 2 sum_{i drawn} g eps, both sums in
            increasing i; ds is exactly 0 for a column that is not stochastic; eps gets none.
            Status NONFINITE: a mu or s of the row or a drawn eps is NaN / Inf, or a sample is not finite after rounding
            (sigma overflowed): all of the row's samples and both of its gradient rows are NaN, other rows untouched.
  NLL       groups (D,) ids in -1 .. G - 1 (-1: the column does not count), G <= 8; row_w (B, G) or None (ones): group k of
            row b counts iff row_w[b, k] > 0 (a select: a term that does not count is 0 and gives no gradient whatever its
            operands hold).  nll[b, k] = w_k / (2 n_k) sum_{d: groups[d] = k} (s_d + (t_d - mu_d)^2 exp(-s_d)), n_k the group's
            column count, the sum in increasing d, log 2 pi left out as `prior_energy` leaves it out; an empty group gives 0.
            G is row_w's width, or the largest id + 1.  target gets no gradient.
            Status NONFINITE: an operand of a counted group is NaN / Inf or a counted term is not finite in fp32: the row's
            nll and gradients are NaN.
  Fusion    G = group_size consecutive rows (1 <= G <= 16, B % G == 0) -> (B / G, D): m = min_i s_i, p_i = exp(-(s_i - m)),
            mu_f = sum mu_i p_i / sum p_i, s_f = m - log sum p_i in increasing i - the precision-weighted mean; the shift by m
            keeps log-variances of +-200 in one group from overflowing or losing the small terms.  G = 1: bit copies.  A NaN /
            Inf operand: that column's outputs are NaN and the group's status is set.  No graph.
  Spread    points (B S, N, 3), a row's S samples consecutive -> mean (B, N, 3) = 1 / S sum_i p_i, rms (B, N) =
            sqrt(max(0, 1 / S sum_i |p_i - mean|^2)), computed in one pass from the sums shifted by the row's sample 0.
            S = 1: rms exactly 0, mean a bit copy.  A NaN / Inf coordinate: that point's outputs are NaN, the row's status
            set.  No graph.  (The paper's mean DISTANCE to the sample mean needs a second pass over memory and is left out.)
  Rounding  all arithmetic in fp64 on the fp32 operands; every output is rounded to fp32 once; no atomics; a row's bits never
            depend on B or on other rows.
Device tensors only (csrc/prob.hip, one kernel launch per call); a CPU tensor raises, like the rest of the package; a tensor on
the meta device gives the outputs' shapes through the torch ops' Meta kernels.  `stochastic` and `groups` are host data (a
list, an array or a CPU tensor: a device tensor is copied to the host, which synchronises).  The `*_torch` functions are the
same definitions in plain torch at the inputs' dtype on any device: what a user would otherwise compose, and what
tools/prob_time.py times the kernels against.
"""
from __future__ import annotations

import ctypes

import torch

from . import _lib
from ._lib import check, ptr, stream
from .rot6d import _rows32
from .supervised import _on_hip

NONFINITE = 1            # SMPLR_PROB_NONFINITE
MAX_D = 256              # SMPLR_PROB_MAX_D
MAX_GROUPS = 8
MAX_FUSE = 16


# ---- arguments ----------------------------------------------------------------------------------------------------------
def _ints(v, D, name):
    """A column table as a tuple of D Python ints (host data)."""
    if isinstance(v, torch.Tensor):
        v = v.detach().reshape(-1).cpu().tolist()
    v = tuple(int(i) for i in v)
    if len(v) != D:
        raise ValueError("%s must hold D = %d entries, got %d" % (name, D, len(v)))
    return v


def _mask(stochastic, D):
    return None if stochastic is None else tuple(int(i != 0) for i in _ints(stochastic, D, "stochastic"))


def _mu_s(mu, s):
    if not isinstance(mu, torch.Tensor) or mu.dim() != 2 or not 1 <= mu.shape[1] <= MAX_D:
        raise ValueError("mu must be a (B, D) tensor with 1 <= D <= %d" % MAX_D)
    if not isinstance(s, torch.Tensor) or s.shape != mu.shape:
        raise ValueError("s must have mu's shape %s" % (tuple(mu.shape),))
    if s.device != mu.device:
        raise RuntimeError("s lives on %s, mu on %s" % (s.device, mu.device))
    return int(mu.shape[0]), int(mu.shape[1])


def _sample_args(mu, s, eps, stochastic):
    B, D = _mu_s(mu, s)
    if not isinstance(eps, torch.Tensor) or eps.dim() != 3 or eps.shape[0] != B or eps.shape[2] != D or eps.shape[1] < 1:
        raise ValueError("eps must be a (B, S, D) = (%d, S >= 1, %d) tensor" % (B, D))
    if eps.device != mu.device:
        raise RuntimeError("eps lives on %s, mu on %s" % (eps.device, mu.device))
    return B, int(eps.shape[1]), D, _mask(stochastic, D)


def _nll_args(mu, s, target, groups, row_w):
    B, D = _mu_s(mu, s)
    if not isinstance(target, torch.Tensor) or target.shape != mu.shape:
        raise ValueError("target must have mu's shape %s" % (tuple(mu.shape),))
    groups = _ints(groups, D, "groups")
    G = int(row_w.shape[1]) if row_w is not None and row_w.dim() == 2 else max(max(groups) + 1, 1)
    if not 1 <= G <= MAX_GROUPS or min(groups) < -1 or max(groups) >= G:
        raise ValueError("group ids must lie in -1 .. G - 1 with G = %d in 1 .. %d" % (G, MAX_GROUPS))
    if row_w is not None and tuple(row_w.shape) != (B, G):
        raise ValueError("row_w must be a (B, G) = (%d, %d) tensor" % (B, G))
    for name, t in (("target", target), ("row_w", row_w)):
        if t is not None and t.device != mu.device:
            raise RuntimeError("%s lives on %s, mu on %s" % (name, t.device, mu.device))
    return B, D, G, groups


def _fuse_args(mu, s, group_size):
    B, D = _mu_s(mu, s)
    G = int(group_size)
    if not 1 <= G <= MAX_FUSE or B % G:
        raise ValueError("group_size = %d must lie in 1 .. %d and divide B = %d" % (G, MAX_FUSE, B))
    return B, D, G


def _spread_args(points, S):
    S = int(S)
    if not isinstance(points, torch.Tensor) or points.dim() != 3 or points.shape[2] != 3 or points.shape[1] < 1:
        raise ValueError("points must be a (B S, N, 3) tensor with N >= 1")
    if S < 1 or points.shape[0] % S:
        raise ValueError("S = %d must be positive and divide the %d rows of points" % (S, points.shape[0]))
    return int(points.shape[0]) // S, S, int(points.shape[1])


def _stride(t):
    return int(t.stride(0)) if t.shape[0] > 1 else int(t.shape[1])


def _host(values, ctype):
    return None if values is None else (ctype * len(values))(*values)


# ---- the definitions in plain torch -----------------------------------------------------------------------------------------
def gaussian_samples_torch(mu, s, eps, stochastic=None, mean_first=False):
    """The module's samples in plain torch at mu's dtype, on any device -> x (B, S, D), differentiable in mu and s by
    autograd.  No status: a non-finite operand simply spreads over what it touches."""
    B, S, D, mask = _sample_args(mu, s, eps, stochastic)
    drawn = torch.ones((S, D), dtype=torch.bool, device=mu.device)
    if mask is not None:
        drawn &= torch.tensor(mask, dtype=torch.bool, device=mu.device)
    if mean_first:
        drawn[0] = False
    e = torch.where(drawn, eps.to(mu.dtype), torch.zeros((), dtype=mu.dtype, device=mu.device))     # (a select: no 0 * NaN)
    m = mu[:, None, :].expand(B, S, D)
    return torch.where(drawn, m + torch.exp(0.5 * s)[:, None, :] * e, m)


def gaussian_nll_torch(mu, s, target, groups, row_w=None):
    """The module's likelihood in plain torch at mu's dtype, on any device -> nll (B, G), differentiable in mu and s."""
    B, D, G, groups = _nll_args(mu, s, target, groups, row_w)
    dt, dev = mu.dtype, mu.device
    zero = torch.zeros((), dtype=dt, device=dev)
    gid = torch.tensor(groups, dtype=torch.int64, device=dev)
    on = torch.ones((B, G), dtype=torch.bool, device=dev) if row_w is None else row_w > 0
    w = torch.ones((B, G), dtype=dt, device=dev) if row_w is None else torch.where(on, row_w.to(dt), zero)
    col_on = on[:, gid.clamp(min=0)] & (gid >= 0)                                 # (B, D)
    r = torch.where(col_on, target.detach().to(dt) - mu, zero)
    sv = torch.where(col_on, s, zero)
    term = torch.where(col_on, sv + r * r * torch.exp(-sv), zero)
    out = []
    for k in range(G):
        cols = [d for d in range(D) if groups[d] == k]
        out.append(w[:, k] * (0.5 / len(cols)) * term[:, cols].sum(1) if cols else torch.zeros((B,), dtype=dt, device=dev))
    return torch.stack(out, 1)


def fuse_gaussians_torch(mu, s, group_size):
    """The module's fusion in plain torch at mu's dtype, on any device -> (mu_f, s_f), each (B / G, D)."""
    B, D, G = _fuse_args(mu, s, group_size)
    m3, s3 = mu.reshape(B // G, G, D), s.reshape(B // G, G, D)
    m = s3.min(1, keepdim=True).values
    p = torch.exp(-(s3 - m))
    den = p.sum(1)
    return (m3 * p).sum(1) / den, m[:, 0] - torch.log(den)


def sample_spread_torch(points, S):
    """The module's statistics in plain torch at points' dtype, on any device -> (mean (B, N, 3), rms (B, N)): a mean, a
    difference and a reduction - three passes over the samples."""
    B, S, N = _spread_args(points, S)
    p = points.reshape(B, S, N, 3)
    mean = p.mean(1)
    return mean, (p - mean[:, None]).square().sum(-1).mean(1).sqrt()


# ---- the kernels ------------------------------------------------------------------------------------------------------------
class _SamplesFn(torch.autograd.Function):
    """mu, s -> x, status: smplr_prob_sample_fwd forward, smplr_prob_sample_bwd backward."""

    @staticmethod
    def forward(ctx, mu, s, eps, mask, mean_first):
        ctx.set_materialize_grads(False)
        B, S, D = (int(v) for v in eps.shape)
        x = torch.empty((B, S, D), dtype=torch.float32, device=mu.device)
        status = torch.empty((B,), dtype=torch.int32, device=mu.device)
        check(_lib.load().smplr_prob_sample_fwd(ptr(mu), _stride(mu), ptr(s), _stride(s), ptr(eps), _host(mask, ctypes.c_uint8),
                                                int(mean_first), B, S, D, ptr(x), ptr(status), stream()), "smplr_prob_sample_fwd")
        ctx.args = (mask, bool(mean_first), B, S, D)
        ctx.save_for_backward(s, eps, status)
        ctx.mark_non_differentiable(status)
        return x, status

    @staticmethod
    def backward(ctx, g, *_):
        s, eps, status = ctx.saved_tensors
        mask, mean_first, B, S, D = ctx.args
        if g is None or not (ctx.needs_input_grad[0] or ctx.needs_input_grad[1]):
            return (None,) * 5
        g = g.to(torch.float32).contiguous()
        dmu = torch.empty((B, D), dtype=torch.float32, device=s.device)
        ds = torch.empty((B, D), dtype=torch.float32, device=s.device)
        with torch.cuda.device(s.device):
            check(_lib.load().smplr_prob_sample_bwd(ptr(s), _stride(s), ptr(eps), _host(mask, ctypes.c_uint8), int(mean_first),
                                                    ptr(status), ptr(g), B, S, D, ptr(dmu), ptr(ds), stream()),
                  "smplr_prob_sample_bwd")
        return dmu if ctx.needs_input_grad[0] else None, ds if ctx.needs_input_grad[1] else None, None, None, None


class _NllFn(torch.autograd.Function):
    """mu, s -> nll, status: smplr_prob_nll_fwd forward, smplr_prob_nll_bwd backward."""

    @staticmethod
    def forward(ctx, mu, s, target, groups, G, row_w):
        ctx.set_materialize_grads(False)
        B, D = int(mu.shape[0]), int(mu.shape[1])
        nll = torch.empty((B, G), dtype=torch.float32, device=mu.device)
        status = torch.empty((B,), dtype=torch.int32, device=mu.device)
        check(_lib.load().smplr_prob_nll_fwd(ptr(mu), _stride(mu), ptr(s), _stride(s), ptr(target), _stride(target),
                                             _host(groups, ctypes.c_int8), ptr(row_w), B, D, G, ptr(nll), ptr(status), stream()),
              "smplr_prob_nll_fwd")
        ctx.args = (groups, G, B, D)
        ctx.save_for_backward(mu, s, target, row_w, status)
        ctx.mark_non_differentiable(status)
        return nll, status

    @staticmethod
    def backward(ctx, g, *_):
        mu, s, target, row_w, status = ctx.saved_tensors
        groups, G, B, D = ctx.args
        if g is None or not (ctx.needs_input_grad[0] or ctx.needs_input_grad[1]):
            return (None,) * 6
        g = g.to(torch.float32).contiguous()
        dmu = torch.empty((B, D), dtype=torch.float32, device=mu.device)
        ds = torch.empty((B, D), dtype=torch.float32, device=mu.device)
        with torch.cuda.device(mu.device):
            check(_lib.load().smplr_prob_nll_bwd(ptr(mu), _stride(mu), ptr(s), _stride(s), ptr(target), _stride(target),
                                                 _host(groups, ctypes.c_int8), ptr(row_w), ptr(status), ptr(g), B, D, G, ptr(dmu),
                                                 ptr(ds), stream()), "smplr_prob_nll_bwd")
        return dmu if ctx.needs_input_grad[0] else None, ds if ctx.needs_input_grad[1] else None, None, None, None, None


@_lib.on_device
def _samples(mu, s, eps, mask, mean_first):
    return _SamplesFn.apply(mu, s, eps, mask, mean_first)


@_lib.on_device
def _nll(mu, s, target, groups, G, row_w):
    return _NllFn.apply(mu, s, target, groups, G, row_w)


@_lib.on_device
def _fuse(mu, s, B, D, G):
    mu_f = torch.empty((B // G, D), dtype=torch.float32, device=mu.device)
    s_f = torch.empty((B // G, D), dtype=torch.float32, device=mu.device)
    status = torch.empty((B // G,), dtype=torch.int32, device=mu.device)
    check(_lib.load().smplr_prob_fuse(ptr(mu), _stride(mu), ptr(s), _stride(s), B, D, G, ptr(mu_f), ptr(s_f), ptr(status), stream()),
          "smplr_prob_fuse")
    return mu_f, s_f, status


@_lib.on_device
def _spread(points, B, S, N):
    mean = torch.empty((B, N, 3), dtype=torch.float32, device=points.device)
    rms = torch.empty((B, N), dtype=torch.float32, device=points.device)
    status = torch.empty((B,), dtype=torch.int32, device=points.device)
    check(_lib.load().smplr_prob_spread(ptr(points), B, S, N, ptr(mean), ptr(rms), ptr(status), stream()), "smplr_prob_spread")
    return mean, rms, status


def _meta(*ts):
    return any(t is not None and t.device.type == "meta" for t in ts)


def _ns():
    from . import torch_ops
    return torch_ops.load()


def gaussian_samples(mu, s, eps, stochastic=None, mean_first=False, return_status=False):
    """mu, s (B, D), eps (B, S, D) fp32 on one HIP device, stochastic (D,) flags or None -> x (B, S, D) fp32, contiguous (so
    x.view(B * S, D) is the decoder's input with a row's samples consecutive), differentiable in mu and s; with
    return_status=True also status (B,) int32.  See the module's definitions."""
    B, S, D, mask = _sample_args(mu, s, eps, stochastic)
    if _meta(mu, s, eps):
        x, status = _ns().prob_sample_fwd(mu, s, eps, None if mask is None else list(mask), bool(mean_first))
    else:
        mu, s = _rows32(_on_hip(mu, "mu")), _rows32(_on_hip(s, "s"))
        x, status = _samples(mu, s, _on_hip(eps.detach(), "eps").contiguous(), mask, bool(mean_first))
    return (x, status) if return_status else x


def gaussian_nll(mu, s, target, groups, row_w=None, return_status=False):
    """mu, s, target (B, D) fp32 on one HIP device, groups (D,) ids in -1 .. G - 1, row_w (B, G) or None -> nll (B, G) fp32,
    differentiable in mu and s; with return_status=True also status (B,) int32.  See the module's definitions."""
    B, D, G, groups = _nll_args(mu, s, target, groups, row_w)
    if _meta(mu, s, target, row_w):
        nll, status = _ns().prob_nll_fwd(mu, s, target, list(groups), G, row_w)
    else:
        mu, s, target = _rows32(_on_hip(mu, "mu")), _rows32(_on_hip(s, "s")), _rows32(_on_hip(target.detach(), "target"))
        if row_w is not None:
            row_w = _lib.require_cuda(row_w.detach(), "row_w")
        nll, status = _nll(mu, s, target, groups, G, row_w)
    return (nll, status) if return_status else nll


@torch.no_grad()
def fuse_gaussians(mu, s, group_size, return_status=False):
    """mu, s (B, D) fp32 on one HIP device -> (mu_f, s_f), each (B / group_size, D) fp32: the product of each group's
    Gaussians per column, no graph; with return_status=True also status (B / group_size,) int32."""
    B, D, G = _fuse_args(mu, s, group_size)
    if _meta(mu, s):
        mu_f, s_f, status = _ns().prob_fuse(mu, s, G)
    else:
        mu_f, s_f, status = _fuse(_rows32(_on_hip(mu, "mu")), _rows32(_on_hip(s, "s")), B, D, G)
    return (mu_f, s_f, status) if return_status else (mu_f, s_f)


@torch.no_grad()
def fuse_shape(x, s, group_size, num_cam=4):
    """x (B, num_cam + 82) the decoder's vectors and s (B, D) the log-variances of the space they were regressed in, beta being
    the last 10 columns of both -> a copy of x in which every row's beta is its group's fused beta (`fuse_gaussians` over
    group_size consecutive rows): the start a grouped `refine_predictions` (group_size=, tie=shape) wants."""
    if not isinstance(x, torch.Tensor) or x.dim() != 2 or x.shape[1] != int(num_cam) + 82:
        raise ValueError("x must be a (B, num_cam + 82 = %d) tensor" % (int(num_cam) + 82))
    if not isinstance(s, torch.Tensor) or s.dim() != 2 or s.shape[0] != x.shape[0] or s.shape[1] < 10:
        raise ValueError("s must be (B, D >= 10) with x's rows")
    beta, _ = fuse_gaussians(x[:, -10:], s[:, -10:], group_size)
    out = x.clone()
    out[:, -10:] = beta.repeat_interleave(int(group_size), 0)
    return out


@torch.no_grad()
def sample_spread(points, S, return_status=False):
    """points (B S, N, 3) fp32 on a HIP device, a row's S samples consecutive (vertices, joints, any N >= 1) -> (mean
    (B, N, 3), rms (B, N)) fp32, no graph; with return_status=True also status (B,) int32.  One pass over points."""
    B, S, N = _spread_args(points, S)
    if _meta(points):
        mean, rms, status = _ns().prob_spread(points, S)
    else:
        mean, rms, status = _spread(_on_hip(points, "points").contiguous(), B, S, N)
    return (mean, rms, status) if return_status else (mean, rms)
