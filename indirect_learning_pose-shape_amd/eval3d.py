"""3D evaluation: how far a predicted point set (SMPL vertices, or joints) lies from the ground truth, in metres, before and
after removing what a single image cannot resolve.  The reference stops at a mean squared error over 69 pose parameters
(`evaluate3d.py:32-65`); these are the standard figures for SMPL regressors.

For each mesh the per-point Euclidean errors |a(p_i) - g_i| under four alignments a of pred to gt, and their means:
    0 none          a(p) = p                                                       (per-vertex error / MPJPE)
    1 translation   both sets minus their centroids, or minus their own point `root` (root-relative MPJPE)
    2 scale         centroids removed, then s pc with s = sum pc.gc / sum |pc|^2    (scale-corrected error)
    3 similarity    s R p + t, the least-squares similarity (Procrustes): M = sum gc pc^T = U S V^T, d = det(U) det(V),
                    R = U diag(1, 1, d) V^T, s = (S1 + S2 + d S3) / sum |pc|^2, t = mean(g) - s R mean(p)   (PA error)
Device tensors go through one HIP launch (csrc/eval3d.hip, smplr_point_errors); CPU tensors through the float64 torch
restatement below, so the API works without a GPU.  Coordinates are meant to stay within ~10 m of the origin: fp32
inputs further out have themselves lost the 1e-4 m the project holds vertices to.
"""
from __future__ import annotations

import torch
import torch.distributed as dist

from . import _lib
from ._lib import check, ptr, stream

MODES = ("none", "translation", "scale", "similarity")
DEGENERATE, NONFINITE, RANK_DEFICIENT = 1, 2, 4      # status bits (SMPLR_PE_* of include/smplraster.h)
RANK_TOL = 1e-5      # S2 <= RANK_TOL * S1: the second direction is within the fp32 inputs' rounding (PE_RANK_TOL of the kernel)


def _mode(m):
    if m is None:
        return None
    if isinstance(m, str):
        if m not in MODES:
            raise ValueError("mode %r is none of %s" % (m, MODES))
        return MODES.index(m)
    m = int(m)
    if not 0 <= m <= 3:
        raise ValueError("mode %d is not in 0..3 (%s)" % (m, ", ".join(MODES)))
    return m


def _check(pred, gt, root):
    if not isinstance(pred, torch.Tensor) or not isinstance(gt, torch.Tensor):
        raise TypeError("pred and gt must be torch tensors")
    if pred.dim() != 3 or pred.shape[2] != 3:
        raise RuntimeError("pred must be (B, N, 3), got %s" % (tuple(pred.shape),))
    if gt.shape != pred.shape:
        raise RuntimeError("gt %s does not have pred's shape %s" % (tuple(gt.shape), tuple(pred.shape)))
    if gt.device != pred.device:
        raise RuntimeError("gt lives on %s, pred on %s" % (gt.device, pred.device))
    N = pred.shape[1]
    if N < 1:
        raise RuntimeError("point sets must hold at least one point")
    root = -1 if root is None else int(root)
    if not -1 <= root < N:
        raise RuntimeError("root = %d outside [0, %d)" % (root, N))
    return root


@_lib.on_device
def _point_errors_hip(pred, gt, root, pp_mode, transform):
    pred = _lib.require_cuda(pred, "pred")
    gt = _lib.require_cuda(gt, "gt")
    B, N = pred.shape[:2]
    mean = torch.empty((B, 4), dtype=torch.float32, device=pred.device)
    status = torch.empty((B,), dtype=torch.int32, device=pred.device)
    pp = torch.empty((B, N), dtype=torch.float32, device=pred.device) if pp_mode is not None else None
    tr = torch.empty((B, 13), dtype=torch.float32, device=pred.device) if transform else None
    check(_lib.load().smplr_point_errors(ptr(pred), ptr(gt), B, N, root, pp_mode or 0, ptr(mean), ptr(tr), ptr(pp),
                                         ptr(status), stream()), "smplr_point_errors")
    return mean, status, pp, tr


def _point_errors_cpu(pred, gt, root, pp_mode, transform):
    """The four modes in float64 torch (batched torch.linalg.svd), with the kernel's treatment of degenerate input."""
    p, g = pred.detach().to(torch.float64), gt.detach().to(torch.float64)
    B, N = p.shape[:2]
    bad = ~(torch.isfinite(p).reshape(B, N * 3).all(1) & torch.isfinite(g).reshape(B, N * 3).all(1))
    p = torch.where(bad[:, None, None], torch.zeros_like(p), p)
    g = torch.where(bad[:, None, None], torch.zeros_like(g), g)
    mp, mg = p.mean(1, keepdim=True), g.mean(1, keepdim=True)
    pc, gc = p - mp, g - mg
    spp = pc.square().sum((1, 2))
    M = torch.einsum("bnr,bnc->brc", gc, pc)
    U, S, Vh = torch.linalg.svd(M)
    d = torch.where(torch.linalg.det(U) * torch.linalg.det(Vh) < 0, -1.0, 1.0).to(torch.float64)
    D = torch.ones(B, 3, dtype=torch.float64)
    D[:, 2] = d
    R = (U * D[:, None, :]) @ Vh
    degen = (spp <= 0) | (N == 1)
    safe = torch.where(degen, torch.ones_like(spp), spp)
    s2 = torch.where(degen, torch.ones_like(spp), torch.einsum("bii->b", M) / safe)
    s3 = torch.where(degen, torch.ones_like(spp), (S[:, 0] + S[:, 1] + d * S[:, 2]) / safe)
    R = torch.where(degen[:, None, None], torch.eye(3, dtype=torch.float64).expand(B, 3, 3), R)
    deficient = ~degen & ~(S[:, 1] > RANK_TOL * S[:, 0])
    if root >= 0:
        e1 = (p - p[:, root:root + 1]) - (g - g[:, root:root + 1])
    else:
        e1 = pc - gc
    errs = torch.stack([(p - g).norm(dim=2), e1.norm(dim=2), (s2[:, None, None] * pc - gc).norm(dim=2),
                        (s3[:, None, None] * (pc @ R.transpose(1, 2)) - gc).norm(dim=2)], 0)        # (4, B, N)
    nan = torch.full((), float("nan"), dtype=torch.float64)
    mean = torch.where(bad[:, None], nan, errs.mean(2).T).to(torch.float32)
    fin = torch.isfinite(mean).all(1)
    mean = torch.where(fin[:, None], mean, nan.to(torch.float32))
    status = (degen & ~bad).to(torch.int32) * DEGENERATE + (~fin).to(torch.int32) * NONFINITE \
        + (deficient & ~bad).to(torch.int32) * RANK_DEFICIENT
    pp = tr = None
    if pp_mode is not None:
        pp = torch.where(bad[:, None], nan, errs[pp_mode]).to(torch.float32)
    if transform:
        t = mg[:, 0] - s3[:, None] * (mp @ R.transpose(1, 2))[:, 0]
        tr = torch.where(bad[:, None], nan, torch.cat([s3[:, None], R.reshape(B, 9), t], 1)).to(torch.float32)
    return mean, status, pp, tr


def point_errors(pred, gt, root=None, per_point=None, transform=False):
    """pred, gt (B, N, 3) -> dict(mean_err (B, 4) fp32: the mean error of each mesh under the modes none / translation /
    scale / similarity; status (B,) int32: DEGENERATE | NONFINITE | RANK_DEFICIENT bits; per_point (B, N) when
    `per_point` names a mode (0..3 or its name); transform (B, 13) = s, R row-major, t of the similarity when `transform`).
    root: index of the point both sets are made relative to in mode 1 (None: their centroids)."""
    root = _check(pred, gt, root)
    pp_mode = _mode(per_point)
    if pred.is_cuda:
        mean, status, pp, tr = _point_errors_hip(pred.detach().float(), gt.detach().float(), root, pp_mode, bool(transform))
    else:
        mean, status, pp, tr = _point_errors_cpu(pred, gt, root, pp_mode, bool(transform))
    out = {"mean_err": mean, "status": status}
    if pp is not None:
        out["per_point"] = pp
    if tr is not None:
        out["transform"] = tr
    return out


class Eval3D:
    """Errors accumulated over any number of batches, in the mould of `SegConfusion`.

        m = Eval3D(device)
        m.update(pred_verts, gt_verts)          # (B, N, 3) each; no host synchronisation
        m.result()                              # {"none": ..., "translation": ..., "scale": ..., "similarity": ...} metres

    The state is six float64 numbers on the device: the four running sums of per-mesh mean errors, the meshes counted,
    and the meshes left out because they held a NaN / Inf (their means are NaN; they do not poison the sums)."""

    def __init__(self, device=None, keep_per_mesh=False):
        self.device = torch.device(device) if device is not None else torch.device("cpu")
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.state = torch.zeros(6, dtype=torch.float64, device=self.device)
        self.keep_per_mesh = bool(keep_per_mesh)
        self._per_mesh = []

    def reset(self):
        self.state.zero_()
        self._per_mesh = []
        return self

    def update(self, pred, gt, root=None):
        if pred.device != self.device:
            raise RuntimeError("pred lives on %s, the accumulator on %s" % (pred.device, self.device))
        mean = point_errors(pred, gt, root=root)["mean_err"]
        ok = torch.isfinite(mean).all(1)
        sums = torch.where(ok[:, None], mean, torch.zeros_like(mean)).to(torch.float64).sum(0)
        n_ok = ok.sum().to(torch.float64)
        self.state += torch.cat([sums, n_ok[None], (mean.shape[0] - n_ok)[None]])
        if self.keep_per_mesh:
            self._per_mesh.append(mean)
        return self

    def all_reduce(self, group=None):
        """Sum the state over the ranks of `group` (every rank ends with the same sums and counts)."""
        if dist.is_available() and dist.is_initialized():
            dist.all_reduce(self.state, op=dist.ReduceOp.SUM, group=group)
        return self

    def count(self):
        return int(self.state[4])

    def nonfinite(self):
        return int(self.state[5])

    def result(self):
        """Means in metres over the meshes counted (NaN when there are none), by mode name, + count and nonfinite."""
        st = self.state.cpu()
        n = float(st[4])
        out = {name: (float(st[i]) / n if n else float("nan")) for i, name in enumerate(MODES)}
        out["count"] = int(st[4])
        out["nonfinite"] = int(st[5])
        return out

    def per_mesh(self):
        """(meshes, 4) fp32 of every update so far, in order (needs keep_per_mesh=True)."""
        if not self.keep_per_mesh:
            raise RuntimeError("Eval3D(..., keep_per_mesh=True) keeps the per-mesh errors")
        if not self._per_mesh:
            return torch.empty((0, 4), dtype=torch.float32, device=self.device)
        return torch.cat(self._per_mesh, 0)
