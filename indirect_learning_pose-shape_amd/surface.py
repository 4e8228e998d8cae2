"""Dense surface correspondences, differentiable: observations that each name the mesh point they belong to - a face and three
barycentric weights - as a data term.  DensePose-style IUV pixels, mocap or registered-scan markers, and what the project's
own renderer (`render_mesh`'s face-id map) and `scan.sample_surface` produce.  Beyond the reference, which compares label
maps only.

    targets = SurfaceTargets(topo, face, bary, target, conf)        # once per target batch: sorts, builds the row CSRs
    e = surface_energy(verts, x[:, :4], targets, sigma=3.0)         # (B, N) fp32, image targets (D = 2)
    e, det = surface_energy(verts, None, targets3d, return_details=True)   # 3D targets; det: d2, point, status

Definitions.
  Topology  faces (F, 3) int32 of a `render.MeshTopology`, 1 <= F <= 2^24.
  Corresp.  correspondence n of row b: face[b, n] int32, bary[b, n, 3] fp32 (the weights need not sum to 1 or be
            non-negative), target[b, n, D] fp32, conf[b, n] fp32.  D = 2: image targets in the decoder's pixel frame; D = 3:
            3D targets in the mesh's frame.  1 <= N <= 65 536 per row; ragged rows are padded with face = -1.  A
            correspondence counts iff 0 <= face < F and conf > 0 (a NaN conf does not count); face >= F is refused on the host.
  Point     P[b, n] = sum_c bary[b, n, c] verts[b, faces[face, c]], as (b_0 x_0 + b_1 x_1) + b_2 x_2 per coordinate.
  Residual  D = 2: r = (u0 + k_u P_x - t_u, v0 + k_v P_y - t_v), cam[b] = (k_u, k_v, u0, v0), the convention of
            `orthographic_project`.  D = 3: r = P - t, cam is None.
  Energy    d2 = |r|^2 (r_u^2 + r_v^2, or (r_x^2 + r_y^2) + r_z^2); e = conf rho(d2) when the correspondence counts, with rho =
            `fitting.robust_rho` (Geman-McClure with sigma; sigma=None: rho(s) = s).  A correspondence that does not count has
            e = 0 exactly and no gradient whatever its weights and target hold (a select, not a product: a NaN target under
            conf = 0 is harmless); its d2 and point entries are 0 as well.
  Status    status (B,) int32 = NONFINITE (1) when a counted correspondence of the row uses a vertex coordinate, a weight or a
            target that is NaN / Inf, or (D = 2) a cam column is: that row's e, d2, point and gradient rows are NaN; other rows
            keep their bits.  A NaN that no counted correspondence touches does not matter.
  Gradient  with cotangent g (B, N) on e: q = g conf rho'(d2) 2 r, rho'(s) = sigma^4 / (sigma^2 + s)^2 (or 1); D = 2: dP =
            (q_u k_u, q_v k_v, 0), D = 3: dP = q; dverts[b, i] = sum over (n, c) with faces[face[b, n], c] = i of
            bary[b, n, c] dP[b, n], written for every vertex (exact zeros where nothing lands); D = 2: dcam = (sum q_u P_x,
            sum q_v P_y, sum q_u, sum q_v).  None for face, bary, target or conf.
  Rounding  all products and sums in fp64 on the fp32 inputs, in an order the launch geometry and the row's own data fix - never
            B or other rows; every output is rounded to fp32 once.
`SurfaceTargets` does the plumbing once per target batch, in stock torch on the data's device: a stable sort of each row by
face (padding last), the sorted copies, `order` (sorted position -> the caller's n) and c_off (B, F + 1), the row's CSR over
faces.  The vertex -> (face, corner) lists (`vertex_corners`) are the second index the backward walks: a face that repeats a
vertex must be summed once per corner, and `MeshTopology.vf_face` carries no corner.
Device tensors run csrc/surface.hip: one forward launch (smplr_sc_fwd) and one backward launch (smplr_sc_bwd), no atomics, the
same bits in every run and whatever else is in the batch; e, d2 and point stay in the caller's order.  CPU tensors run
`surface_energy_torch`, a float64 torch restatement; on device tensors that function is the stock composition the kernels are
timed against.
"""
from __future__ import annotations

import weakref

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr, stream
from ._mesh_common import check_topo, check_verts, nan_rows
from .keypoints import _drho, _rho, check_sigma

NONFINITE = 1          # SMPLR_SC_NONFINITE
MAX_N = 1 << 16
KEYS = ("d2", "point", "status")

_VC = weakref.WeakKeyDictionary()      # topology -> {"np": (off, face, corner), device: (vc_off, vc_fc)}


def vertex_corners(topo):
    """The vertex -> (face, corner) lists of a topology -> (off (V + 1), face (3 F), corner (3 F)) int32 numpy: vertex i is
    corner corner[k] of face face[k] for k in off[i] .. off[i + 1], faces increasing within a vertex and corners increasing
    within a face (a face that repeats a vertex appears once per corner).  Built once per topology."""
    check_topo(topo, ("faces", "num_verts", "num_faces"))
    d = _VC.setdefault(topo, {})
    if "np" not in d:
        flat = np.asarray(topo.faces, np.int64).reshape(-1)                 # (entry 3 f + c: corner c of face f)
        by_vertex = np.argsort(flat, kind="stable")                        # (stable: 3 f + c increasing within a vertex)
        off = np.concatenate([[0], np.cumsum(np.bincount(flat, minlength=topo.num_verts))]).astype(np.int32)
        d["np"] = (off, (by_vertex // 3).astype(np.int32), (by_vertex % 3).astype(np.int32))
    return d["np"]


def _vc_on(topo, device):
    """(vc_off (V + 1), vc_fc (3 F) = 4 face + corner) int32 on `device`, uploaded once per device."""
    off, face, corner = vertex_corners(topo)
    d = _VC[topo]
    if device not in d:
        d[device] = (torch.from_numpy(off).to(device), torch.from_numpy(face * 4 + corner).to(device))
    return d[device]


class SurfaceTargets:
    """One batch of dense correspondences against a topology: see the module's definitions.  face (B, N) integers, bary
    (B, N, 3), target (B, N, D) and conf (B, N) or None (ones) fp32, all on one device.  Everything is checked here, once -
    the kernels trust the arrays.  Attributes: topo, B, N, D, device; face, bary, target, conf (the caller's order); s_face,
    s_bary, s_target, s_conf (each row sorted by face, a stable sort, anything that is no face last), order (B, N) int32 (sorted
    position -> the caller's n), c_off (B, F + 1) int32 (c_off[b, f] = the row's entries on faces below f; c_off[b, F] = its
    entries on the mesh)."""

    def __init__(self, topo, face, bary, target, conf=None):
        check_topo(topo, ("faces", "num_verts", "num_faces", "on"))
        F = int(topo.num_faces)
        if F < 1:
            raise ValueError("the topology has no faces")
        if not isinstance(face, torch.Tensor) or face.dim() != 2 or face.is_floating_point() or face.dtype == torch.bool:
            raise ValueError("face must be a (B, N) integer tensor")
        B, N = int(face.shape[0]), int(face.shape[1])
        if N < 1 or N > MAX_N:
            raise ValueError("1 <= N <= %d correspondences per row, got N = %d" % (MAX_N, N))
        if not isinstance(target, torch.Tensor) or target.dim() != 3 or int(target.shape[2]) not in (2, 3):
            raise ValueError("target must be a (B, N, D) tensor with D = 2 (image) or 3 (3D)")
        D = int(target.shape[2])
        if conf is None:
            conf = torch.ones((B, N), dtype=torch.float32, device=face.device)
        for name, t, shape in (("bary", bary, (B, N, 3)), ("target", target, (B, N, D)), ("conf", conf, (B, N))):
            if not isinstance(t, torch.Tensor) or tuple(t.shape) != shape:
                raise ValueError("%s must be a %s tensor" % (name, shape))
            if t.dtype != torch.float32:
                raise RuntimeError("%s must be float32" % name)
            if t.device != face.device:
                raise RuntimeError("%s lives on %s, face on %s" % (name, t.device, face.device))
        if B and int(face.max()) >= F:
            raise ValueError("face indices must be below F = %d (padding: -1), found %d" % (F, int(face.max())))
        self.topo, self.B, self.N, self.D, self.device = topo, B, N, D, face.device
        self.face = face.detach().to(torch.int32).contiguous()
        self.bary, self.target, self.conf = (t.detach().contiguous() for t in (bary, target, conf))
        key = torch.where(self.face >= 0, self.face, torch.full_like(self.face, F)).long()
        order = torch.argsort(key, dim=1, stable=True)
        self.order = order.to(torch.int32).contiguous()
        self.s_face = self.face.gather(1, order).contiguous()
        self.s_bary = self.bary.gather(1, order[..., None].expand(-1, -1, 3)).contiguous()
        self.s_target = self.target.gather(1, order[..., None].expand(-1, -1, D)).contiguous()
        self.s_conf = self.conf.gather(1, order).contiguous()
        bounds = torch.arange(F + 1, device=face.device).expand(B, F + 1).contiguous()
        self.c_off = torch.searchsorted(key.gather(1, order).contiguous(), bounds).to(torch.int32).contiguous()
        self.faces = topo.on(face.device)["faces"]
        self.vc_off, self.vc_fc = _vc_on(topo, face.device) if face.is_cuda else (None, None)

    def counted(self):
        """(B, N) bool in the caller's order: the correspondences that count."""
        return (self.face >= 0) & (self.conf > 0)


# ---- correspondences from a face-id map --------------------------------------------------------------------------------------

def pixel_barycentrics(verts, faces, cam, face_map):
    """For every pixel of a face-id map (B, H, W) (an integer tensor; negative: background) the barycentric weights of the
    pixel centre in its face's projected triangle, in float64 stock torch on verts' device (CPU tensors too).  The pixel in
    row r, column j has its centre at (j, H - 1 - r) of the projection frame p = (u0 + k_u X, v0 + k_v Y), cam (B, 4) =
    (k_u, k_v, u0, v0): `render_mesh`'s ortho mode at scale 1.  -> (bary (B, H, W, 3) float64 with sum 1, zeros on the
    background and on a face whose projection has no area, centre (B, H, W, 2) float64)."""
    f64 = torch.float64
    fm = face_map.long()
    B, H, W = (int(s) for s in fm.shape)
    dev = verts.device
    faces = torch.as_tensor(np.asarray(faces) if not isinstance(faces, torch.Tensor) else faces).to(dev).long()
    c = cam.to(f64).reshape(B, 4)
    p = torch.stack([c[:, 2, None] + c[:, 0, None] * verts[..., 0].to(f64), c[:, 3, None] + c[:, 1, None] * verts[..., 1].to(f64)], -1)
    on = fm >= 0
    tri = faces[torch.where(on, fm, torch.zeros_like(fm))]                             # (B, H, W, 3) vertex ids
    pt = p[torch.arange(B, device=dev)[:, None, None, None], tri]                       # (B, H, W, 3, 2)
    a, b, cc = pt[..., 0, :], pt[..., 1, :], pt[..., 2, :]
    cols = torch.arange(W, dtype=f64, device=dev).expand(B, H, W)
    rows = (H - 1 - torch.arange(H, dtype=f64, device=dev))[None, :, None].expand(B, H, W)
    s = torch.stack([cols, rows], -1)

    def edge(u, v, w):                                                                  # (v - u) x (w - u)
        return (v[..., 0] - u[..., 0]) * (w[..., 1] - u[..., 1]) - (v[..., 1] - u[..., 1]) * (w[..., 0] - u[..., 0])
    area = edge(a, b, cc)
    ok = on & (area != 0) & torch.isfinite(area)
    den = torch.where(ok, area, torch.ones_like(area))
    w1, w2 = edge(a, s, cc) / den, edge(a, b, s) / den
    bary = torch.stack([1.0 - w1 - w2, w1, w2], -1)
    return torch.where(ok[..., None], bary, torch.zeros_like(bary)), s


def correspondences_from_render(verts, topo, cam, img_wh, max_n=None):
    """An IUV-like ground truth: `render_mesh(verts, topo, cam, img_wh=...)` (ortho, scale 1; HIP tensors), then
    `pixel_barycentrics` of its face-id map -> (face (B, N) int32, bary (B, N, 3) fp32, target (B, N, 2) fp32 = the pixel
    centres), the covered pixels of each image in raster order, padded with face = -1 to N = the largest count of the batch
    (at least 1; a host synchronisation).  max_n: rows with more covered pixels keep max_n of them, evenly spread over the
    raster order."""
    from .render import render_mesh
    fm = render_mesh(verts, topo, cam, img_wh=img_wh)["face"]
    B, H, W = (int(s) for s in fm.shape)
    bary, centre = pixel_barycentrics(verts, topo.on(verts.device)["faces"], torch.as_tensor(cam, device=verts.device).expand(B, 4), fm)
    keep = ((fm >= 0) & (bary != 0).any(-1)).reshape(B, H * W)
    count = keep.sum(1, keepdim=True)
    if max_n is not None:
        m = int(max_n)
        if m < 1 or m > MAX_N:
            raise ValueError("max_n must lie in 1 .. %d, got %r" % (MAX_N, max_n))
        rank = keep.cumsum(1) - 1
        spread = ((rank + 1) * m).div(count.clamp(min=1), rounding_mode="floor") > (rank * m).div(count.clamp(min=1), rounding_mode="floor")
        keep = keep & ((count <= m) | spread)
        count = keep.sum(1, keepdim=True)
    N = max(1, int(count.max())) if B else 1
    if N > MAX_N:
        raise ValueError("%d covered pixels in one image: pass max_n <= %d" % (N, MAX_N))
    first = torch.argsort((~keep).to(torch.int8), dim=1, stable=True)[:, :N]           # (the kept pixels first, in raster order)
    live = torch.arange(N, device=fm.device)[None, :] < count
    face = torch.where(live, fm.reshape(B, -1).gather(1, first), torch.full((), -1, dtype=fm.dtype, device=fm.device))
    b3 = bary.reshape(B, -1, 3).gather(1, first[..., None].expand(-1, -1, 3))
    t2 = centre.reshape(B, -1, 2).gather(1, first[..., None].expand(-1, -1, 2))
    zero = torch.zeros((), dtype=torch.float64, device=fm.device)
    return (face.to(torch.int32).contiguous(), torch.where(live[..., None], b3, zero).to(torch.float32).contiguous(),
            torch.where(live[..., None], t2, zero).to(torch.float32).contiguous())


# ---- the float64 torch restatement -----------------------------------------------------------------------------------------

def _tri(targets):
    """(counted (B, N) bool, tri (B, N, 3) int64 = the faces' vertex ids, face 0's where there is no face) in the caller's order."""
    return targets.counted(), targets.faces.long()[torch.where(targets.face >= 0, targets.face, torch.zeros_like(targets.face)).long()]


def _gather(verts, targets):
    """What the forward starts from, in the caller's order: counted (B, N), and the float64 weights, corner coordinates
    (B, N, 3 corners, 3) and targets with everything of a correspondence that does not count set to 0; fin (B, N): all of it
    finite."""
    f64 = torch.float64
    counted, tri = _tri(targets)
    zero = torch.zeros((), dtype=f64, device=verts.device)
    x = verts.to(f64)[torch.arange(targets.B, device=verts.device)[:, None, None], tri]
    w = targets.bary.to(f64)
    fin = torch.isfinite(x).all(-1).all(-1) & torch.isfinite(w).all(-1) & torch.isfinite(targets.target).all(-1)
    return (counted, torch.where(counted[..., None], w, zero), torch.where(counted[..., None, None], x, zero),
            torch.where(counted[..., None], targets.target.to(f64), zero), fin)


def surface_energy_torch(verts, cam, targets, sigma=None):
    """The definitions in float64 torch on any device (the CPU path, and the stock composition the kernels are timed
    against): a face gather, a (B, N, 3, 3) intermediate and element-wise launches; differentiable in verts and cam by
    autograd (on rows whose status is 0; the scatter of its backward adds in no fixed order on a device).  -> dict of e, d2
    (B, N), point (B, N, 3), ws (B, N, 4) = (P_x, P_y, r_u, r_v) or (r_x, r_y, r_z, 0), all float64 in the caller's order, and
    status (B,) int32."""
    s2 = check_sigma(sigma) ** 2
    f64 = torch.float64
    counted, w, x, t, fin = _gather(verts, targets)
    zero = torch.zeros((), dtype=f64, device=verts.device)
    P = (w[..., 0, None] * x[:, :, 0] + w[..., 1, None] * x[:, :, 1]) + w[..., 2, None] * x[:, :, 2]
    bad = (counted & ~fin).any(1)
    if targets.D == 2:
        c = cam.to(f64)
        r = torch.stack([(c[:, 2, None] + c[:, 0, None] * P[..., 0]) - t[..., 0], (c[:, 3, None] + c[:, 1, None] * P[..., 1]) - t[..., 1]], -1)
        d2 = r[..., 0] * r[..., 0] + r[..., 1] * r[..., 1]
        bad = bad | ~torch.isfinite(c).all(1)
        ws = torch.cat([P[..., :2], r], -1)
    else:
        r = P - t
        d2 = (r[..., 0] * r[..., 0] + r[..., 1] * r[..., 1]) + r[..., 2] * r[..., 2]
        ws = torch.cat([r, torch.zeros_like(r[..., :1])], -1)
    e = torch.where(counted, torch.where(counted, targets.conf.to(f64), zero) * _rho(d2, s2), zero)
    return {"e": nan_rows(bad, e), "d2": nan_rows(bad, torch.where(counted, d2, zero)),
            "point": nan_rows(bad, torch.where(counted[..., None], P, zero)), "ws": ws.detach(),
            "status": bad.to(torch.int32) * NONFINITE}


def _backward_torch(targets, cam, ws, status, g, s2, V):
    """The gradient definition in float64 torch (ws in the caller's order) -> (dverts (B, V, 3), dcam (B, 4) or None)
    float32, rounded once."""
    f64 = torch.float64
    B, N, D = targets.B, targets.N, targets.D
    counted, tri = _tri(targets)
    zero = torch.zeros((), dtype=f64, device=ws.device)
    w = torch.where(counted[..., None], targets.bary.to(f64), zero)
    r = ws[..., 2:4] if D == 2 else ws[..., :3]
    d2 = r[..., 0] * r[..., 0] + r[..., 1] * r[..., 1] if D == 2 else (r[..., 0] * r[..., 0] + r[..., 1] * r[..., 1]) + r[..., 2] * r[..., 2]
    c = g.to(f64) * targets.conf.to(f64) * _drho(d2, s2)
    q = torch.where(counted[..., None], c[..., None] * (2.0 * r), zero)
    dP = torch.cat([q * cam.to(f64)[:, None, :2], torch.zeros_like(q[..., :1])], -1) if D == 2 else q
    contrib = w[..., :, None] * dP[..., None, :]                                        # (B, N, 3 corners, 3)
    dverts = torch.zeros((B, V, 3), dtype=f64, device=ws.device)
    dverts.scatter_add_(1, tri.reshape(B, N * 3, 1).expand(-1, -1, 3), contrib.reshape(B, N * 3, 3))
    bad = status != 0
    dcam = None
    if D == 2:
        Pxy = torch.where(counted[..., None], ws[..., :2], zero)
        dcam = nan_rows(bad, torch.cat([(q * Pxy).sum(1), q.sum(1)], -1)).to(torch.float32)
    return nan_rows(bad, dverts).to(torch.float32), dcam


class _SurfaceFn(torch.autograd.Function):
    """verts, cam (or None) -> e, d2, point, status.  Device tensors: smplr_sc_fwd forward, smplr_sc_bwd backward; CPU
    tensors: the float64 torch path."""

    @staticmethod
    def forward(ctx, verts, cam, targets, sigma, want_point):
        ctx.set_materialize_grads(False)
        dev = verts.device
        B, V, N, D = int(verts.shape[0]), int(verts.shape[1]), targets.N, targets.D
        if verts.is_cuda:
            f32 = dict(dtype=torch.float32, device=dev)
            e, d2 = torch.empty((B, N), **f32), torch.empty((B, N), **f32)
            point = torch.empty((B, N, 3), **f32) if want_point else None
            status = torch.empty((B,), dtype=torch.int32, device=dev)
            ws = torch.empty((B, N, 4), dtype=torch.float64, device=dev)
            check(_lib.load().smplr_sc_fwd(ptr(verts), ptr(cam), ptr(targets.faces), ptr(targets.s_face), ptr(targets.s_bary),
                                           ptr(targets.s_target), ptr(targets.s_conf), ptr(targets.order), B, V,
                                           targets.topo.num_faces, N, D, sigma, ptr(e), ptr(d2), ptr(point), ptr(status),
                                           ptr(ws), stream()), "smplr_sc_fwd")
            if point is None:
                point = torch.empty((0, N, 3), **f32)
        else:
            with torch.no_grad():
                o = surface_energy_torch(verts, cam, targets, sigma or None)
            e, d2, point = (o[n].to(torch.float32) for n in ("e", "d2", "point"))
            status, ws = o["status"], o["ws"]
        ctx.dims = (B, V)
        ctx.targets, ctx.sigma = targets, sigma
        ctx.save_for_backward(cam, status, ws)
        ctx.mark_non_differentiable(d2, point, status)
        return e, d2, point, status

    @staticmethod
    def backward(ctx, g, *_):
        cam, status, ws = ctx.saved_tensors
        B, V = ctx.dims
        t = ctx.targets
        need_v, need_c = ctx.needs_input_grad[0], cam is not None and ctx.needs_input_grad[1]
        if g is None or not (need_v or need_c):
            return (None,) * 5
        g = g.to(torch.float32).contiguous()
        if not ws.is_cuda:
            dverts, dcam = _backward_torch(t, cam, ws, status, g, ctx.sigma ** 2, V)
            return dverts if need_v else None, dcam if need_c else None, None, None, None
        dev = ws.device
        dverts = torch.empty((B, V, 3), dtype=torch.float32, device=dev)
        dcam = torch.empty((B, 4), dtype=torch.float32, device=dev) if need_c else None
        with torch.cuda.device(dev):
            check(_lib.load().smplr_sc_bwd(ptr(cam), ptr(t.vc_off), ptr(t.vc_fc), ptr(t.c_off), ptr(t.s_face), ptr(t.s_bary),
                                           ptr(t.s_conf), ptr(t.order), ptr(status), ptr(ws), ptr(g), B, V, t.topo.num_faces,
                                           t.N, t.D, ctx.sigma, ptr(dverts), ptr(dcam), stream()), "smplr_sc_bwd")
        return dverts if need_v else None, dcam, None, None, None


@_lib.on_device
def _apply(verts, cam, targets, sigma, want_point):
    return _SurfaceFn.apply(verts, cam, targets, sigma, want_point)


def surface_energy(verts, cam, targets, sigma=None, return_details=False):
    """verts (B, V, 3) fp32, targets a `SurfaceTargets` of B rows on verts' device over a topology of V vertices, cam (B, 4)
    fp32 with image targets (D = 2) and None with 3D targets (D = 3) -> e (B, N) fp32 in the caller's order, differentiable
    in verts and cam; with return_details=True also dict(d2 (B, N), point (B, N, 3) fp32, status (B,) int32), constants to
    autograd."""
    if not isinstance(targets, SurfaceTargets):
        raise TypeError("targets must be a SurfaceTargets")
    B, V = check_verts(verts, targets.topo, ("faces", "num_verts"))
    if B != targets.B:
        raise ValueError("verts have %d rows, the targets %d" % (B, targets.B))
    if (cam is not None) != (targets.D == 2):
        raise ValueError("cam (B, 4) goes with image targets (D = 2), and only with them: these targets have D = %d" % targets.D)
    for name, t, shape in [("verts", verts, (B, V, 3))] + ([("cam", cam, (B, 4))] if cam is not None else []):
        if not isinstance(t, torch.Tensor) or tuple(t.shape) != shape:
            raise ValueError("%s must be a %s tensor" % (name, shape))
        if t.dtype != torch.float32:
            raise RuntimeError("%s must be float32" % name)
    if verts.device != targets.device or (cam is not None and cam.device != verts.device):
        raise RuntimeError("verts live on %s, the targets on %s%s" % (verts.device, targets.device,
                                                                     "" if cam is None else ", cam on %s" % cam.device))
    e, d2, point, status = _apply(verts.contiguous(), None if cam is None else cam.contiguous(), targets, check_sigma(sigma),
                                  bool(return_details))
    return (e, dict(zip(KEYS, (d2, point, status)))) if return_details else e
