"""Triangle renderer for predicted meshes: face-id, depth, part-label, coverage and colour maps on the HIP device.

The reference draws its `_rend.png` images (predict.py:47-52, train.py:292, train_stage2_silhouette.py:331) with
renderer.py's `SMPLRenderer`, opendr's CPU OpenGL renderer.  Here the same pictures, and the dense hard part-label maps
of UP-S31 style, come from two HIP launches (csrc/render.hip, smplr_mesh_vertex + smplr_mesh_raster):

    topo = MeshTopology(faces, 6890)                          # once: validated faces, vertex->face CSR, face parts
    out = render_mesh(verts, topo, smpl[:, :4], img_wh=224)  # ortho: the network's own camera
    out["face"], out["depth"], out["part"], out["alpha"], out["rgb"]
    SMPLRenderer(faces=faces)(verts)                          # renderer.py's call surface: uint8 (H, W, 3) numpy

Semantics (the tests restate them in tests/_render_oracle.py):
  * pixel [i, j] samples (x, y) = (j, i) of sample space; no anti-aliasing;
  * ortho (projection.py:54-81): x = s (u0 + k_u X), y = H - 1 - s (v0 + k_v Y), rows flipped as the seg head's;
    nearer = larger z.  perspective (renderer.py:55-69): x = s (f X / Z + px), y = s (f Y / Z + py), nearer = smaller
    z, a face with a vertex Z outside (max(near, 0), far] is dropped (no clipping);
  * coverage is exact (8 sub-pixel bits, int64 edge functions, top-left rule, both windings); the nearest face wins,
    ties go to the lower face id; depth and colour are interpolated (perspective-correct in perspective mode);
  * "lambert": albedo * sum_k c_k max(0, n . l_k) with the reference's three lights and light_blue albedo
    (renderer.py:146-197); "parts": palette[1 + part(v)] per vertex, unlit (render_seg); "vertex": caller colours.
Not reproduced: anti-aliasing, opendr's half-pixel sampling, near-plane clipping.
"""
from __future__ import annotations

import ctypes
import math

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr, stream

ORTHO, PERSPECTIVE = 0, 1
LAMBERT, VERTEX_COLOR = 0, 1
MAX_FACES = MAX_VERTS = 1 << 24
MAX_LIGHTS = 8

# renderer.py:17-21
COLORS = {"light_blue": (0.65098039, 0.74117647, 0.85882353), "light_pink": (.9, .7, .7)}
# renderer.py:166-197 at yrot = 0: (position, colour)
DEFAULT_LIGHTS = (((-200., -100., -100.), (1., 1., 1.)),
                  ((800., 10., 300.), (1., 1., 1.)),
                  ((-500., 500., 1000.), (.7, .7, .7)))
# the default perspective clip range: renderer.py:66-69's defaults, max(min z - 25, -0.2) and max(max z + 25, 25),
# never drop a face of the mesh they are computed from unless it has a vertex at z <= 0, so they reduce to (0, inf)
DEFAULT_NEAR, DEFAULT_FAR = 0.0, 1e30


def default_palette():
    """(32, 3) float32 in [0, 1]: entry 0 (background / no part) mid grey, entries 1..31 the parts, hues spread by the
    golden angle so that neighbouring part numbers differ."""
    pal = np.empty((32, 3), np.float64)
    pal[0] = 0.5
    for k in range(1, 32):
        h = (k * 0.618033988749895) % 1.0
        v = 0.95 if k % 2 else 0.75
        s = 0.55 if k % 3 else 0.8
        i = int(h * 6.0)
        f = h * 6.0 - i
        p, q, t = v * (1 - s), v * (1 - s * f), v * (1 - s * (1 - f))
        pal[k] = [(v, t, p), (q, v, p), (p, v, t), (p, q, v), (t, p, v), (v, p, q)][i % 6]
    return pal.astype(np.float32)


def vertex_parts(part_tables, num_verts):
    """(V,) int64 part of each vertex (0..30), -1 for none, from the (ids, offsets) CSR of `load_part_tables`; a vertex
    listed by several parts takes the lowest."""
    vp = np.full(int(num_verts), -1, np.int64)
    if part_tables is None:
        return vp
    ids, off = (np.asarray(a, np.int64) for a in part_tables)
    if ids.size and (ids.min() < 0 or ids.max() >= num_verts):
        raise ValueError("part tables name vertices outside [0, %d)" % num_verts)
    for p in range(len(off) - 2, -1, -1):
        vp[ids[off[p]:off[p + 1]]] = p
    return vp


def face_parts(faces, vpart):
    """face_part[f] = 1 + the part shared by at least two of the face's vertices, else 1 + the part of its
    lowest-indexed vertex that has one, else 0 (uint8)."""
    f = np.asarray(faces, np.int64)
    p = vpart[f]                                           # (F, 3)
    two = np.where((p[:, 0] >= 0) & ((p[:, 0] == p[:, 1]) | (p[:, 0] == p[:, 2])), p[:, 0],
                   np.where((p[:, 1] >= 0) & (p[:, 1] == p[:, 2]), p[:, 1], -1))
    order = np.argsort(f, axis=1, kind="stable")           # vertices by index
    ps = np.take_along_axis(p, order, axis=1)
    first = np.where(ps[:, 0] >= 0, ps[:, 0], np.where(ps[:, 1] >= 0, ps[:, 1], ps[:, 2]))
    out = np.where(two >= 0, two, first) + 1
    return out.astype(np.uint8)


class MeshTopology:
    """What a mesh's faces give every render, built once: validated faces (F, 3) int32, the vertex -> face CSR (faces in
    increasing id order) the vertex normals sum over, the per-vertex and per-face parts.

    face_part: (F,) integers in 0..31 overriding the rule of `face_parts`; part_tables: (ids, offsets) of the 31 parts
    (default: the package's UP-S31 tables when num_verts is SMPL's 6 890, otherwise no parts)."""

    def __init__(self, faces, num_verts, face_part=None, part_tables=None):
        if isinstance(faces, torch.Tensor):
            faces = faces.detach().cpu().numpy()
        f = np.asarray(faces)
        if f.ndim != 2 or f.shape[1] != 3:
            raise ValueError("faces must be (F, 3), got shape %s" % (f.shape,))
        if not np.issubdtype(f.dtype, np.integer):
            raise ValueError("faces must be integers, got %s" % f.dtype)
        V = int(num_verts)
        if not 1 <= V <= MAX_VERTS:
            raise ValueError("num_verts must be in 1..2^24 (got %d)" % V)
        if f.shape[0] > MAX_FACES:
            raise ValueError("at most 2^24 faces (got %d)" % f.shape[0])
        if f.size and (int(f.min()) < 0 or int(f.max()) >= V):
            raise ValueError("face indices must lie in [0, %d): found %d..%d" % (V, int(f.min()), int(f.max())))
        self.num_verts, self.num_faces = V, int(f.shape[0])
        self.faces = np.ascontiguousarray(f, np.int32)
        flat = self.faces.reshape(-1).astype(np.int64)
        fid = np.repeat(np.arange(self.num_faces, dtype=np.int64), 3)
        order = np.argsort(flat, kind="stable")
        self.vf_face = fid[order].astype(np.int32)
        self.vf_off = np.concatenate([[0], np.cumsum(np.bincount(flat, minlength=V))]).astype(np.int32)
        if part_tables is None and V == 6890:
            from .smpl_model import load_part_tables
            part_tables = load_part_tables(1)
        self.vertex_part = vertex_parts(part_tables, V)
        if face_part is not None:
            fp = np.asarray(face_part)
            if fp.shape != (self.num_faces,) or not np.issubdtype(fp.dtype, np.integer) or (
                    fp.size and (fp.min() < 0 or fp.max() > 31)):
                raise ValueError("face_part must be (F,) integers in 0..31")
            self.face_part = fp.astype(np.uint8)
        else:
            self.face_part = face_parts(self.faces, self.vertex_part)
        self._dev = {}

    def on(self, device):
        """The device copies: faces, vf_off, vf_face, face_part, vertex_part (uploaded once per device)."""
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        d = self._dev.get(device)
        if d is None:
            d = {"faces": torch.from_numpy(self.faces).to(device),
                 "vf_off": torch.from_numpy(self.vf_off).to(device),
                 "vf_face": torch.from_numpy(self.vf_face).to(device),
                 "face_part": torch.from_numpy(self.face_part).to(device),
                 "vertex_part": torch.from_numpy(self.vertex_part).to(device)}
            self._dev[device] = d
        return d


def _wh(img_wh):
    if isinstance(img_wh, (tuple, list)):
        W, H = int(img_wh[0]), int(img_wh[1])
    else:
        W = H = int(img_wh)
    if not (1 <= W <= 4096 and 1 <= H <= 4096):
        raise ValueError("image size %d x %d outside 1..4096" % (W, H))
    return W, H


def _per_mesh(t, B, n, name, dev):
    t = torch.as_tensor(t, dtype=torch.float32, device=dev)
    if t.dim() == 1:
        t = t.expand(B, n)
    if t.shape != (B, n):
        raise ValueError("%s must be (%d,) or (B, %d), got %s" % (name, n, n, tuple(t.shape)))
    return t.contiguous()


def normalize_background(img, B, H, W, dev):
    """(B, H, W, 3) float32 in [0, 1] from an image batch (B, H, W, 3), (B, 3, H, W) or one (H, W, 3) image: uint8 is
    divided by 255, a float image by 255 when its maximum exceeds 1 (renderer.py:235-236), per image and on the
    device (no host synchronisation)."""
    t = torch.as_tensor(img, device=dev)
    if t.dim() == 3:
        t = t.unsqueeze(0)
    if t.dim() != 4:
        raise ValueError("background must be (H, W, 3) or a batch of images")
    if t.shape[-1] != 3 and t.shape[1] == 3:
        t = t.permute(0, 2, 3, 1)
    if tuple(t.shape[1:]) != (H, W, 3):
        raise ValueError("background is %s, the image %d x %d" % (tuple(t.shape), H, W))
    if t.dtype == torch.uint8:
        t = t.to(torch.float32) / 255.0
    else:
        t = t.to(torch.float32)
        big = t.flatten(1).amax(dim=1) > 1
        t = torch.where(big[:, None, None, None], t / 255.0, t)
    return t.expand(B, H, W, 3).contiguous()


@_lib.on_device
def render_mesh(verts, topo, cam, *, mode="ortho", img_wh, scale=1.0, trans=None, near=None, far=None,
                shading="lambert", albedo=None, lights=None, palette=None, vertex_colors=None, background=None):
    """Render B meshes verts (B, V, 3) fp32 on the HIP device with topo's faces.  Returns device tensors
    face (B, H, W) int32 (-1 background), depth (B, H, W) fp32 (0 background), part (B, H, W) uint8 (0 background,
    1..31 the seg head's channels), alpha (B, H, W) bool and rgb (B, H, W, 3) fp32 in [0, 1].

    cam: (B, 4) or (4,) = smpl[:, :4] (k_u, k_v, u0, v0) in "ortho" mode, (B, 3) or (3,) = (f, px, py) in "perspective"
    mode.  img_wh: W or (W, H).  trans: (B, 3) or (3,) added to the vertices.  near / far: the perspective clip range
    (default (0, inf), which is what renderer.py's defaults amount to).  shading: "lambert" (albedo (3,) and lights
    [(position, colour)] default to renderer.py's), "parts" (palette (32, 3), default `default_palette()`) or
    "vertex" (vertex_colors (V, 3) or (B, V, 3)).  background: images (see `normalize_background`), default white.
    No host synchronisation: the call can be captured in a HIP graph (once topo has been used on that device: its first
    use uploads it, `MeshTopology.on`)."""
    if mode not in ("ortho", "perspective"):
        raise ValueError("mode must be 'ortho' or 'perspective'")
    if shading not in ("lambert", "parts", "vertex"):
        raise ValueError("shading must be 'lambert', 'parts' or 'vertex'")
    verts = _lib.require_cuda(verts, "verts")
    if verts.dim() != 3 or verts.shape[2] != 3:
        raise ValueError("verts must be (B, V, 3)")
    B, V = int(verts.shape[0]), int(verts.shape[1])
    if V != topo.num_verts:
        raise ValueError("verts have %d vertices, the topology %d" % (V, topo.num_verts))
    W, H = _wh(img_wh)
    dev = verts.device
    m = ORTHO if mode == "ortho" else PERSPECTIVE
    cam = _per_mesh(cam, B, 4 if m == ORTHO else 3, "cam", dev)
    trans = None if trans is None else _per_mesh(trans, B, 3, "trans", dev)
    t = topo.on(dev)
    light = None
    vcol, bstride = None, 0
    if shading == "lambert":
        alb = COLORS["light_blue"] if albedo is None else albedo
        lts = DEFAULT_LIGHTS if lights is None else lights
        if len(lts) > MAX_LIGHTS:
            raise ValueError("at most %d lights" % MAX_LIGHTS)
        vals = [float(a) for a in alb]
        for pos, c in lts:
            vals += [float(a) for a in pos] + [float(a) for a in c]
        if len(vals) != 3 + 6 * len(lts):
            raise ValueError("albedo is (3,), each light (position (3,), colour (3,))")
        light = (ctypes.c_float * len(vals))(*vals)
        nl = len(lts)
    elif shading == "parts":
        pal = default_palette() if palette is None else palette
        pal = torch.as_tensor(pal, dtype=torch.float32, device=dev)
        if pal.shape != (32, 3):
            raise ValueError("palette must be (32, 3)")
        vcol = pal[t["vertex_part"] + 1].contiguous()
        nl = 0
    else:
        if vertex_colors is None:
            raise ValueError("shading='vertex' needs vertex_colors")
        vcol = torch.as_tensor(vertex_colors, dtype=torch.float32, device=dev).contiguous()
        if vcol.shape == (V, 3):
            bstride = 0
        elif vcol.shape == (B, V, 3):
            bstride = V * 3
        else:
            raise ValueError("vertex_colors must be (V, 3) or (B, V, 3)")
        nl = 0
    bg = None if background is None else normalize_background(background, B, H, W, dev)
    zn = DEFAULT_NEAR if near is None else float(near)
    zf = DEFAULT_FAR if far is None else float(far)
    out = {"face": torch.empty((B, H, W), dtype=torch.int32, device=dev),
           "depth": torch.empty((B, H, W), dtype=torch.float32, device=dev),
           "part": torch.empty((B, H, W), dtype=torch.uint8, device=dev),
           "alpha": torch.empty((B, H, W), dtype=torch.bool, device=dev),
           "rgb": torch.empty((B, H, W, 3), dtype=torch.float32, device=dev)}
    if B == 0:
        return out
    lib = _lib.load()
    vbuf = torch.empty(int(lib.smplr_mesh_vbuf_bytes(B, V)), dtype=torch.uint8, device=dev)
    lam = shading == "lambert"
    check(lib.smplr_mesh_vertex(ptr(verts), ptr(cam), ptr(trans), B, V, m, float(scale), H, W, zn, zf,
                                LAMBERT if lam else VERTEX_COLOR, ptr(t["faces"]), topo.num_faces,
                                ptr(t["vf_off"]) if lam else None, ptr(t["vf_face"]) if lam else None,
                                int(t["vf_face"].numel()) if lam else 0,
                                ctypes.cast(light, ctypes.c_void_p) if lam else None, nl, ptr(vcol), bstride,
                                ptr(vbuf), stream()), "smplr_mesh_vertex")
    check(lib.smplr_mesh_raster(ptr(vbuf), ptr(t["faces"]), ptr(t["face_part"]), B, V, topo.num_faces, H, W, m, ptr(bg),
                                ptr(out["face"]), ptr(out["depth"]), ptr(out["part"]), ptr(out["alpha"]),
                                ptr(out["rgb"]), stream()), "smplr_mesh_raster")
    return out


def to_uint8(rgb):
    """renderer.py:84's (imtmp * 255).astype('uint8') on [0, 1] colours: floor(255 c)."""
    return (rgb * 255.0).to(torch.uint8)


def _rotation(axis, deg):
    """cv2.Rodrigues of `deg` degrees about x, y or z (renderer.py:96-101)."""
    a = math.radians(deg)
    c, s = math.cos(a), math.sin(a)
    if axis == "y":
        return np.array([[c, 0., s], [0., 1., 0.], [-s, 0., c]])
    if axis == "x":
        return np.array([[1., 0., 0.], [0., c, -s], [0., s, c]])
    return np.array([[c, -s, 0.], [s, c, 0.], [0., 0., 1.]])


class SMPLRenderer:
    """renderer.py's SMPLRenderer (:23-115) on the HIP renderer: perspective camera (f, px, py), the three-light
    Lambertian rig, white or image background, uint8 numpy out.

    faces: (F, 3) array; or face_path: a .npy of them (the reference's keras_smpl/smpl_faces.npy); or smpl_path: an SMPL
    pickle whose `f` holds them.  Also takes a batch (B, V, 3) and returns (B, H, W, 3|4), and an optional trans (3,) or
    (B, 3) added to the vertices (the reference renders origin-centred vertices at t = 0, renderer.py:59-64)."""

    def __init__(self, img_size=224, flength=500., faces=None, face_path=None, smpl_path=None, device=None):
        if faces is None and face_path is not None:
            faces = np.load(face_path)
        if faces is None and smpl_path is not None:
            from .smpl_pkl import load_smpl_pkl
            faces = load_smpl_pkl(smpl_path).faces
        if faces is None:
            raise ValueError("SMPLRenderer needs the mesh's faces: pass faces=, face_path= (an (F, 3) .npy) or smpl_path= "
                             "(an SMPL pickle with 'f'); the synthetic SMPL model has no topology")
        self.faces = np.asarray(faces)
        self.w = self.h = img_size
        self.flength = flength
        self.device = torch.device(device) if device is not None else None     # None: the current HIP device at the call
        self._topo = {}

    def topology(self, num_verts):
        t = self._topo.get(num_verts)
        if t is None:
            t = self._topo[num_verts] = MeshTopology(self.faces, num_verts)
        return t

    def __call__(self, verts, cam=None, img=None, do_alpha=False, far=None, near=None, color_id=0, img_size=None,
                 render_seg=False, trans=None):
        """renderer.py:33-84: cam = [f, px, py] (default [flength, w / 2, h / 2]); img: background (its size wins);
        do_alpha: RGBA, alpha = coverage without img and 255 everywhere with one; color_id None -> light_blue, else
        the reference's colour list; render_seg: the part palette, unlit.  near / far: renderer.py's defaults when None."""
        dev = self.device if self.device is not None else torch.device("cuda", torch.cuda.current_device())
        v = torch.as_tensor(np.asarray(verts) if not isinstance(verts, torch.Tensor) else verts, dtype=torch.float32)
        single = v.dim() == 2
        v = (v[None] if single else v).to(dev).contiguous()
        B, V = int(v.shape[0]), int(v.shape[1])
        if img is not None:
            h, w = np.asarray(img).shape[-3:-1] if not isinstance(img, torch.Tensor) else img.shape[-3:-1]
        elif img_size is not None:
            h, w = img_size[0], img_size[1]
        else:
            h, w = self.h, self.w
        h, w = int(h), int(w)
        if cam is None:
            cam = [self.flength, w / 2., h / 2.]
        zz = v[..., 2] if trans is None else v[..., 2] + torch.as_tensor(trans, dtype=torch.float32,
                                                                          device=dev).reshape(-1, 3)[:, 2:3]
        # renderer.py:66-69 (the batch's extremes: the defaults never drop a face at z > 0 either way)
        if near is None:
            near = max(float(torch.nan_to_num(zz, nan=np.inf).min()) - 25, -0.2)
        if far is None:
            far = max(float(torch.nan_to_num(zz, nan=-np.inf).max()) + 25, 25)
        if color_id is None:
            color = COLORS["light_blue"]
        else:
            color = list(COLORS.values())[color_id % len(COLORS)]
        bg = None
        if img is not None:
            bg = torch.as_tensor(np.asarray(img) if not isinstance(img, torch.Tensor) else img).to(dev)
        out = render_mesh(v, self.topology(V), cam, mode="perspective", img_wh=(w, h), trans=trans, near=near, far=far,
                          shading="parts" if render_seg else "lambert", albedo=color, background=bg)
        im = to_uint8(out["rgb"])
        if do_alpha:
            a = torch.full_like(im[..., :1], 255) if img is not None else out["alpha"][..., None].to(torch.uint8) * 255
            im = torch.cat([im, a], dim=-1)
        im = im.cpu().numpy()
        return im[0] if single else im

    def rotated(self, verts, deg, cam=None, axis='y', img=None, do_alpha=True, far=None, near=None, color_id=0,
                img_size=None):
        """renderer.py:86-115: the mesh turned by `deg` degrees about its centroid."""
        v = np.asarray(verts.detach().cpu().numpy() if isinstance(verts, torch.Tensor) else verts, np.float64)
        around = _rotation(axis, deg)
        center = v.mean(axis=-2, keepdims=True)
        new_v = np.matmul(v - center, around) + center
        return self.__call__(new_v.astype(np.float32), cam, img=img, do_alpha=do_alpha, far=far, near=near,
                             img_size=img_size, color_id=color_id)


def render_predictions(pred, topo, images, output_wh, shading="lambert", **kw):
    """predict.py:47-75's `_rend.png` and vertex overlay as one GPU call: the meshes of `inference.predict_batch`'s
    output drawn over the input images with the network's own ortho camera pred["smpl"][:, :4], scaled by
    input_wh / output_wh.  images (N, 3, H, W) or (N, H, W, 3); returns `render_mesh`'s dict at the images' size."""
    imgs = images if isinstance(images, torch.Tensor) else torch.as_tensor(np.asarray(images))
    if imgs.dim() != 4:
        raise ValueError("images must be (N, 3, H, W) or (N, H, W, 3)")
    nchw = imgs.shape[-1] != 3 and imgs.shape[1] == 3
    H, W = (int(imgs.shape[2]), int(imgs.shape[3])) if nchw else (int(imgs.shape[1]), int(imgs.shape[2]))
    verts = pred["verts"]
    imgs = imgs.to(verts.device)
    return render_mesh(verts.contiguous(), topo, pred["smpl"][:, :4].float(), mode="ortho", img_wh=(W, H),
                       scale=float(W) / float(output_wh), shading=shading, background=imgs, **kw)
