"""Prediction figures on the HIP device: the arg-max part map in colour, the projected vertices as discs, both over the
input image, and the panels and PNG files the reference's drivers write.

The reference draws them with matplotlib on the host: `predict.py:28-77` (`_seg.png`, `_projects.png`, `_rend.png`,
`_input.png`, `_verts_overlay.png`), `train.py:283-300` / `train_stage2_silhouette.py:318-339` (`seg_*`, `silh_*`,
`verts_*`, `rend_*`, `image_*` every tenth trial) and `predict_realtime.py:75-96` (the per-frame vertex scatter).  Here
the pictures are uint8 tensors made by two HIP launches (csrc/figure.hip, smplr_seg_colour + smplr_scatter_points) from
the scores and projections where they already live; only finished pictures travel to the host, and `write_png` needs no
imaging library.

    figs = prediction_figures(predict_batch(model, decoder, images), images, output_wh=64)
    save_predictions(figs, fnames, save_dir)                  # predict.py's five files per image
    fit(trainer, batches, ..., on_trial_end=MonitorFigures(monitor_images, "monitor"))

Rules (tests/_figures_oracle.py restates them in NumPy; device and CPU tensors give the same bytes):
  * seg_colour: label = arg-max of the scores with NaN above every number, the first NaN winning and ties going to the
    lower channel (metrics.py), or the given integer map; output pixel [i, j] reads source [(i h) // H, (j w) // W];
    colour = lut[label], `bad_colour` for a label outside the table; over a background, label 0 shows the background and
    every other label (alpha_q colour + (256 - alpha_q) background + 128) >> 8.
  * scatter_points: centre cx = rint(s u), cy = H - 1 - rint(s v) (fp32 product clamped to +-2^20, half to even; rows
    flipped as the seg head's); pixel [i, j] is covered iff (j - cx)^2 + (i - cy)^2 <= r^2; order "index": the highest
    vertex index wins (matplotlib's painter's order); "depth": the largest z, ties to the lower index; vertices with a
    non-finite u or v (in depth order: or z), or keep == 0, are not drawn; uncovered pixels show
    (alpha_q image + (256 - alpha_q) canvas + 128) >> 8, or the canvas.
Not reproduced: imshow's rescaling of the colour range to the labels present in one image (a class always has the same
colour here, that of the triangle renderer's "parts" shading), axes, ticks, anti-aliased markers.
"""
from __future__ import annotations

import os
import struct
import zlib

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr, stream
from .metrics import _argmax_cpu
from .render import default_palette, to_uint8, vertex_parts

ORDERS = ("index", "depth")
MAX_RADIUS = 16
MAX_SIDE = 4096
MAX_VERTS = 1 << 24
CLAMP = float(1 << 20)
MPL_BLUE = (31, 119, 180)          # matplotlib's default scatter colour (C0)
SILH_LUT = ((0, 0, 0), (255, 255, 255))


def default_lut():
    """(32, 3) uint8: floor(255 * default_palette()), the rule of `render.to_uint8` - class k has the colour the triangle
    renderer's "parts" shading gives part k."""
    return to_uint8(torch.from_numpy(default_palette()))


def _pack(c, name):
    c = tuple(int(x) for x in c)
    if len(c) != 3 or not all(0 <= x <= 255 for x in c):
        raise ValueError("%s must be three integers in 0..255, got %r" % (name, c))
    return c[0] | (c[1] << 8) | (c[2] << 16)


def _alpha_q(alpha, name):
    a = float(alpha)
    if not 0.0 <= a <= 1.0:
        raise ValueError("%s must lie in [0, 1], got %r" % (name, alpha))
    return int(round(256.0 * a))


def _hw(size, default=None):
    """size: S, (W, H) as `render.render_mesh`'s img_wh, or None -> (H, W)."""
    if size is None:
        H, W = default
    elif isinstance(size, (tuple, list)):
        W, H = int(size[0]), int(size[1])
    else:
        H = W = int(size)
    if not (1 <= H <= MAX_SIDE and 1 <= W <= MAX_SIDE):
        raise ValueError("picture size %d x %d outside 1..%d" % (H, W, MAX_SIDE))
    return H, W


def _same_device(ref, **others):
    for name, t in others.items():
        if t is not None and t.device != ref.device:
            raise RuntimeError("%s lives on %s, the input on %s" % (name, t.device, ref.device))


def as_uint8_images(images, device=None):
    """(N, H, W, 3) uint8, contiguous, from (N, 3, H, W) or (N, H, W, 3) images: uint8 as they are, floating point in
    [0, 1] as floor(255 c) clamped to [0, 255] with NaN -> 0."""
    t = images if isinstance(images, torch.Tensor) else torch.as_tensor(np.asarray(images))
    if device is not None:
        t = t.to(device)
    if t.dim() != 4:
        raise ValueError("images must be (N, 3, H, W) or (N, H, W, 3), got %s" % (tuple(t.shape),))
    if t.shape[-1] != 3 and t.shape[1] == 3:
        t = t.permute(0, 2, 3, 1)
    if t.shape[-1] != 3:
        raise ValueError("images must have three channels, got %s" % (tuple(t.shape),))
    if t.dtype != torch.uint8:
        if not t.is_floating_point():
            raise ValueError("images must be uint8 or floating point in [0, 1], got %s" % t.dtype)
        t = torch.nan_to_num(t.to(torch.float32) * 255.0, nan=0.0, posinf=255.0, neginf=0.0).clamp_(0.0, 255.0).to(torch.uint8)
    return t.contiguous()


def resize_nearest(img, H, W):
    """(N, h, w, ...) -> (N, H, W, ...) by the integer rule of `seg_colour`: pixel [i, j] reads [(i h) // H, (j w) // W]."""
    h, w = int(img.shape[1]), int(img.shape[2])
    if (h, w) == (H, W):
        return img
    ri = (torch.arange(H, device=img.device) * h) // H
    cj = (torch.arange(W, device=img.device) * w) // W
    return img[:, ri][:, :, cj].contiguous()


# ---- the class map in colour ---------------------------------------------------------------------------------------------
def _seg_colour_cpu(x, is_scores, lut, bad, bg, aq, H, W):
    lab = _argmax_cpu(x.detach().float()) if is_scores else x.detach().to(torch.int64)
    lab = resize_nearest(lab, H, W)
    K = lut.shape[0]
    ok = (lab >= 0) & (lab < K)
    col = lut[lab.clamp(0, K - 1)]
    col = torch.where(ok[..., None], col, torch.tensor([bad & 255, (bad >> 8) & 255, (bad >> 16) & 255], dtype=torch.uint8))
    if bg is not None:
        mix = (aq * col.to(torch.int32) + (256 - aq) * bg.to(torch.int32) + 128) >> 8
        col = torch.where((lab != 0)[..., None], mix.to(torch.uint8), bg)
    return col.contiguous()


@_lib.on_device
def _seg_colour_hip(x, is_scores, lut, bad, bg, aq, H, W):
    x = _lib.require_cuda(x, "scores" if is_scores else "labels", torch.float32 if is_scores else torch.int32)
    B, h, w = (int(s) for s in x.shape[:3])
    rgb = torch.empty((B, H, W, 3), dtype=torch.uint8, device=x.device)
    check(_lib.load().smplr_seg_colour(ptr(x) if is_scores else None, None if is_scores else ptr(x), B, h, w,
                                       int(x.shape[3]) if is_scores else 0, ptr(lut), int(lut.shape[0]), bad, ptr(bg), aq, H, W,
                                       ptr(rgb), stream()), "smplr_seg_colour")
    return rgb


def seg_colour(scores_or_labels, size=None, lut=None, background=None, alpha=None, bad_colour=(0, 0, 0)):
    """Raw scores (B, h, w, C) floating point, 2 <= C <= 32, or an integer class map (B, h, w) -> (B, H, W, 3) uint8.

    size: S or (W, H) of the picture (default: the map's own size); lut: (K, 3) uint8 colour table (default
    `default_lut()`); background: images (see `as_uint8_images`) at the picture's size, shown through class 0 and blended
    under the others with weight 1 - alpha (alpha: float in [0, 1], default 0.5; ignored without a background);
    bad_colour: the colour of a label outside the table.  One HIP launch for device tensors, torch on the CPU."""
    x = scores_or_labels
    if not isinstance(x, torch.Tensor):
        raise TypeError("scores_or_labels must be a torch.Tensor")
    is_scores = x.is_floating_point()
    if is_scores:
        if x.dim() != 4 or not 2 <= x.shape[3] <= 32:
            raise ValueError("scores must be (B, h, w, C) with 2 <= C <= 32, got %s" % (tuple(x.shape),))
    elif x.dtype in (torch.int64, torch.int32, torch.int16, torch.int8, torch.uint8):
        if x.dim() != 3:
            raise ValueError("a class map must be (B, h, w), got %s" % (tuple(x.shape),))
    else:
        raise ValueError("scores_or_labels must be floating point scores or an integer class map, got %s" % x.dtype)
    h, w = int(x.shape[1]), int(x.shape[2])
    if not (1 <= h <= MAX_SIDE and 1 <= w <= MAX_SIDE):
        raise ValueError("source map %d x %d outside 1..%d" % (h, w, MAX_SIDE))
    H, W = _hw(size, (h, w))
    lut = default_lut() if lut is None else torch.as_tensor(lut)
    if lut.dtype != torch.uint8 or lut.dim() != 2 or lut.shape[1] != 3 or lut.shape[0] < 1:
        raise ValueError("lut must be (K, 3) uint8")
    lut = lut.to(x.device).contiguous()
    bad = _pack(bad_colour, "bad_colour")
    aq = _alpha_q(0.5 if alpha is None else alpha, "alpha")
    bg = None
    if background is not None:
        if isinstance(background, torch.Tensor):
            _same_device(x, background=background)
        bg = as_uint8_images(background, x.device)
        if tuple(bg.shape) != (x.shape[0], H, W, 3):
            raise ValueError("background is %s, the picture (%d, %d, %d, 3)" % (tuple(bg.shape), x.shape[0], H, W))
    if x.is_cuda:
        x = x.detach().float() if is_scores else x.detach().to(torch.int32)
        return _seg_colour_hip(x, is_scores, lut, bad, bg, aq, H, W)
    return _seg_colour_cpu(x, is_scores, lut, bad, bg, aq, H, W)


# ---- projected vertices as discs -----------------------------------------------------------------------------------------
def _disc_offsets(r):
    return [(dx, dy) for dy in range(-r, r + 1) for dx in range(-r, r + 1) if dx * dx + dy * dy <= r * r]


def _scatter_points_cpu(proj, keep, colours, colour, image, aq, canvas, scale, radius, order, H, W, want_vertex):
    p = proj.detach().to(torch.float32)
    B, V = int(p.shape[0]), int(p.shape[1])
    s = torch.tensor(scale, dtype=torch.float32)
    fin = torch.isfinite(p[..., 0]) & torch.isfinite(p[..., 1])
    if keep is not None:
        fin = fin & (keep != 0)
    idx = torch.arange(V, dtype=torch.int64).expand(B, V)
    if order == 1:
        z = p[..., 2] + 0.0
        fin = fin & torch.isfinite(z)
        bits = torch.where(fin, z, torch.zeros_like(z)).contiguous().view(torch.int32).to(torch.int64)
        bits = torch.where(bits >= 0, bits, bits ^ 0x7fffffff)             # signed integers in the order of the floats
        key = bits * (1 << 32) + ((1 << 32) - 1 - idx)
    else:
        key = idx + 1
    empty = torch.iinfo(torch.int64).min
    cx = torch.round((s * torch.where(fin, p[..., 0], torch.zeros_like(s))).clamp(-CLAMP, CLAMP)).to(torch.int64)
    cy = (H - 1) - torch.round((s * torch.where(fin, p[..., 1], torch.zeros_like(s))).clamp(-CLAMP, CLAMP)).to(torch.int64)
    buf = torch.full((B * H * W,), empty, dtype=torch.int64)
    base = torch.arange(B, dtype=torch.int64)[:, None] * (H * W)
    offs = torch.tensor(_disc_offsets(radius), dtype=torch.int64)
    for o in offs.split(64):                                                 # 64 offsets of the disc per pass
        j, i = cx[None] + o[:, 0, None, None], cy[None] + o[:, 1, None, None]
        ok = fin[None] & (j >= 0) & (j < W) & (i >= 0) & (i < H)
        buf.scatter_reduce_(0, (base[None] + i * W + j)[ok], key[None].expand_as(ok)[ok], "amax", include_self=True)
    buf = buf.view(B, H, W)
    hit = buf != empty
    if order == 1:
        win = (1 << 32) - 1 - (buf & 0xffffffff)
    else:
        win = buf - 1
    win = torch.where(hit, win, torch.full_like(win, -1))
    unpack = lambda c: torch.tensor([c & 255, (c >> 8) & 255, (c >> 16) & 255], dtype=torch.int32)
    cv = unpack(canvas)
    if image is not None:
        under = ((aq * image.to(torch.int32) + (256 - aq) * cv + 128) >> 8).to(torch.uint8)
    else:
        under = cv.to(torch.uint8).expand(B, H, W, 3)
    top = colours[win.clamp(min=0)] if colours is not None else unpack(colour).to(torch.uint8).expand(B, H, W, 3)
    rgb = torch.where(hit[..., None], top, under).contiguous()
    return rgb, (win.to(torch.int32) if want_vertex else None)


@_lib.on_device
def _scatter_points_hip(proj, keep, colours, colour, image, aq, canvas, scale, radius, order, H, W, want_vertex):
    proj = _lib.require_cuda(proj, "proj")
    B, V = int(proj.shape[0]), int(proj.shape[1])
    rgb = torch.empty((B, H, W, 3), dtype=torch.uint8, device=proj.device)
    vertex = torch.empty((B, H, W), dtype=torch.int32, device=proj.device) if want_vertex else None
    check(_lib.load().smplr_scatter_points(ptr(proj), ptr(keep), ptr(colours), colour, ptr(image), aq, canvas, B, V,
                                           float(scale), radius, order, H, W, ptr(vertex), ptr(rgb), stream()),
          "smplr_scatter_points")
    return rgb, vertex


def scatter_points(proj, img_wh, scale, radius=0, order="index", keep=None, colours=None, colour=MPL_BLUE, image=None,
                   image_alpha=0.9, canvas=(255, 255, 255), return_vertex=False):
    """proj (B, V, 3) = (u, v, z) as `orthographic_project` returns it -> rgb (B, H, W, 3) uint8 [, vertex (B, H, W) int32:
    the vertex each pixel shows, -1 for none].

    img_wh: W or (W, H); scale: multiplies u and v (predict.py:65: input_wh / output_wh); radius: integer disc radius,
    0..16 (0: one pixel per vertex); order: "index" (the highest index on top) or "depth" (the largest z, the nearest under
    the ortho convention); keep: (B, V), zero = not drawn (`keep_from_mask`); colours: (V, 3) uint8 per-vertex colours
    shared by the batch (`part_colours`), else `colour` for all; image: upright images (see `as_uint8_images`) at the
    picture's size, shown with weight image_alpha over `canvas` (0.9 over white: imshow(alpha=0.9) on white axes) under the
    discs; without an image the canvas colour.  One HIP launch for device tensors, torch on the CPU."""
    if not isinstance(proj, torch.Tensor):
        raise TypeError("proj must be a torch.Tensor")
    if proj.dim() != 3 or proj.shape[2] != 3 or not proj.is_floating_point():
        raise ValueError("proj must be (B, V, 3) floating point, got %s %s" % (tuple(proj.shape), proj.dtype))
    B, V = int(proj.shape[0]), int(proj.shape[1])
    if not 1 <= V <= MAX_VERTS:
        raise ValueError("proj holds %d vertices (1..2^24)" % V)
    H, W = _hw(img_wh)
    radius = int(radius)
    if not 0 <= radius <= MAX_RADIUS:
        raise ValueError("radius %d outside 0..%d" % (radius, MAX_RADIUS))
    if order not in ORDERS:
        raise ValueError("order %r is none of %s" % (order, ORDERS))
    scale = float(scale)
    if not np.isfinite(np.float32(scale)):
        raise ValueError("scale must be finite in fp32, got %r" % scale)
    if keep is not None:
        _same_device(proj, keep=keep)
        if tuple(keep.shape) != (B, V):
            raise ValueError("keep must be (B, V) = (%d, %d), got %s" % (B, V, tuple(keep.shape)))
        keep = (keep != 0).to(torch.uint8).contiguous()
    if colours is not None:
        colours = torch.as_tensor(colours)
        if isinstance(colours, torch.Tensor) and colours.device != proj.device and colours.device.type != "cpu":
            _same_device(proj, colours=colours)
        if colours.dtype != torch.uint8 or tuple(colours.shape) != (V, 3):
            raise ValueError("colours must be (V, 3) = (%d, 3) uint8, got %s %s" % (V, tuple(colours.shape), colours.dtype))
        colours = colours.to(proj.device).contiguous()
    colour, canvas = _pack(colour, "colour"), _pack(canvas, "canvas")
    aq = _alpha_q(image_alpha, "image_alpha")
    if image is not None:
        if isinstance(image, torch.Tensor):
            _same_device(proj, image=image)
        image = as_uint8_images(image, proj.device)
        if tuple(image.shape) != (B, H, W, 3):
            raise ValueError("image is %s, the picture (%d, %d, %d, 3)" % (tuple(image.shape), B, H, W))
    fn = _scatter_points_hip if proj.is_cuda else _scatter_points_cpu
    rgb, vertex = fn(proj.detach().float(), keep, colours, colour, image, aq, canvas, scale, radius, ORDERS.index(order), H, W,
                     bool(return_vertex))
    return (rgb, vertex) if return_vertex else rgb


def part_colours(part_tables, num_verts, lut=None):
    """(V, 3) uint8 colour of each vertex by its body part: lut[1 + part(v)] with `render.vertex_parts`' parts (0..30, -1 for
    none -> lut[0]) - predict_realtime.py:38-46's colour map in the colours of `seg_colour`."""
    lut = default_lut() if lut is None else torch.as_tensor(lut)
    if lut.dtype != torch.uint8 or lut.dim() != 2 or lut.shape[1] != 3 or lut.shape[0] < 32:
        raise ValueError("lut must be (K >= 32, 3) uint8")
    vp = torch.from_numpy(vertex_parts(part_tables, num_verts) + 1)
    return lut.cpu()[vp].contiguous()


def keep_from_mask(mask):
    """`compute_mask`'s output -> keep: keras_smpl/compute_mask.py:12-21,68-70 writes 1 for a visible vertex and 500 for a
    hidden one, so a vertex is kept where the mask equals 1."""
    return (mask == 1).to(torch.uint8)


# ---- the reference's figures --------------------------------------------------------------------------------------------------
TILE_ORDER = ("input", "seg", "silh", "projects", "verts_overlay", "seg_overlay", "rend")


def prediction_figures(pred, images, output_wh, topo=None, part_tables=None, size=None, radius=0, seg_alpha=0.5):
    """The pictures of predict.py:28-77 for `inference.predict_batch`'s or `SegTrainer.monitor`'s dict -> dict of uint8
    (N, S, S, 3) tensors on pred's device: "seg" (arg-max part map; "silh" too when pred has a silhouette), "projects"
    (the vertices on white), "verts_overlay" (over the image), "seg_overlay" (the parts blended over the image), "input",
    and "rend" (`render.render_predictions`, device only) when topo is given.

    images: the network's input (see `as_uint8_images`); output_wh: the decoder's image size, projections are scaled by
    S / output_wh; size: S (default: the images' height and width); part_tables: (ids, offsets) - the vertices are then
    coloured by part as in predict_realtime.py:38-46, in "projects" and "verts_overlay"."""
    scores = pred["segs"] if "segs" in pred else pred["seg"]
    proj = pred["projects"]
    dev = proj.device
    img = as_uint8_images(images, dev)
    H, W = _hw(size, (int(img.shape[1]), int(img.shape[2])))
    img = resize_nearest(img, H, W)
    scale = float(W) / float(output_wh)
    cols = None if part_tables is None else part_colours(part_tables, int(proj.shape[1])).to(dev)
    figs = {"input": img, "seg": seg_colour(scores, (W, H))}
    silh = pred.get("silhouette", pred.get("silh"))
    if silh is not None:
        figs["silh"] = seg_colour(silh, (W, H), lut=torch.tensor(SILH_LUT, dtype=torch.uint8))
    figs["projects"] = scatter_points(proj, (W, H), scale, radius=radius, colours=cols)
    figs["verts_overlay"] = scatter_points(proj, (W, H), scale, radius=radius, colours=cols, image=img)
    figs["seg_overlay"] = seg_colour(scores, (W, H), background=img, alpha=seg_alpha)
    if topo is not None:
        from .render import render_predictions
        figs["rend"] = to_uint8(render_predictions(pred, topo, img, output_wh)["rgb"])
    return figs


def prediction_panel(pred, images, output_wh, topo=None, part_tables=None, size=None, **kw):
    """`prediction_figures`' tiles side by side, (N, S, n S, 3) uint8, in the order input, seg[, silh], projects,
    verts_overlay, seg_overlay[, rend]."""
    figs = prediction_figures(pred, images, output_wh, topo=topo, part_tables=part_tables, size=size, **kw)
    return torch.cat([figs[k] for k in TILE_ORDER if k in figs], dim=2)


def write_png(path, array):
    """An 8-bit PNG from (H, W) grey, (H, W, 3) RGB or (H, W, 4) RGBA uint8 (tensor or array) with zlib and struct only."""
    a = array.detach().cpu().numpy() if isinstance(array, torch.Tensor) else np.asarray(array)
    if a.dtype != np.uint8 or a.ndim not in (2, 3) or (a.ndim == 3 and a.shape[2] not in (1, 3, 4)) or a.size == 0:
        raise ValueError("write_png takes (H, W), (H, W, 3) or (H, W, 4) uint8, got %s %s" % (a.shape, a.dtype))
    if a.ndim == 3 and a.shape[2] == 1:
        a = a[:, :, 0]
    H, W = a.shape[:2]
    ctype = {2: 0, 3: 2, 4: 6}[2 if a.ndim == 2 else a.shape[2]]
    rows = np.ascontiguousarray(a).reshape(H, -1)
    raw = np.concatenate([np.zeros((H, 1), np.uint8), rows], axis=1).tobytes()      # filter type 0 in front of every row

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xffffffff)
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, ctype, 0, 0, 0))
                + chunk(b"IDAT", zlib.compress(raw, 6)) + chunk(b"IEND", b""))
    return path


SAVED = (("seg", "_seg.png"), ("projects", "_projects.png"), ("rend", "_rend.png"), ("input", "_input.png"),
         ("verts_overlay", "_verts_overlay.png"))


def save_predictions(figs, fnames, save_dir):
    """predict.py:30-75's files for every image: {fname without extension}_seg.png, _projects.png, _rend.png (when figs has
    it), _input.png and _verts_overlay.png under save_dir -> the list of paths written."""
    n = int(figs["seg"].shape[0])
    if len(fnames) != n:
        raise ValueError("%d file names for %d images" % (len(fnames), n))
    os.makedirs(save_dir, exist_ok=True)
    host = {k: figs[k].cpu() for k, _ in SAVED if k in figs}
    out = []
    for i, fname in enumerate(fnames):
        stem, _ = os.path.splitext(os.path.basename(fname))
        for k, suffix in SAVED:
            if k in host:
                out.append(write_png(os.path.join(save_dir, stem + suffix), host[k][i]))
    return out


class MonitorFigures:
    """The monitor pictures of train.py:264-300 / train_stage2_silhouette.py:300-339 as a hook for
    `training.fit(on_trial_end=...)`: called as (trial, trainer) it runs `trainer.monitor(images)` and writes, for image i,
    seg_{trial}_{i}.png, verts_{trial}_{i}.png (the vertex scatter), silh_{trial}_{i}.png (with a silhouette head),
    rend_{trial}_{i}.png (with topo) and, at trial 0, image_{i}.png.  `written` lists the last call's paths."""

    NAMES = (("seg", "seg"), ("silh", "silh"), ("projects", "verts"), ("rend", "rend"))

    def __init__(self, images, save_dir, topo=None, part_tables=None, size=None, radius=0):
        self.images, self.save_dir = images, save_dir
        self.topo, self.part_tables, self.size, self.radius = topo, part_tables, size, radius
        self.written = []

    def __call__(self, trial, trainer):
        pred = trainer.monitor(self.images)
        figs = prediction_figures(pred, self.images, trainer.output_wh, topo=self.topo, part_tables=self.part_tables,
                                  size=self.size, radius=self.radius)
        os.makedirs(self.save_dir, exist_ok=True)
        host = {k: v.cpu() for k, v in figs.items()}
        self.written = []
        for i in range(int(host["seg"].shape[0])):
            for key, stem in self.NAMES:
                if key in host:
                    self.written.append(write_png(os.path.join(self.save_dir, "%s_%d_%d.png" % (stem, trial, i)), host[key][i]))
            if trial == 0:
                self.written.append(write_png(os.path.join(self.save_dir, "image_%d.png" % i), host["input"][i]))
        return figs
