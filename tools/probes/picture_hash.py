"""Hashes of every output of the image gather kernels (csrc/augment.hip, csrc/preprocess.hip) and the picture kernels
(csrc/render.hip, csrc/figure.hip) for fixed seeded inputs through the Python fronts: run under two builds of the library
(SMPLR_LIB_PATH) to show a kernel change is bit-exact.  One sha256 line per (op, case, output) on stdout;
`HASH_PROBE=tools/probes/picture_hash.py bash tools/hash_ab.sh ENV_A ENV_B` or diff the stdout of two runs.  The cases are
the smallest that reach each path: vec4 and scalar stores, a partly idle last workgroup, an output 4 bytes off 16-B
alignment, every mode and channel count, a clamped index of both widths, partial tiles.  GPU only."""
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import ilps_amd  # noqa: E402,F401
from ilps_amd import augment, figures, preprocess as pp, render  # noqa: E402

DEV = torch.device("cuda", 0)
B = 3
SIZES = [(48, 48), (5, 7)]        # 576 groups of 4 columns: three workgroups, the last partly idle; 35 scalar threads


def emit(op, case, name, t):
    t = t.detach().cpu().contiguous()
    if t.dtype == torch.bool:
        t = t.to(torch.uint8)
    print("%-8s %-44s %-7s %s" % (op, case, name, hashlib.sha256(t.numpy().tobytes()).hexdigest()))


def outputs(shape, dtype):
    """[(tag, out)]: none given, and a contiguous tensor whose first byte lies 4 past a 16-B boundary."""
    n = int(np.prod(shape))
    return [("", None), ("+4B", torch.empty(n + 1, dtype=dtype, device=DEV)[1:].view(shape))]


def indices(N):
    """None, int32 and int64 with one value below 0 and one past the end."""
    v = [-2, 1, N + 94]
    return [("none", None), ("i32", torch.tensor(v, dtype=torch.int32, device=DEV)),
            ("i64", torch.tensor(v, dtype=torch.int64, device=DEV))]


def warp_cases():
    g = torch.Generator().manual_seed(11)
    N = 5
    draws = augment.random_draws(B, g, rotation_range=25, width_shift_range=0.2, height_shift_range=0.2, shear_range=0.3,
                                 zoom_range=0.3, horizontal_flip=True)
    for H, W in SIZES:
        M = augment.affine_matrices(draws, (H, W)).to(DEV)
        wild = M.clone()
        wild[0, 0, 0], wild[1, 1, 2], wild[2, 0, 1] = float("nan"), 1e30, -1e30
        for C in (1, 3):
            pool = torch.randint(0, 256, (N, H, W, C), dtype=torch.uint8, generator=g).to(DEV)
            for mode in ("nearest", "bilinear"):
                for iname, idx in indices(N):
                    for tag, out in outputs((B, C, H, W), torch.float32):
                        emit("warp", "%dx%d C%d %s idx=%s%s" % (H, W, C, mode, iname, tag), "image",
                             augment.warp_images(pool, M, (H, W), idx, 1 / 255., mode, out=out))
                emit("warp", "%dx%d C%d %s wild" % (H, W, C, mode), "image", augment.warp_images(pool, wild, (H, W), None, 1 / 255., mode))
        lab = torch.randint(0, 32, (N, H, W), dtype=torch.uint8, generator=g).to(DEV)
        for binarize in (False, True):
            for iname, idx in indices(N):
                for tag, out in outputs((B, H, W), torch.int32):
                    emit("warp", "%dx%d label bin=%d idx=%s%s" % (H, W, binarize, iname, tag), "label",
                         augment.warp_labels(lab, M, (H, W), idx, binarize, out=out))
            emit("warp", "%dx%d label bin=%d wild" % (H, W, binarize), "label", augment.warp_labels(lab, wild, (H, W), None, binarize))
    M = augment.affine_matrices(draws, 48).to(DEV)                      # a 64 x 64 pool read at 48 x 48
    pool = torch.randint(0, 256, (N, 64, 64, 3), dtype=torch.uint8, generator=g).to(DEV)
    emit("warp", "48x48 from 64x64 C3 nearest", "image", augment.warp_images(pool, M, 48, None, 1 / 255., "nearest"))
    emit("warp", "48x48 from 64x64 label", "label", augment.warp_labels(pool[..., 0].contiguous(), M, 48))


def resize_cases():
    rng = np.random.default_rng(12)
    shapes = [(101, 40), (40, 101), (64, 64)]
    for C in (1, 3):
        arrs = [rng.integers(0, 256, (h, w) + ((3,) if C == 3 else ()), dtype=np.uint8) for h, w in shapes]
        r = pp.RaggedImages.from_arrays(arrs, DEV)
        crop = r.crop([(3, 5, 60, 30), (2, 7, 30, 80), (1, 1, 40, 50)])          # pitch > w C
        bad = pp.RaggedImages(r.data, r.desc_host, C, desc=r.desc.clone())
        bad.desc[1, 0] = int(r.data.numel()) - 5                                  # this row ends past the buffer: zeros
        for H, W in SIZES:
            for pad in (False, True):
                for swap in ((False, True) if C == 3 else (False,)):
                    for quantize in (True, False):
                        emit("resize", "%dx%d C%d linear pad=%d swap=%d q=%d" % (H, W, C, pad, swap, quantize), "image",
                             pp.load_images(r, (H, W), pad=pad, swap_rb=swap, quantize=quantize))
                    for rule in ("cv2", "pil"):
                        emit("resize", "%dx%d C%d nearest pad=%d swap=%d %s" % (H, W, C, pad, swap, rule), "image",
                             pp.load_images(r, (H, W), pad=pad, swap_rb=swap, interpolation="nearest", nearest_rule=rule))
            for interp in ("linear", "nearest"):
                for iname, idx in indices(len(r)):
                    for tag, out in outputs((B, C, H, W), torch.float32):
                        emit("resize", "%dx%d C%d %s idx=%s%s" % (H, W, C, interp, iname, tag), "image",
                             pp.load_images(r, (H, W), idx, pad=True, interpolation=interp, out=out))
                for name, rr in (("crop", crop), ("bad-row", bad)):
                    emit("resize", "%dx%d C%d %s %s" % (H, W, C, interp, name), "image",
                         pp.load_images(rr, (H, W), pad=True, interpolation=interp))
            if C != 1:
                continue
            for binarize in (False, True):
                for rule in ("cv2", "pil"):
                    for pad in (False, True):
                        emit("resize", "%dx%d label bin=%d %s pad=%d" % (H, W, binarize, rule, pad), "label",
                             pp.load_labels(r, (H, W), pad=pad, nearest_rule=rule, binarize=binarize))
                for iname, idx in indices(len(r)):
                    for tag, out in outputs((B, H, W), torch.int32):
                        emit("resize", "%dx%d label bin=%d idx=%s%s" % (H, W, binarize, iname, tag), "label",
                             pp.load_labels(r, (H, W), idx, pad=True, binarize=binarize, out=out))
                for name, rr in (("crop", crop), ("bad-row", bad)):
                    emit("resize", "%dx%d label bin=%d %s" % (H, W, binarize, name), "label",
                         pp.load_labels(rr, (H, W), pad=True, binarize=binarize))


def mesh(rng):
    """60 vertices, 100 faces: an 8 x 7 grid with depth relief, four more vertices far to the right (the faces among them
    are off screen), 16 random faces across the grid; vertex 17 is NaN."""
    gx, gy = np.meshgrid(np.linspace(-1, 1, 8), np.linspace(-1, 1, 7))
    grid = np.stack([gx.ravel(), gy.ravel(), 3.0 + 0.5 * np.sin(3 * gx.ravel()) * np.cos(2 * gy.ravel())], 1)
    far = np.array([[8.0, -1, 3], [9, 1, 3], [8.5, 0, 2.5], [9.5, -0.5, 3.5]])
    v = np.concatenate([grid, far]).astype(np.float32)
    faces = []
    for i in range(6):
        for j in range(7):
            a = i * 8 + j
            faces += [(a, a + 1, a + 8), (a + 1, a + 9, a + 8)]
    faces += [(56, 57, 58)] + [tuple(rng.choice(56, 3, replace=False)) for _ in range(15)]
    return v, np.asarray(faces, np.int32)


def picture_cases():
    rng = np.random.default_rng(13)
    H, W, NB = 70, 130, 2                                                # 2 x 3 tiles, the right and bottom ones partial
    v, faces = mesh(rng)
    verts = np.stack([v, v * np.float32([0.9, 1.1, 1.0]) + np.float32([0.1, -0.05, 0.2])])
    verts[0, 17] = np.nan
    verts = torch.from_numpy(verts).to(DEV)
    topo = render.MeshTopology(faces, v.shape[0], face_part=(np.arange(len(faces)) % 32).astype(np.uint8))
    cams = {"ortho": torch.tensor([[60., 30., 65., 35.], [55., 28., 60., 36.]]),
            "perspective": torch.tensor([[170., 65., 35.], [150., 60., 38.]])}
    vcol = torch.from_numpy(rng.random((NB, v.shape[0], 3), dtype=np.float32)).to(DEV)
    bg = torch.from_numpy(rng.random((NB, H, W, 3), dtype=np.float32)).to(DEV)
    for mode, cam in cams.items():
        for shading, kw in (("lambert", {}), ("vertex", dict(vertex_colors=vcol, background=bg))):
            out = render.render_mesh(verts, topo, cam.to(DEV), mode=mode, img_wh=(W, H), shading=shading, **kw)
            for name in ("face", "depth", "part", "alpha", "rgb"):
                emit("render", "%s %s" % (mode, shading), name, out[name])

    proj = torch.from_numpy(rng.uniform(-5, 75, (NB, 60, 3)).astype(np.float32))
    proj[..., 0] *= W / 70.0
    proj[0, 3, 1], proj[1, 5, 2] = float("nan"), float("inf")
    proj[:, 10:14] = proj[:, 20:24]                                      # discs on one centre: the order decides
    proj[:, 10:14, 2] = torch.tensor([1.0, 1.0, -0.0, 0.0])
    proj = proj.to(DEV)
    keep = torch.from_numpy((rng.random((NB, 60)) > 0.2).astype(np.uint8)).to(DEV)
    colours = torch.from_numpy(rng.integers(0, 256, (60, 3), dtype=np.uint8))
    image = torch.from_numpy(rng.integers(0, 256, (NB, H, W, 3), dtype=np.uint8)).to(DEV)
    for radius in (0, 3):
        for order in ("index", "depth"):
            for name, kw in (("plain", {}), ("keep+colours+image", dict(keep=keep, colours=colours, image=image))):
                rgb, vertex = figures.scatter_points(proj, (W, H), 1.0, radius, order, return_vertex=True, **kw)
                emit("scatter", "r=%d %s %s" % (radius, order, name), "rgb", rgb)
                emit("scatter", "r=%d %s %s" % (radius, order, name), "vertex", vertex)

    bg8 = image
    for C in (32, 5):                                                    # float4 and scalar score reads
        s = torch.from_numpy(rng.standard_normal((NB, 24, 40, C)).astype(np.float32))
        s[0, 0, 0, 1], s[1, 2, 3, 0] = float("nan"), float("inf")
        for name, b in (("", None), (" bg", bg8)):
            emit("segcol", "scores C%d%s" % (C, name), "rgb", figures.seg_colour(s.to(DEV), (W, H), background=b))
    lab = torch.from_numpy(rng.integers(-1, 34, (NB, 24, 40)).astype(np.int32)).to(DEV)
    for name, b in (("", None), (" bg", bg8)):
        emit("segcol", "labels%s" % name, "rgb", figures.seg_colour(lab, (W, H), background=b, bad_colour=(9, 8, 7)))


def main():
    warp_cases()
    resize_cases()
    picture_cases()
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
