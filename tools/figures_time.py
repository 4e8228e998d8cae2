"""Timing of the figure launches (csrc/figure.hip through figures.seg_colour / figures.scatter_points), one GPU:
    python tools/figures_time.py [--iters N]
At B in {1, 16, 128} and 256 x 256 pictures, from (B, 48, 48, 32) scores and the (B, 6 890, 3) projections of an SMPL-sized
mesh (the sphere of tests/_render_oracle.py, projected with render_time.py's camera at 48 x 48 and drawn at scale
256 / 48), radius 1.  Event pairs around N back-to-back calls after a warm-up, so dispatch gaps and the Python argument
handling are included; for the kernels alone run it under `rocprofv3 --kernel-trace --stats -- python ...`.  Per shape, in
us per call:
    seg / seg_overlay         figures.seg_colour, plain and over the image
    scatter / scatter_r0      figures.scatter_points over the image, radius 1 and 0, per-vertex colours
    torch_seg                 the seg picture from stock torch device ops: argmax + table lookup + index upsample
    torch_scatter_r0          the radius-0 overlay from stock torch device ops: blend + round + index_put_ (the last
                              write wins in an order torch does not define: not the same picture where vertices collide)
    render_mesh               the triangle render of the same mesh at the same size (render.render_mesh, all outputs)
and the build id of the library the figures come from."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ilps_amd  # noqa: E402,F401


def timed(fn, iters, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1000.0 / iters          # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    a = ap.parse_args()
    import _render_oracle as ro
    from ilps_amd import _lib, figures
    from ilps_amd.render import MeshTopology, render_mesh
    dev = torch.device("cuda:0")
    S, W = 256, 48
    v, f = ro.posed_sphere(0, 128)
    topo = MeshTopology(f, v.shape[1])
    verts = torch.from_numpy(v).to(dev)
    V = int(verts.shape[1])
    g = torch.Generator(device="cpu").manual_seed(0)
    cols = torch.randint(0, 256, (V, 3), generator=g, dtype=torch.uint8).to(dev)
    lut = figures.default_lut().to(dev)
    scale = S / W
    res = {"build_id": _lib.build_id()[:16], "size": S, "radius": 1, "iters": a.iters}
    for B in (1, 16, 128):
        vb = verts[:B].contiguous()
        cam = torch.tensor([0.3 * S, 0.3 * S, S / 2, S / 2], device=dev).expand(B, 4).contiguous()
        # (u, v, z) at the decoder's 48 x 48, as orthographic_project gives them
        proj = torch.stack([(0.3 * W) * vb[..., 0] + W / 2, (0.3 * W) * vb[..., 1] + W / 2, vb[..., 2]], -1).contiguous()
        scores = torch.randn(B, W, W, 32, generator=g).to(dev)
        img = torch.randint(0, 256, (B, S, S, 3), generator=g, dtype=torch.uint8).to(dev)
        ri = (torch.arange(S, device=dev) * W) // S
        bidx = torch.arange(B, device=dev)[:, None].expand(B, V)

        def torch_seg():
            return lut[scores.argmax(dim=-1)][:, ri][:, :, ri]

        def torch_scatter_r0():
            out = ((230 * img.to(torch.int32) + 26 * 255 + 128) >> 8).to(torch.uint8)
            cx = torch.round(proj[..., 0] * scale).long().clamp_(0, S - 1)
            cy = (S - 1 - torch.round(proj[..., 1] * scale).long()).clamp_(0, S - 1)
            out.index_put_((bidx, cy, cx), cols.expand(B, V, 3))
            return out

        row = {"seg": timed(lambda: figures.seg_colour(scores, S, lut=lut), a.iters),
               "seg_overlay": timed(lambda: figures.seg_colour(scores, S, lut=lut, background=img), a.iters),
               "scatter": timed(lambda: figures.scatter_points(proj, S, scale, radius=1, colours=cols, image=img), a.iters),
               "scatter_r0": timed(lambda: figures.scatter_points(proj, S, scale, radius=0, colours=cols, image=img), a.iters),
               "torch_seg": timed(torch_seg, a.iters),
               "torch_scatter_r0": timed(torch_scatter_r0, a.iters),
               "render_mesh": timed(lambda: render_mesh(vb, topo, cam, img_wh=S), a.iters)}
        res["B%d" % B] = {k: round(us, 1) for k, us in row.items()}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
