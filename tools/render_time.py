"""Timing of the triangle renderer (csrc/render.hip through render.render_mesh), one GPU:
    python tools/render_time.py [--iters N]
An SMPL-sized mesh (the 84 x 82 UV sphere of tests/_render_oracle.py: V = 6 890, F = 13 776), posed per batch row and
filling about a fifth of the image, Lambert shading, all five outputs, ortho camera, at B in {1, 16, 128} and
H = W in {224, 256, 512}.  Prints us per call (event pairs around N back-to-back calls, dispatch gaps and the Python
argument handling included; for the kernels alone run it under `rocprofv3 --kernel-trace --stats -- python ...`) and the
bytes written per pixel (face 4 + depth 4 + part 1 + alpha 1 + rgb 12 = 22 B) with the bandwidth that amounts to."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ilps_amd  # noqa: E402,F401

OUT_BYTES_PER_PX = 4 + 4 + 1 + 1 + 12


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
    from ilps_amd.render import MeshTopology, render_mesh
    dev = torch.device("cuda:0")
    v, f = ro.posed_sphere(0, 128)
    topo = MeshTopology(f, v.shape[1])
    verts = torch.from_numpy(v).to(dev)
    res = {}
    for B in (1, 16, 128):
        for S in (224, 256, 512):
            cam = torch.tensor([0.3 * S, 0.3 * S, S / 2, S / 2], device=dev).expand(B, 4).contiguous()
            vb = verts[:B].contiguous()
            us = timed(lambda: render_mesh(vb, topo, cam, img_wh=S), a.iters)
            mb = B * S * S * OUT_BYTES_PER_PX / 1e6
            res["B%d_%d" % (B, S)] = {"us": round(us, 1), "B_per_px": OUT_BYTES_PER_PX, "MB_written": round(mb, 2),
                                      "GB_per_s": round(mb * 1e3 / us, 1)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
