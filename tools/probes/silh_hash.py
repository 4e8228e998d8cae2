"""Hashes of the silhouette rasteriser's outputs (scores + arg-max vertices) for fixed seeded inputs - decoder
meshes at several W / camera scales, the reference's rand * 80 recipe, sparse meshes, meshes entirely outside the
cell window - run under two builds of the library to show a kernel change is bit-exact; plus HIP-event timings.
Also: the same body in all four forward forms (padded with parked vertices), the hint route, the deterministic
backward of both kinds at 4 and 2 workgroups per mesh, and the loss head as epilogue and as a kernel of its own.
GPU only: python tools/probes/silh_hash.py"""
import hashlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import bench  # noqa: E402
from ilps_amd import _lib, ops  # noqa: E402
from ilps_amd.smpl_model import synthetic_smpl_model  # noqa: E402


def h(t):
    return hashlib.sha1(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()[:12]


def first_vp_of_form(want, W, lo, hi):
    """The smallest VP in (lo, hi] that smplr_silh_fwd_form sends to `want` (form(lo) < want <= form(hi))."""
    form = _lib.load().smplr_silh_fwd_form
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if form(mid, W) >= want else (mid, hi)
    return hi


def pad(p, VP):
    out = torch.full((p.shape[0], VP, 3), 1e6, device=p.device)         # parked vertices: they never win a pixel
    out[:, :p.shape[1]] = p
    return out.contiguous()


def decoder_proj(consts, B, W, seed, dev):
    x = torch.tensor(bench.make_x(B, W, seed), device=dev)
    coef, Rs, J, A, Jt = ops._pose_fwd(x, 4, consts)
    return ops._skin_fwd(ops._blend_fwd(coef, consts, B), A, consts, cam=x)[1].contiguous()


def forms_hint_backward_loss(consts, dev):
    form = _lib.load().smplr_silh_fwd_form
    g = torch.Generator().manual_seed(5)
    # forward, all four forms
    body = decoder_proj(consts, 3, 48, 71, dev)
    vp1 = first_vp_of_form(1, 48, body.shape[1], 8192)
    for W, proj in ((48, body), (48, pad(body, vp1)), (48, pad(body, 8193)), (64, decoder_proj(consts, 3, 64, 72, dev))):
        silh, arg = ops._silh_fwd(proj, W)
        print("form %d W=%d VP=%-5d        silh %s arg %s" % (form(proj.shape[1], W), W, proj.shape[1], h(silh), h(arg)))
    # hint route: a score exp(-1.25 d) <= exp(-d) of the nearest vertex, from the silhouette itself
    silh, arg = ops._silh_fwd(body, 48)
    hs, ha = ops._silh_fwd(body, 48, hint=(silh[..., 1] ** 1.5).contiguous())
    print("%-28s silh %s arg %s" % ("hint W=48", h(hs), h(ha)))
    # deterministic backward of both kinds, 4 and 2 workgroups per mesh; one pixel of dsilh is (2^20, 2^20): g = 0 there,
    # but it is part of the population the scale of silh_bwd_kernel scans
    for B in (3, 128):
        proj = decoder_proj(consts, B, 48, 80 + B, dev)
        silh, arg = ops._silh_fwd(proj, 48)
        dsilh = torch.randn(B, 48, 48, 2, generator=g)
        dsilh[0, 20, 17] = 2.0 ** 20
        dloss = torch.randn(B, 48 * 48, generator=g).to(dev)
        k = torch.randn(B, 48 * 48, generator=g).to(dev)
        print("det backward B=%-3d           silh_bwd %s silh_loss_bwd %s"
              % (B, h(ops._silh_bwd(dsilh.to(dev), silh, arg, proj, 48, True)),
                 h(ops._silh_loss_bwd(dloss, k, silh, arg, proj, 48, True))))
    # loss head, as silh_px_kernel's epilogue and as the kernel behind the forward
    labels = torch.randint(-1, 3, (3, 48, 48), generator=g, dtype=torch.int32).to(dev)     # also outside {0, 1}
    class_w = torch.tensor([0.7, 1.9], device=dev)
    saved = os.environ.get("SMPLR_SILH_LOSS_EPILOGUE")
    for epi in ("0", "1"):
        os.environ["SMPLR_SILH_LOSS_EPILOGUE"] = epi
        conf = torch.zeros(3, 2, dtype=torch.int64, device=dev)
        silh, arg, loss, k = ops._silh_fwd_loss(body, 48, labels, class_w, 2.0, conf=conf)
        print("loss head epilogue=%s         loss %s k %s conf %s silh %s" % (epi, h(loss), h(k), h(conf), h(silh)))
    if saved is None:
        del os.environ["SMPLR_SILH_LOSS_EPILOGUE"]
    else:
        os.environ["SMPLR_SILH_LOSS_EPILOGUE"] = saved


def main():
    dev = torch.device("cuda", 0)
    consts = ops.SMPLConstants.from_model(synthetic_smpl_model(1234), dev)
    cases = []
    for W, B, scale in [(48, 16, 1.0), (48, 5, 2.5), (48, 4, 0.3), (40, 3, 1.0), (33, 3, 1.0), (24, 2, 1.0), (16, 2, 4.0),
                        (48, 3, 8.0), (64, 3, 1.0)]:
        xn = bench.make_x(B, W, 11 + W + B)
        xn[:, 0:2] *= scale
        x = torch.tensor(xn, device=dev)
        coef, Rs, J, A, Jt = ops._pose_fwd(x, 4, consts)
        proj = ops._skin_fwd(ops._blend_fwd(coef, consts, B), A, consts, cam=x)[1]
        cases.append(("decoder W=%d B=%d scale=%g" % (W, B, scale), proj, W))
    g = torch.Generator().manual_seed(3)
    cases.append(("rand*80 W=48", (torch.rand(2, 6890, 3, generator=g) * 80.0).to(dev), 48))
    cases.append(("rand*80-16 W=48", (torch.rand(2, 6890, 3, generator=g) * 80.0 - 16.0).to(dev), 48))
    cases.append(("all outside W=48", (torch.rand(2, 6890, 3, generator=g) * 10.0 + 300.0).to(dev), 48))
    sp = torch.full((2, 6890, 3), 1e4)
    sp[:, :5] = torch.rand(2, 5, 3, generator=g) * 48
    cases.append(("5 vertices W=48", sp.to(dev), 48))
    lat = torch.zeros(1, 6890, 3)
    lat[0, :, 0] = (torch.arange(6890) % 83) * 0.5 + 3.25          # many vertices exactly on half-cell borders / equal keys
    lat[0, :, 1] = (torch.arange(6890) // 83) * 0.5 + 2.5
    cases.append(("lattice ties W=48", lat.to(dev), 48))
    for name, proj, W in cases:
        proj = proj.contiguous()
        silh, arg = ops._silh_fwd(proj, W)
        torch.cuda.synchronize()
        print("%-28s silh %s arg %s" % (name, h(silh), h(arg)))
    forms_hint_backward_loss(consts, dev)
    # timing at the bench's size
    x = torch.tensor(bench.make_x(128, 48, 1000), device=dev)
    coef, Rs, J, A, Jt = ops._pose_fwd(x, 4, consts)
    proj = ops._skin_fwd(ops._blend_fwd(coef, consts, 128), A, consts, cam=x)[1]
    st = torch.cuda.current_stream()
    out = ops._silh_fwd(proj, 48)
    t = bench.graph_time_ms(lambda: ops._silh_fwd(proj, 48, out=out), 20, st)
    sys.stderr.write("silh_fwd B=128 W=48: %.2f us\n" % (t * 1e3))


if __name__ == "__main__":
    main()
