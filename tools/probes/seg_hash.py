"""Hashes of the segmentation raster's outputs for fixed seeded inputs (several W, B, mesh scales, vertex
samplings): run under two builds of the library to show a kernel change is bit-exact.  GPU only.
Per case: one line for the two-call path, then - where the case fits the binning kernel that skins its own vertices -
one line per value of SMPLR_SEG_BIN_WALK for that entry point (verts, proj, mask, seg, goff, lstart, the far-reaching
section of rec with its header, the nearest-pixel records sorted by (pixel, vertex)), and one for ops.visibility."""
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


def skin_line(on, v_posed, A, consts, x, W, pt):
    """The skinning + binning + raster entry point under SMPLR_SEG_BIN_WALK = on -> its hashes, in the order of the
    module docstring."""
    before = os.environ.get("SMPLR_SEG_BIN_WALK")
    os.environ["SMPLR_SEG_BIN_WALK"] = on
    lib = _lib.load()
    B, V, P, K, npix = v_posed.shape[0], consts.V, pt.P, pt.K, W * W
    ws = ops._workspace(lib.smplr_seg_workspace(B, V, W, P, K), v_posed)
    e = lambda shape, dt=torch.float32: torch.zeros(shape, dtype=dt, device=v_posed.device)
    o = dict(verts=e((B, V, 3)), proj=e((B, V, 3)), mask=e((B, V)), seg=e((B, W, W, P + 1)),
             arg=e((B, W, W, 32), torch.int16), rec=e((B, lib.smplr_seg_slots(P, K), 4)), vslot=e((B, V), torch.int16))
    ops._skin_vis_seg_call(v_posed, A, consts, x, W, pt, 64, True, ws, **o)
    torch.cuda.synchronize()
    if before is None:
        del os.environ["SMPLR_SEG_BIN_WALK"]
    else:
        os.environ["SMPLR_SEG_BIN_WALK"] = before
    # the workspace's views (csrc/raster_common.h, seg_ws_layout): goff (B, P + 34) | lstart (B, npix + 1) | lrec
    raw = ws.view(torch.int32).cpu().numpy()
    up = lambda nbytes: (nbytes + 255) // 256 * 256
    gs = P + 2 + 32
    o1 = up(B * gs * 4) // 4
    goff = raw[:B * gs].reshape(B, gs)[:, :2 * P + 2]
    lstart = raw[o1:o1 + B * (npix + 1)].reshape(B, npix + 1)
    rec = o["rec"].cpu().numpy().view(np.int32)
    far, near = [], []
    for n in range(B):
        f, L = int(goff[n, P]), int(lstart[n, npix])
        far.append(rec[n, :f])
        far.append(rec[n, -1:])
        pix = np.repeat(np.arange(npix), np.diff(lstart[n]))
        near.append(rec[n, f:f + L][np.lexsort((rec[n, f:f + L, 3], pix))])
    hb = lambda a: hashlib.sha1(np.ascontiguousarray(a).tobytes()).hexdigest()[:12]
    return " ".join([h(o[k]) for k in ("verts", "proj", "mask", "seg")] +
                    [hb(goff), hb(lstart), hb(np.concatenate(far)), hb(np.concatenate(near))])


def main():
    dev = torch.device("cuda", 0)
    model = synthetic_smpl_model(1234)
    consts = ops.SMPLConstants.from_model(model, dev)
    for W, B, vs, scale in [(48, 16, 1, 1.0), (48, 5, 1, 2.5), (64, 8, 1, 1.0), (32, 4, 1, 1.0), (96, 3, 1, 1.0),
                            (48, 6, 2, 1.0), (40, 3, 1, 0.5), (128, 2, 1, 1.0), (48, 4, 1, 6.0),
                            # (batches that take the large block shape by default)
                            (48, 128, 1, 1.0), (48, 70, 1, 1.3), (64, 37, 1, 1.0)]:
        pt = ops.get_part_table(vs, dev, consts.V)
        xn = bench.make_x(B, W, 7 + W + B)
        xn[:, 0] *= scale                      # camera scale: bigger mesh -> more visible records
        x = torch.tensor(xn, device=dev)
        coef, Rs, J, A, Jt = ops._pose_fwd(x, 4, consts)
        v_posed = ops._blend_fwd(coef, consts, B)
        verts, proj = ops._skin_fwd(v_posed, A, consts, cam=x, vertex_sampling=vs)
        mask, seg, arg, rec = ops._vis_seg_fwd(proj, W, pt)
        # seg from an explicit mask with everything visible (long record lists) and with nothing visible
        # slot ids of the visibility path depend on the (atomic) order of the local lists: hash the vertices
        outs = [seg, ops.argmin_vertices(arg, rec), arg[..., 0]]
        for m in (torch.ones_like(mask), torch.zeros_like(mask)):
            s2, a2, r2 = ops._seg_fwd(proj, m, W, pt)[:3]
            outs += [s2, a2]
        torch.cuda.synchronize()
        print("W=%d B=%d vs=%d scale=%.1f vis=%.0f :" % (W, B, vs, scale, float(mask.float().sum() / B)),
              " ".join(h(o) for o in outs), "bg-sum %.6f" % float(seg[..., 0].double().sum()))
        if vs == 1 and _lib.load().smplr_skin_vis_seg_fits(consts.V, W, 64) == 1:
            for on in ("1", "0"):
                print("  skin+bin WALK=%s :" % on, skin_line(on, v_posed, A, consts, x, W, pt))
        print("  visibility :", h(ops.visibility(proj)))


if __name__ == "__main__":
    main()
