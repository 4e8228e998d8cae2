"""How many of the records the skinning backward is handed carry a gradient: the headline's input (bench.make_x, seed
1000, B = 128, W = 48) through the decoder's forward and _seg_bwd(..., merge=False), then per mesh the global records
(visible vertices, mask 1), the local ones (hidden, near a pixel centre), how many of each have a slot sum that is not
exactly (0, 0), and the records per 1 024-vertex chunk of skin_bwd_rec_kernel before and after that filter.
    python tools/probes/live_records.py [--batch 128] [--wh 48] [--meshes 8]"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import bench  # noqa: E402
from ilps_amd import _lib, ops  # noqa: E402
from ilps_amd.smpl_model import synthetic_smpl_model  # noqa: E402

CHUNK, NSLOT = 1024, 5 * 4096


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--wh", type=int, default=48)
    ap.add_argument("--meshes", type=int, default=8, help="meshes listed one by one (the totals cover the batch)")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    B, W = a.batch, a.wh
    c = ops.SMPLConstants.from_model(synthetic_smpl_model(1234), dev)
    pt = ops.get_part_table(1, dev, c.V)
    x = torch.tensor(bench.make_x(B, W, 1000), device=dev)
    dseg = torch.randn(B, W, W, 32, generator=torch.Generator(device="cpu").manual_seed(0)).to(dev)
    coef, Rs, J, A, Jt = ops._pose_fwd(x, 4, c)
    proj = ops._skin_fwd(ops._blend_fwd(coef, c, B), A, c, cam=x)[1]
    mask = ops.visibility(proj)
    vslot = torch.empty((B, pt.VP), dtype=torch.int16, device=dev)
    seg, arg, rec = ops._seg_fwd(proj, mask, W, pt, vslot=vslot)
    part, nsplit = ops._seg_bwd(dseg, arg, rec, pt.VP, W, pt, merge=False)
    P4 = part[:B * nsplit * NSLOT * 2].view(B, nsplit, NSLOT, 2)
    acc = P4[:, 0].clone()
    for s in range(1, nsplit):
        acc = acc + P4[:, s]
    torch.cuda.synchronize()
    vs_, acc, vis = vslot.cpu().numpy().astype(np.int64), acc.cpu().numpy(), mask.cpu().numpy() == 1.0
    has = vs_ >= 0
    sums = np.take_along_axis(acc, np.maximum(vs_, 0)[:, :, None], 1)              # (B, V, 2)
    live = has & ~((sums[..., 0] == 0) & (sums[..., 1] == 0))
    glob, loc = has & vis, has & ~vis
    print("# build %s%s  B=%d W=%d nsplit=%d" % (_lib.build_id()[:12], " (SMPLR_LIB_PATH)" if _lib.LIB_OVERRIDE else "",
                                                B, W, nsplit))
    print("# mesh | global records | local records | non-zero slot sum: global | local")
    for b in range(min(B, a.meshes)):
        print("%4d | %4d | %4d | %4d | %4d" % (b, glob[b].sum(), loc[b].sum(), (glob[b] & live[b]).sum(), (loc[b] & live[b]).sum()))
    print("batch: records %d (global %d, local %d); live %d (global %d, local %d) = %.1f %% of the records; "
          "live share of the local records %.1f %%"
          % (has.sum(), glob.sum(), loc.sum(), live.sum(), (glob & live).sum(), (loc & live).sum(),
             100.0 * live.sum() / has.sum(), 100.0 * (loc & live).sum() / max(loc.sum(), 1)))
    print("per mesh: records mean %.0f (min %d, max %d); live mean %.0f (min %d, max %d)"
          % (has.sum(1).mean(), has.sum(1).min(), has.sum(1).max(), live.sum(1).mean(), live.sum(1).min(), live.sum(1).max()))
    nch = -(-has.shape[1] // CHUNK)
    for name, m in (("all records", has), ("live records", live)):
        pad = np.zeros((B, nch * CHUNK), bool)
        pad[:, :m.shape[1]] = m
        k = pad.reshape(B, nch, CHUNK).sum(2).ravel()
        print("%s per %d-vertex chunk (%d chunks): median %d, p90 %d, max %d; chunks above 256: %d, above 128: %d"
              % (name, CHUNK, k.size, np.median(k), np.percentile(k, 90), k.max(), (k > 256).sum(), (k > 128).sum()))


if __name__ == "__main__":
    main()
