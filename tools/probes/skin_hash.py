"""Hashes of the skinning kernels' outputs for fixed seeded inputs: run under two builds of the library (SMPLR_LIB_PATH)
to show a change of skin.hip / skin_device.h is bit-exact.  One line per output: the forward (sparse and dense weights,
vertex sampling 1 and 5), dx of the fused backward over the vertices (dverts, dverts + dproj, dproj + the segmentation
slot sums) and over the records (the slot sums alone: two, four, six and seven row blocks, more than 4 096 records),
and the skinning outputs of the binning kernel that skins its own vertices.  GPU only."""
import dataclasses
import hashlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import bench  # noqa: E402
from ilps_amd import ops  # noqa: E402
from ilps_amd.smpl_model import synthetic_smpl_model  # noqa: E402


def h(t):
    return hashlib.sha1(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()[:16]


def main():
    dev = torch.device("cuda", 0)
    sparse = ops.SMPLConstants.from_model(synthetic_smpl_model(1234), dev)
    dense = dataclasses.replace(sparse, lbs_top4=None)
    V = sparse.V
    tn = lambda rng, *s: torch.tensor(rng.normal(0, 1, s).astype(np.float32), device=dev)

    def pose(B, W, seed):
        x = torch.tensor(bench.make_x(B, W, seed), device=dev)
        coef, Rs, J, A, Jt = ops._pose_fwd(x, 4, sparse)
        return x, Rs, J, A, ops._blend_fwd(coef, sparse, B)

    # ---- forward, and the backward over the vertices
    B, W = 3, 48
    x, Rs, J, A, vp = pose(B, W, 5)
    for name, c in (("sparse", sparse), ("dense", dense)):
        for vs in (1, 5):
            verts, proj = ops._skin_fwd(vp, A, c, cam=x, vertex_sampling=vs)
            rng = np.random.default_rng(40 + vs)
            dverts, dproj = tn(rng, B, V, 3), tn(rng, B, proj.shape[1], 3)
            dx1 = ops._smpl_bwd(x, 4, c, Rs, J, A, vp, dverts, None, None, vs)
            dx2 = ops._smpl_bwd(x, 4, c, Rs, J, A, vp, dverts, dproj, None, vs)
            torch.cuda.synchronize()
            print("skin_fwd %s vs=%d: verts %s proj %s" % (name, vs, h(verts), h(proj)))
            print("smpl_bwd %s vs=%d: dx(dverts) %s dx(dverts + dproj) %s" % (name, vs, h(dx1), h(dx2)))

    # ---- the segmentation slot sums: with dproj on the per-vertex kernel, alone on the record kernel
    for W, B, vs, ones in [(48, 3, 1, False), (50, 2, 2, False), (64, 2, 1, True), (16, 3, 1, False), (64, 130, 1, False)]:
        pt = ops.get_part_table(vs, dev, V)
        x, Rs, J, A, vp = pose(B, W, 11 + W + B)
        verts, proj = ops._skin_fwd(vp, A, sparse, cam=x, vertex_sampling=vs)
        VP = proj.shape[1]
        mask = torch.ones((B, VP), device=dev) if ones else ops.visibility(proj)
        vslot = torch.empty((B, VP), dtype=torch.int16, device=dev)
        seg, arg, rec = ops._seg_fwd(proj, mask, W, pt, vslot=vslot)
        g = tn(np.random.default_rng(23), B, W, W, 32)
        part, nsplit = ops._seg_bwd(g, arg, rec, VP, W, pt, merge=False, deterministic=True)
        dproj = tn(np.random.default_rng(24), B, VP, 3)
        dx_rec = ops._smpl_bwd(x, 4, sparse, Rs, J, A, vp, None, None, None, vs, seg_grad=(part, vslot, nsplit))
        dx_ver = ops._smpl_bwd(x, 4, sparse, Rs, J, A, vp, None, dproj, None, vs, seg_grad=(part, vslot, nsplit))
        torch.cuda.synchronize()
        # (the slot ids of the local records depend on seg_bin's atomic order from run to run: the arg-min is hashed as
        # vertices; dx gathers the sums by vertex and does not see the ids)
        print("W=%d B=%d vs=%d mask=%s nsplit=%d records/mesh %d: argmin %s dx(records) %s dx(dproj + slot sums) %s"
              % (W, B, vs, "ones" if ones else "vis", nsplit, int((vslot >= 0).sum()) // B,
                 h(ops.argmin_vertices(arg, rec)), h(dx_rec), h(dx_ver)))

    # ---- the binning kernel that skins its own vertices
    B, W = 5, 48
    x, Rs, J, A, vp = pose(B, W, 77)
    verts, proj, mask = ops._skin_vis_seg_fwd(vp, A, sparse, x, W, ops.get_part_table(1, dev, V))[:3]
    torch.cuda.synchronize()
    print("skin_vis_seg_fwd B=%d W=%d: verts %s proj %s mask %s" % (B, W, h(verts), h(proj), h(mask)))


if __name__ == "__main__":
    main()
