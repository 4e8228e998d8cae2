"""Hashes of the blend GEMM kernels' outputs for fixed seeded inputs on the synthetic model: run under two builds of the
library (SMPLR_LIB_PATH) to show a change of blend.hip / blend3.hip / blend_device.h / pose_device.h is bit-exact.
One line per output: the packed constants, then per batch size both forward GEMMs, the fused pose + blend forward,
smplr_coef3_pack against the fragments smplr_pose_fwd writes (live rows only), both backward GEMMs, and dx of
smplr_smpl_bwd with each GEMM.  B = 1, 37, 128, 200, 513, 1024 (or the list on the command line).  GPU only."""
import hashlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import bench  # noqa: E402
from ilps_amd import _lib, ops  # noqa: E402
from ilps_amd._lib import check, ptr, stream  # noqa: E402
from ilps_amd.smpl_model import synthetic_smpl_model  # noqa: E402


def h(t):
    return hashlib.sha1(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()[:16]


def main():
    batches = [int(a) for a in sys.argv[1:]] or [1, 37, 128, 200, 513, 1024]
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    c3 = ops.SMPLConstants.from_model(synthetic_smpl_model(1234), dev).pack_blend3()
    c1 = c3.fp32_gemm()
    V, N3 = c3.V, 3 * c3.V
    print("blend3_pack: fwd %s bwd %s" % (h(c3.blend3_fwd), h(c3.blend3_bwd)))
    for B in batches:
        x = torch.tensor(bench.make_x(B, 48, 50 + B), device=dev)
        coef, Rs, J, A, Jt = ops._pose_fwd(x, 4, c3, want="both")
        vp1, vp3 = ops._blend_fwd(coef, c1, B), ops._blend_fwd(coef, c3, B)
        fused = ops._pose_blend_fwd(x, 4, c3)
        f3 = torch.empty_like(coef.frag3)
        check(lib.smplr_coef3_pack(ptr(coef.kmajor), B, ptr(f3), stream()), "smplr_coef3_pack")
        rows = torch.arange(64, device=dev) % 32 + 32 * torch.arange((B + 31) // 32, device=dev)[:, None, None, None]
        live = (rows < B).expand(-1, 14, 3, -1)
        frag = lambda f: f.view(-1, 14, 3, 64, 16)[live]
        torch.cuda.synchronize()
        print("B=%d fwd: blend %s blend3 %s fused %s | coef3: pose_fwd %s coef3_pack %s"
              % (B, h(vp1), h(vp3), " ".join(h(o) for o in fused), h(frag(coef.frag3)), h(frag(f3))))
        g = torch.tensor(np.random.default_rng(60 + B).normal(0, 1, (B, V, 3)).astype(np.float32), device=dev)
        dc1, dc3 = torch.empty(B, 220, device=dev), torch.empty(B, 220, device=dev)
        ws1 = torch.empty(lib.smplr_blend_bwd_workspace(B, N3) // 4 + 1, device=dev)
        ws3 = torch.empty(lib.smplr_blend3_bwd_workspace(B, N3) // 4 + 1, device=dev)
        check(lib.smplr_blend_bwd(ptr(g), ptr(c1.blend_t), B, N3, ptr(dc1), ptr(ws1), stream()), "smplr_blend_bwd")
        check(lib.smplr_blend3_bwd(ptr(g), ptr(c3.blend3_bwd), B, N3, ptr(dc3), ptr(ws3), stream()), "smplr_blend3_bwd")
        dx1 = ops._smpl_bwd(x, 4, c1, Rs, J, A, vp3, g, None, None)
        dx3 = ops._smpl_bwd(x, 4, c3, Rs, J, A, vp3, g, None, None)
        torch.cuda.synchronize()
        print("B=%d bwd: blend %s blend3 %s | smpl_bwd dx: blend %s blend3 %s" % (B, h(dc1), h(dc3), h(dx1), h(dx3)))


if __name__ == "__main__":
    main()
