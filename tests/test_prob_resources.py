"""The probabilistic head's kernels (csrc/prob.hip) keep a lane's sums in registers: all six must build without scratch and
without spills; the five row kernels for their 256-thread workgroup at full occupancy (8 waves per SIMD: at most 64 VGPRs),
the spread kernel - 4 points, 16 fp64 sums and three 16-byte loads per sample and lane - for its one-wave workgroup with no
LDS and at most 128 VGPRs (4 waves per SIMD).  Read from the built code object's metadata (tools/kernel_resources.py) - no
GPU."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import kernel_resources as kr  # noqa: E402

ROW_KERNELS = ("prob_sample_fwd_kernel", "prob_sample_bwd_kernel", "prob_nll_fwd_kernel", "prob_nll_bwd_kernel", "prob_fuse_kernel")


def test_prob_kernels_use_no_scratch():
    hit = {n: k for n, k in kr.kernels().items() if "prob_" in n and n.split("prob_")[1].split("_kernel")[0] in
           ("sample_fwd", "sample_bwd", "nll_fwd", "nll_bwd", "fuse", "spread")}
    assert len(hit) == 6, sorted(hit)
    for name, k in hit.items():
        assert k["scratch"] == 0, "%s spills %d B per lane" % (name, k["scratch"])
        assert k.get("sgpr_spills", 0) == 0 and k.get("vgpr_spills", 0) == 0, (name, k)
        if any(r in name for r in ROW_KERNELS):
            assert k["max_threads"] >= 256, name
            assert kr.waves_per_simd(k) == 8 and k["vgpr"] + k["agpr"] <= 64, (name, k)
            assert k["lds"] <= 4096, "%s: %d B of LDS per workgroup" % (name, k["lds"])
        else:
            assert "prob_spread_kernel" in name and k["lds"] == 0, (name, k)
            assert k["vgpr"] + k["agpr"] <= 128 and kr.waves_per_simd(k) >= 4, (name, k)
