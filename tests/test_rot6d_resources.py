"""rot6d_fwd_kernel and rot6d_bwd_kernel (csrc/rot6d.hip) hold a joint's frame, quaternion and gradient in registers: both must
build without scratch and without LDS, for their 256-thread workgroup, at full occupancy (8 waves per SIMD: at most 64 VGPRs).  Read from the built code object's metadata
(tools/kernel_resources.py) - no GPU."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import kernel_resources as kr  # noqa: E402


def test_rot6d_kernels_use_no_scratch():
    hit = {n: k for n, k in kr.kernels().items() if "rot6d_fwd_kernel" in n or "rot6d_bwd_kernel" in n}
    assert len(hit) == 2, sorted(hit)
    for name, k in hit.items():
        assert k["scratch"] == 0, "%s spills %d B per lane" % (name, k["scratch"])
        assert k.get("sgpr_spills", 0) == 0 and k.get("vgpr_spills", 0) == 0, (name, k)
        assert k["lds"] == 0, "%s: %d B of LDS per workgroup" % (name, k["lds"])
        assert k["max_threads"] >= 256, name
        assert kr.waves_per_simd(k) == 8 and k["vgpr"] + k["agpr"] <= 64, (name, k)
