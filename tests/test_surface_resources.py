"""csrc/surface.hip: both kernels of the dense surface-correspondence term, in both target dimensions, must build without
scratch and fit their launch - 1 024 lanes per row for the forward, 256 for the backward, whose only LDS is the four waves'
partial sums of dcam (D = 2).  Read from the built code object's metadata (tools/kernel_resources.py) - no GPU."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import kernel_resources as kr  # noqa: E402


def test_surface_kernels_use_no_scratch_and_fit_their_launch():
    hit = {n: k for n, k in kr.kernels().items() if "sc_fwd_kernel" in n or "sc_bwd_kernel" in n}
    assert len(hit) == 4, sorted(hit)
    assert sorted(("sc_fwd_kernel" in n, "ILi2E" in n) for n in hit) == [(False, False), (False, True), (True, False), (True, True)]
    for name, k in hit.items():
        fwd = "sc_fwd_kernel" in name
        assert k["scratch"] == 0, "%s spills %d B per lane" % (name, k["scratch"])
        assert k["max_threads"] >= (1024 if fwd else 256), name
        assert kr.waves_per_simd(k) >= (4 if fwd else 1), (name, k)          # (1 024 lanes: four waves on each SIMD)
        assert k["lds"] <= 1024, "%s: %d B of LDS per workgroup" % (name, k["lds"])
