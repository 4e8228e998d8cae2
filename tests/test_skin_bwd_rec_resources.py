"""skin_bwd_rec_kernel counts on FIVE 256-thread workgroups per CU (the large batch is bound by the workgroups in flight:
DESIGN.md section 3): five waves per SIMD, no scratch, and five LDS allotments (1 280-B granules) within a CU's 160 KB.
Read from the built code object's metadata (tools/kernel_resources.py) - no GPU."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import kernel_resources as kr  # noqa: E402


def test_skin_bwd_rec_fits_five_workgroups_per_cu():
    hit = {n: k for n, k in kr.kernels().items() if "skin_bwd_rec_kernel" in n}
    assert len(hit) == 1, sorted(hit)
    for name, k in hit.items():
        assert k["scratch"] == 0, "%s spills %d B per lane" % (name, k["scratch"])
        assert k["max_threads"] >= 256, name
        assert kr.waves_per_simd(k) >= 5, "%s: %d registers, %d waves per SIMD" % (name, k["vgpr"], kr.waves_per_simd(k))
        assert 5 * (-(-k["lds"] // 1280) * 1280) <= 160 * 1024, "%s: %d B of LDS per workgroup" % (name, k["lds"])
