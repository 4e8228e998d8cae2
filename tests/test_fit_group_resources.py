"""fit_group_kernel (csrc/fit.hip) walks a group's rows in a loop with every row's gradient parked in LDS: an array indexed by
the row in registers would go to scratch.  Both forms, with and without the prior, must build without scratch, for a
256-thread workgroup, with the 16 x 256 floats of the stash and the prior's LDS within a workgroup's 64 KB.
Read from the built code object's metadata (tools/kernel_resources.py) - no GPU."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import kernel_resources as kr  # noqa: E402


def test_fit_group_kernels_use_no_scratch():
    hit = {n: k for n, k in kr.kernels().items() if "fit_group_kernel" in n}
    assert len(hit) == 2, sorted(hit)
    assert sorted("fit_group_kernelILb1E" in n for n in hit) == [False, True]
    for name, k in hit.items():
        assert k["scratch"] == 0, "%s spills %d B per lane" % (name, k["scratch"])
        assert k["max_threads"] >= 256, name
        assert kr.waves_per_simd(k) >= 1, (name, k)
        assert 16 * 256 * 4 <= k["lds"] <= 64 * 1024, "%s: %d B of LDS per workgroup" % (name, k["lds"])
