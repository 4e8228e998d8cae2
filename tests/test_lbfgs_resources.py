"""lbfgs_step_kernel (csrc/lbfgs.hip) keeps q of the two-loop recursion in registers and parks the first loop's a_i and rho_i in
LDS: an array indexed by the pair in registers would go to scratch, and so would the launch's two dozen operands held
across prior_row.  Both forms, with and without the prior, must build without scratch and for a 256-thread workgroup.
Read from the built code object's metadata (tools/kernel_resources.py) - no GPU."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import kernel_resources as kr  # noqa: E402


def test_lbfgs_kernels_use_no_scratch():
    hit = {n: k for n, k in kr.kernels().items() if "lbfgs_step_kernel" in n}
    assert len(hit) == 2, sorted(hit)
    assert sorted("lbfgs_step_kernelILb1E" in n for n in hit) == [False, True]
    for name, k in hit.items():
        assert k["scratch"] == 0, "%s spills %d B per lane" % (name, k["scratch"])
        assert k["max_threads"] >= 256, name
        assert kr.waves_per_simd(k) >= 1, (name, k)
        # the loss tree, three sums in two copies and 2 x 16 doubles of the recursion; with the prior its own LDS beside them
        assert 2 * 4 * 8 + 2 * 3 * 4 * 8 + 2 * 16 * 8 <= k["lds"] <= 64 * 1024, "%s: %d B of LDS per workgroup" % (name, k["lds"])
