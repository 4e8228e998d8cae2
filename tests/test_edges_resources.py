"""The edge kernels (csrc/edges.hip) keep a handful of integers per lane: every instantiation builds without scratch and
without spills, for the workgroup it is launched with (256 threads for the sixteen classify forms - 4 sources x blur x L2 -
and up to 1024 for the link kernel, whose bit planes are dynamic LDS, so that its static share stays far inside 64 KB).
Read from the built code object's metadata (tools/kernel_resources.py) - no GPU."""
import os
import re
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import kernel_resources as kr  # noqa: E402


def test_edge_kernels_use_no_scratch():
    ks = kr.kernels()
    classify = {n: k for n, k in ks.items() if "edge_classify_kernel" in n}
    link = {n: k for n, k in ks.items() if "edge_link_kernel" in n}
    forms = sorted(re.search(r"edge_classify_kernelILi(\d)ELi(\d)ELi(\d)E", n).groups() for n in classify)
    assert forms == sorted((str(s), str(b), str(l)) for s in range(4) for b in range(2) for l in range(2)), forms
    assert len(link) == 1, sorted(link)
    for name, k in list(classify.items()) + list(link.items()):
        assert k["scratch"] == 0, "%s spills %d B per lane" % (name, k["scratch"])
        assert k.get("sgpr_spills", 0) == 0 and k.get("vgpr_spills", 0) == 0, (name, k)
    for name, k in classify.items():
        assert k["max_threads"] >= 256, name
        assert k["lds"] <= 16 * 1024, "%s: %d B of LDS per workgroup" % (name, k["lds"])      # >= 8 workgroups per CU
        assert kr.waves_per_simd(k) == 8, (name, k)
    for name, k in link.items():
        assert k["max_threads"] >= 1024, name
        assert k["lds"] <= 1024, (name, k)              # static share: the vote's words only (the planes are dynamic LDS)
        assert k["vgpr"] + k["agpr"] <= 128, (name, k)                                        # 1024 threads: 4 waves per SIMD
