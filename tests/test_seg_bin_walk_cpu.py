"""The walk table of the binning kernel (ops.build_walk_table: host side, no GPU) and what seg_bin_own_kernel may cost:
its 1 024-thread workgroup runs 4 waves per SIMD, so 128 registers and no scratch (a form that only fits with spills is
not the form to keep), and at the reference's shapes its LDS stays below the 48 KB a launch gets without raising the
kernel's attribute.  Resources are read from the built code object's metadata (tools/kernel_resources.py)."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import kernel_resources as kr  # noqa: E402


def test_walk_table_of_the_reference_topology(part_tables):
    from ilps_amd import ops
    ids, off = part_tables[1]
    V = 6890
    walk = ops.build_walk_table(ids, V)
    assert walk.dtype == np.int32 and walk.shape == (V,)
    assert np.array_equal(np.sort(walk), np.arange(V))                  # a permutation
    K = len(ids)
    assert K == 6879 and np.array_equal(walk[:K], np.asarray(ids))      # the table's slots first, in table order
    rest = walk[K:]
    assert len(rest) == 11 and np.all(np.diff(rest) > 0)                # then the un-owned vertices, ascending
    assert not np.isin(rest, np.asarray(ids)).any()
    # the table by vertex that the kernel reads: slot | part << 16, -1 for the un-owned
    inv = ops._part_inv(ids, off, V)
    assert np.all(inv[rest] == -1) and np.array_equal(inv[walk[:K]] & 0xffff, np.arange(K))
    part = inv[walk[:K]] >> 16
    for p in range(len(off) - 1):
        assert np.all(part[off[p]:off[p + 1]] == p)
    pt = ops.build_part_table(ids, off, None, V, torch.device("cpu"))
    assert np.array_equal(pt.inv.numpy(), inv)


def test_walk_table_refuses_what_is_no_permutation():
    from ilps_amd import ops
    assert ops.build_walk_table([3, 1, 3], 5) is None                   # a vertex listed twice
    assert ops.build_walk_table([0, 5], 5) is None and ops.build_walk_table([-1, 2], 5) is None
    assert ops.build_walk_table([], 5) is None
    assert ops.build_walk_table([0, 1], ops.WALK_MAX + 1) is None       # more vertices than a walk table takes
    assert ops.build_walk_table([4, 0, 2], 5).tolist() == [4, 0, 2, 1, 3]
    # the vertex-sampled tables qualify or not by the same rule, whatever they hold
    from ilps_amd.smpl_model import load_part_tables
    for vs in (2, 5):
        ids, off = load_part_tables(vs)
        VP = (6890 + vs - 1) // vs
        pos = np.asarray(ids) // vs
        walk = ops.build_walk_table(pos, VP)
        assert (walk is None) == (len(np.unique(pos)) != len(pos))


def test_seg_bin_own_kernel_resources():
    hit = {n: k for n, k in kr.kernels().items() if "seg_bin_own_kernel" in n}
    assert len(hit) == 1, sorted(hit)
    (name, k), = hit.items()
    assert k["scratch"] == 0, "%s spills %d B per lane" % (name, k["scratch"])
    assert k["max_threads"] == 1024, name
    assert k["vgpr"] + k["agpr"] <= 128, "%s: %d registers" % (name, k["vgpr"] + k["agpr"])
    assert kr.waves_per_simd(k) >= 4, name
    # static LDS + pixel counters + 64 x 64 z-buffer keys + visible flags, at W = 48 and V = 6890
    dyn = ((48 * 48 + 1) & ~1) * 4 + 64 * 64 * 8 + (6890 + 31) // 32 * 4
    assert k["lds"] + dyn <= 48 * 1024, "%s: %d + %d B of LDS" % (name, k["lds"], dyn)
