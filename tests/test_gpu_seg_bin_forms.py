"""The launch forms and loop edges of the binning kernels (csrc/seg_bin.hip, csrc/bin_device.h) and of smplr_visibility
that no other test reaches at a small shape: every instantiation of seg_bin_kernel beside seg_bin_own_kernel, the LDS
edge between the staged and the unstaged form, a second trip over the vertices, several table slots per thread, a bitmap
with every word in use.  Between forms: test_gpu_seg_bin_walk's `_same_binning` (everything bit for bit, the
nearest-pixel records of a pixel as a set); masks exactly against np_oracle.compute_mask, seg within test_gpu_parity's
SEG_RTOL / SEG_ATOL of the float64 oracle."""
import numpy as np
import pytest
import torch

from test_gpu_parity import VERT_ATOL
from test_gpu_seg_bin_walk import DEV, _against_oracle, _bin, _same_binning, _toy, _ws_views

pytestmark = pytest.mark.gpu
BIN_T = 1024                       # csrc/raster_common.h


def _plain(proj, mask, W, pt, grid_wh, ref_compat=True, verts=None):
    """smplr_seg_bin + smplr_seg_raster over a given proj -> what `_bin` returns.  grid_wh > 0: seg_bin_kernel<true, .,
    false> computes the mask; grid_wh = 0: seg_bin_kernel<false, ., false> reads `mask`.  (verts: carried along.)"""
    from ilps_amd import _lib, ops
    lib = _lib.load()
    B, VP = proj.shape[:2]
    e = lambda shape, dt=torch.float32: torch.full(shape, -7, dtype=dt, device=proj.device)
    m = e((B, VP)) if mask is None else torch.tensor(mask, device=proj.device)
    rec, vslot = e((B, lib.smplr_seg_slots(pt.P, pt.K), 4)), e((B, VP), torch.int16)
    with torch.cuda.device(proj.device):
        ws, rec = ops._seg_bin(proj, m, W, pt, grid_wh=grid_wh, ref_compat=ref_compat, rec=rec, vslot=vslot)
        seg, arg = ops._seg_raster(ws, rec, B, W, pt)
        torch.cuda.synchronize()
    out = dict(verts=(proj if verts is None else verts).cpu().numpy(), proj=proj.cpu().numpy(), mask=m.cpu().numpy(),
               seg=seg.cpu().numpy(), arg=arg.cpu().numpy(), rec=rec.cpu().numpy(), vslot=vslot.cpu().numpy())
    out["goff"], out["lstart"], out["lrec"] = _ws_views(ws, B, W, pt.P, pt.K)
    out["goff"] = out["goff"][:, :2 * pt.P + 2]
    return out


def _four_forms(monkeypatch, c, vp, A, cam, W, pt, grid_wh=64):
    """seg_bin_own_kernel, seg_bin_kernel<true, true, true>, <true, true, false>, <false, true, false> on one mesh."""
    from ilps_amd import _lib, ops
    assert pt.inv is not None and _lib.load().smplr_skin_vis_seg_fits(c.V, W, grid_wh) == 1       # staged
    own = _bin(monkeypatch, True, vp, A, c, cam, W, pt, grid_wh)
    table = _bin(monkeypatch, False, vp, A, c, cam, W, pt, grid_wh)
    verts, proj = ops._skin_fwd(vp, A, c, cam=cam)
    fused = _plain(proj, None, W, pt, grid_wh, verts=verts)
    given = _plain(proj, fused["mask"], W, pt, 0, verts=verts)
    for other in (table, fused, given):
        _same_binning(own, other, pt.P, W)
    return own


def test_all_staged_forms_on_one_mesh(monkeypatch):
    from ilps_amd import ops
    V, W = 300, 8
    c, vp, A, cam, ids, off, target, (a, b) = _toy(V=V, B=2, W=W)
    pt = ops.build_part_table(ids, off, None, V, torch.device(DEV))
    own = _four_forms(monkeypatch, c, vp, A, cam, W, pt)
    assert np.abs(own["verts"] - target.astype(np.float64)).max() <= VERT_ATOL
    _against_oracle(own, ids, off, W)
    assert own["mask"][0, b] == 1.0 and own["mask"][0, a] == 500.0


# ---- the staged / unstaged edge of the fused-mask form: csrc/seg_bin.hip, bin_lds
def _bin_lds(V, W, grid_wh, cap):
    base = ((W * W + 1) & ~1) * 4 + (grid_wh * grid_wh * 8 + (V + 31) // 32 * 4 if grid_wh else 0)
    return base, base + 8 * V <= cap


def _lds_edge(W=160, grid_wh=78):
    """-> the largest V whose (u, v) still fit beside the counters, the grid and the flags, by the library's own
    answer (smplr_skin_vis_seg_fits: bin_lds against its cap), and the bytes that V takes: at most the cap, and less than
    12 B below it."""
    from ilps_amd import _lib
    lib = _lib.load()
    v = 1
    while lib.smplr_skin_vis_seg_fits(v + 1, W, grid_wh) == 1:
        v += 1
    assert v < 7 * BIN_T                                 # (the answer is 0 above that, whatever the bytes)
    # (the bytes stand in for the cap in _bin_lds below: they are <= the cap and V + 1 takes more than the cap, and the
    # bytes grow with V, so "fits these bytes" and "fits the cap" say the same of every V)
    return v, _bin_lds(v, W, grid_wh, 0)[0] + 8 * v


@pytest.mark.parametrize("side", ["unstaged", "staged"])
def test_fused_mask_at_the_lds_edge(side):
    """W = 160, grid_wh = 78: 102 400 + 48 672 B of counters and grid; V = 330 (+ 44 B of flags + 2 640 B of (u, v))
    passes 150 KB and takes seg_bin_kernel<true, false, false>, V = 300 stays below (153 512 B) and takes <true, true,
    false>; the edge is V = 311, and the two V are taken 19 above and 11 below wherever the library puts it.  Each
    against <false, true, false> with its mask fed in, and against the oracle."""
    from ilps_amd import ops
    W, grid = 160, 78
    edge, cap = _lds_edge(W, grid)
    V = edge - 11 if side == "staged" else edge + 19
    assert 291 <= V <= 7 * BIN_T
    base, staged = _bin_lds(V, W, grid, cap)
    assert staged == (side == "staged") and base <= cap and _bin_lds(edge, W, grid, cap)[1] and not _bin_lds(edge + 1, W, grid, cap)[1]
    assert _bin_lds(V, W, 0, cap)[1]                     # the given-mask run is staged on either side
    c, vp, A, cam, ids, off, target, _ = _toy(V=V, B=1, W=W, seed=11)
    pt = ops.build_part_table(ids, off, None, V, torch.device(DEV))
    verts, proj = ops._skin_fwd(vp, A, c, cam=cam)
    fused = _plain(proj, None, W, pt, grid, verts=verts)
    given = _plain(proj, fused["mask"], W, pt, 0, verts=verts)
    _same_binning(fused, given, pt.P, W)
    _against_oracle(fused, ids, off, W, grid)


# ---- VP > 8 BIN_T: a second trip over the vertices (plain forms only)
def _two_trip_inputs(B, W, seed=21):
    VP, K = 8200, 280
    rng = np.random.default_rng(seed)
    proj = np.concatenate([rng.uniform(-1.0, W + 1.0, (B, VP, 2)), rng.normal(0, 1, (B, VP, 1))], axis=2).astype(np.float32)
    low = rng.permutation(8 * BIN_T)
    ids = np.concatenate([low[:K - 8], np.arange(8 * BIN_T, VP)])       # every vertex of the second trip is in the table
    ids = [int(v) for v in rng.permutation(ids)]
    off = [0, 60, 60, 127, 200, 280]
    lo, hi = int(low[5]), 8 * BIN_T + 3
    proj[0, lo] = [3.2, 4.1, 0.0]
    proj[0, hi] = [2.9, 3.8, 5.0]                                       # the later vertex lies in front, in cell (3, 4)
    return VP, proj, ids, off, lo, hi


@pytest.mark.parametrize("W,B", [(8, 2), (160, 1)])
def test_second_trip_over_the_vertices(W, B):
    """VP = 8 200: W = 8 is staged (<true, true, false>, <false, true, false>), W = 160 is not (<true, false, false>,
    <false, false, false>: 102 400 B of counters + 65 600 B of (u, v) pass 150 KB)."""
    from ilps_amd import ops
    VP, projn, ids, off, lo, hi = _two_trip_inputs(B, W)
    assert VP > 8 * BIN_T and max(ids) >= 8 * BIN_T
    cap = _lds_edge()[1]
    assert _bin_lds(VP, W, 64, cap)[1] == (W == 8) and _bin_lds(VP, W, 0, cap)[1] == (W == 8)
    pt = ops.build_part_table(ids, off, None, VP, torch.device(DEV))
    proj = torch.tensor(projn, device=DEV)
    fused = _plain(proj, None, W, pt, 64)
    given = _plain(proj, fused["mask"], W, pt, 0)
    _same_binning(fused, given, pt.P, W)
    _against_oracle(fused, ids, off, W)
    assert fused["mask"][0, hi] == 1.0 and fused["mask"][0, lo] == 500.0


# ---- several table slots per thread; every word of the owner form's bitmap
def test_three_slots_per_thread(monkeypatch):
    """K = 2 500: three slots per thread; an empty part in the middle, an empty last part that starts at K, part
    boundaries (700, 1 300) inside a thread's slots."""
    from ilps_amd import ops
    V, W, off = 2600, 8, [0, 700, 1300, 1300, 2500, 2500]
    ipt = (off[-1] + BIN_T - 1) // BIN_T
    assert ipt == 3 and off[1] % ipt and off[2] % ipt and off[2] == off[3] and off[4] == off[5] == off[-1]
    c, vp, A, cam, ids, off, target, (a, b) = _toy(V=V, B=2, W=W, seed=31, off=off)
    pt = ops.build_part_table(ids, off, None, V, torch.device(DEV))
    assert pt.P == 5 and pt.K == 2500
    own = _four_forms(monkeypatch, c, vp, A, cam, W, pt)
    _against_oracle(own, ids, off, W)
    assert own["mask"][0, b] == 1.0 and own["mask"][0, a] == 500.0
    assert own["goff"][0, 2] == own["goff"][0, 3] and own["goff"][0, 4] == own["goff"][0, 5]      # the empty parts


def test_largest_mesh_of_the_owner_form(monkeypatch):
    """V = K = 7 168 = 7 BIN_T: every thread owns seven vertices and every word of the far-reaching bitmap is in use."""
    from ilps_amd import ops
    V, W, off = 7 * BIN_T, 8, [0, 1500, 3000, 4500, 6000, 7 * BIN_T]
    c, vp, A, cam, ids, off, _, _ = _toy(V=V, B=1, W=W, seed=41, off=off)
    pt = ops.build_part_table(ids, off, None, V, torch.device(DEV))
    assert pt.inv is not None and pt.K == V
    own, table = _bin(monkeypatch, True, vp, A, c, cam, W, pt), _bin(monkeypatch, False, vp, A, c, cam, W, pt)
    _same_binning(own, table, pt.P, W)
    assert int((own["vslot"] >= 0).sum()) > 0


# ---- smplr_visibility alone
def _vis_proj(B, VP, grid_wh, seed):
    rng = np.random.default_rng(seed)
    return np.concatenate([rng.uniform(-1.0, grid_wh + 1.0, (B, VP, 2)), rng.normal(0, 1, (B, VP, 1))], axis=2).astype(np.float32)


@pytest.mark.parametrize("VP,grid_wh,ref_compat", [(1, 64, True),        # no vertex 1 exists
                                                   (33, 64, True),       # two flag words
                                                   (300, 2, True),       # no empty cell: vertex 1 is not forced
                                                   (300, 64, True), (300, 64, False),
                                                   (300, 80, True)])     # 51 240 B of LDS: the attribute is raised
def test_visibility_alone(VP, grid_wh, ref_compat):
    from ilps_amd import ops
    from oracle import np_oracle as o
    projn = _vis_proj(2, VP, grid_wh, 50 + VP + grid_wh)
    if VP >= 300:
        projn[0, 7] = projn[0, 5]                                        # a tie in z on one cell: the lower index wins
        projn[1, 1] = [-5.0, -5.0, 0.0]                                  # vertex 1 off the grid: visible only if forced
    inside = lambda p: (np.rint(p[:, 0]) >= 0) & (np.rint(p[:, 0]) < grid_wh) & (np.rint(p[:, 1]) >= 0) & (np.rint(p[:, 1]) < grid_wh)
    cells = [len({(int(np.rint(u)), int(np.rint(v))) for u, v, _ in p[inside(p)]}) for p in projn]
    assert all(n == grid_wh * grid_wh for n in cells) == (grid_wh == 2) and all(n < grid_wh * grid_wh for n in cells) == (grid_wh != 2)
    assert (grid_wh * grid_wh * 8 + (VP + 31) // 32 * 4 > 48 * 1024) == (grid_wh == 80)
    want = o.compute_mask(projn.astype(np.float64), grid_wh, ref_compat)
    got = ops.visibility(torch.tensor(projn, device=DEV), grid_wh, ref_compat).cpu().numpy()
    assert np.array_equal(got, want)
    if VP >= 300:
        assert got[1, 1] == (1.0 if ref_compat and grid_wh != 2 else 500.0)
        assert got[0, 7] == 500.0                                        # the tie's higher index never wins its cell
