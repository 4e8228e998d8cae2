"""The skinning backward over records walks only the LIVE ones: a record whose slot sum is exactly (0, 0) - a hidden
vertex near a pixel centre that never won an arg-min - is treated like a vertex without a record (its dv_posed row is
stored as zeros, it takes no lane of the dA product).  The reference in every case is the per-vertex kernel of the same
process fed the merged d proj scattered from the same sums (as test_skin_backward_over_records_equals_per_vertex gets
its reference), at that test's bar: grad_close(..., 2e-5).  V = 6 890: seven 1 024-vertex chunks, the last one ragged."""
import numpy as np
import pytest
import torch

from _inputs import make_x
from test_gpu_parity import dev, grad_close, t

pytestmark = pytest.mark.gpu

NSLOT = 5 * 4096                       # slots per row block of the partial buffer (SB_NWIN * SB_SLOTS)
PIPELINE = [(16, 1), (24, 1), (16, 5), (24, 5)]      # (W, vertex sampling): two and three row blocks at B = 3
BAR = 2e-5


def pipeline_case(model, W, vs, B=3):
    """The real pipeline: dx over the records against dx over the vertices, repeatable, and independent of the batch."""
    from ilps_amd import ops
    d = dev()
    c = ops.SMPLConstants.from_model(model, d)
    pt = ops.get_part_table(vs, d, c.V)
    x = t(make_x(B, W, seed=1300 + W + vs))
    coef, Rs, J, A, Jt = ops._pose_fwd(x, 4, c)
    vp = ops._blend_fwd(coef, c, B)
    verts, proj = ops._skin_fwd(vp, A, c, cam=x, vertex_sampling=vs)
    VP = proj.shape[1]
    mask = ops.visibility(proj)
    vslot = torch.empty((B, VP), dtype=torch.int16, device=d)
    seg, arg, rec = ops._seg_fwd(proj, mask, W, pt, vslot=vslot)
    g = t(np.random.default_rng(23).normal(0, 1, (B, W, W, 32)))
    part, nsplit = ops._seg_bwd(g, arg, rec, VP, W, pt, merge=False, deterministic=True)
    dproj = ops._seg_bwd(g, arg, rec, VP, W, pt, deterministic=True)
    want = ops._smpl_bwd(x, 4, c, Rs, J, A, vp, None, dproj, None, vs)
    got = ops._smpl_bwd(x, 4, c, Rs, J, A, vp, None, None, None, vs, seg_grad=(part, vslot, nsplit))
    again = ops._smpl_bwd(x, 4, c, Rs, J, A, vp, None, None, None, vs, seg_grad=(part, vslot, nsplit))
    torch.cuda.synchronize()
    # (what the case is for: records of both kinds reach the kernel)
    has = (vslot >= 0).cpu().numpy()
    nz = (dproj[..., :2] != 0).any(-1).cpu().numpy()
    print("W=%d vs=%d nsplit=%d: records %s, with a non-zero sum %s" % (W, vs, nsplit, has.sum(1), (has & nz).sum(1)))
    assert (has & nz).any() and (has & ~nz).any(), "the case holds no live or no dead record"
    assert torch.equal(got, again)
    grad_close(got.cpu().numpy(), want.cpu().numpy(), BAR, "dx (live records) vs dx (vertices)")
    k = B - 1
    part1, ns1 = ops._seg_bwd(g[k:k + 1].contiguous(), arg[k:k + 1].contiguous(), rec[k:k + 1].contiguous(), VP, W, pt,
                              merge=False, deterministic=True)
    one = ops._smpl_bwd(x[k:k + 1].contiguous(), 4, c, Rs[k:k + 1].contiguous(), J[k:k + 1].contiguous(),
                        A[k:k + 1].contiguous(), vp[k:k + 1].contiguous(), None, None, None, vs,
                        seg_grad=(part1, vslot[k:k + 1].contiguous(), ns1))
    torch.cuda.synchronize()
    if ns1 == nsplit:
        assert torch.equal(one[0], got[k])


@pytest.mark.parametrize("W,vs", PIPELINE)
def test_live_records_real_pipeline(smpl_model, W, vs):
    pipeline_case(smpl_model, W, vs)


# --------------------------------------------------------------------------------- hand-built (part, vslot, nsplit)
@pytest.fixture(scope="module")
def ctx(smpl_model):
    """One forward at B = 3, W = 16 (shared, never modified) and the row-block count _seg_bwd(merge=False) reports."""
    from ilps_amd import ops
    d = dev()
    B, W = 3, 16
    c = ops.SMPLConstants.from_model(smpl_model, d)
    pt = ops.get_part_table(1, d, c.V)
    x = t(make_x(B, W, seed=1400))
    coef, Rs, J, A, Jt = ops._pose_fwd(x, 4, c)
    vp = ops._blend_fwd(coef, c, B)
    verts, proj = ops._skin_fwd(vp, A, c, cam=x, vertex_sampling=1)
    seg, arg, rec = ops._seg_fwd(proj, ops.visibility(proj), W, pt)
    part, nsplit = ops._seg_bwd(t(np.zeros((B, W, W, 32))), arg, rec, c.V, W, pt, merge=False, deterministic=True)
    torch.cuda.synchronize()
    assert nsplit >= 2 and part.numel() * part.element_size() >= B * nsplit * NSLOT * 2 * 4
    return dict(ops=ops, c=c, x=x, Rs=Rs, J=J, A=A, vp=vp, B=B, V=c.V, nsplit=nsplit)


def run_both(ctx, vslot, sums):
    """vslot (B, V) int, sums (B, nsplit, NSLOT, 2) fp32 -> dx over the records, dx over the vertices (merged d proj)."""
    ops, c, B, V = ctx["ops"], ctx["c"], ctx["B"], ctx["V"]
    acc = sums[:, 0].copy()
    for s in range(1, ctx["nsplit"]):                  # (block order, fp32: the merge kernel's sum)
        acc = acc + sums[:, s]
    merged = np.zeros((B, V, 3), np.float32)
    for b in range(B):
        has = vslot[b] >= 0
        merged[b, has, :2] = acc[b, vslot[b, has]]
    part, vs16 = t(sums.reshape(-1)), t(vslot, torch.int16)
    a = (ctx["x"], 4, c, ctx["Rs"], ctx["J"], ctx["A"], ctx["vp"], None)
    want = ops._smpl_bwd(*a, t(merged), None, 1)
    got = ops._smpl_bwd(*a, None, None, 1, seg_grad=(part, vs16, ctx["nsplit"]))
    again = ops._smpl_bwd(*a, None, None, 1, seg_grad=(part, vs16, ctx["nsplit"]))
    torch.cuda.synchronize()
    assert torch.equal(got, again) or torch.isnan(got).any()
    return got, want


def layout(ctx, owners, seed, perm=False):
    """Slots 0.. handed to the vertices `owners` (bool (V,)) in vertex order (or in a seeded random order), and random
    sums, none of them zero, spread over the first and the last row block."""
    B, V, ns = ctx["B"], ctx["V"], ctx["nsplit"]
    rng = np.random.default_rng(seed)
    vslot = np.full((B, V), -1, np.int64)
    sums = np.zeros((B, ns, NSLOT, 2), np.float32)
    idx = np.flatnonzero(owners)
    for b in range(B):
        vslot[b, idx] = rng.permutation(idx.size) if perm else np.arange(idx.size)
        for s in (0, ns - 1):
            v = rng.normal(0, 1, (idx.size, 2)).astype(np.float32)
            sums[b, s, :idx.size] = np.where(np.abs(v) < 0.05, 0.05, v)
    return vslot, sums


def test_all_sums_zero(ctx):
    vslot, sums = layout(ctx, np.arange(ctx["V"]) % 3 == 0, 1)
    sums[:] = 0.0
    got, want = run_both(ctx, vslot, sums)
    assert torch.equal(got, want) and not got.any()


def test_sums_cancelling_across_row_blocks(ctx):
    """t0 = -t1 for every second record: those are dead (the sum is exactly +0), the others live."""
    vslot, sums = layout(ctx, np.arange(ctx["V"]) % 3 == 0, 2)
    sums[:, -1, 0::2] = -sums[:, 0, 0::2]
    got, want = run_both(ctx, vslot, sums)
    assert want.any()
    grad_close(got.cpu().numpy(), want.cpu().numpy(), BAR, "dx, half of the records cancelled")


def test_every_vertex_live(ctx):
    """1 024 live records per chunk (four rounds), slots beyond the first 4 096-slot window."""
    vslot, sums = layout(ctx, np.ones(ctx["V"], bool), 3, perm=True)
    assert vslot.max() > 4096 and (sums[:, 0] + sums[:, -1])[:, :ctx["V"]].all()
    got, want = run_both(ctx, vslot, sums)
    grad_close(got.cpu().numpy(), want.cpu().numpy(), BAR, "dx, every vertex live")


def test_chunk_without_live_record_between_two_with(ctx):
    v = np.arange(ctx["V"])
    owners = (v < 3072) & (v % 2 == 0)
    vslot, sums = layout(ctx, owners, 4)
    dead = vslot[0, (v >= 1024) & (v < 2048) & owners]          # (the slots are in vertex order, alike in every mesh)
    sums[:, :, dead] = 0.0
    got, want = run_both(ctx, vslot, sums)
    assert want.any()
    grad_close(got.cpu().numpy(), want.cpu().numpy(), BAR, "dx, an all-dead chunk")


def test_live_records_only_in_the_ragged_chunk(ctx):
    v = np.arange(ctx["V"])
    owners = (v % 4 == 1) | (v >= 6144)
    vslot, sums = layout(ctx, owners, 5)
    sums[:, :, vslot[0, owners & (v < 6144)]] = 0.0
    got, want = run_both(ctx, vslot, sums)
    assert want.any()
    grad_close(got.cpu().numpy(), want.cpu().numpy(), BAR, "dx, live records in the last chunk only")


def test_nan_sum_stays_live_and_stays_in_its_mesh(ctx):
    vslot, sums = layout(ctx, np.arange(ctx["V"]) % 3 == 0, 6)
    sums[:, -1, 0::2] = -sums[:, 0, 0::2]
    clean, _ = run_both(ctx, vslot, sums)
    sums[1, 0, 78, 0] = np.nan                 # (a record whose finite sums cancel: NaN is not zero, it stays live)
    got, want = run_both(ctx, vslot, sums)
    assert torch.isnan(got[1]).any() and torch.isnan(want[1]).any()
    assert torch.equal(got[0], clean[0]) and torch.equal(got[2], clean[2])
