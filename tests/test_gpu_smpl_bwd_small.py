"""smplr_smpl_bwd (the C ABI, through ctypes) at SMALL vertex counts against the staged float64 reference of
tests/_smpl_bwd_oracle.py: the fused call runs the skinning backward, the blend GEMM backward and the pose backward,
the last one folding the partial sums of the first two - skin_nblk = ceil(V / 256) blocks of the per-vertex kernel or
ceil(V / 1 024) of the record kernel, nslices x nmt tiles of the GEMM.

Cases (_smpl_bwd_oracle.CASES, each run with the bf16x3 and the fp32 GEMM and with the sparse and a dense weight table):
    V = 8 (3V = 24: one ragged k-tile, one partly filled wave)   64 (exactly one wave)   257 (a second 256-vertex block
    of one vertex, one short record chunk)   1 024 (exactly one record chunk)   1 025 (a second chunk of one vertex)
    2 049 (three chunks, the last of one vertex);   B = 1, 33 (one past a mesh tile), and 513 at V = 257 (17 mesh
    tiles: the two-tile GEMM form);   vertex sampling 1, 3;   cotangents dverts | dproj | dverts + dproj + dJt | slot sums
    alone (skin_bwd_rec_kernel with the sparse table) | slot sums + dverts | slot sums + dproj + dJt (the per-vertex kernel
    with the slot gather).
Slot sums are built by hand (_smpl_bwd_oracle.layout): nsplit = 1, 2, 3, 7 (slot_sum's three forms; 7 = a second group of
six holding one block), slots in vertex order or permuted over all five 4 096-slot windows, 0 / 1 / 64 / 65 / 256 / 257
/ 1 024 live records per 1 024-vertex chunk (257: a second round with three idle waves; a chunk without a live record
between two with; live records in the one-vertex chunk only), dead records without a slot, with all blocks zero and with
blocks that cancel exactly, live ones with sx == 0.

Float64 bar, every entry of all 86 columns: |dx - ref| <= K 2^-24 mag_dx,
    K = 2 (V + 8) + (nsplit - 1) + (4e-6 / 2^-24 = 67.1 for bf16x3 | 3 V + 1 for fp32) + K_pose,
K_pose = 4 x the float32 pose stage's own error over these cases' rows, measured by _smpl_bwd_oracle.k_pose() and printed
(24.4 = 4 x 6.10 when this file was written); the achieved error / bar of every case is printed (RATIO lines).
Bit for bit: the fused call == smplr_skin_bwd -> smplr_blend(3)_bwd -> smplr_pose_bwd for every cotangent set without
slot sums; the sparse kernel == the dense kernel on the sparse weights (where both run the per-vertex kernel); two
launches; a workspace prefilled with NaN or with zeros (no partial is read that was not written); all-dead slot sums
without dJt give exactly 0; the per-vertex kernel's slot gather == the same call fed the merged dproj (the slot sums
added on the host in block order, fp32: slot_sum's three forms and the five windows, bit for bit).  The record kernel
against that merged call: dv_posed has its bits and dA / the camera sums add the same n = live records per mesh terms in
another order, so |difference| <= (4 (n + 8) + 2 K_pose) 2^-24 mag_dx - far below the float64 bar where few records
are live at a large V (RECORD lines).  The workspace is the size the library reports plus a NaN guard that must come back
untouched; with x_stride = 90 columns 86..89 of a NaN-filled dx stay NaN.  BatchSMPLFn's forward at every V against
float64 at VERT_ATOL, in passing."""
import dataclasses
import functools

import numpy as np
import pytest
import torch

import _smpl_bwd_oracle as so
from _smpl_bwd_oracle import CASES, CASE_IDS
from test_gpu_parity import VERT_ATOL, dev

pytestmark = pytest.mark.gpu

GUARD = 64                                 # floats of NaN behind the workspace


def t(a, dtype=torch.float32):
    """a device copy (the oracle's cached inputs are read-only)"""
    import test_gpu_parity
    return test_gpu_parity.t(np.array(a), dtype)


# ------------------------------------------------------------------------------------------------ operands
@functools.lru_cache(maxsize=None)
def _consts(V, weights):
    from ilps_amd import ops
    c = ops.SMPLConstants.from_model(so.model(V, weights), dev()).pack_blend3()
    assert (c.lbs_top4 is not None) == (weights == "sparse")
    return c


def consts(V, weights, gemm):
    c = _consts(V, weights)
    return c if gemm == "bf16x3" else c.fp32_gemm()


@functools.lru_cache(maxsize=None)
def forward(V, B, gemm):
    """What the backward takes from the forward (shared, never modified): x, Rs, J, A, v_posed on the device."""
    from ilps_amd import ops
    c = consts(V, "sparse", gemm)                           # (the weight table plays no part before the skinning)
    x = t(so.x_rows(B))
    coef, Rs, J, A, Jt = ops._pose_fwd(x, 4, c)
    vp = ops._blend_fwd(coef, c, B)
    torch.cuda.synchronize()
    return dict(x=x, Rs=Rs, J=J, A=A, vp=vp)


def cotangents(case):
    inp = so.inputs(case)
    d = {k: (None if inp[k] is None else t(inp[k])) for k in ("dverts", "dproj", "dJt")}
    lay = inp["lay"]
    d["seg"] = None if lay is None else (t(lay["part"].reshape(-1)), t(lay["vslot"], torch.int16), case.nsplit)
    return d


def merged(case, g):
    """The case's cotangents with the slot sums merged into dproj on the host: block order, fp32, as slot_sum adds."""
    inp = so.inputs(case)
    s = so.gather(inp["lay"], so.block_sum32(inp["lay"]["part"]))
    d = s if inp["dproj"] is None else inp["dproj"] + s
    assert d.dtype == np.float32
    return dict(dverts=g["dverts"], dproj=t(d), dJt=g["dJt"], seg=None)


def fused(c, f, g, vs, fill=float("nan"), stride=86, x=None):
    """smplr_smpl_bwd into a NaN-filled dx (B, stride); the workspace holds `fill`, its guard NaN."""
    from ilps_amd import _lib
    from ilps_amd._lib import ptr, stream, check
    lib = _lib.load()
    x = f["x"] if x is None else x
    B, V = x.shape[0], c.V
    n = lib.smplr_smpl_bwd_workspace(B, V) // 4
    ws = torch.full((n + GUARD,), float("nan"), device=dev())
    ws[:n] = fill
    dx = torch.full((B, stride), float("nan"), device=dev())
    sp, sv, sn = g["seg"] if g["seg"] is not None else (None, None, 0)
    check(lib.smplr_smpl_bwd(ptr(g["dverts"]), ptr(g["dproj"]), ptr(sp), ptr(sv), int(sn), ptr(g["dJt"]), ptr(x), stride, 4,
                             B, V, vs, ptr(c.blend_t), ptr(c.blend3_bwd), ptr(c.lbs_weights), ptr(c.lbs_top4),
                             ptr(c.J_dirs), ptr(c.parents), ptr(f["Rs"]), ptr(f["J"]), ptr(f["A"]), ptr(f["vp"]), ptr(dx),
                             ptr(ws), stream()), "smplr_smpl_bwd")
    torch.cuda.synchronize()
    assert bool(torch.isnan(ws[n:]).all()), "the guard behind the workspace was written"
    return dx


def chain(c, f, g, vs):
    """smplr_skin_bwd -> smplr_blend3_bwd | smplr_blend_bwd -> smplr_pose_bwd, the granular entry points."""
    from ilps_amd import _lib
    from ilps_amd._lib import ptr, stream, check
    lib = _lib.load()
    d = dev()
    x = f["x"]
    B, V = x.shape[0], c.V
    dvp, dA, dcam = torch.empty(B, V, 3, device=d), torch.empty(B, 24, 12, device=d), torch.empty(B, 4, device=d)
    ws = torch.empty(lib.smplr_skin_bwd_workspace(B, V) // 4 + 1, device=d)
    check(lib.smplr_skin_bwd(ptr(g["dverts"]), ptr(g["dproj"]), ptr(f["vp"]), ptr(c.lbs_weights), ptr(c.lbs_top4), ptr(f["A"]),
                             ptr(x), 86, B, V, vs, ptr(dvp), ptr(dA), ptr(dcam), ptr(ws), stream()), "smplr_skin_bwd")
    dcoef = torch.empty(B, 220, device=d)
    if c.blend3_bwd is None:
        ws2 = torch.empty(lib.smplr_blend_bwd_workspace(B, 3 * V) // 4 + 1, device=d)
        check(lib.smplr_blend_bwd(ptr(dvp), ptr(c.blend_t), B, 3 * V, ptr(dcoef), ptr(ws2), stream()), "smplr_blend_bwd")
    else:
        ws2 = torch.empty(lib.smplr_blend3_bwd_workspace(B, 3 * V) // 4 + 1, device=d)
        check(lib.smplr_blend3_bwd(ptr(dvp), ptr(c.blend3_bwd), B, 3 * V, ptr(dcoef), ptr(ws2), stream()), "smplr_blend3_bwd")
    dx = torch.empty(B, 86, device=d)
    check(lib.smplr_pose_bwd(ptr(x), 86, 4, B, ptr(c.J_dirs), ptr(c.parents), ptr(f["Rs"]), ptr(f["J"]), ptr(f["A"]),
                             ptr(dcoef), ptr(dA), ptr(g["dJt"]), ptr(dcam if g["dproj"] is not None else None), ptr(dx),
                             stream()), "smplr_pose_bwd")
    torch.cuda.synchronize()
    return dx


def skin_path(case, weights):
    if case.live is None:
        return "per-vertex"
    return "record" if case.cot == "slots" and weights == "sparse" else "per-vertex+gather"


# ------------------------------------------------------------------------------------------------ the tests
def test_k_pose():
    kp = so.k_pose()
    print("K_pose = %.2f (4 x %.2f: the float32 pose stage over the rows of %d cases)" % (kp, kp / 4, len(CASES)))
    assert 4.0 <= kp < 4096.0


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_fused_backward(case):
    V, B, vs = case.V, case.B, case.vs
    g = cotangents(case)
    for weights in so.WEIGHTS:
        ref = so.reference(case, weights)
        for gemm in so.GEMMS:
            c, f = consts(V, weights, gemm), forward(V, B, gemm)
            label = "%s %s %s" % (so._id(case), weights, gemm)
            dx = fused(c, f, g, vs)
            assert bool(torch.isfinite(dx).all()), label + ": dx is not finite over a NaN-filled workspace"
            assert torch.equal(dx, fused(c, f, g, vs, fill=0.0)), label + ": dx depends on what the workspace held"
            assert torch.equal(dx, fused(c, f, g, vs)), label + ": two launches differ"
            K = so.bar_k(case, gemm)
            r = so.ratio(dx.cpu().numpy(), ref, K)
            print("RATIO %-62s %-7s %-6s %-17s K %8.1f  error / bar %.4f" % (so._id(case), weights, gemm,
                                                                             skin_path(case, weights), K, r))
            assert r <= 1.0, "%s: %.3f of K 2^-24 mag_dx, K = %.1f" % (label, r, K)
            if case.live is None:
                assert torch.equal(dx, chain(c, f, g, vs)), label + ": the fused call differs from the granular chain"
            if weights == "sparse" and skin_path(case, weights) != "record":
                dense = dataclasses.replace(c, lbs_top4=None)
                assert torch.equal(dx, fused(dense, f, g, vs)), label + ": sparse and dense kernels differ on the sparse weights"
            if case.live is not None:
                # the same gradient handed over as a merged dproj (the slot sums added on the host in block order, fp32)
                # runs the per-vertex kernel without the gather: the gather's bits; for the record kernel dv_posed's
                # bits and the same n = live records per mesh non-zero terms of dA and the camera sums in another
                # order, so two fp32 sums of n terms apart before the pose stage and two pose roundings after it
                want = fused(c, f, merged(case, g), vs)
                if skin_path(case, weights) == "record":
                    Kr = 4 * (sum(case.live) + 8) + 2 * so.k_pose()
                    rr = so.ratio(dx.cpu().numpy(), dict(dx=want.cpu().numpy().astype(np.float64), mag_dx=ref["mag_dx"]), Kr)
                    print("RECORD vs per-vertex %-48s %-6s K %7.1f  difference / bar %.4f" % (so._id(case), gemm, Kr, rr))
                    assert rr <= 1.0, "%s: record kernel vs per-vertex kernel, %.3f of K 2^-24 mag_dx, K = %.1f" % (label, rr, Kr)
                else:
                    assert torch.equal(dx, want), label + ": the slot gather differs from the merged dproj"
            if case.live is not None and not any(case.live) and g["dJt"] is None and g["dverts"] is None and g["dproj"] is None:
                assert not dx.any(), label + ": all records dead, dx must be exactly 0"


STRIDE_CASES = [c for c in CASES if c.B == 1 and c.V in (257, 1025) and c.cot in ("all", "slots")][:4]


@pytest.mark.parametrize("case", STRIDE_CASES, ids=[so._id(c) for c in STRIDE_CASES])
def test_row_stride_90(case):
    """x and dx rows of 90 floats: the four surplus columns of x hold NaN and are not read, those of dx are not written,
    the 86 others are the narrow call's bits."""
    g = cotangents(case)
    for gemm in so.GEMMS:
        c, f = consts(case.V, "sparse", gemm), forward(case.V, case.B, gemm)
        wide = torch.cat([f["x"], torch.full((case.B, 4), float("nan"), device=dev())], dim=1).contiguous()
        dx = fused(c, f, g, case.vs, stride=90, x=wide)
        assert bool(torch.isnan(dx[:, 86:]).all()), "columns 86..89 of dx were written"
        assert torch.equal(dx[:, :86], fused(c, f, g, case.vs))


@pytest.mark.parametrize("V", so.SHAPES)
def test_forward_in_passing(V):
    from ilps_amd import ops
    from oracle.torch_oracle import TorchSMPL
    B = 33
    with torch.no_grad():
        verts64, Jt64, _ = TorchSMPL(so.model(V), torch.float64)(torch.tensor(so.x_rows(B), dtype=torch.float64),
                                                                 return_all=True)
    for gemm in so.GEMMS:
        verts, Jt = ops.BatchSMPLFn.apply(t(so.x_rows(B)), consts(V, "sparse", gemm), 4)
        ev = float(np.abs(verts.cpu().numpy() - verts64.numpy()).max())
        ej = float(np.abs(Jt.cpu().numpy() - Jt64.numpy()).max())
        print("FORWARD V=%d %s: verts %.3e J_transformed %.3e" % (V, gemm, ev, ej))
        assert ev <= VERT_ATOL and ej <= VERT_ATOL
