"""The pose path (pose_device.h, pose.hip, the pose role of blend3.hip, the camera / stride handling of skin.hip and
seg_bin.hip) away from make_x's corner: joint angles from exactly 0 through 1e-7 .. 1e-2, around pi and 2 pi, to 12 rad;
camera widths other than 4; rows wider than num_cam + 82.  The gradient's bar is 4 x the float32 ORACLE's own error
in the same regime (tests/_pose_regimes.py), so it is ~4e-6 at |theta| = 1 and ~4e-4 at 1e-4, never grad_close's 2e-3."""
import numpy as np
import pytest
import torch

import _pose_regimes as pr
from _inputs import make_x
from test_gpu_parity import SEG_RTOL, VERT_ATOL, dev, grad_close, t

pytestmark = pytest.mark.gpu

RS_ATOL = 2e-6            # Rs against float64 batch_rodrigues
ORTHO_ATOL = 4e-6         # R R^T = I on the HIP Rs


@pytest.fixture(scope="module")
def ref(smpl_model):
    return pr.reference(smpl_model)


@pytest.fixture(scope="module")
def consts(smpl_model):
    from ilps_amd import ops
    return ops.SMPLConstants.from_model(smpl_model, dev()).pack_blend3()


def _hip_dx(c, x, seeds, num_cam=4):
    """-> dx (S, B, num_cam + 82) float64, verts, J_transformed float64 arrays: BatchSMPLFn with constants `c`."""
    from ilps_amd import ops
    out = []
    for s in seeds:
        gv, gj = pr.cotangents(x.shape[0], s)
        xg = t(x).requires_grad_(True)
        v, jt = ops.BatchSMPLFn.apply(xg, c, num_cam)
        ((v * t(gv)).sum() + (jt * t(gj)).sum()).backward()
        out.append(xg.grad.cpu().numpy().astype(np.float64))
    return np.stack(out), v.detach().cpu().numpy().astype(np.float64), jt.detach().cpu().numpy().astype(np.float64)


@pytest.fixture(scope="module")
def hip(ref, consts):
    """The whole regime batch (75 rows: crosses the 32-mesh GEMM tile and the 4- and 8-mesh pose blocks), default
    bf16x3 GEMMs, all cotangent seeds; Rs from the stand-alone pose kernel."""
    from ilps_amd import ops
    dx, verts, jt = _hip_dx(consts, ref["x"], pr.SEEDS)
    Rs = ops._pose_fwd(t(ref["x"]), 4, consts)[1].cpu().numpy().astype(np.float64).reshape(-1, 24, 3, 3)
    return dict(dx=dx, verts=verts, J_transformed=jt, Rs=Rs)


def _rows(ref, regime, kinds=None):
    return [n for n, (lab, kind) in enumerate(ref["rows"]) if lab == regime and (kinds is None or kind in kinds)]


def _check_dx(dx, d64, rows, ref, regimes, what, num_cam=4):
    """dx, d64 (S, B, P) restricted to batch rows `rows` (their regime labels in `regimes`): finite, camera columns
    exactly 0, per row and block max|dx - d64| / max|d64| <= the row's regime bar.  Prints achieved next to ref_err."""
    assert np.isfinite(dx).all(), "%s: non-finite gradient" % what
    assert np.all(dx[:, :, :num_cam] == 0), "%s: camera columns must be exactly 0" % what
    err = pr.block_errors(dx, d64, num_cam)
    fails = []
    for b in pr.BLOCKS:
        e = err[b].max(axis=0)                                            # over the seeds -> (rows,)
        for reg in sorted(set(regimes), key=pr.REGIMES.index):
            got = max(e[i] for i, r in enumerate(regimes) if r == reg)
            re_, bar = ref["ref_err"][b][reg], ref["bar"][b][reg]
            print("REGIME %-22s %-9s %-5s ref_err %.3e hip %.3e bar %.3e ratio %.2f" % (what, reg, b, re_, got, bar, got / re_))
            if not got <= bar:
                fails.append("%s %s: %.3e > %.3e = 4 x %.3e" % (reg, b, got, bar, re_))
    assert not fails, "%s: %s" % (what, "; ".join(fails))


# ---- a. forward, per regime --------------------------------------------------------------------------------------
@pytest.mark.parametrize("regime", pr.REGIMES)
def test_forward_regime(ref, hip, regime):
    rows = _rows(ref, regime)
    ev = np.abs(hip["verts"][rows] - ref["verts"][rows]).max()
    ej = np.abs(hip["J_transformed"][rows] - ref["J_transformed"][rows]).max()
    er = np.abs(hip["Rs"][rows] - ref["Rs"][rows]).max()
    R = hip["Rs"][rows].reshape(-1, 3, 3)
    eo = np.abs(R @ R.transpose(0, 2, 1) - np.eye(3)).max()
    print("FORWARD %-9s verts %.3e J_transformed %.3e Rs %.3e R R^T - I %.3e" % (regime, ev, ej, er, eo))
    assert np.isfinite(hip["verts"][rows]).all()
    assert ev <= VERT_ATOL and ej <= VERT_ATOL
    assert er <= RS_ATOL
    assert eo <= ORTHO_ATOL


# ---- b. backward, per regime -------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", ["every_joint", "one_joint"])
@pytest.mark.parametrize("regime", pr.REGIMES)
def test_backward_regime(ref, hip, regime, group):
    """dx of (verts . gv + J_transformed . gj).sum() against float64 autograd, default bf16x3 GEMMs, three cotangent
    seeds, every row of the regime at the regime's bar.  every_joint: the rows whose 24 joints all sit at the regime's
    magnitude (random axes, the coordinate axes, exact zeros, the T-pose); one_joint: root, joint 9 or a leaf there,
    the other 23 at make_x's angles."""
    rows = [n for n in _rows(ref, regime) if ref["rows"][n][1].startswith("joint") == (group == "one_joint")]
    if regime == pr.TPOSE and group == "one_joint":
        assert not rows
        return
    assert rows
    _check_dx(hip["dx"][:, rows], ref["d64"][:, rows], rows, ref, [regime] * len(rows), "bf16x3 " + group)


@pytest.mark.parametrize("lo,hi", [(12, 13), (12, 17)])
def test_backward_small_batches(ref, consts, hip, smpl_model, lo, hi):
    """B = 1 (the '1e-4 all' row, the regime with the largest reference error) and B = 5 (on into 1e-3): one pose
    block, a ragged GEMM tile; the same bars, and the rows do not depend on the batch they sit in."""
    x = ref["x"][lo:hi]
    dx, verts, jt = _hip_dx(consts, x, pr.SEEDS[:1])
    # (cotangents are drawn per batch size, so the float64 reference is taken afresh for the slice's own)
    d64 = pr.oracle_dx(smpl_model, x, torch.float64, seeds=pr.SEEDS[:1])
    regs = [ref["rows"][n][0] for n in range(lo, hi)]
    _check_dx(dx, d64, list(range(hi - lo)), ref, regs, "bf16x3 B=%d" % (hi - lo))
    assert np.array_equal(verts, hip["verts"][lo:hi]) and np.array_equal(jt, hip["J_transformed"][lo:hi])


def test_backward_fp32_gemm_all_joint_rows(ref, consts, smpl_model):
    """The exact-fp32 blend GEMMs (SMPLR_BLEND_GEMM=f32's constants) over the rows with all 24 joints at the regime's
    magnitude; their own cotangents (the batch is another size), their own float64 reference."""
    rows = [n for n, (_, kind) in enumerate(ref["rows"]) if kind == "all"]
    assert len(rows) == len(pr.MAGNITUDES)
    x = ref["x"][rows]
    dx, verts, _ = _hip_dx(consts.fp32_gemm(), x, pr.SEEDS)
    d64 = pr.oracle_dx(smpl_model, x, torch.float64)
    assert np.abs(verts - ref["verts"][rows]).max() <= VERT_ATOL
    _check_dx(dx, d64, rows, ref, [ref["rows"][n][0] for n in rows], "f32 gemm")


# ---- c. fused against separate launches at the regimes ------------------------------------------------------------
@pytest.mark.parametrize("lo,hi", [(0, None), (20, 53)])
def test_fused_pose_blend_equals_separate_calls_at_the_regimes(ref, consts, lo, hi):
    """The GEMM waves of pose_blend3_fwd_kernel re-evaluate Rodrigues for their coefficient rows: bit for bit
    pose_fwd_kernel's, also at tiny, exactly-zero and large angles (whole batch, and B = 33: one mesh past a tile)."""
    from ilps_amd import ops
    x = t(ref["x"][lo:hi])
    B = x.shape[0]
    assert hi is None or B == 33
    coef, Rs, J, A, Jt = ops._pose_fwd(x, 4, consts)
    vp = ops._blend_fwd(coef, consts, B)
    Rs2, J2, A2, Jt2, vp2 = ops._pose_blend_fwd(x, 4, consts)
    torch.cuda.synchronize()
    for a, b, name in ((Rs, Rs2, "Rs"), (J, J2, "J"), (A, A2, "A"), (Jt, Jt2, "J_transformed"), (vp, vp2, "v_posed")):
        assert torch.equal(a, b), name
        assert bool(torch.isfinite(a).all()), name


@pytest.mark.parametrize("gemm", ["bf16x3", "f32"])
def test_granular_backward_chain_equals_fused_at_the_regimes(ref, consts, gemm):
    """test_granular_backward_chain_equals_fused on the regime batch: smplr_skin_bwd -> smplr_blend(3)_bwd ->
    smplr_pose_bwd == smplr_smpl_bwd, bit for bit."""
    from ilps_amd import ops, _lib
    from ilps_amd._lib import ptr, stream, check
    lib = _lib.load()
    d = dev()
    c = consts if gemm == "bf16x3" else consts.fp32_gemm()
    x = t(ref["x"])
    B, V = x.shape[0], c.V
    coef, Rs, J, A, Jt = ops._pose_fwd(x, 4, c)
    v_posed = ops._blend_fwd(coef, c, B)
    rng = np.random.default_rng(2)
    dverts, dproj, dJt = t(rng.normal(0, 1, (B, V, 3))), t(rng.normal(0, 1, (B, V, 3))), t(rng.normal(0, 1, (B, 24, 3)))
    fused = ops._smpl_bwd(x, 4, c, Rs, J, A, v_posed, dverts, dproj, dJt)
    dv_posed, dA, dcam = torch.empty(B, V, 3, device=d), torch.empty(B, 24, 12, device=d), torch.empty(B, 4, device=d)
    ws = torch.empty(lib.smplr_skin_bwd_workspace(B, V) // 4 + 1, device=d)
    check(lib.smplr_skin_bwd(ptr(dverts), ptr(dproj), ptr(v_posed), ptr(c.lbs_weights), ptr(c.lbs_top4), ptr(A), ptr(x),
                             86, B, V, 1, ptr(dv_posed), ptr(dA), ptr(dcam), ptr(ws), stream()), "skin_bwd")
    dcoef = torch.empty(B, 220, device=d)
    if gemm == "f32":
        ws2 = torch.empty(lib.smplr_blend_bwd_workspace(B, 3 * V) // 4 + 1, device=d)
        check(lib.smplr_blend_bwd(ptr(dv_posed), ptr(c.blend_t), B, 3 * V, ptr(dcoef), ptr(ws2), stream()), "blend_bwd")
    else:
        ws2 = torch.empty(lib.smplr_blend3_bwd_workspace(B, 3 * V) // 4 + 1, device=d)
        check(lib.smplr_blend3_bwd(ptr(dv_posed), ptr(c.blend3_bwd), B, 3 * V, ptr(dcoef), ptr(ws2), stream()),
              "blend3_bwd")
    dx = torch.empty(B, 86, device=d)
    check(lib.smplr_pose_bwd(ptr(x), 86, 4, B, ptr(c.J_dirs), ptr(c.parents), ptr(Rs), ptr(J), ptr(A), ptr(dcoef),
                             ptr(dA), ptr(dJt), ptr(dcam), ptr(dx), stream()), "pose_bwd")
    torch.cuda.synchronize()
    assert torch.equal(dx, fused) and bool(torch.isfinite(dx).all())


# ---- d. the T-pose through the decoder ----------------------------------------------------------------------------
def test_tpose_through_the_decoder(ref, smpl_model, part_tables):
    """Where a fit starts: 23 joints exactly 0 (root from mean86), three cameras and shapes, a segmentation cotangent.
    test_decoder_end_to_end's oracle (given the HIP mask) and its bars."""
    from ilps_amd.decoder import SMPLDecoder
    from oracle import torch_oracle as to
    W, B = 48, 3
    tp = [n for n, (lab, _) in enumerate(ref["rows"]) if lab == pr.TPOSE]
    x = make_x(B, W, seed=67)
    x[:, 4:76] = ref["x"][tp[0], 4:76]
    gs = np.random.default_rng(19).normal(0, 1, (B, W, W, 32))
    dec = SMPLDecoder(smpl_model, img_wh=W)
    xg = t(x).requires_grad_(True)
    out = dec(xg)
    (out["seg"] * t(gs)).sum().backward()
    ids, off = part_tables[1]
    xo = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    mo = torch.tensor(out["mask"].cpu().numpy(), dtype=torch.float64)
    vo, po, _, so = to.decoder_forward(to.TorchSMPL(smpl_model), xo, lambda p: mo, W, ids, off)
    (so * torch.tensor(gs)).sum().backward()
    assert np.abs(out["verts"].detach().cpu().numpy() - vo.detach().numpy()).max() <= VERT_ATOL
    sg, sw = out["seg"].detach().cpu().numpy(), so.detach().numpy()
    assert np.all(np.abs(sg - sw) <= SEG_RTOL * np.abs(sw) + 1e-4)
    got, want = xg.grad.cpu().numpy(), xo.grad.numpy()
    assert np.isfinite(got).all()
    for sl, name in ((slice(0, 4), "dcam"), (slice(4, 76), "dtheta"), (slice(76, 86), "dbeta")):
        grad_close(got[:, sl], want[:, sl], 5e-3, "T-pose " + name)


# ---- e. camera widths ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [0, 3, 7, 16])
def test_num_cam(ref, smpl_model, k):
    """SMPLLayer(num_cam=k): theta starts at column k in pose_fwd_wave, the GEMM waves' producer and pose_bwd_kernel.
    An offset wrong by one column in any of them moves every joint angle (forward: metres; backward: the bar of the
    |theta| = 1 regime, ~4e-6).  The k camera columns get exactly 0."""
    from ilps_amd.keras_smpl.batch_smpl import SMPLLayer
    B = 5
    x = pr.make_x_cam(B, k, seed=900 + k)
    assert x.shape == (B, k + 82)
    d64, verts, jt = pr.oracle_dx(smpl_model, x, torch.float64, num_cam=k, seeds=pr.SEEDS[:1], return_forward=True)
    layer = SMPLLayer(smpl_model, num_cam=k)
    gv, gj = pr.cotangents(B, pr.SEEDS[0])
    xg = t(x).requires_grad_(True)
    v = layer(xg)
    ((v * t(gv)).sum() + (layer.J_transformed * t(gj)).sum()).backward()
    assert np.abs(v.detach().cpu().numpy() - verts).max() <= VERT_ATOL
    assert np.abs(layer.J_transformed.detach().cpu().numpy() - jt).max() <= VERT_ATOL
    dx = xg.grad.cpu().numpy().astype(np.float64)[None]
    assert dx.shape == (1, B, k + 82)
    _check_dx(dx, d64, list(range(B)), ref, ["1"] * B, "num_cam=%d" % k, num_cam=k)


# ---- f. the decoder with extra camera columns ---------------------------------------------------------------------
def test_decoder_with_extra_camera_columns(smpl_model, monkeypatch):
    """SMPLDecoder(num_cam=6) on [cam 4 | 2 x NaN | theta | beta]: the projection reads columns 0..3 at the row's own
    stride, theta starts at column 6; nothing reads the filler, and its gradient is exactly 0.  Gradient-free fast path
    (torch.ops.smplraster.decoder_fwd, seen being called) and the autograd node alike: bit for bit SMPLDecoder(num_cam=4)
    on the same rows without the filler."""
    from ilps_amd import torch_ops
    from ilps_amd.decoder import SMPLDecoder
    W, B = 48, 5
    x4 = make_x(B, W, seed=73)
    x6 = np.concatenate([x4[:, :4], np.full((B, 2), np.nan, np.float32), x4[:, 4:]], axis=1)
    g = np.random.default_rng(5).normal(0, 1, (B, W, W, 32))
    keys = ("verts", "projects", "mask", "seg", "J_transformed")
    assert torch_ops.available()
    real, seen = torch_ops.load(), []

    class Spy:
        def __getattr__(self, name):
            return getattr(real, name)

        def decoder_fwd(self, *a):
            seen.append(a[-1])                                       # num_cam, the last argument
            return real.decoder_fwd(*a)

    monkeypatch.setattr(torch_ops, "load", lambda: Spy())
    res = {}
    for k, x in ((4, x4), (6, x6)):
        dec = SMPLDecoder(smpl_model, img_wh=W, num_cam=k)
        n0 = len(seen)
        with torch.no_grad():
            fast = dec(t(x))
        assert seen[n0:] == [k], "the gradient-free forward must go through decoder_fwd"
        xg = t(x).requires_grad_(True)
        out = dec(xg)
        assert len(seen) == n0 + 1                                   # the autograd node, not the op
        (out["seg"] * t(g)).sum().backward()
        torch.cuda.synchronize()
        res[k] = (fast, {q: out[q].detach() for q in keys}, xg.grad.cpu().numpy())
    for q in keys:
        assert bool(torch.isfinite(res[6][0][q]).all()) and bool(torch.isfinite(res[6][1][q]).all()), q
        assert torch.equal(res[6][0][q], res[4][0][q]), "fast path " + q
        assert torch.equal(res[6][1][q], res[4][1][q]), "autograd path " + q
        assert torch.equal(res[6][0][q], res[6][1][q]), "fast vs autograd " + q
    # (both widths could be wrong alike: the vertices are also held to float64)
    from oracle import np_oracle as o
    want = o.smpl_layer_call(x4.astype(np.float64), smpl_model)
    assert np.abs(res[6][0]["verts"].cpu().numpy() - want).max() <= VERT_ATOL
    d4, d6 = res[4][2], res[6][2]
    assert d6.shape == (B, 88) and np.isfinite(d6).all()
    assert np.all(d6[:, 4:6] == 0)
    # (the rasteriser's backward adds with LDS atomics: equal to rounding, the bar of test_concurrent_chunks_identical)
    grad_close(np.concatenate([d6[:, :4], d6[:, 6:]], axis=1), d4, 1e-5, "dx num_cam=6 vs 4")


# ---- g. row stride --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pad", [1, 10])
def test_row_stride(consts, smpl_model, pad):
    """x (B, 86 + pad) with num_cam = 4 and NaN in the surplus columns through the four entry points that take a row
    stride: every output equals the (B, 86) call's bit for bit, the surplus columns of dx are 0.  Both could be wrong
    alike, so the wide call is also held to float64: verts and the projection to 1e-4, dx per row and block to 4 x the
    float32 oracle's own error on these rows and cotangents (capped by 2e-3), as in the regime tests."""
    from ilps_amd import ops
    d = dev()
    c = consts
    pt = ops.get_part_table(1, d, c.V)
    B, W = 5, 48
    x86 = make_x(B, W, seed=83)
    xw = np.concatenate([x86, np.full((B, pad), np.nan, np.float32)], axis=1)
    rng = np.random.default_rng(4)
    dverts, dproj, dJt = t(rng.normal(0, 1, (B, c.V, 3))), t(rng.normal(0, 1, (B, c.V, 3))), t(rng.normal(0, 1, (B, 24, 3)))
    res = []
    for x in (t(x86), t(xw)):
        coef, Rs, J, A, Jt = ops._pose_fwd(x, 4, c, want="both")
        fused = ops._pose_blend_fwd(x, 4, c)
        vs = torch.empty(B, c.V, dtype=torch.int16, device=d)
        verts, proj, mask, seg, arg, rec = ops._skin_vis_seg_fwd(fused[4], fused[2], c, x, W, pt, vslot=vs)
        dx = ops._smpl_bwd(x, 4, c, fused[0], fused[1], fused[2], fused[4], dverts, dproj, dJt)
        torch.cuda.synchronize()
        assert dx.shape == x.shape
        res.append(dict(kmajor=coef.kmajor, frag3=coef.frag3, Rs=Rs, J=J, A=A, Jt=Jt, Rs2=fused[0], J2=fused[1], A2=fused[2],
                        Jt2=fused[3], v_posed=fused[4], verts=verts, proj=proj, mask=mask, seg=seg, gate=arg[..., 0],
                        winners=ops.argmin_vertices(arg, rec), dx=dx))
        # (the slot ids in vslot / arg depend on the order of the binning kernel's LDS atomics: winners are compared)
    a, b = res
    live = slice(0, B)                                                # (columns of the k-major operand past B are padding)
    assert torch.equal(a["kmajor"][:, live], b["kmajor"][:, live])
    for q in a:
        if q in ("kmajor", "dx", "frag3"):
            continue
        assert torch.equal(a[q], b[q]), q
        assert a[q].dtype != torch.float32 or bool(torch.isfinite(b[q]).all()), q
    assert torch.equal(a["dx"], b["dx"][:, :86])
    assert bool((b["dx"][:, 86:] == 0).all())
    g = [q.cpu().numpy().astype(np.float64) for q in (dverts, dproj, dJt)]
    d64, v64, p64 = pr.oracle_dx_proj(smpl_model, x86, torch.float64, *g)
    d32 = pr.oracle_dx_proj(smpl_model, x86, torch.float32, *g)[0]
    assert np.abs(b["verts"].cpu().numpy() - v64).max() <= VERT_ATOL
    assert np.abs(b["proj"].cpu().numpy() - p64).max() <= VERT_ATOL * np.abs(x86[:, :2]).max()    # pixels = k x metres
    got = b["dx"][:, :86].cpu().numpy().astype(np.float64)
    for blk, sl in (("cam", slice(0, 4)), ("theta", slice(4, 76)), ("beta", slice(76, 86))):
        scale = np.abs(d64[:, sl]).max(axis=1)
        e32 = (np.abs(d32[:, sl] - d64[:, sl]).max(axis=1) / scale).max()
        e = (np.abs(got[:, sl] - d64[:, sl]).max(axis=1) / scale).max()
        print("STRIDE pad=%d %-5s ref_err %.3e hip %.3e" % (pad, blk, e32, e))
        assert e <= min(pr.FACTOR * e32, pr.CAP), (blk, e, e32)


# ---- h. refusals: nothing is launched -------------------------------------------------------------------------------
def test_refusals(smpl_model, consts):
    """Sizes the pose path cannot serve are refused before any launch - by SMPLR_REQUIRE in the launchers
    (num_cam <= 16, x_stride >= num_cam + 82, dproj needs num_cam >= 4) or by the Python shape checks (SMPLDecoder
    needs the 4 camera columns: the projection would read joint angles for a camera otherwise, and no launcher can
    tell) - and leave the library usable."""
    from ilps_amd import ops, _lib
    from ilps_amd._lib import ptr, stream, check
    from ilps_amd.decoder import SMPLDecoder
    from ilps_amd.keras_smpl.batch_smpl import SMPLLayer
    from oracle import np_oracle as o
    lib = _lib.load()
    d = dev()
    c = consts
    B = 2
    with pytest.raises(RuntimeError, match="num_cam"):
        SMPLDecoder(smpl_model, img_wh=48, num_cam=3)(torch.zeros(B, 85, device=d))
    with pytest.raises(RuntimeError, match="num_cam"):
        SMPLDecoder(smpl_model, img_wh=48, num_cam=3)(torch.zeros(B, 85, device=d, requires_grad=True))
    with pytest.raises(RuntimeError, match="num_cam"):
        SMPLDecoder(smpl_model, img_wh=48, num_cam=17)(torch.zeros(B, 99, device=d))
    with pytest.raises(RuntimeError, match="bad sizes"):
        SMPLLayer(smpl_model, num_cam=17)(torch.zeros(B, 99, device=d))
    # dproj with three camera columns: a legitimate num_cam = 3 forward first, then the refused backward
    x3 = t(pr.make_x_cam(B, 3, seed=5))
    Rs, J, A, Jt, vp = ops._pose_blend_fwd(x3, 3, c)
    g = torch.ones(B, c.V, 3, device=d)
    with pytest.raises(RuntimeError, match="dproj needs the 4 camera columns"):
        ops._smpl_bwd(x3, 3, c, Rs, J, A, vp, g, g, None)
    assert bool(torch.isfinite(ops._smpl_bwd(x3, 3, c, Rs, J, A, vp, g, None, None)).all())   # without dproj it is served
    # a row stride shorter than num_cam + 82, straight through the C ABI
    x = t(make_x(B, 48, seed=6))
    Rs, J, A, Jt = (torch.empty(B, 24, n, device=d) for n in (9, 3, 12, 3))
    f3 = torch.empty(max(int(lib.smplr_coef3_bytes(B)), 16), dtype=torch.uint8, device=d)
    vp = torch.empty(B, c.V, 3, device=d)
    dx = torch.empty(B, 86, device=d)
    ws = torch.empty(lib.smplr_smpl_bwd_workspace(B, c.V) // 4 + 1, device=d)
    with pytest.raises(RuntimeError, match="bad sizes"):
        check(lib.smplr_pose_fwd(ptr(x), 85, 4, B, ptr(c.J_template), ptr(c.J_dirs), ptr(c.parents), None, ptr(f3), ptr(Rs),
                                 ptr(J), ptr(A), ptr(Jt), stream()), "smplr_pose_fwd")
    with pytest.raises(RuntimeError, match="bad sizes"):
        check(lib.smplr_pose_blend3_fwd(ptr(x), 85, 4, B, ptr(c.J_template), ptr(c.J_dirs), ptr(c.parents),
                                        ptr(c.blend3_fwd), ptr(c.v_template), 3 * c.V, ptr(Rs), ptr(J), ptr(A), ptr(Jt),
                                        ptr(vp), stream()), "smplr_pose_blend3_fwd")
    with pytest.raises(RuntimeError, match="bad sizes"):
        check(lib.smplr_smpl_bwd(ptr(g), None, None, None, 0, None, ptr(x), 85, 4, B, c.V, 1, ptr(c.blend_t),
                                 ptr(c.blend3_bwd), ptr(c.lbs_weights), ptr(c.lbs_top4), ptr(c.J_dirs), ptr(c.parents),
                                 ptr(Rs), ptr(J), ptr(A), ptr(vp), ptr(dx), ptr(ws), stream()), "smplr_smpl_bwd")
    with pytest.raises(RuntimeError, match="bad sizes"):
        check(lib.smplr_pose_bwd(ptr(x), 85, 4, B, ptr(c.J_dirs), ptr(c.parents), ptr(Rs), ptr(J), ptr(A), ptr(dx),
                                 ptr(A), None, None, ptr(dx), stream()), "smplr_pose_bwd")
    torch.cuda.synchronize()
    # ... and an ordinary forward still matches its oracle
    x = make_x(B, 48, seed=7)
    got = SMPLLayer(smpl_model)(t(x)).cpu().numpy()
    assert np.abs(got - o.smpl_layer_call(x.astype(np.float64), smpl_model)).max() <= VERT_ATOL
