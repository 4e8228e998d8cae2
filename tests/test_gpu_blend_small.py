"""The blend-shape GEMMs (the C ABI, through ctypes) at the SMALLEST shapes that reach every branch of their kernels,
against a float64 numpy reference written here:  v_posed = a @ b + vt  (a = coef^T (B, 220), b = blend (220, N3)) and
dcoef = g @ b^T.  Operands: seeded normal fp32, rows 217..219 of the constant zero.

Forward (smplr_blend_fwd; smplr_coef3_pack -> smplr_blend3_fwd), N3 x B:
    N3 = 95: lane 31 of the only column tile takes the scalar tail    97: a second tile that holds ONE column, every
    other lane clamped and storing nothing    290: four tiles, the last ragged    16: the backward's minimum
    B = 1    33: one row past a mesh tile    129: a second group of 128 meshes with three empty waves
Fused forward (smplr_pose_blend3_fwd == smplr_pose_fwd + smplr_blend3_fwd, all five outputs, bit for bit) at
    (B, N3) = (1, 18), (33, 97), (129, 290); B = 129 takes the empty pair of waves through the barrier.
Backward (smplr_blend3_bwd, smplr_blend_bwd), N3 x B:
    N3 = 16: no ragged k-tile    22: the ragged k-tile is the whole second slice    150 = 8 * 18 + 6: ten slices, so
    the second group of eight has six empty ones; also the fp32 kernel's ragged group of columns
    B = 1, 33    512: the first use of the two-tile form    513: 17 tiles, the last group holds one live tile

Bars.  bf16x3 paths: the project's own of test_blend3_wide_dynamic_range, |got - ref| <= 2e-6 mag forward and 4e-6 mag
backward, mag = |a| @ |b| + |vt| resp. |g| @ |b^T|.  fp32 matrix-core paths: the worst-case bound of a sequential fp32
sum, (n + 1) 2^-24 mag with n = the number of terms: 220 forward, N3 backward.  dcoef[:, 217:] is exactly 0.  Every
output, packed operand and workspace is allocated with a NaN guard behind the size the library reports, and the guard
must come back untouched.  (No forward N3 here is a multiple of 3, unlike every 3 V: the fp32 forward's lane that
straddles the end of the matrix used to store the columns of its clamped load, off by 0.1 of mag; fixed with this file.)

Without a GPU: a numpy emulation of the kernels' arithmetic at the same shapes (the round-to-nearest three-term bf16
split, the six partial products in the kernels' order into separate hi / lo fp32 sums; for the fp32 path an fp32
running sum) lands inside the same bars, i.e. the reference alone leaves room; the fragment layouts documented in
csrc/blend_device.h, restated here, are bijections onto their buffers; the byte counts are the library's."""
import functools

import numpy as np
import pytest

U = 2.0 ** -24
KP, NKT, BN, NT = 220, 14, 96, 7          # csrc/blend_device.h: KP, NKT, BL_BN, BL_NT
FWD_N3, FWD_B = [16, 95, 97, 290], [1, 33, 129]
BWD_N3, BWD_B = [16, 22, 150], [1, 33, 512, 513]
FUSED = [(1, 18), (33, 97), (129, 290)]
BAR3_FWD, BAR3_BWD = 2e-6, 4e-6
GUARD = 64                                 # floats of NaN behind every buffer the kernels write


# ------------------------------------------------------------------------------------------------ inputs and reference
@functools.lru_cache(maxsize=None)
def constant(N3):
    rng = np.random.default_rng(7000 + N3)
    blend = rng.normal(0, 1, (KP, N3)).astype(np.float32)
    blend[217:] = 0
    vt = rng.normal(0, 1, N3).astype(np.float32)
    for a in (blend, vt):
        a.setflags(write=False)
    return blend, vt


@functools.lru_cache(maxsize=None)
def fwd_case(B, N3):
    blend, vt = constant(N3)
    a = np.random.default_rng(100 * B + N3).normal(0, 1, (B, KP)).astype(np.float32)
    a64, b64 = a.astype(np.float64), blend.astype(np.float64)
    c = dict(a=a, ref=a64 @ b64 + vt, mag=np.abs(a64) @ np.abs(b64) + np.abs(vt.astype(np.float64)))
    for v in c.values():
        v.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def bwd_case(B, N3):
    blend, _ = constant(N3)
    g = np.random.default_rng(100 * B + N3 + 1).normal(0, 1, (B, N3)).astype(np.float32)
    g64, bt64 = g.astype(np.float64), blend.astype(np.float64).T
    c = dict(g=g, ref=g64 @ bt64, mag=np.abs(g64) @ np.abs(bt64))
    for v in c.values():
        v.setflags(write=False)
    return c


def ratio(got, c, bar):
    """max |got - ref| / (bar * mag) over the entries with a non-zero magnitude; the others must be exactly equal."""
    err, lim = np.abs(got.astype(np.float64) - c["ref"]), bar * c["mag"]
    assert np.all(err[lim == 0] == 0)
    return float((err[lim > 0] / lim[lim > 0]).max())


# ------------------------------------------------------------------------------------------------ emulation (no GPU)
def bf16_rne(x):
    """float32 -> the nearest bf16 (ties to even), as a float32."""
    b = np.ascontiguousarray(x, np.float32).view(np.uint32)
    return ((b + 0x7fff + ((b >> 16) & 1)) & 0xffff0000).astype(np.uint32).view(np.float32)


def split3(x):
    h = bf16_rne(x)
    r = (x - h).astype(np.float32)
    m = bf16_rne(r)
    return h, m, bf16_rne((r - m).astype(np.float32))


def emulate3(a, b):
    """(M, K) x (K, N) as the bf16x3 kernels do it: per k, the six products (l h, h l, m m, m h, h m into `lo`, h h into
    `hi`), every partial sum rounded to fp32; hi + lo at the end."""
    ah, am, al = split3(a)
    bh, bm, bl = split3(b)
    for parts in ((ah, am, al), (bh, bm, bl)):          # the split is exact
        assert np.array_equal(parts[0].astype(np.float64) + parts[1] + parts[2], (a if parts[0] is ah else b))
    hi, lo = np.zeros((a.shape[0], b.shape[1]), np.float32), np.zeros((a.shape[0], b.shape[1]), np.float32)
    for k in range(a.shape[1]):
        for x, y in ((al, bh), (ah, bl), (am, bm), (am, bh), (ah, bm)):
            lo = lo + x[:, k, None] * y[None, k, :]
        hi = hi + ah[:, k, None] * bh[None, k, :]
    assert hi.dtype == np.float32 and lo.dtype == np.float32
    return hi + lo


def emulate1(a, b):
    acc = np.zeros((a.shape[0], b.shape[1]), np.float32)
    for k in range(a.shape[1]):
        acc = acc + a[:, k, None] * b[None, k, :]
    assert acc.dtype == np.float32
    return acc


def test_split_is_round_to_nearest_and_exact():
    x = (np.random.default_rng(3).normal(0, 1, 4096) * 10.0 ** np.random.default_rng(4).uniform(-6, 6, 4096)).astype(np.float32)
    h, m, l = split3(x)
    assert np.array_equal(h.astype(np.float64) + m + l, x)
    assert np.all(np.abs(x - h) <= np.abs(x) * 2.0 ** -8) and np.all(h.view(np.uint32) & 0xffff == 0)
    one = np.array([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8], np.float32)      # ties: to the even bf16 neighbour
    assert np.array_equal(bf16_rne(one), np.array([1.0, 1.0 + 2.0 ** -6], np.float32))


def test_emulated_forward_is_inside_the_bars():
    worst3 = worst1 = 0.0
    for N3 in FWD_N3:
        blend, vt = constant(N3)
        for B in FWD_B:
            c = fwd_case(B, N3)
            worst3 = max(worst3, ratio(emulate3(c["a"], blend) + vt, c, BAR3_FWD))
            worst1 = max(worst1, ratio(emulate1(c["a"], blend) + vt, c, (KP + 1) * U))
    print("forward, worst error / bar: bf16x3 %.3f, fp32 %.3f" % (worst3, worst1))
    assert worst3 <= 1 and worst1 <= 1


def test_emulated_backward_is_inside_the_bars():
    worst3 = worst1 = 0.0
    for N3 in BWD_N3:
        bt = np.ascontiguousarray(constant(N3)[0].T)
        for B in BWD_B:
            c = bwd_case(B, N3)
            got3, got1 = emulate3(c["g"], bt), emulate1(c["g"], bt)
            assert not got3[:, 217:].any() and not got1[:, 217:].any()
            worst3 = max(worst3, ratio(got3, c, BAR3_BWD))
            worst1 = max(worst1, ratio(got1, c, (N3 + 1) * U))
    print("backward, worst error / bar: bf16x3 %.3f, fp32 %.3f" % (worst3, worst1))
    assert worst3 <= 1 and worst1 <= 1


def layouts(B, N3):
    """name -> (unit index of every fragment lane, (row, col, split) it holds per element j) for the three layouts of
    csrc/blend_device.h; a unit = 16 bytes = 8 bf16."""
    lane = np.arange(64)
    i, h, j = lane & 31, lane >> 5, np.arange(8)
    out = {}
    # coef3 [mesh tile][k-tile NKT][split 3][lane 64]: element j = split_s(coef[16 kt + 8h + j][32 mt + i])
    mt, kt, s = np.meshgrid(np.arange((B + 31) // 32), np.arange(NKT), np.arange(3), indexing="ij")
    idx = ((mt * NKT + kt) * 3 * 64 + s * 64)[..., None] + lane
    k = (16 * kt)[..., None, None] + (8 * h)[:, None] + j
    m = (32 * mt)[..., None, None] + i[:, None] + 0 * j
    out["coef3"] = (idx, k, m, s[..., None, None] + 0 * k, (NKT * 16, (B + 31) // 32 * 32))
    # pk_fwd [column tile][k-tile NKT][t 3][split 3][lane 64]: element j = split_s(blend[16 kt + 8h + j][96 ct + 3i + t])
    ct, kt, t, s = np.meshgrid(np.arange((N3 + BN - 1) // BN), np.arange(NKT), np.arange(3), np.arange(3), indexing="ij")
    idx = ((ct * NKT + kt) * 9 * 64 + (t * 3 + s) * 64)[..., None] + lane
    k = (16 * kt)[..., None, None] + (8 * h)[:, None] + j
    col = (BN * ct + t)[..., None, None] + (3 * i)[:, None] + 0 * j
    out["pk_fwd"] = (idx, k, col, s[..., None, None] + 0 * k, (NKT * 16, (N3 + BN - 1) // BN * BN))
    # pk_bwd [k-tile ceil(N3 / 16)][out tile 7][split 3][lane 64]: element j = split_s(blend[32u + i][16 kt + 8h + j])
    kt, u, s = np.meshgrid(np.arange((N3 + 15) // 16), np.arange(NT), np.arange(3), indexing="ij")
    idx = ((kt * NT + u) * 3 * 64 + s * 64)[..., None] + lane
    row = (32 * u)[..., None, None] + i[:, None] + 0 * j
    col = (16 * kt)[..., None, None] + (8 * h)[:, None] + j
    out["pk_bwd"] = (idx, row, col, s[..., None, None] + 0 * row, (NT * 32, (N3 + 15) // 16 * 16))
    return out


@pytest.mark.parametrize("B", [1, 33])
@pytest.mark.parametrize("N3", [16, 97])
def test_fragment_layouts_are_bijections(B, N3):
    from ilps_amd import _lib
    lib = _lib.load()
    nbytes = {"coef3": lib.smplr_coef3_bytes(B), "pk_fwd": lib.smplr_blend3_fwd_bytes(N3),
              "pk_bwd": lib.smplr_blend3_bwd_bytes(N3)}
    for name, (idx, r, c, s, (nr, nc)) in layouts(B, N3).items():
        assert nbytes[name] % 16 == 0
        assert np.array_equal(np.sort(idx.ravel()), np.arange(nbytes[name] // 16)), name      # units <-> buffer
        key = (s.ravel() * nr + r.ravel()) * nc + c.ravel()                                   # elements <-> padded matrix
        assert r.min() == 0 and r.max() == nr - 1 and c.min() == 0 and c.max() == nc - 1, name
        assert np.array_equal(np.sort(key), np.arange(3 * nr * nc)), name
        assert nr >= KP and nc >= (N3 if name != "coef3" else B)


def test_byte_counts():
    from ilps_amd import _lib
    lib = _lib.load()
    for B in (0, 1, 32, 33, 129, 513):
        assert lib.smplr_coef3_bytes(B) == (B + 31) // 32 * NKT * 3 * 64 * 16
        assert lib.smplr_coef_ld(B) == (B + 31) // 32 * 32
    for N3 in (0, 16, 22, 95, 96, 97, 290, 20670):
        assert lib.smplr_blend3_fwd_bytes(N3) == (N3 + BN - 1) // BN * NKT * 9 * 64 * 16
        assert lib.smplr_blend3_bwd_bytes(N3) == (N3 + 15) // 16 * NT * 3 * 64 * 16


# --------------------------------------------------------------------------------------------------------- GPU
def t(a):
    """a device copy (the cached inputs are read-only)"""
    import test_gpu_parity
    return test_gpu_parity.t(np.array(a))


def guarded(nfloat):
    """nfloat + GUARD floats of NaN on the device; the kernels own the first nfloat."""
    import torch
    from test_gpu_parity import dev
    return torch.full((int(nfloat) + GUARD,), np.nan, device=dev())


def intact(buf, nfloat):
    import torch
    return bool(torch.isnan(buf[int(nfloat):]).all())


def pack_constant(lib, N3):
    from ilps_amd._lib import ptr, stream, check
    blend, _ = constant(N3)
    nf, nb = lib.smplr_blend3_fwd_bytes(N3) // 4, lib.smplr_blend3_bwd_bytes(N3) // 4
    pf, pb, bl = guarded(nf), guarded(nb), t(blend)
    check(lib.smplr_blend3_pack(ptr(bl), N3, ptr(pf), ptr(pb), stream()), "smplr_blend3_pack")
    return pf, pb, nf, nb


@pytest.mark.gpu
@pytest.mark.parametrize("B", FWD_B)
@pytest.mark.parametrize("N3", FWD_N3)
def test_blend_fwd_small(N3, B):
    import torch
    from ilps_amd import _lib
    from ilps_amd._lib import ptr, stream, check
    lib = _lib.load()
    c, (blend, vt) = fwd_case(B, N3), constant(N3)
    coef = np.zeros((KP, lib.smplr_coef_ld(B)), np.float32)
    coef[:, :B] = c["a"].T
    cf, bl, vtd = t(coef), t(blend), t(vt)
    out1 = guarded(B * N3)
    check(lib.smplr_blend_fwd(ptr(cf), ptr(bl), ptr(vtd), B, N3, ptr(out1), stream()), "smplr_blend_fwd")
    pf, pb, nf, nb = pack_constant(lib, N3)
    n3 = lib.smplr_coef3_bytes(B) // 4
    c3, out3 = guarded(n3), guarded(B * N3)
    check(lib.smplr_coef3_pack(ptr(cf), B, ptr(c3), stream()), "smplr_coef3_pack")
    check(lib.smplr_blend3_fwd(ptr(c3), ptr(pf), ptr(vtd), B, N3, ptr(out3), stream()), "smplr_blend3_fwd")
    torch.cuda.synchronize()
    for name, buf, n in (("v_posed (fp32)", out1, B * N3), ("v_posed (bf16x3)", out3, B * N3), ("coef3", c3, n3),
                         ("pk_fwd", pf, nf), ("pk_bwd", pb, nb)):
        assert intact(buf, n), "%s: the guard behind the buffer was written" % name
    r1 = ratio(out1[:B * N3].cpu().numpy().reshape(B, N3), c, (KP + 1) * U)
    r3 = ratio(out3[:B * N3].cpu().numpy().reshape(B, N3), c, BAR3_FWD)
    print("B=%d N3=%d forward, error / bar: fp32 %.3f, bf16x3 %.3f" % (B, N3, r1, r3))
    assert r1 <= 1, "smplr_blend_fwd: %.3f of (220 + 1) 2^-24 mag" % r1
    assert r3 <= 1, "smplr_blend3_fwd: %.3f of 2e-6 mag" % r3


@pytest.mark.gpu
@pytest.mark.parametrize("B", BWD_B)
@pytest.mark.parametrize("N3", BWD_N3)
def test_blend_bwd_small(N3, B):
    import torch
    from ilps_amd import _lib
    from ilps_amd._lib import ptr, stream, check
    lib = _lib.load()
    c, (blend, _) = bwd_case(B, N3), constant(N3)
    blend_t = np.zeros((N3, 224), np.float32)
    blend_t[:, :KP] = blend.T
    g, bt = t(c["g"]), t(blend_t)
    pf, pb, nf, nb = pack_constant(lib, N3)
    w3, w1 = lib.smplr_blend3_bwd_workspace(B, N3) // 4, lib.smplr_blend_bwd_workspace(B, N3) // 4
    ws3, ws1, dc3, dc1 = guarded(w3), guarded(w1), guarded(B * KP), guarded(B * KP)
    check(lib.smplr_blend3_bwd(ptr(g), ptr(pb), B, N3, ptr(dc3), ptr(ws3), stream()), "smplr_blend3_bwd")
    check(lib.smplr_blend_bwd(ptr(g), ptr(bt), B, N3, ptr(dc1), ptr(ws1), stream()), "smplr_blend_bwd")
    torch.cuda.synchronize()
    for name, buf, n in (("dcoef (bf16x3)", dc3, B * KP), ("dcoef (fp32)", dc1, B * KP), ("workspace (bf16x3)", ws3, w3),
                         ("workspace (fp32)", ws1, w1), ("pk_fwd", pf, nf), ("pk_bwd", pb, nb)):
        assert intact(buf, n), "%s: the guard behind the buffer was written" % name
    got3, got1 = dc3[:B * KP].cpu().numpy().reshape(B, KP), dc1[:B * KP].cpu().numpy().reshape(B, KP)
    assert np.all(got3[:, 217:] == 0) and np.all(got1[:, 217:] == 0)
    r3, r1 = ratio(got3, c, BAR3_BWD), ratio(got1, c, (N3 + 1) * U)
    print("B=%d N3=%d backward, error / bar: fp32 %.3f, bf16x3 %.3f" % (B, N3, r1, r3))
    assert r3 <= 1, "smplr_blend3_bwd: %.3f of 4e-6 mag" % r3
    assert r1 <= 1, "smplr_blend_bwd: %.3f of (N3 + 1) 2^-24 mag" % r1


@pytest.mark.gpu
@pytest.mark.parametrize("B,N3", FUSED)
def test_pose_blend3_fwd_small_equals_the_two_launches(smpl_model, B, N3):
    import torch
    from ilps_amd import _lib, ops
    from ilps_amd._lib import ptr, stream, check
    from _inputs import make_x
    from test_gpu_parity import dev
    lib = _lib.load()
    k = ops.SMPLConstants.from_model(smpl_model, dev())
    x, vtd = t(make_x(B, 48, seed=900 + B)), t(constant(N3)[1])
    pf, pb, nf, nb = pack_constant(lib, N3)
    sizes = (B * 216, B * 72, B * 288, B * 72, B * N3)                 # Rs, J, A, J_transformed, v_posed
    two, one = [guarded(n) for n in sizes], [guarded(n) for n in sizes]
    n3 = lib.smplr_coef3_bytes(B) // 4
    c3 = guarded(n3)
    check(lib.smplr_pose_fwd(ptr(x), x.shape[1], 4, B, ptr(k.J_template), ptr(k.J_dirs), ptr(k.parents), None, ptr(c3),
                             ptr(two[0]), ptr(two[1]), ptr(two[2]), ptr(two[3]), stream()), "smplr_pose_fwd")
    check(lib.smplr_blend3_fwd(ptr(c3), ptr(pf), ptr(vtd), B, N3, ptr(two[4]), stream()), "smplr_blend3_fwd")
    check(lib.smplr_pose_blend3_fwd(ptr(x), x.shape[1], 4, B, ptr(k.J_template), ptr(k.J_dirs), ptr(k.parents), ptr(pf),
                                    ptr(vtd), N3, ptr(one[0]), ptr(one[1]), ptr(one[2]), ptr(one[3]), ptr(one[4]),
                                    stream()), "smplr_pose_blend3_fwd")
    torch.cuda.synchronize()
    for name, a, b, n in zip(("Rs", "J", "A", "J_transformed", "v_posed"), two, one, sizes):
        assert intact(a, n) and intact(b, n), "%s: the guard behind the buffer was written" % name
        assert not torch.isnan(a[:n]).any(), name
        assert torch.equal(a[:n], b[:n]), "%s differs between the fused launch and the two launches" % name
    assert intact(c3, n3) and intact(pf, nf)
