"""smplr_smpl_bwd restated in float64, stage by stage, with a MAGNITUDE beside every value (the same expression on
absolute values): the reference of tests/test_gpu_smpl_bwd_small.py and tests/test_smpl_bwd_oracle_cpu.py.

    S  skinning backward (the definition is in test_gpu_skin_small.py's docstring; `oracle` / `top4_of` live here and
       that file imports them back):   g_v = dverts_v + (k_u du, k_v dv, dz)  ->  dv_posed, dA, dcam.
       With slot sums, (du, dv) of vertex v is the float64 sum of its slot's fp32 row-block sums t_s (dz = 0) and its
       magnitude is sum_s |t_s|.
    G  blend GEMM backward:            dcoef = dv_posed @ blend^T,   mag = mag_dv_posed @ |blend^T|.
    P  pose backward:                  Jp = the float64 Jacobian of x -> (coef 217, A 288, J_transformed 72), per mesh,
       torch.autograd.functional.jacobian over oracle/torch_oracle.py's batch_rodrigues and
       batch_global_rigid_transformation (577 x 86, cached per vertex count and mesh);
       dx[4:] = Jp^T [dcoef; dA; dJt], dx[:4] = dcam;  mag_dx = |Jp|^T [mag_dcoef; mag_dA; |dJt|], camera: mag_dcam.

The forward values S and P are linearised at are the float64 ones of the same x (fp32 rows of _inputs.make_x), so the
staged dx is the true gradient: it equals autograd through TorchSMPL + orthographic_project (the CPU file checks that).

The bar of the GPU file per entry of dx is K 2^-24 mag_dx with
    K = 2 (V + 8)  [test_gpu_skin_small.py's bound for dA and the camera sums]  +  (nsplit - 1)  [the block sum]
      + BAR3_BWD / 2^-24 for bf16x3 | 3 V + 1 for fp32  [test_gpu_blend_small.py]  +  K_pose,
K_pose = 4 x the largest error / (2^-24 mag_dx) of the FLOAT32 pose stage (autograd through TorchSMPL(float32)'s
constants, fed the float64 stages S and G rounded to fp32) over the rows of every case in CASES; `k_pose()` measures
it, nothing here is taken from the HIP output.

Hand-built slot sums (`layout`): part (B, nsplit, 5 x 4096, 2), vslot (B, VP) as _seg_bwd(merge=False) and the
forward's vslot would leave them; records are live (non-zero block sum), or dead in one of three ways - no slot, all
blocks zero, blocks that cancel exactly; a live record may have sx == 0."""
import collections
import dataclasses
import functools

import numpy as np
import torch

U = 2.0 ** -24
NSLOT = 5 * 4096                   # slots per row block of the partial buffer (SB_NWIN * SB_SLOTS, csrc/common.h)
CHUNK = 1024                       # vertices per workgroup of skin_bwd_rec_kernel
BLOCK = 256                        # vertices per workgroup of skin_bwd_kernel
W_IMG = 48                         # make_x's image width (the camera's scale)
NX = 513                           # rows of the one x every case takes its first B rows of
SHAPES = [8, 64, 257, 1024, 1025, 2049]
COTS = ["dverts", "dproj", "all", "slots", "slots+dverts", "slots+dproj+dJt"]
GEMMS = ["bf16x3", "f32"]
WEIGHTS = ["sparse", "dense"]


# ------------------------------------------------------------------------------------------------ stage S
def top4_of(w32):
    """(V, 8) [w0..w3 | j0..j3] as ops.SMPLConstants.from_model lays it out: non-zero joints first, ascending."""
    order = np.argsort(w32 == 0, axis=1, kind="stable")[:, :4]
    wv = np.take_along_axis(w32, order, 1)
    idx = np.where(wv != 0, order, 0)
    return np.concatenate([wv, idx.astype(np.float32)], axis=1)


def oracle(c, w, dverts, dproj, mag_dproj=None):
    """float64 values and magnitudes (the same expressions on absolute values) of every output of the skinning stage.
    c: dict(V, vs, vp (B, V, 3), A (B, 24, 12), x (B, >= 4)); mag_dproj: the magnitude of dproj where it is itself a
    sum (slot sums), else |dproj|."""
    V, vs = c["V"], c["vs"]
    B = c["A"].shape[0]
    out = {}
    for tag, ab in (("", lambda a: a), ("mag_", np.abs)):
        w64, A, p = ab(w.astype(np.float64)), ab(c["A"].astype(np.float64)), ab(c["vp"].astype(np.float64))
        cam = ab(c["x"][:, :4].astype(np.float64))
        T = np.einsum("vj,bje->bve", w64, A).reshape(B, V, 3, 4)
        ph = np.concatenate([p, np.ones((B, V, 1))], axis=2)
        verts = np.einsum("bvrc,bvc->bvr", T, ph)
        s = verts[:, ::vs]
        proj = np.stack([cam[:, None, 2] + s[..., 0] * cam[:, None, 0], cam[:, None, 3] + s[..., 1] * cam[:, None, 1],
                         s[..., 2]], axis=2)
        g = np.zeros((B, V, 3)) if dverts is None else ab(dverts.astype(np.float64)).copy()
        dcam = np.zeros((B, 4))
        if dproj is not None:
            d = ab(dproj.astype(np.float64))
            if tag and mag_dproj is not None:
                d = np.asarray(mag_dproj, np.float64)
            g[:, ::vs, 0] += cam[:, None, 0] * d[..., 0]
            g[:, ::vs, 1] += cam[:, None, 1] * d[..., 1]
            g[:, ::vs, 2] += d[..., 2]
            dcam = np.stack([(s[..., 0] * d[..., 0]).sum(1), (s[..., 1] * d[..., 1]).sum(1), d[..., 0].sum(1),
                             d[..., 1].sum(1)], axis=1)
        out[tag + "verts"], out[tag + "proj"] = verts, proj
        out[tag + "dv_posed"] = np.einsum("bvrc,bvr->bvc", T[..., :3], g)
        out[tag + "dA"] = np.einsum("vj,bvr,bvc->bjrc", w64, g, ph).reshape(B, 24, 12)
        out[tag + "dcam"] = dcam
    return out


# ------------------------------------------------------------------------------------------------ models and x
def dense_weights(V, seed):
    """(V, 24) fp32 rows with exactly 7 non-zeros that sum to ~1: no top4 table, the dense kernels."""
    rng = np.random.default_rng(seed)
    w = np.zeros((V, 24), np.float32)
    for v in range(V):
        j = rng.choice(24, 7, replace=False)
        r = rng.uniform(0.05, 1.0, 7)
        w[v, j] = (r / r.sum()).astype(np.float32)
    return w


@functools.lru_cache(maxsize=None)
def model(V, weights="sparse"):
    """synthetic_smpl_model(num_verts=V) with fp32-exact skinning weights; sparse: rows 0..3 overwritten so that rows
    of exactly 1, 2 and 4 non-zeros exist and joints 0, 15, 16 and 23 (both 16-joint tiles of the dA product, their
    first and last rows) occur; dense: 7 non-zeros per row."""
    from ilps_amd.smpl_model import synthetic_smpl_model
    m = synthetic_smpl_model(1234, num_verts=V)
    if weights == "dense":
        w = dense_weights(V, 77 + V)
    else:
        w = np.asarray(m.weights, np.float32).copy()
        w[:4] = 0
        w[0, 0] = 1.0
        w[1, [15, 16]] = [0.25, 0.75]
        w[2, [23, 0]] = [0.5, 0.5]
        r = np.array([0.4, 0.3, 0.2, 0.1])
        w[3, [0, 15, 16, 23]] = (r / r.sum()).astype(np.float32)
        nz = (w != 0).sum(1)
        assert nz.max() <= 4 and (nz == 1).any() and (nz == 2).any() and (nz == 4).any()
        assert all((w[:, j] != 0).any() for j in (0, 15, 16, 23))
    m = dataclasses.replace(m, weights=w.astype(np.float64))
    m.validate()
    return m


@functools.lru_cache(maxsize=None)
def x_all():
    from _inputs import make_x
    x = make_x(NX, W_IMG, seed=4242)
    x.setflags(write=False)
    return x


def x_rows(B):
    return x_all()[:B]


# ------------------------------------------------------------------------------------------------ stage P
@functools.lru_cache(maxsize=None)
def torch_smpl(V, dtype):
    from oracle.torch_oracle import TorchSMPL
    return TorchSMPL(model(V), dtype)


def pose_stage(ts, x):
    """x (N, 86) -> (N, 577) = [coef 217 | A rows 0..2 (24 x 12) | J_transformed 72], by TorchSMPL's constants and
    formulas (batch_smpl.py:96-153 up to the skinning)."""
    from oracle import torch_oracle as to
    N, V = x.shape[0], ts.V
    thetas, betas = x[:, 4:76], x[:, 76:86]
    v_shaped = (betas @ ts.shapedirs).reshape(-1, V, 3) + ts.v_template
    J = torch.stack([v_shaped[:, :, c] @ ts.J_regressor for c in range(3)], dim=2)
    Rs = to.batch_rodrigues(thetas.reshape(-1, 3)).reshape(-1, 24, 3, 3)
    pose_feature = (Rs[:, 1:] - torch.eye(3, dtype=x.dtype)).reshape(-1, 207)
    Jt, A = to.batch_global_rigid_transformation(Rs, J, ts.parents)
    return torch.cat([betas, pose_feature, A[:, :, :3, :].reshape(N, 288), Jt.reshape(N, 72)], dim=1)


_jac = {}


def jacobian(V, B):
    """Jp (B, 577, 86) float64, one mesh at a time, cached per (V, mesh)."""
    ts, x = torch_smpl(V, torch.float64), torch.tensor(x_all(), dtype=torch.float64)
    for n in range(B):
        if (V, n) not in _jac:
            f = lambda row: pose_stage(ts, row[None])[0]
            _jac[(V, n)] = torch.autograd.functional.jacobian(f, x[n], vectorize=True, strategy="forward-mode").numpy()
    return np.stack([_jac[(V, n)] for n in range(B)])


@functools.lru_cache(maxsize=None)
def forward(V, B, dtype=torch.float64):
    """The forward values the backward is linearised at, in `dtype`: dict(coef (B, 217), A (B, 24, 12), Jt (B, 24, 3),
    vp (B, V, 3)) as numpy arrays of that precision."""
    ts = torch_smpl(V, dtype)
    with torch.no_grad():
        out = pose_stage(ts, torch.tensor(x_rows(B), dtype=dtype))
        coef = out[:, :217]
        blend = torch.cat([ts.shapedirs, ts.posedirs], dim=0)                    # (217, 3V)
        vp = (coef @ blend).reshape(B, V, 3) + ts.v_template
    return dict(coef=coef.numpy(), A=out[:, 217:505].reshape(B, 24, 12).numpy(), Jt=out[:, 505:].reshape(B, 24, 3).numpy(),
                vp=vp.numpy())


@functools.lru_cache(maxsize=None)
def blend_t(V):
    """blend^T (3V, 217) float64: rows of [shapedirs | posedirs] as SMPLConstants.from_model stacks them."""
    m = model(V)
    return np.concatenate([np.asarray(m.shapedirs, np.float64).reshape(-1, 10),
                           np.asarray(m.posedirs, np.float64).reshape(-1, 207)], axis=1)


# ------------------------------------------------------------------------------------------------ cases
Case = collections.namedtuple("Case", "V B vs cot nsplit perm live")
# live: live records per 1 024-vertex chunk (None without slot sums)


def _id(c):
    s = "V%d-B%d-vs%d-%s" % (c.V, c.B, c.vs, c.cot)
    if c.live is not None:
        s += "-ns%d-%s-live%s" % (c.nsplit, "perm" if c.perm else "order", "_".join(map(str, c.live)))
    return s


def nchunk(V):
    return (V + CHUNK - 1) // CHUNK


def sampled_in_chunk(V, vs, c):
    """how many of chunk c's vertices are sampled (a multiple of vs)"""
    lo, hi = c * CHUNK, min(V, (c + 1) * CHUNK)
    return (hi - 1) // vs - (lo - 1) // vs if lo > 0 else (hi - 1) // vs + 1


def _cases():
    """A covering list: every V meets B = 1 and 33, both samplings, a cotangent set without slot sums (the per-vertex
    kernel), slot sums alone (the record kernel) and slot sums beside dverts / dproj (the per-vertex kernel with the
    slot gather); every case is run with both GEMMs and both weight tables by the tests themselves.  nsplit rotates
    through 1, 2, 3, 7 so that each meets the record kernel and the gather; live counts 0, 1, 64, 65, 256, 257, 1 024."""
    NS = [1, 2, 3, 7]
    out = []
    for i, V in enumerate(SHAPES):
        nc = nchunk(V)
        full = [sampled_in_chunk(V, 1, c) for c in range(nc)]
        third = [sampled_in_chunk(V, 3, c) for c in range(nc)]
        some = lambda cap, avail: [min(cap, a) for a in avail]
        out += [Case(V, 1, 1, "all", 0, False, None),
                Case(V, 33, 3, "dproj" if i % 2 else "dverts", 0, False, None),
                Case(V, 33, 1, "slots", NS[i % 4], bool(i % 2), some([64, 65, 256, 1, 65, 64][i], full)),
                Case(V, 1, 3, "slots", NS[(i + 1) % 4], not i % 2, some([1, 1, 64, 256, 65, 1][i], third)),
                Case(V, 1, 1, "slots+dverts", NS[(i + 2) % 4], bool(i % 2), some(65, full)),
                Case(V, 33, 3, "slots+dproj+dJt", NS[(i + 3) % 4], not i % 2, some(64, third))]
    out += [Case(8, 1, 1, "dproj", 0, False, None), Case(64, 1, 3, "dverts", 0, False, None),
            Case(257, 513, 1, "all", 0, False, None),                      # 17 mesh tiles: the two-tile GEMM form
            Case(257, 1, 1, "slots", 7, True, [257]),                      # a second round, three waves of it idle
            Case(1024, 1, 1, "slots", 3, True, [1024]),
            Case(1025, 1, 1, "slots", 2, False, [1024, 1]),
            Case(1025, 33, 1, "slots", 1, True, [0, 1]),                   # live records only in the one-vertex chunk
            Case(2049, 1, 1, "slots", 7, True, [64, 0, 1]),                # a chunk without a live record between two with
            Case(2049, 1, 1, "slots", 3, False, [0, 0, 1]),
            Case(2049, 1, 1, "slots", 2, True, [256, 257, 0]),
            Case(64, 33, 1, "slots", 7, True, [0]),                        # all dead: dx is exactly 0
            Case(2049, 1, 3, "slots", 3, False, [0, 0, 0])]
    out = [c._replace(live=None if c.live is None else tuple(c.live)) for c in out]      # (hashable: the caches' key)
    assert len(set(out)) == len(out)
    return out


CASES = _cases()
CASE_IDS = [_id(c) for c in CASES]


# ------------------------------------------------------------------------------------------------ cotangents, slot sums
def _normal(rng, shape):
    """N(0, 1) fp32 with |value| >= 0.05 (as `layout` of test_gpu_skin_bwd_live.py draws its sums; a small value is
    moved out by 0.05, not set to it: two of them must not cancel exactly)."""
    v = rng.normal(0, 1, shape).astype(np.float32)
    return np.where(np.abs(v) < 0.05, v + np.float32(0.05) * np.where(v < 0, -1, 1).astype(np.float32), v)


def layout(V, B, vs, nsplit, perm, live, seed):
    """-> dict(vslot (B, VP) int16, part (B, nsplit, NSLOT, 2) fp32, live (B, VP) bool, kind (B, VP) int8:
    0 no slot, 1 live, 2 dead with all blocks zero, 3 dead with cancelling blocks).
    Chunk c gets exactly live[c] live records per mesh, at seeded positions; of the other sampled vertices every fifth
    has no slot (where the chunk can spare them), the rest own dead records.  Slots: 0.. in vertex order, or (perm)
    distinct random ones over all five windows, window 1 and window 4 always among them when there are two records."""
    VP = (V + vs - 1) // vs
    rng = np.random.default_rng(seed)
    chunk = (np.arange(VP) * vs) // CHUNK
    vslot = np.full((B, VP), -1, np.int16)
    kind = np.zeros((B, VP), np.int8)
    part = np.zeros((B, nsplit, NSLOT, 2), np.float32)
    assert len(live) == nchunk(V)
    for b in range(B):
        owners = np.zeros(VP, bool)
        for c, want in enumerate(live):
            idx = np.flatnonzero(chunk == c)
            assert want <= idx.size, "chunk %d has %d sampled vertices, %d live asked for" % (c, idx.size, want)
            own = idx[np.arange(idx.size) % 5 != 4]
            if own.size < want:
                own = idx
            owners[own] = True
            pick = rng.choice(own, want, replace=False) if want else np.zeros(0, np.int64)
            kind[b, own] = 2 + (np.arange(own.size) % 2 if nsplit > 1 else 0)
            kind[b, pick] = 1
        own = np.flatnonzero(owners)
        if perm:
            slots = rng.permutation(NSLOT)[:own.size]
            forced = [s for s in (16384 + 5, 4096 + 7)][:own.size]
            slots = np.array(forced + [s for s in slots if s not in forced][:own.size - len(forced)], np.int64)
            slots = slots[rng.permutation(own.size)]
        else:
            slots = np.arange(own.size)
        vslot[b, own] = slots
        for n, (i, s) in enumerate(zip(own, slots)):
            if kind[b, i] == 1:
                part[b, :, s] = _normal(rng, (nsplit, 2))
                if n % 7 == 3:
                    part[b, :, s, 0] = 0.0                              # sx == 0, sy != 0: live
            elif kind[b, i] == 3:
                v = _normal(rng, (2,))
                part[b, 0, s], part[b, nsplit - 1, s] = v, -v
    return dict(vslot=vslot, part=part, live=kind == 1, kind=kind)


def block_sum32(part, first=0, last=None):
    """(B, nsplit, NSLOT, 2) -> (B, NSLOT, 2): the fp32 sum in block order (slot_sum's, whatever its grouping: one
    running sum)."""
    acc = part[:, first].copy()
    for s in range(first + 1, part.shape[1] if last is None else last):
        acc = acc + part[:, s]
    assert acc.dtype == np.float32
    return acc


def gather(lay, table):
    """table (B, NSLOT, 2) -> (B, VP, 3): each vertex' slot entry in columns 0, 1 (0 without a slot), column 2 zero."""
    vslot = lay["vslot"].astype(np.int64)
    B, VP = vslot.shape
    out = np.zeros((B, VP, 3), table.dtype)
    got = np.take_along_axis(table, np.maximum(vslot, 0)[:, :, None], axis=1)
    out[..., :2] = np.where((vslot >= 0)[:, :, None], got, 0)
    return out


@functools.lru_cache(maxsize=None)
def inputs(case):
    """The case's cotangents (fp32, read-only): dict(dverts | None, dproj | None, dJt | None, lay | None)."""
    V, B, vs = case.V, case.B, case.vs
    VP = (V + vs - 1) // vs
    rng = np.random.default_rng(100000 * COTS.index(case.cot) + 40 * V + 4 * (B % 10) + vs)
    out = dict(dverts=None, dproj=None, dJt=None, lay=None)
    if case.cot in ("dverts", "all", "slots+dverts"):
        out["dverts"] = _normal(rng, (B, V, 3))
    if case.cot in ("dproj", "all", "slots+dproj+dJt"):
        out["dproj"] = _normal(rng, (B, VP, 3))
    if case.cot in ("all", "slots+dproj+dJt"):
        out["dJt"] = _normal(rng, (B, 24, 3))
    if case.live is not None:
        out["lay"] = layout(V, B, vs, case.nsplit, case.perm, case.live, seed=V + 7 * B + vs)
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def proj_cotangent(inp):
    """-> (dproj total (B, VP, 3) float64, its magnitude) or (None, None): the merged dproj plus the slot sums."""
    d = m = None
    if inp["dproj"] is not None:
        d = inp["dproj"].astype(np.float64)
        m = np.abs(d)
    if inp["lay"] is not None:
        p64 = inp["lay"]["part"].astype(np.float64)
        s, ms = gather(inp["lay"], p64.sum(1)), gather(inp["lay"], np.abs(p64).sum(1))
        d, m = (s, ms) if d is None else (d + s, m + ms)
    return d, m


# ------------------------------------------------------------------------------------------------ the staged reference
def staged(V, B, vs, w, dverts, dproj, mag_dproj, dJt, fold_blocks=None):
    """Stages S, G, P in float64 -> dict(dx, mag_dx (B, 86), and every stage's values and magnitudes).
    fold_blocks = (vertices per block, blocks folded): dA and the camera sums take only the vertices of the first so
    many blocks (a mutation the CPU file uses; None: all)."""
    fw = forward(V, B)
    c = dict(V=V, vs=vs, vp=fw["vp"], A=fw["A"], x=x_rows(B))
    o = oracle(c, w, dverts, dproj, mag_dproj)
    if fold_blocks is not None:
        size, n = fold_blocks
        keepv = lambda a: None if a is None else np.where((np.arange(V) < size * n)[None, :, None], a, 0)
        keepp = lambda a: None if a is None else np.where((np.arange(a.shape[1]) * vs < size * n)[None, :, None], a, 0)
        o2 = oracle(c, w, keepv(dverts), keepp(dproj), keepp(mag_dproj))
        for k in ("dA", "dcam", "mag_dA", "mag_dcam"):
            o[k] = o2[k]
    bt = blend_t(V)
    dcoef = o["dv_posed"].reshape(B, 3 * V) @ bt
    mag_dcoef = o["mag_dv_posed"].reshape(B, 3 * V) @ np.abs(bt)
    z = np.zeros((B, 72)) if dJt is None else dJt.astype(np.float64).reshape(B, 72)
    cot = np.concatenate([dcoef, o["dA"].reshape(B, 288), z], axis=1)
    mag = np.concatenate([mag_dcoef, o["mag_dA"].reshape(B, 288), np.abs(z)], axis=1)
    Jp = jacobian(V, B)
    dx = np.einsum("bko,bk->bo", Jp, cot)
    mag_dx = np.einsum("bko,bk->bo", np.abs(Jp), mag)
    assert not dx[:, :4].any() and not mag_dx[:, :4].any()
    dx[:, :4], mag_dx[:, :4] = o["dcam"], o["mag_dcam"]
    return dict(dx=dx, mag_dx=mag_dx, cot=cot, mag_cot=mag, dcam=o["dcam"], mag_dcam=o["mag_dcam"], stage=o)


def weights_of(V, kind):
    return np.asarray(model(V, kind).weights, np.float32)


@functools.lru_cache(maxsize=None)
def reference(case, weights="sparse"):
    inp = inputs(case)
    d, m = proj_cotangent(inp)
    return staged(case.V, case.B, case.vs, weights_of(case.V, weights), inp["dverts"], d, m, inp["dJt"])


# ------------------------------------------------------------------------------------------------ the float32 pose stage
def pose_vjp32(V, B, cot, dcam):
    """dx (B, 86) float64 of the pose stage in FLOAT32: autograd through pose_stage over TorchSMPL(float32)'s constants
    with the cotangent `cot` (B, 577) rounded to fp32; the camera columns are dcam's fp32 values."""
    ts = torch_smpl(V, torch.float32)
    x = torch.tensor(x_rows(B), dtype=torch.float32, requires_grad=True)
    out = pose_stage(ts, x)
    g, = torch.autograd.grad((out * torch.tensor(np.asarray(cot, np.float32))).sum(), x)
    dx = g.numpy().astype(np.float64)
    dx[:, :4] = np.asarray(dcam, np.float32)
    return dx


def k_general(V, nsplit, gemm):
    from test_gpu_blend_small import BAR3_BWD
    return 2 * (V + 8) + max(nsplit - 1, 0) + (BAR3_BWD / U if gemm == "bf16x3" else 3 * V + 1)


@functools.lru_cache(maxsize=None)
def k_pose():
    """4 x the largest |dx32 - dx64| / (2^-24 mag_dx) of the float32 pose stage over every case's rows (sparse
    weights), each fed the float64 cotangent of its own stages S and G."""
    worst = 0.0
    for case in CASES:
        ref = reference(case)
        dx32 = pose_vjp32(case.V, case.B, ref["cot"], ref["dcam"])
        err, lim = np.abs(dx32 - ref["dx"]), U * ref["mag_dx"]
        assert np.all(err[lim == 0] == 0)
        if (lim > 0).any():
            worst = max(worst, float((err[lim > 0] / lim[lim > 0]).max()))
    return 4.0 * worst


def bar_k(case, gemm):
    return k_general(case.V, case.nsplit, gemm) + k_pose()


def ratio(dx, ref, K):
    """max |dx - ref| / (K 2^-24 mag_dx); entries of magnitude 0 must be exactly equal."""
    err, lim = np.abs(np.asarray(dx, np.float64) - ref["dx"]), K * U * ref["mag_dx"]
    assert np.all(err[lim == 0] == 0), "an entry whose magnitude is 0 is not 0"
    return float((err[lim > 0] / lim[lim > 0]).max()) if (lim > 0).any() else 0.0
