"""smplr_skin_fwd and smplr_skin_bwd (the C ABI, through ctypes) at SMALL vertex counts, where the tail handling and the
lane maps of the skinning kernels decide the result, against a float64 numpy restatement written here:

    T_v = sum_j w_vj A_j (3 x 4)        verts_v = T_v [p_v; 1]        proj = (c2 + X c0, c3 + Y c1, Z) of every vs-th vertex
    g_v = dverts_v + (c0 du, c1 dv, dz) dv_posed_v = T_v[:, :3]^T g_v dA_j = sum_v w_vj g_v (x) [p_v; 1]
    dcam = (sum X du, sum Y dv, sum du, sum dv)

Shapes (B = 2): V = 5 (one partly filled wave; the range check of the weight table's buffer loads on almost every row),
64 (exactly one wave, three waves of pure tail), 257 (a second block that holds one vertex), 1 030 (five blocks per mesh
for the reduction; more than one 1 024-vertex chunk).  vs in {1, 3}; sparse weights (<= 4 non-zeros, top4 built as
ops.SMPLConstants.from_model builds it) and dense ones (7 non-zeros per row, top4 = NULL); dverts only, dproj only, both.

Bars, derived: |got - ref| <= 2 n 2^-24 mag per entry, mag = the same expression on absolute values in float64, n = the
number of terms summed into the entry: 27 for verts and dv_posed (24 of T, 3 of the product), 29 for proj's u and v (one
more product and sum), V + 8 for dA and the camera sums.  That is the forward bound of an fp32 sum in any order, doubled
because the b operand g * p of the matrix cores is rounded once before the product.
Also: the sparse and the dense kernels give equal bits on the sparse weights, and so do two launches."""
import numpy as np
import pytest

from _smpl_bwd_oracle import oracle, top4_of          # (the float64 restatement: shared with the fused backward's tests)

U = 2.0 ** -24
B = 2
XS = 6                                   # row stride of the camera rows (the kernels read columns 0..3)
SHAPES = [5, 64, 257, 1030]
GRADS = ["dverts", "dproj", "both"]


# ------------------------------------------------------------------------------------------------ inputs and oracle
def make_weights(V, nnz_max, exact, seed):
    """(V, 24) fp32 rows that sum to ~1 with `exact` ? exactly nnz_max : 1..nnz_max non-zeros at random joints."""
    rng = np.random.default_rng(seed)
    w = np.zeros((V, 24), np.float32)
    for v in range(V):
        k = nnz_max if exact else 1 + (v + int(rng.integers(0, 4))) % nnz_max
        j = rng.choice(24, k, replace=False)
        r = rng.uniform(0.05, 1.0, k)
        w[v, j] = (r / r.sum()).astype(np.float32)
    return w


def make_case(V, vs, seed=0):
    rng = np.random.default_rng(1000 * V + 10 * vs + seed)
    VP = (V + vs - 1) // vs
    f = lambda *s: rng.normal(0, 1, s).astype(np.float32)
    return dict(V=V, vs=vs, VP=VP, vp=f(B, V, 3), A=f(B, 24, 12), x=f(B, XS), dverts=f(B, V, 3), dproj=f(B, VP, 3),
                w_sparse=make_weights(V, 4, False, V), w_dense=make_weights(V, 7, True, V + 1))


def terms(name, V):
    return {"verts": 27, "dv_posed": 27, "proj": 29, "dA": V + 8, "dcam": V + 8}[name]


def check(name, got, ref, V, label):
    err, bar = np.abs(got.astype(np.float64) - ref[name]), 2 * terms(name, V) * U * ref["mag_" + name]
    worst = float((err / np.maximum(bar, 1e-300)).max())
    print("%-28s %-8s max err %.3e, max err / bar %.3f" % (label, name, float(err.max()), worst))
    assert np.all(err <= bar), "%s %s: %d entries outside 2 n u mag (n = %d), worst err / bar %.3f" % (
        label, name, int((err > bar).sum()), terms(name, V), worst)


# ---------------------------------------------------------------------------------------------- CPU checks of the oracle
def test_top4_holds_the_sparse_rows():
    w = make_weights(257, 4, False, 3)
    t4 = top4_of(w)
    assert ((w != 0).sum(1) <= 4).all() and ((w != 0).sum(1) < 4).any() and ((w != 0).sum(1) == 4).any()
    back = np.zeros_like(w)
    for k in range(4):
        np.add.at(back, (np.arange(257), t4[:, 4 + k].astype(int)), t4[:, k])
    assert np.array_equal(back, w)
    jj = np.where(t4[:, :4] != 0, t4[:, 4:], 99)
    assert (np.diff(np.sort(jj, axis=1), axis=1) >= 0).all() and np.array_equal(np.sort(jj, axis=1), jj)   # ascending
    assert ((make_weights(64, 7, True, 1) != 0).sum(1) == 7).all()


def test_oracle_forward_equals_a_vertex_loop():
    c = make_case(5, 3)
    ref = oracle(c, c["w_dense"], None, None)
    for b in range(B):
        for v in range(5):
            T = sum(float(c["w_dense"][v, j]) * c["A"][b, j].astype(np.float64).reshape(3, 4) for j in range(24))
            X = T[:, :3] @ c["vp"][b, v].astype(np.float64) + T[:, 3]
            assert np.allclose(ref["verts"][b, v], X, rtol=1e-13, atol=1e-13)
            if v % 3 == 0:
                cam = c["x"][b].astype(np.float64)
                assert np.allclose(ref["proj"][b, v // 3], [cam[2] + X[0] * cam[0], cam[3] + X[1] * cam[1], X[2]], rtol=1e-13)
    for k in ("verts", "proj"):
        assert (ref["mag_" + k] >= np.abs(ref[k])).all()


@pytest.mark.parametrize("vs", [1, 3])
def test_oracle_backward_equals_finite_differences(vs):
    """L = <dverts, verts> + <dproj, proj>: central differences in v_posed, A and the camera columns at V = 5."""
    c = make_case(5, vs)
    w, dv, dp = c["w_sparse"], c["dverts"], c["dproj"]
    ref = oracle(c, w, dv, dp)

    def loss(cc):
        o = oracle(cc, w, None, None)
        return float((o["verts"] * dv).sum() + (o["proj"] * dp).sum())

    def fd(key, idx, h=1e-3):
        vals = []
        for sgn in (+1, -1):
            cc = dict(c)
            a = c[key].astype(np.float64).copy()     # (the oracle is multilinear in each of these: central differences
            a[idx] += sgn * h                        #  are exact up to float64 rounding)
            cc[key] = a
            vals.append(loss(cc))
        return (vals[0] - vals[1]) / (2 * h)

    rng = np.random.default_rng(0)
    for _ in range(12):
        i = (int(rng.integers(B)), int(rng.integers(5)), int(rng.integers(3)))
        assert np.isclose(fd("vp", i), ref["dv_posed"][i], rtol=1e-7, atol=1e-9)
        i = (int(rng.integers(B)), int(rng.integers(24)), int(rng.integers(12)))
        assert np.isclose(fd("A", i), ref["dA"][i], rtol=1e-7, atol=1e-9)
    for b in range(B):
        # d/d c0 = sum X du, d/d c1 = sum Y dv, d/d c2 = sum du, d/d c3 = sum dv
        for k in range(4):
            assert np.isclose(fd("x", (b, k)), ref["dcam"][b, k], rtol=1e-7, atol=1e-9)
    for k in ("dv_posed", "dA", "dcam"):
        assert (ref["mag_" + k] >= np.abs(ref[k])).all()


# --------------------------------------------------------------------------------------------------------- GPU
def run_fwd(c, w, top4):
    import torch
    from ilps_amd import _lib
    from ilps_amd._lib import ptr, stream
    from test_gpu_parity import dev, t
    lib = _lib.load()
    V, vs, VP = c["V"], c["vs"], c["VP"]
    verts, proj = torch.full((B, V, 3), np.nan, device=dev()), torch.full((B, VP, 3), np.nan, device=dev())
    tw, tt = t(w), (t(top4) if top4 is not None else None)
    tp, tA, tx = t(c["vp"]), t(c["A"]), t(c["x"])          # (named: alive until the launch has run)
    _lib.check(lib.smplr_skin_fwd(ptr(tp), ptr(tw), ptr(tt), ptr(tA), ptr(tx), XS, B, V, vs, ptr(verts), ptr(proj),
                                  stream()), "smplr_skin_fwd")
    torch.cuda.synchronize()
    return {"verts": verts.cpu().numpy(), "proj": proj.cpu().numpy()}


def run_bwd(c, w, top4, dverts, dproj):
    import torch
    from ilps_amd import _lib
    from ilps_amd._lib import ptr, stream
    from test_gpu_parity import dev, t
    lib = _lib.load()
    V, vs = c["V"], c["vs"]
    d = dev()
    dv_posed, dA = torch.full((B, V, 3), np.nan, device=d), torch.full((B, 24, 12), np.nan, device=d)
    dcam = torch.full((B, 4), np.nan, device=d)
    ws = torch.empty(lib.smplr_skin_bwd_workspace(B, V) // 4, device=d)
    tw, tt = t(w), (t(top4) if top4 is not None else None)
    tdv, tdp = (t(dverts) if dverts is not None else None), (t(dproj) if dproj is not None else None)
    tp, tA, tx = t(c["vp"]), t(c["A"]), t(c["x"])          # (named: alive until the launch has run)
    _lib.check(lib.smplr_skin_bwd(ptr(tdv), ptr(tdp), ptr(tp), ptr(tw), ptr(tt), ptr(tA), ptr(tx), XS, B, V, vs,
                                  ptr(dv_posed), ptr(dA), ptr(dcam), ptr(ws), stream()), "smplr_skin_bwd")
    torch.cuda.synchronize()
    return {"dv_posed": dv_posed.cpu().numpy(), "dA": dA.cpu().numpy(), "dcam": dcam.cpu().numpy()}


def same_bits(a, b):
    return all(np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)) for k in a)


@pytest.mark.gpu
@pytest.mark.parametrize("vs", [1, 3])
@pytest.mark.parametrize("V", SHAPES)
def test_skin_fwd_small(V, vs):
    c = make_case(V, vs)
    for kind, w, top4 in (("sparse", c["w_sparse"], top4_of(c["w_sparse"])), ("dense7", c["w_dense"], None)):
        ref, got = oracle(c, w, None, None), run_fwd(c, w, top4)
        for name in ("verts", "proj"):
            check(name, got[name], ref, V, "V=%d vs=%d %s" % (V, vs, kind))
        assert same_bits(got, run_fwd(c, w, top4)), "two launches differ"
        if top4 is not None:
            assert same_bits(got, run_fwd(c, w, None)), "sparse and dense kernels differ on the sparse weights"


@pytest.mark.gpu
@pytest.mark.parametrize("grads", GRADS)
@pytest.mark.parametrize("vs", [1, 3])
@pytest.mark.parametrize("V", SHAPES)
def test_skin_bwd_small(V, vs, grads):
    c = make_case(V, vs)
    dverts = c["dverts"] if grads in ("dverts", "both") else None
    dproj = c["dproj"] if grads in ("dproj", "both") else None
    for kind, w, top4 in (("sparse", c["w_sparse"], top4_of(c["w_sparse"])), ("dense7", c["w_dense"], None)):
        ref, got = oracle(c, w, dverts, dproj), run_bwd(c, w, top4, dverts, dproj)
        for name in ("dv_posed", "dA", "dcam"):
            check(name, got[name], ref, V, "V=%d vs=%d %s %s" % (V, vs, grads, kind))
        if dproj is None:
            assert not got["dcam"].any()
        assert same_bits(got, run_bwd(c, w, top4, dverts, dproj)), "two launches differ"
        if top4 is not None:
            assert same_bits(got, run_bwd(c, w, None, dverts, dproj)), "sparse and dense kernels differ on the sparse weights"
