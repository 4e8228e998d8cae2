"""The data generator without a GPU: known answers of the NumPy oracle (tests/_augment_oracle.py, the restatement of
INTEGRATION.md section 4d), the oracle against scipy.ndimage, the matrix builder and the draws, the batch index stream,
the C ABI's and the torch op's argument checks, unsupported Keras options, and the kernels' resources."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _augment_oracle as ao  # noqa: E402
from ilps_amd import augment  # noqa: E402

I23 = np.array([[1, 0, 0], [0, 1, 0]], np.float32)


def plane(h, w, seed=0, C=None):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (h, w) if C is None else (h, w, C), dtype=np.uint8)


def neutral(B=1, **kw):
    d = {"theta": np.zeros(B), "tx": np.zeros(B), "ty": np.zeros(B), "shear": np.zeros(B), "zx": np.ones(B),
         "zy": np.ones(B), "flip": np.zeros(B)}
    for k, v in kw.items():
        d[k] = np.full(B, float(v))
    return d


def f32(m):
    return np.asarray(m, np.float64).astype(np.float32)


# ---- oracle known answers ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_identity_shift_flip(dtype):
    p = plane(48, 64, 1, 3)
    assert np.array_equal(ao.warp_nearest(p, I23, 48, 64, dtype), p)
    assert np.array_equal(ao.warp_nearest(p, f32(ao.matrix_from_draws(neutral(), 48, 64)[0]), 48, 64, dtype), p)
    # an integer shift is a slice with edge replication
    got = ao.warp_nearest(p, np.array([[1, 0, 3], [0, 1, -2]], np.float32), 48, 64, dtype)
    want = np.pad(p, ((0, 3), (2, 0), (0, 0)), mode="edge")[3:, :64]
    assert np.array_equal(got, want)
    # a flip alone is [:, ::-1]
    M = f32(ao.matrix_from_draws(neutral(flip=1), 48, 64)[0])
    assert np.array_equal(M, np.array([[1, 0, 0], [0, -1, 63]], np.float32))
    assert np.array_equal(ao.warp_nearest(p, M, 48, 64, dtype), p[:, ::-1])


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_quarter_turn(dtype):
    """A quarter turn about the plane's centre ((h - 1) / 2) is np.rot90 exactly.  Built from draws, theta = 90 turns
    about Keras' centre h / 2 + 0.5 (`transform_matrix_offset_center`), one pixel off the true centre on each axis:
    the same np.rot90, moved by two pixels along the columns with the edge replicated."""
    p = plane(48, 48, 2)
    assert np.array_equal(ao.warp_nearest(p, np.array([[0, -1, 47], [1, 0, 0]], np.float32), 48, 48, dtype), np.rot90(p, -1))
    assert np.array_equal(ao.warp_nearest(p, np.array([[0, 1, 0], [-1, 0, 47]], np.float32), 48, 48, dtype), np.rot90(p, 1))
    M = f32(ao.matrix_from_draws(neutral(theta=90), 48, 48)[0])
    np.testing.assert_allclose(M, [[0, -1, 49], [1, 0, 0]], atol=1e-5)
    rot = np.rot90(p, -1)
    want = np.pad(rot, ((0, 0), (2, 0)), mode="edge")[:, :48]
    assert np.array_equal(ao.warp_nearest(p, M, 48, 48, dtype), want)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_zoom_two_and_a_half(dtype):
    h = 48
    p = plane(h, h, 3)
    i = np.arange(h)
    M = f32(ao.matrix_from_draws(neutral(zx=2, zy=2), h, h)[0])            # sr = 2 r - 24.5 -> floor(2 r - 24)
    k = np.clip(2 * i - 24, 0, h - 1)
    assert np.array_equal(ao.warp_nearest(p, M, h, h, dtype), p[k[:, None], k[None, :]])
    M = f32(ao.matrix_from_draws(neutral(zx=0.5, zy=0.5), h, h)[0])        # sr = r / 2 + 12.25 -> floor(r / 2 + 12.75)
    k = np.clip((i + 25) // 2, 0, h - 1)
    assert np.array_equal(ao.warp_nearest(p, M, h, h, dtype), p[k[:, None], k[None, :]])


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_wild_matrices_select_the_clamped_pixels(dtype):
    h, w = 12, 16
    p = plane(h, w, 4)
    nan, inf = np.nan, np.inf
    assert (ao.warp_nearest(p, np.full((2, 3), nan, np.float32), h, w, dtype) == p[0, 0]).all()
    assert (ao.warp_nearest(p, np.array([[0, 0, inf], [0, 0, -inf]], np.float32), h, w, dtype) == p[h - 1, 0]).all()
    got = ao.warp_nearest(p, np.array([[1e30, 0, 0], [0, -1e30, 0]], np.float32), h, w, dtype)
    assert (got[0] == p[0, 0]).all() and (got[1:] == p[h - 1, 0]).all()
    # inf * 0 is NaN and counts as 0: row 0 of a matrix of infinities reads (0, 0) at r = c = 0
    got = ao.warp_nearest(p, np.full((2, 3), inf, np.float32), h, w, dtype)
    assert got[0, 0] == p[0, 0] and got[5, 5] == p[h - 1, w - 1]
    bl = ao.warp_bilinear(p, np.full((2, 3), nan, np.float32), dtype)
    assert (bl == p[0, 0]).all()


def test_pool_of_another_size_is_read_like_a_nearest_resize():
    for S, n in ((256, 64), (300, 48), (513, 64), (100, 256), (256, 48), (64, 64)):
        i = np.arange(n)
        want = np.floor((i + 0.5) * S / n + 1e-12).astype(np.int64)
        assert np.array_equal(ao.pool_index(i, n, S), want), (S, n)
        assert ao.pool_index(i, n, S).max() <= S - 1
    p = plane(300, 256, 5)
    got = ao.warp_nearest(p, I23, 48, 64)
    assert np.array_equal(got, p[ao.pool_index(np.arange(48), 48, 300)[:, None], ao.pool_index(np.arange(64), 64, 256)[None, :]])


def test_bilinear_known_answers():
    p = plane(32, 32, 6, 3)
    assert np.array_equal(ao.warp_bilinear(p, I23, np.float32), p.astype(np.float32))
    half = ao.warp_bilinear(p, np.array([[1, 0, 0.5], [0, 1, 0]], np.float32), np.float64)
    want = 0.5 * (p[:-1].astype(np.float64) + p[1:])
    assert np.array_equal(half[:-1], want) and np.array_equal(half[-1], p[-1])


@pytest.mark.parametrize("size", [48, 64, 256])
def test_float64_oracle_equals_scipy(size):
    ndi = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(size)
    p = plane(size, size, size)
    bad = total = 0
    for kw in (ao.REF_DRAWS, ao.WIDE_DRAWS):
        mats = f32(ao.matrix_from_draws(ao.draws(rng, 10, **kw), size, size))
        tie = ao.near_tie(mats, (size, size), 1e-9)
        for b, M in enumerate(mats):
            want = ndi.affine_transform(p, M[:, :2].astype(np.float64), offset=M[:, 2].astype(np.float64), order=0,
                                        mode="nearest")
            got = ao.warp_nearest(p, M, size, size, np.float64)
            bad += int(((got != want) & ~tie[b]).sum())
            total += int(tie[b].sum())
    assert bad == 0
    assert total <= 1e-4 * 20 * size * size


def test_float32_restatement_differs_from_float64_only_at_near_ties():
    rng = np.random.default_rng(7)
    size = 256
    p = plane(size, size, 8)
    mats = f32(ao.matrix_from_draws(ao.draws(rng, 16, **ao.WIDE_DRAWS), size, size))
    tie = ao.near_tie(mats, (size, size), ao.delta_for(size))
    a = ao.warp_labels(p[None].repeat(16, 0), mats, (size, size), dtype=np.float32)
    b = ao.warp_labels(p[None].repeat(16, 0), mats, (size, size), dtype=np.float64)
    assert not ((a != b) & ~tie).any()
    assert tie.mean() <= 0.005


# ---- matrix builder and draws ------------------------------------------------------------------------------------------
def test_affine_matrices_match_the_composed_products():
    """Against C R T S Z C^-1 [F] composed as 3 x 3 float64 products: at most 1 fp32 ulp per entry (half an ulp from
    the one rounding, plus the float64 rounding of sums of terms up to 2 * 513, below 1e-12)."""
    rng = np.random.default_rng(11)
    for kw in (ao.REF_DRAWS, ao.WIDE_DRAWS):
        d = ao.draws(rng, 64, **kw)
        td = {k: torch.from_numpy(v) for k, v in d.items()}
        for h, w in ((256, 256), (48, 48), (64, 48), (512, 300)):
            got = augment.affine_matrices(td, (h, w))
            assert got.dtype == torch.float32 and tuple(got.shape) == (64, 2, 3)
            want = ao.matrix_from_draws(d, h, w)
            ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
            assert (np.abs(got.numpy().astype(np.float64) - want) <= ulp + 1e-12).all()
    deg = dict(d, shear=np.rad2deg(d["shear"]))
    a = augment.affine_matrices({k: torch.from_numpy(v) for k, v in deg.items()}, 48, shear_in_degrees=True)
    want = ao.matrix_from_draws(d, 48, 48)
    assert np.abs(a.numpy() - want).max() <= 1e-5
    if kw["horizontal_flip"]:
        assert 0 < d["flip"].sum() < 64                                   # both branches of the flip folding ran


def test_zero_ranges_give_the_exact_identity():
    g = torch.Generator().manual_seed(3)
    d = augment.random_draws(9, g)
    for size in (48, (64, 48), 256, 513):
        m = augment.affine_matrices(d, size)
        assert torch.equal(m, torch.from_numpy(I23).expand(9, 2, 3))
        assert not torch.signbit(m).any()
    m = augment.affine_matrices({"theta": torch.zeros(2)}, 48)
    assert torch.equal(m, torch.from_numpy(I23).expand(2, 2, 3))


def test_draws_stay_in_range_and_follow_the_seed():
    kw = dict(rotation_range=40., width_shift_range=0.2, height_shift_range=0.1, shear_range=0.3, zoom_range=(0.7, 1.5),
              horizontal_flip=True)
    d = augment.random_draws(4096, torch.Generator().manual_seed(5), **kw)
    assert sorted(d) == sorted(augment.DRAW_KEYS)
    for k, (lo, hi) in {"theta": (-40, 40), "tx": (-0.1, 0.1), "ty": (-0.2, 0.2), "shear": (-0.3, 0.3), "zx": (0.7, 1.5),
                        "zy": (0.7, 1.5)}.items():
        v = d[k]
        assert v.dtype == torch.float64 and v.shape == (4096,)
        assert lo <= float(v.min()) and float(v.max()) <= hi
        assert float(v.max()) - float(v.min()) > 0.9 * (hi - lo) and v.unique().numel() > 4000
    assert set(d["flip"].tolist()) == {0.0, 1.0} and 0.4 < float(d["flip"].mean()) < 0.6
    assert not torch.equal(d["zx"], d["zy"])
    d2 = augment.random_draws(4096, torch.Generator().manual_seed(5), **kw)
    d3 = augment.random_draws(4096, torch.Generator().manual_seed(6), **kw)
    assert all(torch.equal(d[k], d2[k]) for k in d) and not torch.equal(d["theta"], d3["theta"])
    assert float(augment.random_draws(64, torch.Generator().manual_seed(1), rotation_range=10)["flip"].sum()) == 0
    u = torch.rand(7, 5, dtype=torch.float64)
    du = augment.random_draws(5, uniform=u, zoom_range=0.15)
    assert torch.equal(du["zx"], 0.85 + u[4] * (1.15 - 0.85))
    gen = augment.ImageDataGenerator(**{k: v for k, v in ao.REF_DRAWS.items()}, rescale=1 / 255., fill_mode="nearest")
    dg = gen.random_draws(100, torch.Generator().manual_seed(2))
    assert float(dg["theta"].abs().max()) <= 10 and float((dg["zx"] - 1).abs().max()) <= 0.15 + 1e-12


def test_unsupported_keras_options_raise_by_name():
    for kw, word in ((dict(fill_mode="constant"), "fill_mode"), (dict(fill_mode="reflect"), "fill_mode"),
                     (dict(channel_shift_range=0.1), "channel_shift_range"), (dict(zca_whitening=True), "zca_whitening"),
                     (dict(vertical_flip=True), "vertical_flip"), (dict(featurewise_center=True), "featurewise_center"),
                     (dict(preprocessing_function=abs), "preprocessing_function"), (dict(cval=1.0), "cval")):
        with pytest.raises(NotImplementedError, match=word):
            augment.ImageDataGenerator(**kw)
    g = augment.ImageDataGenerator(rotation_range=40, width_shift_range=0.2, height_shift_range=0.2, shear_range=0.2,
                                   zoom_range=0.2, horizontal_flip=True, fill_mode='nearest')
    assert g.zoom_range == (0.8, 1.2) and g.horizontal_flip and g.rescale is None


# ---- batch index stream ------------------------------------------------------------------------------------------------
def test_batch_indexer_visits_every_row_once_per_epoch():
    N, bs = 37, 8
    it = augment.BatchIndexer(N, bs, True, torch.Generator().manual_seed(1))
    stream = torch.cat([next(it) for _ in range(N)])                      # 8 * 37 indices = 8 epochs exactly
    assert stream.dtype == torch.int64 and stream.numel() == bs * N
    for e in range(bs):
        assert sorted(stream[e * N:(e + 1) * N].tolist()) == list(range(N))
    assert not torch.equal(stream[:N], stream[N:2 * N])                   # a new permutation per epoch
    assert it.epochs == bs
    # the short batch wraps round: batch 4 = the epoch's last 5 rows + the first 3 of the next epoch
    again = augment.BatchIndexer(N, bs, True, torch.Generator().manual_seed(1))
    b = [next(again) for _ in range(5)]
    assert all(x.shape == (bs,) for x in b)
    assert torch.equal(torch.cat(b), stream[:5 * bs])                     # same seed, same order
    other = augment.BatchIndexer(N, bs, True, torch.Generator().manual_seed(2))
    assert not torch.equal(torch.cat([next(other) for _ in range(5)]), stream[:5 * bs])
    plain = augment.BatchIndexer(5, 3, False)
    assert [next(plain).tolist() for _ in range(4)] == [[0, 1, 2], [3, 4, 0], [1, 2, 3], [4, 0, 1]]
    big = augment.BatchIndexer(3, 8, False)                               # a batch larger than the pool
    assert next(big).tolist() == [0, 1, 2, 0, 1, 2, 0, 1] and next(big).tolist() == [2, 0, 1, 2, 0, 1, 2, 0]
    with pytest.raises(ValueError):
        augment.BatchIndexer(0, 4)


# ---- C ABI, torch op, Python front ------------------------------------------------------------------------------------
def test_abi_entry_refuses_bad_arguments_without_a_gpu():
    from ilps_amd import _lib
    lib = _lib.load()
    one = 1

    def warp(pool=one, N=4, Hs=64, Ws=64, C=3, mat=one, B=2, H=64, W=64, mode=0, out=one):
        return lib.smplr_affine_warp(pool, N, Hs, Ws, C, mat, None, 0, B, H, W, mode, 1.0, out, None)

    for kw, word in ((dict(pool=None), b"pool"), (dict(mat=None), b"mat"), (dict(out=None), b"out"), (dict(H=0), b"output"),
                     (dict(W=4097), b"output"), (dict(Hs=0), b"pool planes"), (dict(Ws=8193), b"pool planes"),
                     (dict(N=0), b"N="), (dict(B=-1), b"B="), (dict(mode=4), b"mode"), (dict(mode=-1), b"mode"),
                     (dict(C=2), b"channels"), (dict(C=3, mode=2), b"channels"), (dict(C=3, mode=3), b"channels"),
                     (dict(mode=1, Hs=32), b"bilinear")):
        assert warp(**kw) == -1, kw
        err = lib.smplr_last_error()
        assert word in err and b"smplr_affine_warp" in err, (kw, err)
    assert warp(B=0) == 0 and warp(B=0, pool=None, mat=None, out=None) == 0      # an empty batch is a no-op


def test_affine_warp_op_has_a_meta_kernel():
    from ilps_amd import torch_ops
    ns = torch_ops.load()
    assert str(ns.affine_warp.default._schema) == torch_ops.SCHEMAS["affine_warp"]
    m = lambda *s, dt=torch.float32: torch.empty(*s, dtype=dt, device="meta")
    u8, i32, i64 = torch.uint8, torch.int32, torch.int64
    assert ns.affine_warp(m(10, 300, 256, 3, dt=u8), m(4, 2, 3), m(4, dt=i64), m(4, 3, 256, 256), 0, 1 / 255.) is None
    ns.affine_warp(m(10, 64, 64, dt=u8), m(4, 2, 3), None, m(4, 1, 64, 64), 1, 1.0)
    ns.affine_warp(m(10, 64, 64, dt=u8), m(4, 2, 3), m(4, dt=i32), m(4, 48, 48, dt=i32), 2)
    ns.affine_warp(m(10, 64, 64, 1, dt=u8), m(0, 2, 3), None, m(0, 48, 48, dt=i32), 3)
    for args in ((m(10, 64, 64, 3), m(4, 2, 3), None, m(4, 3, 64, 64), 0),                       # pool not uint8
                 (m(10, 64, 64, 3, dt=u8), m(4, 2, 3), None, m(4, 1, 64, 64), 0),                # channel mismatch
                 (m(10, 64, 64, 3, dt=u8), m(5, 2, 3), None, m(4, 3, 64, 64), 0),                # B mismatch
                 (m(10, 64, 64, 3, dt=u8), m(4, 3, 2), None, m(4, 3, 64, 64), 0),                # matrix shape
                 (m(10, 64, 64, 3, dt=u8), m(4, 2, 3), m(4), m(4, 3, 64, 64), 0),                # float index
                 (m(10, 64, 64, 3, dt=u8), m(4, 2, 3), m(3, dt=i64), m(4, 3, 64, 64), 0),        # index length
                 (m(10, 64, 64, 3, dt=u8), m(4, 2, 3), None, m(4, 3, 32, 32), 1),                # bilinear resize
                 (m(10, 64, 64, 3, dt=u8), m(4, 2, 3), None, m(4, 64, 64, dt=i32), 2),           # 3-channel labels
                 (m(10, 64, 64, dt=u8), m(4, 2, 3), None, m(4, 64, 64), 2),                      # fp32 label output
                 (m(10, 64, 64, dt=u8), m(4, 2, 3), None, m(4, 1, 64, 64, dt=i32), 0),           # int image output
                 (m(10, 64, 64, dt=u8), m(4, 2, 3), None, m(4, 1, 64, 64), 4),                   # mode
                 (m(10, 64, 64, dt=u8), m(4, 2, 3), None, m(4, 1, 64, 5000), 0)):                # too wide
        with pytest.raises(RuntimeError):
            ns.affine_warp(*args)
    with pytest.raises((RuntimeError, NotImplementedError)):       # CPU tensors: no kernel registered for them
        ns.affine_warp(torch.zeros(2, 8, 8, dtype=u8), torch.zeros(2, 2, 3), None, torch.zeros(2, 1, 8, 8), 0, 1.0)


def test_python_front_refuses_cpu_tensors_and_bad_arguments():
    pool = torch.zeros(2, 8, 8, 3, dtype=torch.uint8)
    mats = torch.from_numpy(I23).expand(2, 2, 3).contiguous()
    with pytest.raises(RuntimeError, match="HIP device"):
        augment.warp_images(pool, mats, 8)
    with pytest.raises(RuntimeError, match="HIP device"):
        augment.warp_labels(pool[..., 0], mats, 8)
    with pytest.raises(RuntimeError):
        augment.DeviceBatches(pool, pool[..., 0], 2, 8, 8, {})
    with pytest.raises(ValueError, match="interpolation"):
        augment.warp_images(pool, mats, 8, interpolation="bicubic")
    import ilps_amd
    for name in ("ImageDataGenerator", "DeviceBatches", "affine_matrices", "random_draws", "warp_images", "warp_labels"):
        assert getattr(ilps_amd, name) is getattr(augment, name)
    import inspect
    sig = inspect.signature(augment.ImageDataGenerator.__init__)
    got = [(n, p.default) for n, p in sig.parameters.items() if p.kind == p.POSITIONAL_OR_KEYWORD and n != "self"]
    assert got == [("rotation_range", 0), ("width_shift_range", 0), ("height_shift_range", 0), ("shear_range", 0),
                   ("zoom_range", 0), ("horizontal_flip", False), ("rescale", None), ("fill_mode", "nearest")]
    sig = inspect.signature(augment.DeviceBatches.__init__)
    got = [(n, p.default) for n, p in sig.parameters.items() if n != "self"]
    assert got[:10] == [("images_pool", inspect._empty), ("labels_pool", inspect._empty), ("batch_size", inspect._empty),
                        ("input_wh", inspect._empty), ("output_wh", inspect._empty), ("image_args", inspect._empty),
                        ("silh_wh", None), ("shuffle", True), ("seed", 1), ("generator", None)]


# ---- kernel resources --------------------------------------------------------------------------------------------------
def test_warp_kernels_fit_the_budget():
    """Every instantiation (C channels, kind 0 nearest image / 1 bilinear image / 2 labels, 1 or 4 columns per thread):
    no scratch, no LDS, 8 waves per SIMD; the VGPR counts are the compiler's."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr
    ks = {}
    for n, k in kr.kernels().items():
        m = re.search(r"affine_warp_kernelILi(\d)ELi(\d)ELi(\d)E", n)
        if m:
            ks[tuple(int(x) for x in m.groups())] = k
    want = {(1, 0, 1): 8, (1, 0, 4): 16, (1, 1, 1): 19, (1, 1, 4): 45, (1, 2, 1): 8, (1, 2, 4): 16,
            (3, 0, 1): 9, (3, 0, 4): 24, (3, 1, 1): 23, (3, 1, 4): 58}
    assert sorted(ks) == sorted(want)
    for key, k in ks.items():
        assert k["scratch"] == 0 and k["lds"] == 0 and k["agpr"] == 0, key
        assert k["max_threads"] == 256, key
        assert k["vgpr"] == want[key], (key, k["vgpr"])
        assert kr.waves_per_simd(k) == 8, key


# ---- the timing tool's device-free parts ---------------------------------------------------------------------------
def test_timing_tool_byte_counts_and_trace_summary(tmp_path):
    import importlib.util
    spec = importlib.util.spec_from_file_location("augment_time", os.path.join(ROOT, "tools", "augment_time.py"))
    at = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(at)
    r, w = at.hip_bytes(128)
    assert r == 128 * (256 * 256 * 3 + 48 * 48) and w == 128 * 4 * (256 * 256 * 3 + 48 * 48)
    assert abs((r + w) / 1e6 - 127.3) < 0.1                               # about 127 MB, 20 us at 6.3 TB/s
    assert abs((r + w) / (at.HBM_TBPS * 1e12) * 1e6 - 20.2) < 0.1
    # the stock formulation: gathered uint8 copy, fp32 copy, rescale, grid written and read, sampled output; labels alike
    img = 128 * 256 * 256 * (3 * 2 + 3 * 5 + 3 * 8 + 2 * 8 + 3 * 8)
    lab = 128 * (256 * 256 * (2 + 5) + 48 * 48 * (2 * 8 + 8 + 8))
    assert at.stock_bytes(128) == img + lab and 6.0 < at.stock_bytes(128) / (r + w) < 6.3
    name = "void smplr::affine_warp_kernel<%s>(unsigned char const*, int, int)"
    rows = [("other_kernel(float*)", 0, 9000, 64)]
    rows += [(name % "3, 0, 4", 1000 * k, 1000 * k + d, 2097152) for k, d in enumerate((31000, 30000, 35000))]
    rows += [(name % "1, 2, 4", 5, 2005, 98304)]
    p = tmp_path / "x_kernel_trace.csv"
    p.write_text('"Kernel_Name","Start_Timestamp","End_Timestamp","Grid_Size_X"\n'
                 + "".join('"%s",%d,%d,%d\n' % row for row in rows))
    got = at.trace_medians(str(p))
    assert got == {"<1, 2, 4> grid 98304": {"n": 1, "median_us": 2.0, "min_us": 2.0},
                   "<3, 0, 4> grid 2097152": {"n": 3, "median_us": 31.0, "min_us": 30.0}}
