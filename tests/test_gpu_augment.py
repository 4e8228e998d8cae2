"""The HIP data generator (csrc/augment.hip through ilps_amd.augment) against its NumPy restatement
(tests/_augment_oracle.py): label maps and nearest-mode images bit for bit against the float32 form, against the float64
definition everywhere but at near-ties, bilinear images within the bound the coordinate error gives, row independence,
graph replay, the torch op against the Python front, and `DeviceBatches` feeding `training.fit`."""
import numpy as np
import pytest
import torch

import _augment_oracle as ao
from ilps_amd import augment

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
EXEMPT_CAP = 0.005          # at most this share of a test's pixels may sit on a near-tie


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def pools(seed, N, Hs, hs, C=3):
    rng = np.random.default_rng(seed)
    shape = (N, Hs, Hs) if C is None else (N, Hs, Hs, C)
    img = rng.integers(0, 256, shape, dtype=np.uint8)
    lab = rng.integers(0, 32, (N, hs, hs), dtype=np.uint8)
    lab[rng.uniform(size=lab.shape) < 0.5] = 0                            # background, for binarize
    return img, lab


def mats_for(seed, B, kw, size):
    d = ao.draws(np.random.default_rng(seed), B, **kw)
    return d, ao.matrix_from_draws(d, size, size).astype(np.float32)


def index_for(seed, B, N):
    """Rows that repeat and permute (B > N repeats by necessity; otherwise two entries are forced equal)."""
    idx = np.random.default_rng(seed).integers(0, N, B)
    if B > 1:
        idx[-1] = idx[0]
    return idx


def check_float64(got, want64, tie, tag):
    diff = got != want64
    share = float(tie.mean())
    print("%s: %d of %d pixels differ from float64, %.4f %% of the pixels are near-ties"
          % (tag, int(diff.sum()), diff.size, 100 * share))
    assert share <= EXEMPT_CAP, tag
    assert not (diff & ~tie).any(), tag


@pytest.mark.parametrize("B", [1, 7, 128])
@pytest.mark.parametrize("kw", [ao.REF_DRAWS, ao.WIDE_DRAWS], ids=["ref10", "wide40"])
def test_images_nearest_bit_for_bit(B, kw):
    N, S = 9, 256
    img, _ = pools(B, N, S, 8)
    idx = index_for(B + 1, B, N)
    _, M = mats_for(B + 2, B, kw, S)
    want = ao.warp_images(img, M, (S, S), idx)
    for index in (dev(idx), dev(idx.astype(np.int32))):
        got = augment.warp_images(dev(img), dev(M), S, index).cpu().numpy()
        assert got.shape == (B, 3, S, S) and got.dtype == np.float32
        assert np.array_equal(bits(got), bits(want))
    want64 = ao.warp_images(img, M, (S, S), idx, dtype=np.float64)
    tie = np.broadcast_to(ao.near_tie(M, (S, S), ao.delta_for(S))[:, None], got.shape)
    check_float64(got, want64, tie, "images B=%d" % B)


@pytest.mark.parametrize("B", [1, 7, 128])
@pytest.mark.parametrize("kw", [ao.REF_DRAWS, ao.WIDE_DRAWS], ids=["ref10", "wide40"])
@pytest.mark.parametrize("Hs,h", [(256, 48), (300, 48), (64, 64), (256, 64)])
def test_labels_bit_for_bit(B, kw, Hs, h):
    N = 11
    _, lab = pools(Hs + h + B, N, 8, Hs)
    idx = index_for(B + 3, B, N)
    _, M = mats_for(B + 4, B, kw, h)
    pool = dev(lab)
    tie = ao.near_tie(M, (h, h), ao.delta_for(h))
    for binarize in (False, True):
        got = augment.warp_labels(pool if not binarize else pool[..., None], dev(M), h, dev(idx), binarize=binarize)
        assert got.dtype == torch.int32 and tuple(got.shape) == (B, h, h) and got.is_contiguous()
        got = got.cpu().numpy()
        assert np.array_equal(got, ao.warp_labels(lab, M, (h, h), idx, binarize))
        check_float64(got, ao.warp_labels(lab, M, (h, h), idx, binarize, dtype=np.float64), tie,
                      "labels %d->%d B=%d binarize=%d" % (Hs, h, B, binarize))
    if binarize:
        assert set(np.unique(got)) <= {0, 1}


@pytest.mark.parametrize("C", [None, 1])
def test_one_channel_pool_and_resized_image_pool(C):
    """train_autoencoder.py's grayscale input: a (N, Hs, Ws) or (N, Hs, Ws, 1) pool gives (B, 1, H, W); the image pool
    may be stored at another size as well (300 -> 256, 100 -> 256, 513 -> 64)."""
    B = 7
    for Hs, H in ((256, 256), (300, 256), (100, 256), (513, 64)):
        img, _ = pools(Hs + H, 5, Hs, 8, C)
        _, M = mats_for(Hs, B, ao.WIDE_DRAWS, H)
        idx = index_for(Hs, B, 5)
        got = augment.warp_images(dev(img), dev(M), H, dev(idx), rescale=1 / 255.).cpu().numpy()
        assert got.shape == (B, 1, H, H)
        assert np.array_equal(bits(got), bits(ao.warp_images(img, M, (H, H), idx)))


def test_odd_widths_and_rectangles():
    """Widths that are no multiple of 4 take the one-column-per-thread kernels; rescale None multiplies by one."""
    img, lab = pools(77, 3, 37, 21, 3)
    for H, W in ((50, 50), (50, 30), (33, 63)):
        d = ao.draws(np.random.default_rng(H + W), 3, **ao.REF_DRAWS)
        M = ao.matrix_from_draws(d, H, W).astype(np.float32)
        got = augment.warp_images(dev(img), dev(M), (H, W), rescale=None).cpu().numpy()
        assert got.shape == (3, 3, H, W)
        assert np.array_equal(bits(got), bits(ao.warp_images(img, M, (H, W), None, 1.0)))
        got = augment.warp_images(dev(img[..., 0]), dev(M), (H, W)).cpu().numpy()
        assert np.array_equal(bits(got), bits(ao.warp_images(img[..., 0], M, (H, W))))
        got = augment.warp_labels(dev(lab), dev(M), (H, W)).cpu().numpy()
        assert np.array_equal(got, ao.warp_labels(lab, M, (H, W)))


@pytest.mark.parametrize("S", [256, 512])
def test_bilinear_against_float64(S):
    """The interpolant is continuous: a coordinate error of delta moves it by at most 2 delta x the largest step
    between neighbours (255 rescale), plus 4 ulp of the value for the interpolation's own fp32 arithmetic.  Uniform
    noise is the worst case (full-range steps)."""
    B, rescale = 7, 1 / 255.
    img, _ = pools(S, 4, S, 8)
    _, M = mats_for(S + 1, B, ao.WIDE_DRAWS, S)
    idx = index_for(S + 2, B, 4)
    got = augment.warp_images(dev(img), dev(M), S, dev(idx), rescale, "bilinear").cpu().numpy()
    want = ao.warp_images(img, M, (S, S), idx, rescale, "bilinear", dtype=np.float64)
    atol = 2 * ao.delta_for(S) * 255 * rescale
    err = np.abs(got.astype(np.float64) - want)
    worst = float(err.max())
    print("bilinear %d: max |gpu - float64| = %.3e (bound %.1e + 4 ulp)" % (S, worst, atol))
    assert (err <= atol + 4 * np.spacing(np.abs(want).astype(np.float32))).all()
    # the float32 restatement of the same arithmetic, for the record (not asserted bit for bit: not required)
    r32 = ao.warp_images(img, M, (S, S), idx, rescale, "bilinear")
    print("bilinear %d: %d of %d values differ in bits from the float32 restatement"
          % (S, int((bits(got) != bits(r32)).sum()), got.size))
    with pytest.raises(ValueError):
        augment.warp_images(dev(img), dev(M), S // 2, dev(idx), rescale, "bilinear")


def test_identity_returns_the_pool():
    img, lab = pools(5, 6, 64, 48)
    eye = np.tile(np.array([[1, 0, 0], [0, 1, 0]], np.float32), (6, 1, 1))
    for mode in ("nearest", "bilinear"):
        got = augment.warp_images(dev(img), dev(eye), 64, interpolation=mode)
        want = dev(img).permute(0, 3, 1, 2).float() * (1 / 255.)
        assert torch.equal(got, want) and got.is_contiguous()
    assert torch.equal(augment.warp_labels(dev(lab), dev(eye), 48), dev(lab).to(torch.int32))
    assert torch.equal(augment.warp_labels(dev(lab), dev(eye), 48, binarize=True), (dev(lab) > 0).to(torch.int32))
    # the zero-range generator is the identity as well
    m = augment.affine_matrices(augment.random_draws(6, torch.Generator(device=DEV).manual_seed(1)), 64)
    assert m.device.type == "cuda" and torch.equal(m.cpu(), torch.from_numpy(eye))
    # an empty batch is a no-op
    assert tuple(augment.warp_labels(dev(lab), torch.empty(0, 2, 3, device=DEV), 48).shape) == (0, 48, 48)


def test_indices_outside_the_pool_are_clamped():
    img, lab = pools(6, 4, 32, 32)
    eye = np.tile(np.array([[1, 0, 0], [0, 1, 0]], np.float32), (5, 1, 1))
    idx = np.array([-7, 0, 3, 4, 2 ** 40], np.int64)
    got = augment.warp_labels(dev(lab), dev(eye), 32, dev(idx)).cpu().numpy()
    assert np.array_equal(got, lab[[0, 0, 3, 3, 3]].astype(np.int32))
    got = augment.warp_labels(dev(lab), dev(eye), 32, dev(np.array([-1, 9, 1, 2, 2 ** 31 - 1], np.int32))).cpu().numpy()
    assert np.array_equal(got, lab[[0, 3, 1, 2, 3]].astype(np.int32))
    got = augment.warp_labels(dev(lab), dev(eye), 32).cpu().numpy()          # no index, B > N: the last row repeats
    assert np.array_equal(got, lab[[0, 1, 2, 3, 3]].astype(np.int32))


def test_rows_are_independent_and_wild_matrices_stay_inside():
    """Sample i of a B = 128 call equals the same sample run alone; rows whose matrices are NaN / inf / 1e30 give the
    clamped pixels the definition names (every read is in bounds by construction) and leave their neighbours alone."""
    B, N, S, h = 128, 9, 256, 48
    img, lab = pools(8, N, S, 64)
    idx = index_for(9, B, N)
    _, M = mats_for(10, B, ao.WIDE_DRAWS, S)
    _, Ml = mats_for(10, B, ao.WIDE_DRAWS, h)
    full = augment.warp_images(dev(img), dev(M), S, dev(idx))
    full_l = augment.warp_labels(dev(lab), dev(Ml), h, dev(idx))
    for i in (0, 1, 63, 127):
        one = augment.warp_images(dev(img), dev(M[i:i + 1]), S, dev(idx[i:i + 1]))
        assert torch.equal(one[0], full[i])
        assert torch.equal(augment.warp_labels(dev(lab), dev(Ml[i:i + 1]), h, dev(idx[i:i + 1]))[0], full_l[i])
    wild = {5: np.full((2, 3), np.nan), 6: np.array([[0, 0, np.inf], [0, 0, -np.inf]]),
            70: np.array([[1e30, 0, 0], [0, -1e30, 0]]), 127: np.full((2, 3), np.inf)}
    Mw, Mlw = M.copy(), Ml.copy()
    for i, m in wild.items():
        Mw[i] = Mlw[i] = m.astype(np.float32)
    for interpolation in ("nearest", "bilinear"):
        base = augment.warp_images(dev(img), dev(M), S, dev(idx), interpolation=interpolation)
        got = augment.warp_images(dev(img), dev(Mw), S, dev(idx), interpolation=interpolation)
        keep = [i for i in range(B) if i not in wild]
        assert torch.equal(got[keep], base[keep])
        assert bool(torch.isfinite(got).all())
        want = ao.warp_images(img, Mw, (S, S), idx, interpolation=interpolation)
        for i in wild:
            assert np.array_equal(bits(got[i].cpu().numpy()), bits(want[i])), (interpolation, i)
    px = lambda n, r, c: img[n, r, c].astype(np.float32) * np.float32(1 / 255.)
    g = augment.warp_images(dev(img), dev(Mw), S, dev(idx)).cpu().numpy()
    assert (g[5] == px(idx[5], 0, 0)[:, None, None]).all()
    assert (g[6] == px(idx[6], S - 1, 0)[:, None, None]).all()
    assert (g[70][:, 0] == px(idx[70], 0, 0)[:, None]).all() and (g[70][:, 1:] == px(idx[70], S - 1, 0)[:, None, None]).all()
    gl = augment.warp_labels(dev(lab), dev(Mlw), h, dev(idx)).cpu().numpy()
    assert np.array_equal(gl, ao.warp_labels(lab, Mlw, (h, h), idx))
    assert (gl[5] == lab[idx[5], 0, 0]).all()


def test_graph_replay_equals_eager():
    """uniform numbers -> draws -> matrices -> image and label warps captured once on one stream; every replay, fed
    the generator's next numbers, equals the eager result for the same numbers bit for bit."""
    B, N, S, h = 16, 8, 256, 48
    img, lab = pools(11, N, S, 64)
    pi, pl = dev(img), dev(lab)
    gen = augment.ImageDataGenerator(**ao.REF_DRAWS, rescale=1 / 255.)
    g = torch.Generator(device=DEV).manual_seed(4)
    u = torch.rand(7, B, dtype=torch.float64, device=DEV, generator=g)
    idx = torch.randint(0, N, (B,), device=DEV, generator=g)
    out_i = torch.empty(B, 3, S, S, device=DEV)
    out_l = torch.empty(B, h, h, dtype=torch.int32, device=DEV)

    def run(oi, ol):
        d = gen.random_draws(B, uniform=u)
        augment.warp_images(pi, augment.affine_matrices(d, S), S, idx, gen.rescale, out=oi)
        augment.warp_labels(pl, augment.affine_matrices(d, h), h, idx, out=ol)

    run(out_i, out_l)                                                        # warm-up: libraries loaded, kernels resident
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run(out_i, out_l)
    seen = []
    for _ in range(3):
        u.copy_(torch.rand(7, B, dtype=torch.float64, device=DEV, generator=g))     # the generator advances
        idx.copy_(torch.randint(0, N, (B,), device=DEV, generator=g))
        graph.replay()
        ei, el = torch.empty_like(out_i), torch.empty_like(out_l)
        run(ei, el)
        assert torch.equal(ei, out_i) and torch.equal(el, out_l)
        Mh = augment.affine_matrices(gen.random_draws(B, uniform=u), h).cpu().numpy()
        assert np.array_equal(out_l.cpu().numpy(), ao.warp_labels(lab, Mh, (h, h), idx.cpu().numpy()))
        seen.append(out_l.clone())
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2])
    with pytest.raises(ValueError):
        augment.warp_labels(pl, augment.affine_matrices(gen.random_draws(B, uniform=u), h), h, idx, out=out_i)


def test_torch_op_equals_the_python_front():
    """torch.ops.smplraster.affine_warp runs the same launch as warp_images / warp_labels: every mode, a 3- and a
    1-channel pool, a resized label pool, int32 / int64 / no index, an empty batch, and refused operands."""
    from ilps_amd import torch_ops
    ns = torch_ops.load()
    B, N, S, h = 7, 5, 64, 48
    img, lab = pools(31, N, S, 300)
    _, M = mats_for(32, B, ao.WIDE_DRAWS, S)
    _, Ml = mats_for(32, B, ao.WIDE_DRAWS, h)
    idx = index_for(33, B, N)
    pi, p1, pl, Md, Mld = dev(img), dev(img[..., 0]), dev(lab), dev(M), dev(Ml)
    for index in (dev(idx), dev(idx.astype(np.int32)), None):
        for pool in (pi, p1, p1[..., None]):
            C = 3 if pool is pi else 1
            for mode, name in ((0, "nearest"), (1, "bilinear")):
                out = torch.full((B, C, S, S), -1.0, device=DEV)
                assert ns.affine_warp(pool, Md, index, out, mode, 1 / 255.) is None
                assert torch.equal(out, augment.warp_images(pool, Md, S, index, 1 / 255., name)), (C, name)
        for mode in (2, 3):
            out = torch.full((B, h, h), -1, dtype=torch.int32, device=DEV)
            ns.affine_warp(pl, Mld, index, out, mode, 1.0)
            assert torch.equal(out, augment.warp_labels(pl, Mld, h, index, binarize=mode == 3)), mode
    want = ao.warp_labels(lab, Ml, (h, h), idx)                               # and the front itself is the oracle's
    out = torch.empty(B, h, h, dtype=torch.int32, device=DEV)
    ns.affine_warp(pl, Mld, dev(idx), out, 2, 1.0)
    assert np.array_equal(out.cpu().numpy(), want)
    out = torch.empty(B, 3, S, S, device=DEV)                                  # rescale reaches the kernel
    ns.affine_warp(pi, Md, None, out, 0, 0.5)
    assert torch.equal(out, augment.warp_images(pi, Md, S, None, 0.5))
    ns.affine_warp(pl, torch.empty(0, 2, 3, device=DEV), None, torch.empty(0, h, h, dtype=torch.int32, device=DEV), 2, 1.0)
    big = torch.empty(B, 3, S, 2 * S, device=DEV)
    for args in ((pi, Md, None, big[..., ::2], 0, 1.0),                        # out not contiguous
                 (pi.float(), Md, None, out, 0, 1.0),                          # pool not uint8
                 (pi, Md.double(), None, out, 0, 1.0),                         # matrices not fp32
                 (pi, Md, dev(idx).float(), out, 0, 1.0),                      # index not an integer tensor
                 (pi, Md, None, out.cpu(), 0, 1.0),                            # out on the host
                 (pi, Md.cpu(), None, out, 0, 1.0)):                           # matrices on the host
        with pytest.raises((RuntimeError, NotImplementedError)):
            ns.affine_warp(*args)


def test_an_out_tensor_off_16_bytes_takes_the_narrow_kernel():
    """W % 4 = 0 but `out` starts 4 bytes past a 16-byte boundary: the launcher must fall back to one column per
    thread (a 16-byte store there would be misaligned); the result is the same, and the words around it stay."""
    B, N, S, h = 3, 4, 64, 48
    img, lab = pools(41, N, S, h)
    _, M = mats_for(42, B, ao.WIDE_DRAWS, S)
    _, Ml = mats_for(42, B, ao.WIDE_DRAWS, h)
    for shape, dtype, fn in (((B, 3, S, S), torch.float32, lambda o: augment.warp_images(dev(img), dev(M), S, out=o)),
                             ((B, h, h), torch.int32, lambda o: augment.warp_labels(dev(lab), dev(Ml), h, out=o))):
        n = int(np.prod(shape))
        big = torch.full((n + 8,), 77, dtype=dtype, device=DEV)
        out = big[1:1 + n].view(shape)
        assert out.data_ptr() % 16 == 4 and out.is_contiguous()
        got = fn(out)
        assert got.data_ptr() == out.data_ptr()
        assert torch.equal(out, fn(None))
        assert bool((big[:1] == 77).all()) and bool((big[1 + n:] == 77).all())


def synthetic_pools(smpl_model, N, seed):
    """Images random uint8; label maps rendered by the package's own decoder from seeded parameters."""
    from ilps_amd.decoder import SMPLDecoder
    from ilps_amd.smpl_model import mean86
    g = torch.Generator().manual_seed(seed)
    x = torch.tensor(np.tile(mean86(48), (N, 1)), dtype=torch.float32)
    x[:, 4:76] += 0.1 * torch.randn(N, 72, generator=g)
    with torch.no_grad():
        lab = SMPLDecoder(smpl_model, img_wh=48)(x.to(DEV))["seg"].argmax(-1).to(torch.uint8)       # (N, 48, 48), 0..31
    img = torch.randint(0, 256, (N, 256, 256, 3), generator=g, dtype=torch.uint8).to(DEV)
    return img, lab


@pytest.mark.parametrize("silh_wh", [None, 64])
def test_device_batches_feed_fit(smpl_model, silh_wh):
    from ilps_amd.training import SegTrainer, fit
    N, B = 10, 4
    img, lab = synthetic_pools(smpl_model, N, 21)
    assert int(lab.max()) > 0
    gen = augment.ImageDataGenerator(rotation_range=10, width_shift_range=0.05, height_shift_range=0.05, shear_range=0.15,
                                     zoom_range=0.15, fill_mode='nearest', rescale=1 / 255.)
    batches = augment.DeviceBatches(img, lab[..., None], B, 256, 48, gen, silh_wh=silh_wh, seed=3)
    first = next(batches)
    assert len(first) == (2 if silh_wh is None else 3)
    images, labels = first[:2]
    assert images.dtype == torch.float32 and tuple(images.shape) == (B, 3, 256, 256) and images.is_contiguous()
    assert labels.dtype == torch.int32 and tuple(labels.shape) == (B, 48, 48) and labels.is_contiguous()
    assert images.device == DEV and 0 <= float(images.min()) and float(images.max()) <= 1
    assert int(labels.max()) <= 31 and int(labels.min()) >= 0
    if silh_wh is not None:
        silh = first[2]
        assert silh.dtype == torch.int32 and tuple(silh.shape) == (B, 64, 64) and silh.is_contiguous()
        assert set(silh.unique().tolist()) <= {0, 1} and int(silh.sum()) > 0
    # the same seed gives the same batches
    again = augment.DeviceBatches(img, lab, B, 256, 48, gen, silh_wh=silh_wh, seed=3)
    assert all(torch.equal(a, b) for a, b in zip(next(again), first))
    torch.manual_seed(0)
    tr = SegTrainer(smpl_model, output_wh=48, encoder_architecture="enet", use_IEF=True, device=DEV,
                    with_silhouette=silh_wh is not None, silh_wh=silh_wh)
    tr.smpl_model.train()
    hist = fit(tr, batches, trials=1, steps_per_trial=3)
    assert len(hist) == 1 and np.isfinite(hist).all()


def test_zero_ranges_step_equals_the_batch_fed_by_hand(smpl_model):
    from ilps_amd.training import SegTrainer
    N, B = 6, 4
    img, lab = synthetic_pools(smpl_model, N, 22)
    batches = augment.DeviceBatches(img, lab, B, 256, 48, augment.ImageDataGenerator(rescale=1 / 255.), shuffle=False)
    images, labels = next(batches)
    by_hand = (img[:B].permute(0, 3, 1, 2).float() * (1 / 255.)).contiguous()
    assert torch.equal(images, by_hand) and torch.equal(labels, lab[:B].to(torch.int32))
    losses = []
    for im, lb in ((images, labels), (by_hand, lab[:B].to(torch.int32))):
        torch.manual_seed(0)
        tr = SegTrainer(smpl_model, output_wh=48, encoder_architecture="enet", use_IEF=True, device=DEV)
        tr.smpl_model.train()
        losses.append(tr.step(im, lb))
    assert bool(torch.isfinite(losses[0])) and torch.equal(losses[0], losses[1])
    nxt = next(batches)[1]                                                    # rows 4, 5, 0, 1: the short batch wraps round
    assert torch.equal(nxt, lab[[4, 5, 0, 1]].to(torch.int32))
