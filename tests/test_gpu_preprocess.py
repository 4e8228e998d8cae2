"""Input preprocessing on the GPU (csrc/preprocess.hip through preprocess.load_images / load_labels / EvalBatches and
torch.ops.smplraster.resize_pad) against the int64 NumPy restatement of INTEGRATION.md section 4e
(tests/_preprocess_oracle.py).  Every comparison is exact (the definition has no near-ties) except quantize=False, whose
bound is three fp32 ulps of the result's binade.  Derivation: the value is fl(fl(fl(num) / D) * rescale) with D exact in
fp32, so three correctly rounded operations, each a relative error of at most 2^-24: 3 * 2^-24 of the value in all (the
second-order terms are below 2^-46).  An ulp of the binade [2^e, 2^(e+1)) is 2^(e-23), between 2^-24 and 2^-23 of the
value, so the error is below 3 ulps at the top of a binade and below 1.5 at its bottom.  Not measured; the achieved
maximum is printed."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _preprocess_oracle as po  # noqa: E402
from ilps_amd import preprocess as pp  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
# 1 x 1, odd sizes, portrait and landscape, exact 2x of 256, enlargement and reduction, one side at 8192
SIZES = [(1, 1), (37, 91), (101, 40), (480, 640), (640, 480), (512, 512), (3, 8192), (8192, 2), (255, 257), (64, 64), (200, 1000)]


def images(C, seed=0, sizes=SIZES, hi=256):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, hi, (h, w) if C == 1 else (h, w, C), dtype=np.uint8) for h, w in sizes]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def index_for(B, N, seed):
    if B == 7:
        return np.array([3, 0, 3, N - 1, 1, 6, 2])                        # repeats
    rng = np.random.default_rng(seed)
    return np.concatenate([np.arange(N), rng.integers(0, N, B - N)]) if B >= N else np.array([5])[:B]


class Cache:
    """oracle results per (image number, arguments)"""

    def __init__(self, arrs, fn):
        self.arrs, self.fn, self.memo = arrs, fn, {}

    def batch(self, idx, *a, **kw):
        key = (a, tuple(sorted(kw.items())))
        out = []
        for i in idx:
            if (int(i), key) not in self.memo:
                self.memo[(int(i), key)] = self.fn(self.arrs[int(i)], *a, **kw)
            out.append(self.memo[(int(i), key)])
        return np.stack(out)


@pytest.mark.parametrize("C", [1, 3])
def test_quantised_bilinear_images_bit_for_bit(C):
    arrs = images(C, C)
    r = pp.RaggedImages.from_arrays(arrs, DEV)
    oracle = Cache(arrs, po.load_image)
    N = len(arrs)
    for out_hw in ((256, 256), (48, 64)):
        for pad in (False, True):
            for swap in ((False, True) if C == 3 else (False,)):
                for B in (1, 7, 128):
                    idx = index_for(B, N, B)
                    got = pp.load_images(r, out_hw, torch.from_numpy(idx).to(DEV), pad=pad, swap_rb=swap)
                    assert got.shape == (B, C) + out_hw and got.dtype == torch.float32 and got.is_contiguous()
                    want = oracle.batch(idx, out_hw, pad=pad, swap_rb=swap)
                    assert np.array_equal(bits(got.cpu().numpy()), bits(want)), (out_hw, pad, swap, B)
    # every image in order when no index is given, and another rescale
    got = pp.load_images(r, 256, pad=True, rescale=0.5)
    assert np.array_equal(bits(got.cpu().numpy()), bits(oracle.batch(range(N), (256, 256), pad=True, rescale=0.5)))
    got = pp.load_images(r, 32, rescale=None)
    assert np.array_equal(bits(got.cpu().numpy()), bits(oracle.batch(range(N), (32, 32), rescale=None)))


def test_unquantised_bilinear_within_three_ulps():
    worst = 0.0
    for C in (1, 3):
        arrs = images(C, 10 + C)
        r = pp.RaggedImages.from_arrays(arrs, DEV)
        for out_hw, pad in (((256, 256), True), ((48, 64), False), ((255, 130), True)):
            got = pp.load_images(r, out_hw, pad=pad, quantize=False).cpu().numpy().astype(np.float64)
            want = np.stack([po.load_image(a, out_hw, pad=pad, quantize=False) for a in arrs])
            ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
            err = np.abs(got - want) / ulp
            assert (got[want == 0] == 0).all()
            worst = max(worst, float(err.max()))
            print("quantize=False C=%d %s pad=%s: max error %.3f ulp" % (C, out_hw, pad, err.max()))
            assert err.max() <= 3.0, (C, out_hw, pad, err.max())
    print("quantize=False: achieved maximum %.3f ulp (bound 3)" % worst)


def test_labels_and_nearest_images_both_rules():
    masks = images(1, 20, hi=32)
    rm = pp.RaggedImages.from_arrays(masks, DEV)
    for rule in ("cv2", "pil"):
        for pad in (False, True):
            for out_hw in ((48, 48), (64, 50), (256, 256)):
                for binarize in (False, True):
                    got = pp.load_labels(rm, out_hw, pad=pad, nearest_rule=rule, binarize=binarize)
                    assert got.dtype == torch.int32 and got.shape == (len(masks),) + out_hw
                    want = np.stack([po.load_label(m, out_hw, pad=pad, nearest_rule=rule, binarize=binarize) for m in masks])
                    assert np.array_equal(got.cpu().numpy(), want), (rule, pad, out_hw, binarize)
                # the autoencoder's input: the same texels as a 1-channel image, times 1 / (num_classes - 1)
                got = pp.load_images(rm, out_hw, pad=pad, interpolation="nearest", nearest_rule=rule, rescale=1 / 31.)
                want = np.stack([po.load_image(m, out_hw, pad=pad, interpolation="nearest", nearest_rule=rule, rescale=1 / 31.)
                                 for m in masks])
                assert np.array_equal(bits(got.cpu().numpy()), bits(want)), (rule, pad, out_hw)
    arrs = images(3, 21)
    r = pp.RaggedImages.from_arrays(arrs, DEV)
    for rule in ("cv2", "pil"):
        got = pp.load_images(r, (64, 48), pad=True, interpolation="nearest", nearest_rule=rule, swap_rb=True)
        want = np.stack([po.load_image(a, (64, 48), pad=True, interpolation="nearest", nearest_rule=rule, swap_rb=True) for a in arrs])
        assert np.array_equal(bits(got.cpu().numpy()), bits(want)), rule


def test_index_forms_repeats_and_clamping():
    arrs = images(3, 30)
    r = pp.RaggedImages.from_arrays(arrs, DEV)
    N = len(arrs)
    oracle = Cache(arrs, po.load_image)
    base = pp.load_images(r, 64, pad=True)
    assert np.array_equal(bits(base.cpu().numpy()), bits(oracle.batch(range(N), (64, 64), pad=True)))
    idx = np.array([4, 4, 0, N - 1, 4, 2, 2, 9])
    for dt in (torch.int32, torch.int64):
        got = pp.load_images(r, 64, torch.from_numpy(idx).to(DEV).to(dt), pad=True)
        assert np.array_equal(bits(got.cpu().numpy()), bits(oracle.batch(idx, (64, 64), pad=True))), dt
        wild = torch.tensor([-1, -2 ** 31 if dt == torch.int32 else -2 ** 62, N, N + 7, 2 ** 31 - 1 if dt == torch.int32 else 2 ** 62, 3],
                            dtype=dt, device=DEV)
        got = pp.load_images(r, 64, wild, pad=True)
        assert np.array_equal(bits(got.cpu().numpy()), bits(oracle.batch([0, 0, N - 1, N - 1, N - 1, 3], (64, 64), pad=True))), dt
    masks = images(1, 31, hi=32)
    rm = pp.RaggedImages.from_arrays(masks, DEV)
    got = pp.load_labels(rm, 48, torch.tensor([N + 1, 1, 1, -3], device=DEV))
    want = np.stack([po.load_label(masks[i], (48, 48)) for i in (N - 1, 1, 1, 0)])
    assert np.array_equal(got.cpu().numpy(), want)
    assert pp.load_images(r, 64, torch.empty(0, dtype=torch.int64, device=DEV)).shape == (0, 3, 64, 64)
    with pytest.raises(TypeError):
        pp.load_images(r, 64, torch.zeros(2, device=DEV))
    with pytest.raises(ValueError):
        pp.load_images(r, 64, out=torch.empty(N, 3, 64, 65, device=DEV))


def cut_of(arrs, rects):
    return [a[t:t + h, l:l + w] for a, (t, l, h, w) in zip(arrs, rects)]


def test_crops_are_descriptors_with_a_larger_pitch():
    sizes = [(480, 640), (101, 40), (64, 64), (720, 1280)]
    for C in (1, 3):
        arrs = images(C, 40 + C, sizes)
        r = pp.RaggedImages.from_arrays(arrs, DEV)
        rects = [(10, 33, 400, 501), (50, 7, 51, 30), (0, 0, 64, 64), (1, 320, 718, 640)]
        c = r.crop(rects)
        cut = cut_of(arrs, rects)
        got = pp.load_images(c, 256, pad=True)
        want = np.stack([po.load_image(a, (256, 256), pad=True) for a in cut])
        assert np.array_equal(bits(got.cpu().numpy()), bits(want)), C
        if C == 1:
            got = pp.load_labels(c, 48, pad=True)
            assert np.array_equal(got.cpu().numpy(), np.stack([po.load_label(a, (48, 48), pad=True) for a in cut]))
        w = r.center_crop_width()
        cut = [a[:, int(0.25 * a.shape[1]):int(0.75 * a.shape[1])] for a in arrs]
        got = pp.load_images(w, 256, pad=True)
        want = np.stack([po.load_image(a, (256, 256), pad=True) for a in cut])
        assert np.array_equal(bits(got.cpu().numpy()), bits(want)), C
    # from_dense: a pool of equal-sized frames, no copy
    frames = np.random.default_rng(5).integers(0, 256, (3, 72, 128, 3), dtype=np.uint8)
    d = pp.RaggedImages.from_dense(torch.from_numpy(frames).to(DEV))
    got = pp.load_images(d.center_crop_width(), 32, pad=True, swap_rb=True)
    want = np.stack([po.load_image(f[:, 32:96], (32, 32), pad=True, swap_rb=True) for f in frames])
    assert np.array_equal(bits(got.cpu().numpy()), bits(want))


def test_scalar_store_path_equals_the_vector_path():
    arrs = images(3, 50)
    r = pp.RaggedImages.from_arrays(arrs, DEV)
    N = len(arrs)
    # an output that is off 16-byte alignment
    big = torch.zeros(N * 3 * 64 * 64 + 1, device=DEV)
    out = big[1:].view(N, 3, 64, 64)
    assert out.data_ptr() % 16 == 4
    assert pp.load_images(r, 64, pad=True, out=out) is out
    assert torch.equal(out, pp.load_images(r, 64, pad=True))
    assert float(big[0]) == 0
    out.zero_()
    pp.load_images(r, 64, pad=True, quantize=False, out=out)
    assert torch.equal(out, pp.load_images(r, 64, pad=True, quantize=False))
    # a width that is no multiple of 4
    for W in (50, 1, 63):
        got = pp.load_images(r, (40, W), pad=True)
        want = np.stack([po.load_image(a, (40, W), pad=True) for a in arrs])
        assert np.array_equal(bits(got.cpu().numpy()), bits(want)), W
    masks = images(1, 51, hi=32)
    rm = pp.RaggedImages.from_arrays(masks, DEV)
    bigl = torch.zeros(N * 48 * 48 + 3, dtype=torch.int32, device=DEV)
    outl = bigl[3:].view(N, 48, 48)
    pp.load_labels(rm, 48, out=outl)
    assert torch.equal(outl, pp.load_labels(rm, 48)) and int(bigl[:3].abs().sum()) == 0
    got = pp.load_labels(rm, (48, 47), pad=True)
    assert np.array_equal(got.cpu().numpy(), np.stack([po.load_label(m, (48, 47), pad=True) for m in masks]))


def test_bad_descriptors_give_zeros_and_read_nothing():
    """`data` is a slice in the middle of an allocation filled with 255; the bad rows point outside the slice (or are
    malformed) but stay inside the allocation, so a broken guard shows up as non-zero pixels, never as an out-of-bounds access."""
    sizes = [(40, 60), (64, 64), (30, 20)]
    for C in (1, 3):
        arrs = images(C, 60 + C, sizes, hi=255)
        arrs = [np.maximum(a, 1) for a in arrs]                         # no zero texel: a valid sample is never all zero
        payload, desc = po.pack(arrs)
        n = 40000
        assert payload.size <= n
        alloc = torch.full((2 * n + 128,), 255, dtype=torch.uint8, device=DEV)
        data = alloc[64:64 + n]
        data[:payload.size] = torch.from_numpy(payload).to(DEV)
        good = pp.RaggedImages(data, desc, C)
        bad_rows = [(n + 16, 4 * C, 4, 4),                # starts past the slice
                    (n - 8, 4 * C, 4, 4),                 # straddles its end
                    (n - 1, 4 * C, 1, 4),                 # the last byte, then past it
                    (0, 4 * C - 1, 4, 4),                 # pitch below w C
                    (0, 8193 * C, 1, 8193),               # a side out of range
                    (-4, 4 * C, 4, 4),                    # negative offset
                    (0, n, 2, 4),                         # the second row lies past the slice
                    (16, 4 * C, 0, 4)]                    # no rows
        table = np.concatenate([desc, np.asarray(bad_rows, np.int64)])
        order = [3, 0, 4, 5, 1, 6, 7, 8, 2, 9, 10, 0]
        r = pp.RaggedImages(data, desc, C)
        r.desc = torch.from_numpy(table).to(DEV)            # past the host validation, on purpose
        r.desc_host = table
        idx = torch.tensor(order, device=DEV)
        for kw in (dict(), dict(quantize=False), dict(interpolation="nearest")):
            got = pp.load_images(r, 32, idx, pad=True, **kw).cpu().numpy()
            ref = pp.load_images(good, 32, pad=True, **kw).cpu().numpy()
            for k, row in enumerate(order):
                if row < 3:
                    assert np.array_equal(got[k], ref[row]) and got[k].any(), (C, kw, k)
                else:
                    assert not got[k].any(), (C, kw, k, row)
        if C == 1:
            got = pp.load_labels(r, 32, idx).cpu().numpy()
            ref = pp.load_labels(good, 32).cpu().numpy()
            for k, row in enumerate(order):
                assert np.array_equal(got[k], ref[row]) if row < 3 else not got[k].any(), (k, row)
        assert int(alloc[:64].min()) == 255 and int(alloc[64 + n:].min()) == 255


def test_a_sample_does_not_depend_on_its_neighbours():
    arrs = images(3, 70)
    r = pp.RaggedImages.from_arrays(arrs, DEV)
    N = len(arrs)
    idx = index_for(128, N, 7)
    full = pp.load_images(r, 256, torch.from_numpy(idx).to(DEV), pad=True)
    for k in (0, 5, 64, 127):
        alone = pp.load_images(r, 256, torch.tensor([int(idx[k])], device=DEV), pad=True)
        assert torch.equal(alone[0], full[k]), k
    rev = pp.load_images(r, 256, torch.from_numpy(idx[::-1].copy()).to(DEV), pad=True)
    assert torch.equal(rev.flip(0), full)


def test_torch_op_equals_the_python_front():
    from ilps_amd import torch_ops
    ns = torch_ops.load()
    arrs, masks = images(3, 80), images(1, 81, hi=32)
    r, rm = pp.RaggedImages.from_arrays(arrs, DEV), pp.RaggedImages.from_arrays(masks, DEV)
    N = len(arrs)
    idx = torch.tensor([2, 2, N - 1, 0, 5], device=DEV)
    for index in (None, idx, idx.to(torch.int32)):
        B = N if index is None else 5
        for pad in (False, True):
            for kw, mode, flags in ((dict(), 0, 4), (dict(quantize=False), 0, 0), (dict(swap_rb=True), 0, 6),
                                    (dict(interpolation="nearest"), 1, 4), (dict(interpolation="nearest", nearest_rule="pil"), 1, 12)):
                out = torch.empty(B, 3, 64, 64, device=DEV)
                assert ns.resize_pad(r.data, r.desc, index, out, 3, mode, flags | int(pad), 1 / 255.) is None
                assert torch.equal(out, pp.load_images(r, 64, index, pad=pad, **kw)), (kw, pad)
            for binarize in (False, True):
                for rule in ("cv2", "pil"):
                    out = torch.empty(B, 48, 48, dtype=torch.int32, device=DEV)
                    ns.resize_pad(rm.data, rm.desc, index, out, 1, 3 if binarize else 2, int(pad) | (8 if rule == "pil" else 0), 1.0)
                    assert torch.equal(out, pp.load_labels(rm, 48, index, pad=pad, nearest_rule=rule, binarize=binarize))
    ns.resize_pad(r.data, r.desc, None, torch.empty(0, 3, 8, 8, device=DEV), 3, 0, 4, 1.0)
    for args in ((r.data.cpu(), r.desc, None, torch.empty(N, 3, 8, 8, device=DEV), 3),
                 (r.data, r.desc.cpu(), None, torch.empty(N, 3, 8, 8, device=DEV), 3),
                 (r.data, r.desc, idx.cpu(), torch.empty(5, 3, 8, 8, device=DEV), 3),
                 (r.data, r.desc, None, torch.empty(N, 3, 8, 8, device=DEV).transpose(2, 3), 3),
                 (r.data, r.desc.to(torch.int32), None, torch.empty(N, 3, 8, 8, device=DEV), 3)):
        with pytest.raises(RuntimeError):
            ns.resize_pad(*args)


def test_load_images_replays_from_a_hip_graph():
    frames = np.random.default_rng(90).integers(0, 256, (1, 72, 128, 3), dtype=np.uint8)
    t = torch.from_numpy(frames).to(DEV)
    crop = pp.RaggedImages.from_dense(t).center_crop_width()
    out = torch.zeros(1, 3, 64, 64, device=DEV)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        pp.load_images(crop, 64, pad=True, swap_rb=True, out=out)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        pp.load_images(crop, 64, pad=True, swap_rb=True, out=out)
    for seed in (91, 92):
        new = np.random.default_rng(seed).integers(0, 256, (1, 72, 128, 3), dtype=np.uint8)
        t.copy_(torch.from_numpy(new).to(DEV))
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        want = po.load_image(new[0][:, 32:96], (64, 64), pad=True, swap_rb=True)[None]
        assert np.array_equal(bits(out.cpu().numpy()), bits(want)), seed


def test_end_to_end_evaluation_and_prediction(smpl_model):
    from ilps_amd.decoder import SMPLDecoder
    from ilps_amd.evaluation import evaluate_iou_and_acc
    from ilps_amd.focal_loss import softmax_focal_loss
    from ilps_amd.inference import GraphedPredictor, predict_batch
    from ilps_amd.model import SMPLRegressor
    W = 48
    sizes = [(300, 200), (101, 40), (256, 256), (480, 640), (97, 131)]
    arrs, masks = images(3, 100, sizes), images(1, 101, sizes, hi=32)
    imgs, gts = pp.RaggedImages.from_arrays(arrs, DEV), pp.RaggedImages.from_arrays(masks, DEV)
    torch.manual_seed(1)
    net = SMPLRegressor(W, "enet", True).to(DEV)
    dec = SMPLDecoder(smpl_model, img_wh=W, outputs=(), loss=softmax_focal_loss(2.0, True))
    batches = pp.EvalBatches(imgs, gts, 2, 256, W, pad=True, swap_rb=True)
    assert len(batches) == 3
    shapes = [(tuple(i.shape), tuple(g.shape), g.dtype) for i, g in batches]
    assert shapes == [((2, 3, 256, 256), (2, W, W), torch.int32)] * 2 + [((1, 3, 256, 256), (1, W, W), torch.int32)]
    got = evaluate_iou_and_acc(net, dec, batches)
    want_batches = []
    for s in range(0, 5, 2):
        im = np.stack([po.load_image(a, (256, 256), pad=True, swap_rb=True) for a in arrs[s:s + 2]])
        gt = np.stack([po.load_label(m, (W, W), pad=True) for m in masks[s:s + 2]])
        want_batches.append((torch.from_numpy(im).to(DEV), torch.from_numpy(gt).to(DEV)))
    want = evaluate_iou_and_acc(net, dec, want_batches)
    assert torch.equal(got["counts"], want["counts"]) and got["total"] == 5 * W * W
    # the autoencoder's pair from one mask set
    (ai, ag), = list(pp.EvalBatches.autoencoder(gts, 8, 64, W, num_classes=32))
    assert np.array_equal(bits(ai.cpu().numpy()),
                          bits(np.stack([po.load_image(m, (64, 64), interpolation="nearest", rescale=1 / 31.) for m in masks])))
    assert np.array_equal(ag.cpu().numpy(), np.stack([po.load_label(m, (W, W)) for m in masks]))
    # predict_batch over images alone
    plain = SMPLDecoder(smpl_model, img_wh=W).share_constants(dec)
    n = 0
    for images_ in pp.EvalBatches(imgs, None, 2, 256, None, pad=True, swap_rb=True):
        out = predict_batch(net, plain, images_)
        assert out["seg_maps"].shape == (images_.shape[0], W, W) and torch.isfinite(out["segs"]).all()
        n += images_.shape[0]
    assert n == 5
    # the per-frame path: the frame is written straight into the captured graph's input
    first = pp.load_images(imgs, 256, torch.tensor([3], device=DEV), pad=True, swap_rb=True)
    predictor = GraphedPredictor(net, plain, torch.zeros_like(first))
    assert predictor.input.shape == first.shape
    want = {k: v.clone() for k, v in predictor(first).items()}
    predictor.input.zero_()
    assert pp.load_images(imgs, 256, torch.tensor([3], device=DEV), pad=True, swap_rb=True, out=predictor.input) is predictor.input
    assert torch.equal(predictor.input, first)                          # the graph's input is bit for bit the same frame ...
    got = predictor.replay()
    # ... so what is left is the forward's own run-to-run variation: the tolerance of test_gpu_train.py's graph test
    assert torch.allclose(got["smpl"], want["smpl"], rtol=1e-4, atol=1e-5)
    assert torch.allclose(got["verts"], want["verts"], rtol=1e-4, atol=1e-5)
    assert got["seg_maps"].shape == want["seg_maps"].shape == (1, W, W)
