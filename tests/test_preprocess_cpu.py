"""Input preprocessing without a GPU: the int64 oracle (tests/_preprocess_oracle.py, the restatement of INTEGRATION.md
section 4e) against float64 `F.interpolate` and known answers, the nearest rules against Pillow, `RaggedImages`,
`EvalBatches`, `evaluate_pose_param_mse`, the C ABI's and the torch op's argument checks, the kernels' resources and the
timing tool's byte counts."""
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _preprocess_oracle as po  # noqa: E402
from ilps_amd import preprocess as pp  # noqa: E402

F = torch.nn.functional


def image(h, w, seed=0, C=3):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (h, w) if C is None else (h, w, C), dtype=np.uint8)


# ---- the oracle is the definition: against float64 F.interpolate and known answers ------------------------------------
SHAPES = [(480, 640, 256, 256, True), (101, 40, 256, 256, True), (1, 1, 5, 5, False), (300, 200, 48, 64, False),
          (37, 91, 256, 256, True), (512, 512, 256, 256, False), (64, 64, 257, 130, False), (8, 1000, 31, 17, True)]


@pytest.mark.parametrize("h,w,H,W,pad", SHAPES)
def test_oracle_equals_float64_interpolate(h, w, H, W, pad):
    img = image(h, w, h + w)
    plane = po.padded_plane(img, pad)                                     # (with pad: built by hand below as well)
    if pad:
        Hp, Wp, top, left = po.pad_geometry(h, w)
        byhand = np.zeros((Hp, Wp, 3), np.int64)
        byhand[top:top + h, left:left + w] = img
        assert np.array_equal(plane, byhand)
    num, D = po.bilinear_num(plane, H, W)
    assert num.max() < 2 ** 34 and num.min() >= 0
    want = F.interpolate(torch.from_numpy(plane.astype(np.float64)).permute(2, 0, 1)[None], size=(H, W), mode="bilinear",
                         align_corners=False)[0].permute(1, 2, 0).numpy()
    err = np.abs(num.astype(np.float64) / D - want).max()
    assert err <= 1e-9, err
    got = po.load_image(img, (H, W), pad=pad, quantize=False)
    assert np.abs(got - want.transpose(2, 0, 1) * np.float64(np.float32(1 / 255.))).max() <= 1e-9


def test_pad_geometry():
    for h, w, want in ((101, 40, (101, 100, 0, 30)), (40, 101, (100, 101, 30, 0)), (480, 640, (640, 640, 80, 0)),
                       (640, 480, (640, 640, 0, 80)), (7, 7, (7, 7, 0, 0)), (1, 2, (1, 2, 0, 0)), (3, 1, (3, 3, 0, 1))):
        assert pp.pad_geometry(h, w) == want == po.pad_geometry(h, w)
        assert pp.pad_geometry(h, w, pad=False) == (h, w, 0, 0)
    assert po.padded_plane(image(101, 40), True).shape == (101, 100, 3)
    with pytest.raises(ValueError):
        pp.pad_geometry(0, 4)


def test_known_answers():
    img = image(32, 48, 1)
    # same size: the identity
    assert np.array_equal(po.quantized_levels(img, (32, 48)), img)
    # 2x reduction: the 2 x 2 mean, ties rounded up
    a = img.astype(np.int64)
    s = a[0::2, 0::2] + a[0::2, 1::2] + a[1::2, 0::2] + a[1::2, 1::2]
    assert np.array_equal(po.quantized_levels(img, (16, 24)), (s + 2) // 4)
    assert ((s % 4) == 2).any()                                            # ties occur, and go up
    tie = np.array([[1, 2], [0, 0]], np.uint8)[..., None]                  # mean 0.75 -> 1; [[1, 1], [0, 0]]: 0.5 -> 1
    assert po.quantized_levels(tie, (1, 1))[0, 0, 0] == 1
    assert po.quantized_levels(np.array([[1, 1], [0, 0]], np.uint8), (1, 1))[0, 0, 0] == 1
    assert po.quantized_levels(np.array([[1, 0], [0, 0]], np.uint8), (1, 1))[0, 0, 0] == 0
    # 2x enlargement: weights 1/4, 3/4 inside, the edge replicated
    row = np.array([[0, 100, 200, 40]], np.uint8)
    num, D = po.bilinear_num(po.padded_plane(row, False), 1, 8)
    assert np.array_equal(num[0, :, 0], np.array([0, 25, 75, 125, 175, 160, 80, 40]) * D)
    # a white image with pad: 4 x 2 -> padded 4 x 4 (one zero column either side) -> 4 x 8: the border columns blend
    white = np.full((4, 2), 255, np.uint8)
    num, D = po.bilinear_num(po.padded_plane(white, True), 4, 8)
    assert np.array_equal(num[:, :, 0] * 4, np.tile(np.array([0, 255, 765, 1020, 1020, 765, 255, 0]) * D, (4, 1)))
    assert np.array_equal(po.quantized_levels(white, (4, 8), pad=True)[0, :, 0], [0, 64, 191, 255, 255, 191, 64, 0])
    # a 1 x 1 source fills the output
    one = np.array([[[7, 8, 9]]], np.uint8)
    assert (po.quantized_levels(one, (5, 5)) == np.array([7, 8, 9])).all()
    got = po.load_image(one, (5, 5), swap_rb=True, rescale=1 / 255.)
    assert got.shape == (3, 5, 5) and got.dtype == np.float32
    assert np.array_equal(got[:, 0, 0], np.float32([9, 8, 7]) * np.float32(1 / 255.))
    # labels
    m = image(30, 20, 2, None) % 32
    assert np.array_equal(po.load_label(m, (30, 20)), m)
    assert np.array_equal(po.load_label(m, (30, 20), binarize=True), (m > 0).astype(np.int32))
    assert np.array_equal(po.load_label(m, (15, 10)), m[::2, ::2])


def test_nearest_rules():
    from PIL import Image
    for S, n in ((256, 64), (300, 48), (513, 64), (100, 256), (480, 256)):
        i = np.arange(n)
        assert np.array_equal(po.nearest_index(n, S, "cv2"), (i * S) // n)
        assert po.nearest_index(n, S, "cv2").max() <= S - 1 and po.nearest_index(n, S, "pil").max() <= S - 1
    for S, n in ((256, 64), (300, 48), (513, 64), (100, 256)):             # (256 -> 48 is excluded: INTEGRATION 4d)
        src = (np.arange(S) % 251).astype(np.uint8)
        plane = np.ascontiguousarray(np.broadcast_to(src[None, :], (S, S)))
        want = np.asarray(Image.fromarray(plane).resize((n, n), Image.NEAREST))
        assert np.array_equal(plane[po.nearest_index(n, S, "pil")][:, po.nearest_index(n, S, "pil")], want), (S, n)
        m = image(S, S, S, None)
        want = np.asarray(Image.fromarray(m).resize((n, n), Image.NEAREST))
        assert np.array_equal(po.load_label(m, (n, n), nearest_rule="pil"), want)
    assert not np.array_equal(po.nearest_index(48, 300, "cv2"), po.nearest_index(48, 300, "pil"))


# ---- RaggedImages ------------------------------------------------------------------------------------------------------
def test_ragged_images_pack_and_crop():
    arrs = [image(5, 7, 1), image(3, 2, 2), image(1, 1, 3), image(9, 4, 4)]
    r = pp.RaggedImages.from_arrays(arrs, "cpu")
    data, desc = po.pack(arrs)
    assert len(r) == 4 and r.channels == 3 and r.sizes == [(5, 7), (3, 2), (1, 1), (9, 4)]
    assert np.array_equal(r.desc_host, desc) and np.array_equal(r.desc.numpy(), desc)
    assert r.desc.dtype == torch.int64 and r.data.dtype == torch.uint8
    assert np.array_equal(r.data.numpy(), data)
    assert r.data.numel() == sum(a.size for a in arrs)
    # descriptors and pixels share one upload
    assert r.desc.untyped_storage().data_ptr() == r.data.untyped_storage().data_ptr()
    # grayscale, from tensors
    g = pp.RaggedImages.from_arrays([torch.from_numpy(image(4, 6, 5, None)), image(2, 2, 6, None)], "cpu")
    assert g.channels == 1 and g.desc_host.tolist() == [[0, 6, 4, 6], [24, 2, 2, 2]]
    # crops: new descriptors over the same buffer
    c = r.crop([(1, 2, 3, 4), (0, 0, 3, 2), (0, 0, 1, 1), (8, 3, 1, 1)])
    assert c.data is r.data
    assert c.desc_host.tolist() == [[0 + 1 * 21 + 2 * 3, 21, 3, 4], [105, 6, 3, 2], [123, 3, 1, 1], [126 + 8 * 12 + 9, 12, 1, 1]]
    o, p, h, w = c.desc_host[0]
    view = np.stack([data[o + y * p:o + y * p + w * 3].reshape(w, 3) for y in range(h)])
    assert np.array_equal(view, arrs[0][1:4, 2:6])
    cc = c.crop([(1, 1, 2, 2), (0, 0, 1, 1), (0, 0, 1, 1), (0, 0, 1, 1)])
    assert cc.desc_host[0].tolist() == [27 + 21 + 3, 21, 2, 2]
    # one rectangle for all, and the webcam crop
    d = pp.RaggedImages.from_dense(torch.zeros(2, 720, 1280, 3, dtype=torch.uint8))
    assert d.sizes == [(720, 1280)] * 2 and d.desc_host[1].tolist() == [720 * 1280 * 3, 3840, 720, 1280]
    assert d.data.data_ptr() == d.data.untyped_storage().data_ptr()
    w = d.center_crop_width()
    assert w.sizes == [(720, 640)] * 2 and w.desc_host[1].tolist() == [720 * 1280 * 3 + 320 * 3, 3840, 720, 640]
    assert d.crop((10, 20, 30, 40)).desc_host[0].tolist() == [10 * 3840 + 60, 3840, 30, 40]
    d1 = pp.RaggedImages.from_dense(torch.zeros(3, 8, 9, dtype=torch.uint8))
    assert d1.channels == 1 and d1.desc_host[2].tolist() == [144, 9, 8, 9]


def test_ragged_images_host_validation():
    data = torch.zeros(100, dtype=torch.uint8)
    ok = [[0, 10, 10, 10]]
    pp.RaggedImages(data, ok, 1)
    for desc, C, word in (([[-1, 10, 2, 2]], 1, "offset"), ([[0, 10, 0, 2]], 1, "sides"), ([[0, 10, 2, 8193]], 1, "sides"),
                          ([[0, 5, 2, 2]], 3, "pitch"), ([[0, 10, 11, 10]], 1, "ends"), ([[91, 10, 1, 10]], 1, "ends"),
                          ([[0, 12, 9, 4]], 3, "ends"), (ok + [[0, 10, 10, 11]], 1, "descriptor 1")):
        with pytest.raises(ValueError, match=word):
            pp.RaggedImages(data, desc, C)
    pp.RaggedImages(data, [[90, 10, 1, 10]], 1)                            # the last byte is in reach
    pp.RaggedImages(data, [[88, 10 ** 9, 1, 4]], 3)                        # one row: the pitch is never stepped
    with pytest.raises(ValueError):
        pp.RaggedImages(data, ok, 2)
    with pytest.raises(ValueError):
        pp.RaggedImages(data.float(), ok, 1)
    with pytest.raises(ValueError, match="channels"):
        pp.RaggedImages.from_arrays([image(2, 2), image(2, 2, 0, None)], "cpu")
    with pytest.raises(ValueError):
        pp.RaggedImages.from_arrays([image(2, 2).astype(np.float32)], "cpu")
    with pytest.raises(ValueError):
        pp.RaggedImages.from_arrays([], "cpu")
    r = pp.RaggedImages.from_arrays([image(4, 4)], "cpu")
    for rect in ((0, 0, 5, 4), (-1, 0, 2, 2), (0, 3, 1, 2), (0, 0, 0, 1)):
        with pytest.raises(ValueError, match="crop"):
            r.crop([rect])
    with pytest.raises(ValueError):
        r.crop([(0, 0, 1, 1)] * 2)
    with pytest.raises(ValueError):
        pp.RaggedImages.from_dense(torch.zeros(2, 4, 4, 3, dtype=torch.uint8)[:, :, ::2])


def test_python_front_refuses_cpu_tensors_and_bad_arguments():
    r = pp.RaggedImages.from_arrays([image(4, 4)], "cpu")
    g = pp.RaggedImages.from_arrays([image(4, 4, 0, None)], "cpu")
    with pytest.raises(RuntimeError, match="HIP device"):
        pp.load_images(r, 8)
    with pytest.raises(RuntimeError, match="HIP device"):
        pp.load_labels(g, 8)
    with pytest.raises(ValueError, match="interpolation"):
        pp.load_images(r, 8, interpolation="cubic")
    with pytest.raises(ValueError, match="nearest_rule"):
        pp.load_labels(g, 8, nearest_rule="keras")
    with pytest.raises(ValueError, match="out_hw"):
        pp.load_images(r, 4097)
    with pytest.raises(TypeError):
        pp.load_images(torch.zeros(1, 4, 4, 3, dtype=torch.uint8), 8)
    import ilps_amd
    for name in ("RaggedImages", "EvalBatches", "load_images", "load_labels", "pad_geometry"):
        assert getattr(ilps_amd, name) is getattr(pp, name)
    import inspect
    got = [(n, p.default) for n, p in inspect.signature(pp.load_images).parameters.items()]
    assert got == [("ragged", inspect._empty), ("out_hw", inspect._empty), ("index", None), ("pad", False),
                   ("interpolation", "linear"), ("swap_rb", False), ("rescale", 1 / 255.), ("quantize", True),
                   ("nearest_rule", "cv2"), ("out", None)]
    got = [(n, p.default) for n, p in inspect.signature(pp.load_labels).parameters.items()]
    assert got == [("ragged", inspect._empty), ("out_hw", inspect._empty), ("index", None), ("pad", False),
                   ("nearest_rule", "cv2"), ("binarize", False), ("out", None)]
    got = [n for n in inspect.signature(pp.EvalBatches.__init__).parameters][1:7]
    assert got == ["images", "masks", "batch_size", "input_wh", "output_wh", "pad"]
    from ilps_amd.inference import GraphedPredictor
    assert isinstance(GraphedPredictor.input, property)


# ---- EvalBatches: order and the short last batch (the two loaders stubbed: they need the device) ---------------------
def test_eval_batches_order_and_short_last_batch(monkeypatch):
    imgs = pp.RaggedImages.from_arrays([image(3 + k, 4, k) for k in range(7)], "cpu")
    masks = pp.RaggedImages.from_arrays([image(3 + k, 4, k, None) for k in range(7)], "cpu")
    calls = []

    def fake_images(ragged, out_hw, index, **kw):
        calls.append(("img", ragged, out_hw, index.tolist(), kw))
        return ("images", index.tolist())

    def fake_labels(ragged, out_hw, index, **kw):
        calls.append(("lab", ragged, out_hw, index.tolist(), kw))
        return ("labels", index.tolist())

    monkeypatch.setattr(pp, "load_images", fake_images)
    monkeypatch.setattr(pp, "load_labels", fake_labels)
    eb = pp.EvalBatches(imgs, masks, 3, 256, 48, pad=True, swap_rb=True)
    assert len(eb) == 3
    got = list(eb)
    assert got == [(("images", [0, 1, 2]), ("labels", [0, 1, 2])), (("images", [3, 4, 5]), ("labels", [3, 4, 5])),
                   (("images", [6]), ("labels", [6]))]
    assert calls[0][1] is imgs and calls[0][2] == (256, 256) and calls[1][1] is masks and calls[1][2] == (48, 48)
    assert calls[0][4] == dict(pad=True, interpolation="linear", swap_rb=True, rescale=1 / 255., quantize=True, nearest_rule="cv2")
    assert calls[1][4] == dict(pad=True, nearest_rule="cv2", binarize=False)
    assert list(eb) == got                                                # a second pass starts over
    only = list(pp.EvalBatches(imgs, None, 4, 256, None))
    assert only == [("images", [0, 1, 2, 3]), ("images", [4, 5, 6])]
    calls.clear()
    ae = pp.EvalBatches.autoencoder(masks, 7, 64, 48, num_classes=32)
    assert len(ae) == 1 and list(ae) == [(("images", list(range(7))), ("labels", list(range(7))))]
    assert calls[0][1] is masks and calls[0][4]["interpolation"] == "nearest" and calls[0][4]["rescale"] == 1 / 31.
    with pytest.raises(ValueError):
        pp.EvalBatches(imgs, pp.RaggedImages.from_arrays([image(2, 2, 0, None)], "cpu"), 3, 256, 48)
    with pytest.raises(ValueError):
        pp.EvalBatches(imgs, masks, 0, 256, 48)


def test_evaluate_pose_param_mse_with_a_stub_model():
    from ilps_amd.evaluation import evaluate_pose_param_mse

    class Stub(torch.nn.Module):
        def forward(self, images):
            return images[:, :86] * 1.0

    rng = np.random.default_rng(0)
    smpl = [rng.normal(size=(n, 90)).astype(np.float32) for n in (3, 2)]
    gt = [rng.normal(size=(n, 72)).astype(np.float32) for n in (3, 2)]
    want = np.mean(np.concatenate([np.square(g[:, 3:].astype(np.float64) - s[:, 7:76]) for s, g in zip(smpl, gt)]).reshape(-1))
    m = Stub().train()
    got = evaluate_pose_param_mse(m, [(torch.from_numpy(s), torch.from_numpy(g)) for s, g in zip(smpl, gt)])
    assert abs(got - want) <= 1e-12 * max(1.0, want) and m.training
    with pytest.raises(ValueError):
        evaluate_pose_param_mse(m, [])
    with pytest.raises(ValueError):
        evaluate_pose_param_mse(m, [(torch.from_numpy(smpl[0]), torch.zeros(3, 69))])


# ---- C ABI, torch op -------------------------------------------------------------------------------------------------
def test_abi_entry_refuses_bad_arguments_without_a_gpu():
    from ilps_amd import _lib
    lib = _lib.load()
    one = 1

    def call(data=one, nbytes=1000, desc=one, N=4, C=3, B=2, H=64, W=64, mode=0, flags=4, out=one):
        return lib.smplr_resize_pad(data, nbytes, desc, N, C, None, 0, B, H, W, mode, flags, 1.0, out, None)

    for kw, word in ((dict(data=None), b"data"), (dict(desc=None), b"desc"), (dict(out=None), b"out"), (dict(H=0), b"output"),
                     (dict(W=4097), b"output"), (dict(N=0), b"N="), (dict(B=-1), b"B="), (dict(mode=4), b"mode"),
                     (dict(mode=-1), b"mode"), (dict(flags=16), b"flags"), (dict(flags=-1), b"flags"),
                     (dict(nbytes=0), b"data_bytes"), (dict(nbytes=(1 << 48) + 1), b"data_bytes"),
                     (dict(C=2), b"channels"), (dict(C=3, mode=2), b"channels"), (dict(C=3, mode=3), b"channels")):
        assert call(**kw) == -1, kw
        err = lib.smplr_last_error()
        assert word in err and b"smplr_resize_pad" in err, (kw, err)
    assert call(B=0) == 0 and call(B=0, data=None, desc=None, out=None) == 0      # an empty batch is a no-op
    assert lib.smplr_abi_version() == 7


def test_resize_pad_op_has_a_meta_kernel():
    from ilps_amd import torch_ops
    ns = torch_ops.load()
    assert str(ns.resize_pad.default._schema) == torch_ops.SCHEMAS["resize_pad"]
    m = lambda *s, dt=torch.float32: torch.empty(*s, dtype=dt, device="meta")
    u8, i32, i64 = torch.uint8, torch.int32, torch.int64
    assert ns.resize_pad(m(5000, dt=u8), m(10, 4, dt=i64), m(4, dt=i64), m(4, 3, 256, 256), 3, 0, 7, 1 / 255.) is None
    ns.resize_pad(m(5000, dt=u8), m(10, 4, dt=i64), None, m(4, 1, 64, 64), 1, 1, 8, 1.0)
    ns.resize_pad(m(5000, dt=u8), m(10, 4, dt=i64), m(4, dt=i32), m(4, 48, 48, dt=i32), 1, 2)
    ns.resize_pad(m(5000, dt=u8), m(10, 4, dt=i64), None, m(0, 48, 48, dt=i32), 1, 3, 1)
    D = lambda: m(10, 4, dt=i64)
    for args in ((m(5000), D(), None, m(4, 3, 64, 64), 3, 0),                                    # data not uint8
                 (m(0, dt=u8), D(), None, m(4, 3, 64, 64), 3, 0),                                # empty data
                 (m(5000, dt=u8), m(10, 4, dt=i32), None, m(4, 3, 64, 64), 3, 0),                # desc not int64
                 (m(5000, dt=u8), m(10, 3, dt=i64), None, m(4, 3, 64, 64), 3, 0),                # desc shape
                 (m(5000, dt=u8), m(0, 4, dt=i64), None, m(4, 3, 64, 64), 3, 0),                 # no descriptors
                 (m(5000, dt=u8), D(), None, m(4, 1, 64, 64), 3, 0),                             # channel mismatch
                 (m(5000, dt=u8), D(), None, m(4, 2, 64, 64), 2, 0),                             # two channels
                 (m(5000, dt=u8), D(), m(4), m(4, 3, 64, 64), 3, 0),                             # float index
                 (m(5000, dt=u8), D(), m(3, dt=i64), m(4, 3, 64, 64), 3, 0),                     # index length
                 (m(5000, dt=u8), D(), None, m(4, 64, 64, dt=i32), 3, 2),                        # 3-channel labels
                 (m(5000, dt=u8), D(), None, m(4, 64, 64), 1, 2),                                # fp32 label output
                 (m(5000, dt=u8), D(), None, m(4, 1, 64, 64, dt=i32), 1, 0),                     # int image output
                 (m(5000, dt=u8), D(), None, m(4, 1, 64, 64), 1, 4),                             # mode
                 (m(5000, dt=u8), D(), None, m(4, 1, 64, 64), 1, 0, 16),                         # flags
                 (m(5000, dt=u8), D(), None, m(4, 1, 64, 5000), 1, 0)):                          # too wide
        with pytest.raises(RuntimeError):
            ns.resize_pad(*args)
    with pytest.raises((RuntimeError, NotImplementedError)):       # CPU tensors: no kernel registered for them
        ns.resize_pad(torch.zeros(64, dtype=u8), torch.zeros(1, 4, dtype=i64), None, torch.zeros(1, 1, 8, 8), 1, 0, 4, 1.0)


# ---- kernel resources --------------------------------------------------------------------------------------------------
def test_resize_kernels_use_no_scratch_and_no_lds():
    """Every instantiation (C channels, kind 0 bilinear image / 1 nearest image / 2 labels, 1 or 4 columns per thread):
    no scratch, no spills (AGPRs), no LDS, 8 waves per SIMD."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr
    ks = {}
    for n, k in kr.kernels().items():
        m = re.search(r"resize_pad_kernelILi(\d)ELi(\d)ELi(\d)E", n)
        if m:
            ks[tuple(int(x) for x in m.groups())] = k
    assert sorted(ks) == [(1, 0, 1), (1, 0, 4), (1, 1, 1), (1, 1, 4), (1, 2, 1), (1, 2, 4), (3, 0, 1), (3, 0, 4), (3, 1, 1),
                          (3, 1, 4)]
    for key, k in ks.items():
        assert k["scratch"] == 0 and k["lds"] == 0 and k["agpr"] == 0, key
        assert k["max_threads"] == 256, key
        assert k["vgpr"] <= 64, (key, k["vgpr"])
        assert kr.waves_per_simd(k) == 8, key


# ---- the timing tool's device-free parts ---------------------------------------------------------------------------
def test_timing_tool_byte_counts_and_trace_summary(tmp_path):
    import importlib.util
    spec = importlib.util.spec_from_file_location("preprocess_time", os.path.join(ROOT, "tools", "preprocess_time.py"))
    pt = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(pt)
    sizes = pt.ragged_sizes()
    assert len(sizes) == 128 and all(200 <= s <= 1000 for hw in sizes for s in hw) and sizes == pt.ragged_sizes()
    assert len(set(sizes)) == 128
    assert pt.frame_crop() == (720, 640)
    # small views are read whole, large ones at most `taps` bytes per output item
    assert pt.hip_bytes([(10, 20), (3, 4)], 3, (256, 256), 4) == (3 * (200 + 12) + 64, 2 * 3 * 256 * 256 * 4)
    assert pt.hip_bytes([(10, 20)], 1, (48, 48), 1) == (200 + 32, 48 * 48 * 4)
    assert pt.hip_bytes([(1000, 1000), (200, 200)], 3, (256, 256), 4) == (4 * 256 * 256 * 3 + 200 * 200 * 3 + 64, 2 * 3 * 256 * 256 * 4)
    assert pt.hip_bytes([(1000, 1000)], 1, (48, 48), 1) == (48 * 48 + 32, 48 * 48 * 4)
    wl = pt.workloads()
    assert sorted(wl) == ["frame", "images", "masks"]
    assert [wl[k][1:] for k in ("images", "masks", "frame")] == [(3, (256, 256), 4), (1, (48, 48), 1), (3, (256, 256), 4)]
    assert wl["images"][0] == sizes == wl["masks"][0] and wl["frame"][0] == [(720, 640)]
    want = sum(min(h * w * 3, 4 * 256 * 256 * 3) for h, w in sizes) + 128 * 32
    assert pt.hip_bytes(*wl["images"]) == (want, 128 * 3 * 256 * 256 * 4)
    assert pt.hip_bytes(*wl["masks"]) == (128 * (48 * 48 + 32), 128 * 48 * 48 * 4)
    assert pt.hip_bytes(*wl["frame"]) == (4 * 256 * 256 * 3 + 32, 3 * 256 * 256 * 4)
    name = "void smplr::resize_pad_kernel<%s>(unsigned char const*, long long)"
    rows = [("other_kernel(float*)", 0, 9000, 64)]
    rows += [(name % "3, 0, 4", 1000 * k, 1000 * k + d, 2097152) for k, d in enumerate((31000, 30000, 35000))]
    rows += [(name % "1, 2, 4", 5, 2005, 98304)]
    p = tmp_path / "x_kernel_trace.csv"
    p.write_text('"Kernel_Name","Start_Timestamp","End_Timestamp","Grid_Size_X"\n'
                 + "".join('"%s",%d,%d,%d\n' % row for row in rows))
    assert pt.trace_medians(str(p)) == {"<1, 2, 4> grid 98304": {"n": 1, "median_us": 2.0, "min_us": 2.0},
                                        "<3, 0, 4> grid 2097152": {"n": 3, "median_us": 31.0, "min_us": 30.0}}
