"""The edge detector's definition on the CPU: known answers, `canny_edges_torch` (the CPU path of `ilps_amd.edges`) against
tests/_edges_oracle.py bit for bit, the float quantisation, and every ValueError of the Python layer.  No GPU."""
import numpy as np
import pytest
import torch

import _edges_oracle as eo
from ilps_amd import edges as ed

SETTINGS = {False: (300, 600), True: (60, 120)}            # (low, high) by blur: every class and every stage shows


def test_step_edge_is_one_column_by_the_asymmetric_tie_rule():
    """Left half 0, right half 200: columns 3 and 4 carry the same magnitude; `>` on the left and `>=` on the right keep
    exactly one of them (a symmetric rule gives two columns or none)."""
    img = np.zeros((1, 8, 8), np.uint8)
    img[:, :, 4:] = 200
    want = np.tile(np.array([0, 0, 0, 2, 0, 0, 0, 0], np.uint8), (8, 1))
    cls, status = eo.classes(img, "GREY_U8", 50, 100, blur=False, l2=False)
    assert np.array_equal(cls[0], want) and status[0] == 0
    got = ed.edge_classes(torch.from_numpy(img), low=50, high=100, blur=False, l2=False)
    assert got.dtype == torch.uint8 and np.array_equal(got[0].numpy(), want)
    assert np.array_equal(ed.canny_edges(torch.from_numpy(img), low=50, high=100, blur=False, l2=False)[0].numpy(), want // 2)


@pytest.mark.parametrize("shape", [(6, 9), (1, 1), (1, 5), (5, 1)])
def test_constant_and_tiny_images_have_no_edges(shape):
    img = np.full((2,) + shape, 137, np.uint8)
    for blur in (False, True):
        for l2 in (False, True):
            assert not eo.canny(img, "GREY_U8", low=0, high=0, blur=blur, l2=l2)[0].any()
            assert not ed.canny_edges(torch.from_numpy(img), low=0, high=0, blur=blur, l2=l2).any()


@pytest.mark.parametrize("l2", [False, True])
@pytest.mark.parametrize("blur", [False, True])
@pytest.mark.parametrize("hw", [(5, 7), (33, 65), (64, 64)])
def test_torch_restatement_equals_the_oracle(hw, blur, l2):
    rng = np.random.default_rng(hw[0] * 100 + hw[1] + 2 * blur + l2)
    img = rng.integers(0, 256, (2,) + hw, dtype=np.uint8)
    low, high = SETTINGS[blur]
    cls, _ = eo.classes(img, "GREY_U8", low, high, blur=blur, l2=l2)
    want = np.stack([eo.link(c) for c in cls])
    t = torch.from_numpy(img)
    got_cls, status = ed.edge_classes(t, low=low, high=high, blur=blur, l2=l2, return_status=True)
    assert torch.equal(got_cls, torch.from_numpy(cls)) and not status.any()
    assert torch.equal(ed.link_edges(got_cls), torch.from_numpy(want))
    assert torch.equal(ed.canny_edges_torch(t, low=low, high=high, blur=blur, l2=l2), torch.from_numpy(want))
    assert torch.equal(ed.canny_edges(t, low=low, high=high, blur=blur, l2=l2, value=255), torch.from_numpy(want) * 255)
    strong, weak, edges = int((cls == 2).sum()), int((cls == 1).sum()), int(want.sum())
    print("%s blur %d l2 %d: strong %d weak %d edges %d of %d" % (hw, blur, l2, strong, weak, edges, cls.size))
    if hw == (33, 65):                                       # every stage is visible in the result
        assert strong > 0 and weak > 0 and (cls == 0).any()
        assert strong < edges < strong + weak


def test_torch_restatement_on_every_form_and_per_row_thresholds():
    rng = np.random.default_rng(3)
    rgb = rng.integers(0, 256, (3, 9, 12, 3), dtype=np.uint8)
    f32 = (rgb.astype(np.float32) * np.float32(1 / 255.0)).astype(np.float32)
    srcs = {"RGB_U8": rgb, "RGB_F32_HWC": f32, "RGB_F32_CHW": np.ascontiguousarray(np.moveaxis(f32, 3, 1))}
    thr = np.array([[60, 120], [120, 60], [0, 2047]], np.int32)
    ref = None
    for form, src in srcs.items():
        for bgr in (False, True):
            want, wstat = eo.canny(src, form, thr=thr, bgr=bgr)
            got, stat = ed.canny_edges(torch.from_numpy(src), thr=torch.from_numpy(thr), bgr=bgr, return_status=True)
            assert ed.infer_form(torch.from_numpy(src)) == form
            assert torch.equal(got, torch.from_numpy(want)) and stat.tolist() == wstat.tolist() == [0, 1, 0]
            assert not got[1].any() and got[0].any()
            if not bgr:                                      # the three forms hold the same picture
                ref = want if ref is None else ref
                assert np.array_equal(want, ref)


def test_quantisation_returns_every_byte():
    """`load_images` hands out fp32(v) * fp32(1 / 255); the default scale 255 returns v."""
    v = np.arange(256)
    c = (v.astype(np.float32) * np.float32(1.0 / 255.0)).astype(np.float32)
    assert np.array_equal(eo.quantize(c), v)
    assert ed.quantize_torch(torch.from_numpy(c)).tolist() == v.tolist()


def test_hostile_floats():
    c = np.array([np.nan, np.inf, -np.inf, 1e30, -1.0, 0.0, 1.0, 0.5], np.float32)
    want = [0, 255, 0, 255, 0, 0, 255, 128]
    assert eo.quantize(c).tolist() == want
    assert ed.quantize_torch(torch.from_numpy(c)).tolist() == want
    img = np.tile(c[:6], (1, 4, 2))[..., None].repeat(3, -1).astype(np.float32)          # (1, 4, 12, 3)
    want, _ = eo.canny(img, "RGB_F32_HWC", low=10, high=20, blur=False)
    assert torch.equal(ed.canny_edges(torch.from_numpy(img), low=10, high=20, blur=False), torch.from_numpy(want)) and want.any()


def test_link_on_hand_built_maps():
    c, n = eo.boustrophedon(33, 33)
    assert n == 577
    for m in (c, c.T.copy()):
        want = eo.link(m)
        assert int(want.sum()) == 577
        assert torch.equal(ed.link_edges(torch.from_numpy(m[None])), torch.from_numpy(want[None]))
    m = np.zeros((1, 4, 6), np.uint8)
    m[0, 1, 1:3], m[0, 3, 4] = (1, 7), 1                       # 7 is strong; the lone weak pixel stays out
    assert ed.link_edges(torch.from_numpy(m), 255).tolist() == [[[0] * 6, [0, 255, 255, 0, 0, 0], [0] * 6, [0] * 6]]


def test_value_errors():
    u8 = torch.zeros((2, 8, 8), dtype=torch.uint8)
    f32 = torch.zeros((2, 8, 8, 3))
    bad = [
        lambda: ed.edge_classes(u8),                                                    # no thresholds
        lambda: ed.edge_classes(u8, low=1),
        lambda: ed.edge_classes(u8, low=5, high=4),
        lambda: ed.edge_classes(u8, low=-1, high=4),
        lambda: ed.edge_classes(u8, low=0, high=2048),
        lambda: ed.edge_classes(u8, low=1.5, high=4),
        lambda: ed.edge_classes(u8, low=1, high=2, thr=torch.zeros((2, 2), dtype=torch.int32)),
        lambda: ed.edge_classes(u8, thr=torch.zeros((2, 2), dtype=torch.int64)),
        lambda: ed.edge_classes(u8, thr=torch.zeros((3, 2), dtype=torch.int32)),
        lambda: ed.edge_classes(u8, low=1, high=2, form="GREY"),
        lambda: ed.edge_classes(u8, low=1, high=2, form="RGB_U8"),
        lambda: ed.edge_classes(f32, low=1, high=2, form="RGB_F32_CHW"),
        lambda: ed.edge_classes(f32.double(), low=1, high=2),
        lambda: ed.edge_classes(torch.zeros((2, 8, 8, 4)), low=1, high=2),
        lambda: ed.edge_classes(u8.numpy(), low=1, high=2),
        lambda: ed.edge_classes(torch.zeros((1, 513, 8), dtype=torch.uint8), low=1, high=2),
        lambda: ed.edge_classes(torch.zeros((1, 8, 0), dtype=torch.uint8), low=1, high=2),
        lambda: ed.edge_classes(f32, low=1, high=2, scale=float("inf")),
        lambda: ed.link_edges(u8, 0),
        lambda: ed.link_edges(u8, 256),
        lambda: ed.link_edges(u8.to(torch.int32)),
        lambda: ed.link_edges(u8[0]),
        lambda: ed.link_edges(torch.zeros((1, 8, 513), dtype=torch.uint8)),
        lambda: ed.link_edges(u8, out=torch.zeros((2, 8, 8))),
        lambda: ed.canny_edges(u8, low=1, high=2, value=300),
        lambda: ed.edge_proxy_inputs(u8, low=1, high=2, value=255),
    ]
    for i, fn in enumerate(bad):
        with pytest.raises(ValueError):
            fn()
            pytest.fail("case %d raised nothing" % i)
    assert ed.canny_edges(torch.zeros((0, 8, 8), dtype=torch.uint8), low=1, high=2).shape == (0, 8, 8)


def test_c_abi_argument_errors_name_the_function():
    """Argument errors return -1 with the function's name in smplr_last_error(), without touching the GPU."""
    from ilps_amd import _lib
    lib = _lib.load()
    one = 1                                                                             # (a non-null pointer; never read)
    cases = [dict(form=4), dict(B=-1), dict(H=0), dict(W=513), dict(scale=float("nan")), dict(blur=2), dict(l2=-1), dict(bgr=2),
             dict(low=5, high=4), dict(high=2048), dict(src=None), dict(classes=None)]
    for kw in cases:
        a = dict(src=one, form=0, B=1, H=8, W=8, scale=255.0, bgr=0, blur=1, l2=1, low=1, high=2, thr=None, classes=one)
        a.update(kw)
        rc = lib.smplr_edge_classify(a["src"], a["form"], a["B"], a["H"], a["W"], a["scale"], a["bgr"], a["blur"], a["l2"],
                                     a["low"], a["high"], a["thr"], a["classes"], None, None)
        assert rc == -1 and b"smplr_edge_classify" in lib.smplr_last_error(), kw
    assert lib.smplr_edge_classify(None, 0, 0, 8, 8, 255.0, 0, 1, 1, 1, 2, None, None, None, None) == 0
    for kw in (dict(B=-1), dict(H=513), dict(W=0), dict(value=0), dict(value=256), dict(classes=None), dict(edges=None)):
        a = dict(classes=one, B=1, H=8, W=8, value=1, edges=one)
        a.update(kw)
        rc = lib.smplr_edge_link(a["classes"], a["B"], a["H"], a["W"], a["value"], a["edges"], None)
        assert rc == -1 and b"smplr_edge_link" in lib.smplr_last_error(), kw
    assert lib.smplr_edge_link(None, 0, 8, 8, 1, None, None) == 0


def test_torch_ops_have_meta_kernels_and_refuse_cpu_tensors():
    from ilps_amd import torch_ops
    ns = torch_ops.load()
    for name in ("edge_classify", "edge_link"):
        assert str(getattr(ns, name).default._schema) == torch_ops.SCHEMAS[name]
    m = lambda *s, dt=torch.float32: torch.empty(*s, dtype=dt, device="meta")
    cls, status = ns.edge_classify(m(4, 3, 32, 48), 3, None, 60, 120)
    assert cls.shape == (4, 32, 48) and cls.dtype == torch.uint8 and status.shape == (4,) and status.dtype == torch.int32
    assert ns.edge_classify(m(2, 9, 7, dt=torch.uint8), 0, m(2, 2, dt=torch.int32))[0].shape == (2, 9, 7)
    assert ns.edge_link(cls, 255).shape == (4, 32, 48)
    for args in ((m(4, 3, 32, 48), 2, None, 60, 120), (m(4, 32, 48), 0, None, 60, 120), (m(4, 3, 32, 48), 3, None, 120, 60),
                 (m(1, 600, 8, dt=torch.uint8), 0, None, 1, 2), (m(2, 9, 7, dt=torch.uint8), 0, m(2, 3, dt=torch.int32))):
        with pytest.raises(RuntimeError):
            ns.edge_classify(*args)
    with pytest.raises(RuntimeError):
        ns.edge_link(cls, 0)
    with pytest.raises((RuntimeError, NotImplementedError)):
        ns.edge_classify(torch.zeros(1, 8, 8, dtype=torch.uint8), 0, None, 1, 2)        # a CPU tensor
    with pytest.raises((RuntimeError, NotImplementedError)):
        ns.edge_link(torch.zeros(1, 8, 8, dtype=torch.uint8))
