"""csrc/edges.hip through `ilps_amd.edges` on the GPU against tests/_edges_oracle.py (the definition in NumPy int64).  Every
comparison is `torch.equal`: the detector is integer arithmetic and has no tolerance.

Sizes: 1 x 1 is smaller than any halo, 1 x 9 and 9 x 1 have one clamped axis, 67 x 131 is no multiple of the 16 x 64 tile nor
of the link kernel's 64-bit row word and spans several of both, 512 x 512 is the limit (64 KB of bit planes, the raised LDS
attribute, 1024-thread workgroup)."""
import numpy as np
import pytest
import torch

import _edges_oracle as eo
from ilps_amd import edges as ed

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SETTINGS = {False: (300, 600), True: (60, 120)}            # (low, high) by blur, as tests/test_edges_cpu.py
SIZES = [(1, 1), (1, 9), (9, 1), (5, 7), (33, 65), (64, 64), (67, 131)]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def picture(B, H, W, seed):
    """uint8 RGB noise over a few flat rectangles: dense gradients of every direction, plateaus, ties."""
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    for b in range(B):
        for _ in range(3):
            y, x = int(rng.integers(0, H)), int(rng.integers(0, W))
            img[b, y:y + max(H // 3, 1), x:x + max(W // 3, 1)] = rng.integers(0, 256, 3, dtype=np.uint8)
    return img


def as_form(rgb, form):
    """The uint8 RGB batch in a source form (grey: the green channel); the float forms carry fp32(v) * fp32(1 / 255)."""
    if form == "GREY_U8":
        return np.ascontiguousarray(rgb[..., 1])
    if form == "RGB_U8":
        return rgb
    f = (rgb.astype(np.float32) * np.float32(1.0 / 255.0)).astype(np.float32)
    return f if form == "RGB_F32_HWC" else np.ascontiguousarray(np.moveaxis(f, 3, 1))


def check(src, form, **kw):
    """classify == oracle, canny == oracle, status == oracle, on one batch; -> (classes, edges) of the oracle."""
    want_cls, want_status = eo.classes(src, form, **kw)
    want = np.stack([eo.link(c) for c in want_cls])
    t = dev(src)
    tkw = dict(kw)
    if tkw.get("thr") is not None:
        tkw["thr"] = dev(np.asarray(tkw["thr"], np.int32))
    cls, status = ed.edge_classes(t, form=form, return_status=True, **tkw)
    assert cls.dtype == torch.uint8 and cls.is_contiguous() and cls.device == DEV
    assert torch.equal(cls.cpu(), torch.from_numpy(want_cls)), (form, kw, "classes")
    assert status.cpu().tolist() == want_status.tolist()
    got = ed.canny_edges(t, **tkw)                                        # (the form inferred)
    assert torch.equal(got.cpu(), torch.from_numpy(want)), (form, kw, "edges")
    return want_cls, want


@pytest.mark.parametrize("l2", [False, True])
@pytest.mark.parametrize("blur", [False, True])
@pytest.mark.parametrize("hw", SIZES)
def test_kernels_equal_the_oracle(hw, blur, l2):
    low, high = SETTINGS[blur]
    src = as_form(picture(2, hw[0], hw[1], seed=hw[0] * 1000 + hw[1]), "GREY_U8")
    cls, edges = check(src, "GREY_U8", low=low, high=high, blur=blur, l2=l2)
    if hw[0] >= 33:
        strong, weak = int((cls == 2).sum()), int((cls == 1).sum())
        assert strong > 0 and weak > 0 and strong < int(edges.sum()) < strong + weak


def test_kernels_equal_the_oracle_at_the_size_limit():
    src = as_form(picture(1, 512, 512, seed=512), "GREY_U8")
    cls, edges = check(src, "GREY_U8", low=60, high=120, blur=True, l2=True)
    assert int((cls == 2).sum()) < int(edges.sum()) < int((cls > 0).sum())


@pytest.mark.parametrize("form", eo.FORMS)
def test_every_source_form(form):
    rgb = picture(2, 33, 65, seed=7)
    src = as_form(rgb, form)
    for bgr in (False, True):
        for blur, l2 in ((True, True), (False, False)):
            low, high = SETTINGS[blur]
            check(src, form, low=low, high=high, blur=blur, l2=l2, bgr=bgr)
    if form.startswith("RGB_F32"):                                        # fp32(v) / 255 at scale 255 is the byte picture
        a = ed.canny_edges(dev(src), low=60, high=120)
        assert torch.equal(a, ed.canny_edges(dev(rgb), low=60, high=120))
        half = ed.canny_edges(dev(src * np.float32(0.5)), low=60, high=120, scale=510.0)
        assert torch.equal(a, half)                                       # (a power of two moves between picture and scale)
        check(src * np.float32(3.0) - np.float32(1.0), form, low=60, high=120)     # clamped at both ends


def test_per_row_thresholds_and_status():
    src = as_form(picture(5, 33, 65, seed=11), "RGB_U8")
    thr = [[60, 120], [120, 60], [-1, 5], [0, 2048], [0, 2047]]
    for blur, l2 in ((True, True), (True, False), (False, True)):
        cls, edges = check(src, "RGB_U8", thr=thr, blur=blur, l2=l2)
        assert edges[0].any() and not cls[1:4].any() and cls[4].any()
    t = dev(src)
    _, status = ed.edge_classes(t, thr=dev(np.array(thr, np.int32)), return_status=True)
    assert status.tolist() == [0, 1, 1, 1, 0]
    same = ed.edge_classes(t, thr=dev(np.array([[60, 120]] * 5, np.int32)))
    assert torch.equal(same, ed.edge_classes(t, low=60, high=120))


@pytest.mark.parametrize("hw", [(20, 70), (16, 64), (3, 3)])
def test_structure_on_all_four_borders(hw):
    """A one-pixel frame on the image's border and nothing else: the Sobel taps beyond the border must replicate (zero
    padding would see a step there), the magnitudes beyond it must be zero (replicating them would suppress the frame)."""
    H, W = hw
    img = np.zeros((1, H, W), np.uint8)
    img[0, 0], img[0, -1], img[0, :, 0], img[0, :, -1] = 255, 255, 255, 255
    for blur in (False, True):
        for l2 in (False, True):
            cls, edges = check(img, "GREY_U8", low=40, high=80, blur=blur, l2=l2)
            assert H < 16 or edges.any()


# ---- link alone ---------------------------------------------------------------------------------------------------------------
def link_check(c, value=1):
    want = eo.link(c, value)
    got = ed.link_edges(dev(c[None]), value)
    assert got.dtype == torch.uint8 and torch.equal(got.cpu()[0], torch.from_numpy(want))
    return want


@pytest.mark.parametrize("hw", [(33, 33), (67, 131)])
def test_link_follows_a_boustrophedon_to_its_end(hw):
    """One strong pixel at the start of a path that sweeps the image row by row: a closure that wins one ring per sweep
    needs 545 sweeps at 33 x 33, and a capped loop stops short.  Transposed, the in-word row flood cannot help."""
    c, n = eo.boustrophedon(*hw)
    assert hw != (33, 33) or n == 577
    assert int(link_check(c).sum()) == n
    assert int(link_check(np.ascontiguousarray(c.T)).sum()) == n


def test_link_on_hand_built_maps():
    s = eo.staircase(40, 70)
    assert int(link_check(s).sum()) == 40
    assert int(link_check(np.ascontiguousarray(s[:, ::-1])).sum()) == 40          # the other diagonal
    two = np.zeros((9, 140), np.uint8)
    two[2, 3:130], two[6, 60:135] = 1, 1                       # two weak components over three words; one holds the strong pixel
    two[6, 100] = 2
    want = link_check(two)
    assert not want[2].any() and int(want[6].sum()) == 75
    weak_only = (two > 0).astype(np.uint8)
    assert not link_check(weak_only).any()                     # no strong pixel: all zero
    seven = weak_only.copy()
    seven[2, 64] = 7                                           # any value >= 2 is strong
    want = link_check(seven, 255)
    assert int((want == 255).sum()) == 127 and not want[6].any() and set(np.unique(want)) == {0, 255}
    full = np.ones((64, 128), np.uint8)
    full[63, 127] = 2
    assert link_check(full).all()


# ---- other --------------------------------------------------------------------------------------------------------------------
def test_rows_are_independent():
    f = as_form(picture(4, 20, 70, seed=5), "RGB_F32_HWC")
    f[1, ::2] = np.nan
    f[1, 1::4] = np.inf
    f[1, 3::4] = -1e30
    t = dev(f)
    full = ed.canny_edges(t, low=60, high=120)
    check(f, "RGB_F32_HWC", low=60, high=120)
    for b in range(4):
        assert torch.equal(ed.canny_edges(t[b:b + 1], low=60, high=120)[0], full[b]), b


def test_empty_batch():
    e = ed.canny_edges(torch.empty((0, 8, 8, 3), device=DEV), low=1, high=2)
    assert e.shape == (0, 8, 8) and e.dtype == torch.uint8 and e.device == DEV
    c, s = ed.edge_classes(torch.empty((0, 3, 8, 8), device=DEV), low=1, high=2, form="RGB_F32_CHW", return_status=True)
    assert c.shape == (0, 8, 8) and s.shape == (0,)


def test_non_contiguous_source_is_made_contiguous():
    hwc = dev(as_form(picture(2, 33, 65, seed=3), "RGB_F32_HWC"))
    chw_view = hwc.permute(0, 3, 1, 2)
    assert not chw_view.is_contiguous()
    a = ed.canny_edges(chw_view, form="RGB_F32_CHW", low=60, high=120)
    assert torch.equal(a, ed.canny_edges(hwc, low=60, high=120)) and a.any()
    cls = ed.edge_classes(hwc, low=60, high=120)
    wide = torch.zeros((2, 33, 130), dtype=torch.uint8, device=DEV)
    wide[:, :, ::2] = cls
    assert torch.equal(ed.link_edges(wide[:, :, ::2]), ed.link_edges(cls))


def test_torch_ops_equal_the_ctypes_path():
    from ilps_amd import torch_ops
    ns = torch_ops.load()
    rgb = picture(3, 20, 70, seed=9)
    thr = dev(np.array([[60, 120], [5, 1], [30, 300]], np.int32))
    for form, f in ed.FORMS.items():
        t = dev(as_form(rgb, form))
        for blur, l2, bgr in ((True, True, False), (False, False, True)):
            want, wstat = ed.edge_classes(t, form=form, low=60, high=120, blur=blur, l2=l2, bgr=bgr, return_status=True)
            cls, status = ns.edge_classify(t, f, None, 60, 120, blur, l2, 255.0, bgr)
            assert torch.equal(cls, want) and torch.equal(status, wstat)
        want, wstat = ed.edge_classes(t, form=form, thr=thr, return_status=True)
        cls, status = ns.edge_classify(t, f, thr)
        assert torch.equal(cls, want) and torch.equal(status, wstat) and status.tolist() == [0, 1, 0]
        assert torch.equal(ns.edge_link(cls), ed.link_edges(want))
        assert torch.equal(ns.edge_link(cls, 255), ed.link_edges(want, 255))
    with pytest.raises(RuntimeError):
        ns.edge_classify(t, 0, None, 60, 120)


def test_graph_capture_replays_on_new_pixels():
    H, W = 33, 65
    first, second = (as_form(picture(2, H, W, seed=s), "RGB_F32_HWC") for s in (21, 22))
    src = dev(first)
    out = torch.zeros((2, H, W), dtype=torch.uint8, device=DEV)
    ed.canny_edges(src, low=60, high=120, out=out)                       # warm-up: library loaded, kernels resident
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ed.canny_edges(src, low=60, high=120, out=out)
    for pix in (second, first):
        src.copy_(dev(pix))
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        want, _ = eo.canny(pix, "RGB_F32_HWC", low=60, high=120)
        assert torch.equal(out.cpu(), torch.from_numpy(want)) and want.any()


def test_device_torch_restatement_equals_the_kernels():
    """`canny_edges_torch` on the device (the timing baseline) computes the same map."""
    t = dev(as_form(picture(2, 33, 65, seed=13), "RGB_F32_CHW"))
    for blur, l2 in ((True, True), (False, False)):
        low, high = SETTINGS[blur]
        assert torch.equal(ed.canny_edges(t, low=low, high=high, blur=blur, l2=l2),
                           ed.canny_edges_torch(t, low=low, high=high, blur=blur, l2=l2))


# ---- edge_proxy_inputs ----------------------------------------------------------------------------------------------------------
def test_edge_proxy_inputs():
    from ilps_amd.synthetic import proxy_inputs
    B, H, W, J = 3, 33, 65, 5
    rgb = picture(B, H, W, seed=17)
    src = as_form(rgb, "RGB_F32_CHW")
    rng = np.random.default_rng(0)
    joints = dev((rng.random((B, J, 2)) * [W, H]).astype(np.float32))
    keep = dev(np.array([[1, 1, 0, 1, 1]] * B, np.uint8))
    boxes = np.array([[[4, 5, 30, 20]], [[0, 0, 0, 0]], [[-5, 10, 70, 12]]], np.int32)
    got = ed.edge_proxy_inputs(dev(src), joints, keep, dev(boxes), sigma=3.0, low=60, high=120)
    assert got.shape == (B, 1 + J, H, W) and got.dtype == torch.float32 and got.is_contiguous()
    want, _ = eo.canny(src, "RGB_F32_CHW", low=60, high=120)
    want = want.astype(np.float32)
    assert want[0, 5:20, 4:30].any() and want[2, 10:12].any()            # the boxes have something to remove
    want[0, 5:20, 4:30] = 0
    want[2, 10:12, 0:W] = 0
    assert torch.equal(got[:, 0].cpu(), torch.from_numpy(want))
    heat = proxy_inputs(torch.zeros((B, H, W), dtype=torch.uint8, device=DEV), joints, keep, seg="none", sigma=3.0)
    assert torch.equal(got[:, 1:].view(torch.int32), heat.view(torch.int32)) and float(heat.max()) > 0
    only = ed.edge_proxy_inputs(dev(rgb), low=60, high=120)              # no joints: the edge channel alone
    assert only.shape == (B, 1, H, W) and torch.equal(only[:, 0].cpu(), torch.from_numpy(eo.canny(rgb, "RGB_U8", low=60, high=120)[0]
                                                                                          .astype(np.float32)))
