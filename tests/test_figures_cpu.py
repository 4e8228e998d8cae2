"""ilps_amd.figures without a GPU: the CPU path against the NumPy oracle (tests/_figures_oracle.py) on the cases the GPU
test runs, argument errors of the Python API and of the C ABI (reported before any launch), the PNG writer, the figure
set / panel shapes and the files `save_predictions` and `MonitorFigures` write, and the torch ops' Meta kernels."""
import os
import struct
import zlib

import numpy as np
import pytest
import torch

import _figures_oracle as fo
from ilps_amd import _lib, figures


@pytest.mark.parametrize("hw", fo.SEG_SRC)
@pytest.mark.parametrize("HW", fo.SEG_OUT)
def test_seg_colour_cpu_equals_oracle(hw, HW):
    fo.check_seg_colour("cpu", hw, HW)


@pytest.mark.parametrize("HW", fo.SC_HW)
@pytest.mark.parametrize("r", fo.SC_R)
def test_scatter_cpu_equals_oracle(HW, r):
    fo.check_scatter("cpu", HW, r)


def test_scatter_cpu_inexact_scale_and_sampled_vertices():
    """predict.py:65's scale at 256 / 48 (no fp32 product is exact) on the 1 378 sampled projections."""
    fo.check_scatter("cpu", (96, 130), 1, Bs=(2,), Vs=(1378,), s=256.0 / 48.0)


def test_default_lut_is_the_renderers_palette():
    from ilps_amd.render import default_palette, to_uint8
    lut = figures.default_lut()
    assert lut.dtype == torch.uint8 and tuple(lut.shape) == (32, 3)
    assert np.array_equal(lut.numpy(), fo.default_lut())
    assert torch.equal(lut, to_uint8(torch.from_numpy(default_palette())))


def test_python_argument_errors():
    s = torch.zeros(1, 4, 4, 32)
    p = torch.zeros(1, 5, 3)
    with pytest.raises(ValueError, match="2 <= C <= 32"):
        figures.seg_colour(torch.zeros(1, 4, 4, 33))
    with pytest.raises(ValueError, match="2 <= C <= 32"):
        figures.seg_colour(torch.zeros(1, 4, 4, 1))
    with pytest.raises(ValueError, match="outside 1"):
        figures.seg_colour(s, size=(4, 0))
    with pytest.raises(ValueError, match="background"):
        figures.seg_colour(s, size=8, background=torch.zeros(1, 4, 4, 3, dtype=torch.uint8))
    with pytest.raises(ValueError, match="radius"):
        figures.scatter_points(p, 8, 1.0, radius=17)
    with pytest.raises(ValueError, match="outside 1"):
        figures.scatter_points(p, (8, 0), 1.0)
    with pytest.raises(ValueError, match="colours"):
        figures.scatter_points(p, 8, 1.0, colours=torch.zeros(4, 3, dtype=torch.uint8))
    with pytest.raises(ValueError, match="order"):
        figures.scatter_points(p, 8, 1.0, order="z")
    with pytest.raises(ValueError, match="image_alpha"):
        figures.scatter_points(p, 8, 1.0, image_alpha=1.5)
    with pytest.raises(RuntimeError, match="lives on"):
        figures.scatter_points(p, 8, 1.0, keep=torch.ones(1, 5, dtype=torch.uint8, device="meta"))
    with pytest.raises(RuntimeError, match="lives on"):
        figures.scatter_points(p, 8, 1.0, image=torch.zeros(1, 8, 8, 3, dtype=torch.uint8, device="meta"))
    with pytest.raises(RuntimeError, match="lives on"):
        figures.seg_colour(s, background=torch.zeros(1, 4, 4, 3, dtype=torch.uint8, device="meta"))


def test_c_abi_refuses_bad_arguments_without_a_launch():
    """SMPLR_EINVAL + smplr_last_error() for each limit of the two launchers; an empty batch is a no-op (no GPU here)."""
    lib = _lib.load()
    one = 1                                                               # (a non-null pointer that is never followed)

    def seg(scores=one, labels=None, B=1, h=4, w=4, C=32, K=32, bad=0, aq=128, H=8, W=8):
        return lib.smplr_seg_colour(scores, labels, B, h, w, C, one, K, bad, None, aq, H, W, one, None)

    def sc(B=1, V=10, scale=1.0, r=1, order=0, H=8, W=8, aq=230, colour=0, canvas=0):
        return lib.smplr_scatter_points(one, None, None, colour, None, aq, canvas, B, V, scale, r, order, H, W, one, one, None)

    for call, text in ((lambda: seg(C=33), b"33 score channels"), (lambda: seg(C=1), b"1 score channels"),
                       (lambda: seg(H=0), b"picture 0 x 8"), (lambda: seg(W=4097), b"picture 8 x 4097"),
                       (lambda: seg(h=0), b"source map"), (lambda: seg(labels=one), b"exactly one"),
                       (lambda: seg(scores=None), b"exactly one"), (lambda: seg(aq=257), b"alpha_q"),
                       (lambda: seg(K=0), b"colour table"), (lambda: seg(B=-1), b"negative batch"),
                       (lambda: seg(bad=1 << 24), b"bad_colour"), (lambda: sc(r=17), b"radius 17"),
                       (lambda: sc(r=-1), b"radius -1"), (lambda: sc(H=0), b"image 0 x 8"), (lambda: sc(W=4097), b"image 8 x 4097"),
                       (lambda: sc(V=0), b"V=0"), (lambda: sc(V=(1 << 24) + 1), b"bad sizes"), (lambda: sc(order=2), b"order 2"),
                       (lambda: sc(scale=float("inf")), b"scale"), (lambda: sc(scale=float("nan")), b"scale"),
                       (lambda: sc(aq=-1), b"alpha_q"), (lambda: sc(canvas=-1), b"canvas")):
        rc = call()
        assert rc == -1 and text in lib.smplr_last_error(), (rc, text, lib.smplr_last_error())
    assert seg(B=0) == 0 and sc(B=0) == 0
    assert lib.smplr_seg_colour(None, None, 0, 4, 4, 32, None, 32, 0, None, 0, 8, 8, None, None) == 0
    assert lib.smplr_scatter_points(None, None, None, 0, None, 0, 0, 0, 10, 1.0, 0, 0, 8, 8, None, None, None) == 0


def decode_png(path):
    """An 8-bit, non-interlaced PNG with filter type 0 on every row, by hand: -> (H, W[, channels]) uint8."""
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, chunks = 8, []
    while pos < len(data):
        n, tag = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        assert struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(tag + body) & 0xffffffff
        chunks.append((tag, body))
        pos += 12 + n
    assert chunks[0][0] == b"IHDR" and chunks[-1] == (b"IEND", b"")
    W, H, depth, ctype, comp, filt, lace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, comp, filt, lace) == (8, 0, 0, 0)
    ch = {0: 1, 2: 3, 6: 4}[ctype]
    raw = np.frombuffer(zlib.decompress(b"".join(b for t, b in chunks if t == b"IDAT")), np.uint8).reshape(H, 1 + W * ch)
    assert (raw[:, 0] == 0).all()
    px = raw[:, 1:].reshape(H, W, ch)
    return px[:, :, 0] if ch == 1 else px


@pytest.mark.parametrize("shape", [(5, 7, 3), (1, 1, 3), (6, 4), (3, 9, 4), (64, 33, 3)])
def test_write_png_round_trips(tmp_path, shape):
    a = np.random.default_rng(sum(shape)).integers(0, 256, shape).astype(np.uint8)
    path = figures.write_png(str(tmp_path / "a.png"), torch.from_numpy(a))
    assert np.array_equal(decode_png(path), a)
    try:
        from PIL import Image
    except ImportError:
        return
    assert np.array_equal(np.asarray(Image.open(path)), a)


def test_write_png_refuses_other_arrays(tmp_path):
    with pytest.raises(ValueError):
        figures.write_png(str(tmp_path / "a.png"), np.zeros((4, 4, 3), np.float32))
    with pytest.raises(ValueError):
        figures.write_png(str(tmp_path / "a.png"), np.zeros((4, 4, 2), np.uint8))


def test_image_conversion_rule():
    x = torch.tensor([0.0, 0.5, 1.0, 254.9 / 255, -0.2, 1.7, float("nan"), float("inf")]).reshape(1, 1, 8, 1).expand(1, 3, 8, 1)
    u = figures.as_uint8_images(x)
    assert tuple(u.shape) == (1, 8, 1, 3) and u.dtype == torch.uint8
    assert u[0, :, 0, 0].tolist() == [0, 127, 255, 254, 0, 255, 0, 255]
    same = torch.arange(24, dtype=torch.uint8).reshape(1, 2, 4, 3)
    assert torch.equal(figures.as_uint8_images(same), same)
    assert torch.equal(figures.as_uint8_images(same.permute(0, 3, 1, 2)), same)


def test_keep_from_mask_and_part_colours(part_tables):
    """compute_mask.py writes 1 for a visible vertex and 500 for a hidden one; part colours are lut[1 + part]."""
    from ilps_amd.render import vertex_parts
    m = torch.tensor([[1.0, 500.0, 1.0, 500.0]])
    assert figures.keep_from_mask(m).tolist() == [[1, 0, 1, 0]] and figures.keep_from_mask(m).dtype == torch.uint8
    cols = figures.part_colours(part_tables[1], 6890)
    assert cols.dtype == torch.uint8 and tuple(cols.shape) == (6890, 3)
    assert np.array_equal(cols.numpy(), fo.default_lut()[vertex_parts(part_tables[1], 6890) + 1])


def fake_pred(N, W, V, seed, silh=False):
    rng = np.random.default_rng(seed)
    pred = {"segs": torch.from_numpy(fo.seg_scores(N, W, W, 32, seed)),
            "projects": torch.from_numpy(rng.uniform(0, W, (N, V, 3)).astype(np.float32))}
    if silh:
        pred["silhouette"] = torch.from_numpy(fo.seg_scores(N, W, W, 2, seed + 1))
    return pred


def test_prediction_figures_panel_and_saved_files(tmp_path, part_tables):
    N, W, S = 2, 12, 40
    pred = fake_pred(N, W, 6890, 3, silh=True)
    images = torch.from_numpy(np.random.default_rng(0).random((N, 3, S, S)).astype(np.float32))
    figs = figures.prediction_figures(pred, images, W, part_tables=part_tables[1])
    assert sorted(figs) == ["input", "projects", "seg", "seg_overlay", "silh", "verts_overlay"]
    for k, v in figs.items():
        assert v.dtype == torch.uint8 and tuple(v.shape) == (N, S, S, 3), k
    img = figures.as_uint8_images(images).numpy()
    proj = pred["projects"].numpy()
    cols = figures.part_colours(part_tables[1], 6890).numpy()
    win = fo.scatter_vertex(proj, S, S, S / W, 0, "index")
    assert np.array_equal(figs["input"].numpy(), img)
    assert np.array_equal(figs["seg"].numpy(), fo.seg_colour(pred["segs"].numpy(), S, S))
    assert np.array_equal(figs["silh"].numpy(), fo.seg_colour(pred["silhouette"].numpy(), S, S, lut=figures.SILH_LUT))
    assert np.array_equal(figs["projects"].numpy(), fo.scatter_rgb(win, cols))
    assert np.array_equal(figs["verts_overlay"].numpy(), fo.scatter_rgb(win, cols, image=img))
    assert np.array_equal(figs["seg_overlay"].numpy(), fo.seg_colour(pred["segs"].numpy(), S, S, background=img, alpha_q=128))
    panel = figures.prediction_panel(pred, images, W, part_tables=part_tables[1], size=16)
    assert panel.dtype == torch.uint8 and tuple(panel.shape) == (N, 16, 6 * 16, 3)
    small = figures.prediction_figures(pred, images, W, part_tables=part_tables[1], size=16)
    assert torch.equal(panel[:, :, 16:32], small["seg"]) and torch.equal(panel[:, :, :16], small["input"])
    paths = figures.save_predictions(figs, ["a/first.jpg", "second.png"], str(tmp_path / "out"))
    want = sorted("%s_%s.png" % (stem, k) for stem in ("first", "second") for k in ("seg", "projects", "input", "verts_overlay"))
    assert sorted(os.listdir(tmp_path / "out")) == want and sorted(os.path.basename(p) for p in paths) == want
    assert np.array_equal(decode_png(str(tmp_path / "out" / "second_verts_overlay.png")), figs["verts_overlay"][1].numpy())
    with pytest.raises(ValueError):
        figures.save_predictions(figs, ["only_one.png"], str(tmp_path / "out"))


class FakeTrainer:
    """What `MonitorFigures` uses of a `SegTrainer`: output_wh and monitor(images)."""

    def __init__(self, W, silh):
        self.output_wh, self.silh, self.calls = W, silh, 0

    def monitor(self, images):
        self.calls += 1
        out = fake_pred(int(images.shape[0]), self.output_wh, 300, 7 + self.calls, self.silh)
        out["seg"] = out.pop("segs")
        return out


@pytest.mark.parametrize("silh", [False, True])
def test_monitor_figures_writes_the_references_file_names(tmp_path, silh):
    images = torch.from_numpy(np.random.default_rng(1).integers(0, 256, (2, 24, 24, 3)).astype(np.uint8))
    hook = figures.MonitorFigures(images, str(tmp_path / "mon"))
    trainer = FakeTrainer(12, silh)
    hook(0, trainer)
    kinds = ("seg", "verts") + (("silh",) if silh else ())
    want0 = sorted(["%s_0_%d.png" % (k, i) for k in kinds for i in range(2)] + ["image_%d.png" % i for i in range(2)])
    assert sorted(os.listdir(tmp_path / "mon")) == want0
    figs = hook(10, trainer)
    want10 = sorted(want0 + ["%s_10_%d.png" % (k, i) for k in kinds for i in range(2)])
    assert sorted(os.listdir(tmp_path / "mon")) == want10 and len(hook.written) == 2 * len(kinds)
    assert np.array_equal(decode_png(str(tmp_path / "mon" / "seg_10_1.png")), figs["seg"][1].numpy())
    assert np.array_equal(decode_png(str(tmp_path / "mon" / "image_0.png")), images[0].numpy())


def test_meta_kernels_give_shapes_and_dtypes():
    from ilps_amd import torch_ops
    ns = torch_ops.load()
    m = lambda *s, dt=torch.float32: torch.empty(*s, dtype=dt, device="meta")
    u8 = torch.uint8
    rgb = ns.seg_colour(m(2, 48, 48, 32), m(32, 3, dt=u8), None, 100, 37)
    assert tuple(rgb.shape) == (2, 100, 37, 3) and rgb.dtype == u8
    rgb = ns.seg_colour(m(2, 5, 7, dt=torch.int32), m(4, 3, dt=u8), m(2, 63, 65, 3, dt=u8), 63, 65, 128, 255)
    assert tuple(rgb.shape) == (2, 63, 65, 3) and rgb.dtype == u8
    rgb, vert = ns.scatter_points(m(3, 6890, 3), m(3, 6890, dt=u8), m(6890, 3, dt=u8), m(3, 96, 130, 3, dt=u8), 96, 130, 2.0, 3, 1)
    assert tuple(rgb.shape) == (3, 96, 130, 3) and rgb.dtype == u8
    assert tuple(vert.shape) == (3, 96, 130) and vert.dtype == torch.int32
    rgb, vert = ns.scatter_points(m(1, 10, 3), None, None, None, 8, 8, 1.0, return_vertex=False)
    assert tuple(rgb.shape) == (1, 8, 8, 3) and vert.numel() == 0
    for bad in (lambda: ns.seg_colour(m(2, 4, 4, 33), m(32, 3, dt=u8), None, 8, 8),
                lambda: ns.seg_colour(m(2, 4, 4, 32), m(32, 3, dt=u8), None, 0, 8),
                lambda: ns.scatter_points(m(1, 10, 3), None, None, None, 8, 8, 1.0, 17),
                lambda: ns.scatter_points(m(1, 10, 3), None, m(9, 3, dt=u8), None, 8, 8, 1.0),
                lambda: ns.scatter_points(m(1, 10, 3), None, None, m(1, 8, 9, 3, dt=u8), 8, 8, 1.0)):
        with pytest.raises(RuntimeError):
            bad()
    with pytest.raises((RuntimeError, NotImplementedError)):
        ns.scatter_points(torch.zeros(1, 10, 3), None, None, None, 8, 8, 1.0)       # a CPU tensor: no kernel registered


def test_kernel_resources():
    """What the code objects say (no GPU): no scratch, registers for 8 waves per SIMD, and the LDS the design counts on -
    the 64 x 64 key buffer (32 KB: five workgroups per CU, the occupancy limit) and the 4 096 packed colours (16 KB)."""
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import kernel_resources as kr
    ks = {n: k for n, k in kr.kernels().items() if "seg_colour_kernel" in n or "scatter_points_kernel" in n}
    assert len(ks) == 2, sorted(ks)
    for name, k in ks.items():
        assert k["scratch"] == 0 and k["agpr"] == 0, name
        assert kr.waves_per_simd(k) == 8, name
        assert k["lds"] == (32768 if "scatter_points_kernel" in name else 16384), name
