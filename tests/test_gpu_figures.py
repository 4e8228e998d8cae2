"""The HIP figure kernels (csrc/figure.hip through ilps_amd.figures and torch.ops.smplraster) against their NumPy
restatement (tests/_figures_oracle.py): every byte of rgb and every winner of vertex equal - the ordering is total and the
arithmetic integer, so nothing is exempt.  Shapes are small and sit where the kernels can break: one pixel, one short
of / exactly / one past the 64-pixel tile, a non-square picture over several tiles, one vertex, one short of / one past
the 256 threads of a workgroup, the full mesh."""
import numpy as np
import pytest
import torch

import _figures_oracle as fo
from ilps_amd import _lib, figures, torch_ops

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def via_torch_op(proj, img_wh, scale, radius=0, order="index", keep=None, colours=None, colour=figures.MPL_BLUE, image=None,
                 image_alpha=0.9, canvas=(255, 255, 255), return_vertex=False):
    """`figures.scatter_points`' call through torch.ops.smplraster.scatter_points."""
    W, H = img_wh
    pack = lambda c: c[0] | (c[1] << 8) | (c[2] << 16)
    rgb, vert = torch_ops.load().scatter_points(proj, keep, colours, image, H, W, scale, radius, figures.ORDERS.index(order),
                                                pack(colour), int(round(256 * image_alpha)), pack(canvas), return_vertex)
    return rgb, vert


@pytest.mark.parametrize("hw", fo.SEG_SRC)
@pytest.mark.parametrize("HW", fo.SEG_OUT)
def test_seg_colour_equals_oracle(hw, HW):
    fo.check_seg_colour(DEV, hw, HW)


def test_seg_colour_torch_op_and_unaligned_scores():
    """The torch op gives the bytes of the ctypes path; scores that do not start on 16 bytes take the scalar loads."""
    ns = torch_ops.load()
    B, h, w, H, W = 2, 5, 7, 63, 65
    s = fo.seg_scores(B, h, w, 32, 77)
    lut = figures.default_lut().to(DEV)
    bg = torch.from_numpy(fo.random_image(B, H, W, 4)).to(DEV)
    want = fo.seg_colour(s, H, W, background=bg.cpu().numpy(), alpha_q=77)
    got = ns.seg_colour(torch.from_numpy(s).to(DEV), lut, bg, H, W, 77, 0)
    assert np.array_equal(got.cpu().numpy(), want)
    flat = torch.empty(s.size + 1, dtype=torch.float32, device=DEV)
    flat[1:] = torch.from_numpy(s).to(DEV).reshape(-1)
    shifted = flat[1:].view(B, h, w, 32)
    assert shifted.data_ptr() % 16 == 4 and shifted.is_contiguous()
    got = ns.seg_colour(shifted, lut, bg, H, W, 77, 0)
    assert np.array_equal(got.cpu().numpy(), want)
    l = fo.seg_labels(B, h, w, 32, 9)
    got = ns.seg_colour(torch.from_numpy(l).to(DEV), lut, None, H, W, 256, 0x0201fa)
    assert np.array_equal(got.cpu().numpy(), fo.seg_colour(l, H, W, bad=(250, 1, 2)))
    assert ns.seg_colour(torch.empty(0, h, w, 32, device=DEV), lut, None, H, W).shape == (0, H, W, 3)


@pytest.mark.parametrize("HW", fo.SC_HW)
@pytest.mark.parametrize("r", fo.SC_R)
def test_scatter_equals_oracle(HW, r):
    fo.check_scatter(DEV, HW, r)


@pytest.mark.parametrize("HW,r", [((65, 65), 3), ((96, 130), 16), ((1, 1), 1)])
def test_scatter_torch_op_equals_oracle(HW, r):
    fo.check_scatter(DEV, HW, r, Vs=(1, 257, 6890), run=via_torch_op)


def test_scatter_sampled_vertices_inexact_scale():
    """predict.py:65's scale at 256 / 48 (no fp32 product is exact) on the 1 378 sampled projections."""
    fo.check_scatter(DEV, (96, 130), 1, Bs=(2,), Vs=(1378,), s=256.0 / 48.0)


def test_scatter_rows_do_not_depend_on_the_batch_and_runs_repeat():
    """At B = 128 row b equals the same mesh run alone, and a second run gives the same bits."""
    B, V, H, W, r = 128, 257, 65, 65, 3
    p = torch.from_numpy(fo.scatter_proj(B, V, H, W, r, 2.0, 5)).to(DEV)
    cols = torch.from_numpy(fo.vertex_colours(V, 5)).to(DEV)
    img = torch.from_numpy(fo.random_image(B, H, W, 5)).to(DEV)
    for order in figures.ORDERS:
        rgb, vert = figures.scatter_points(p, (W, H), 2.0, radius=r, order=order, colours=cols, image=img, return_vertex=True)
        rgb2, vert2 = figures.scatter_points(p, (W, H), 2.0, radius=r, order=order, colours=cols, image=img, return_vertex=True)
        assert torch.equal(rgb, rgb2) and torch.equal(vert, vert2)
        for b in (0, 63, 127):
            r1, v1 = figures.scatter_points(p[b:b + 1], (W, H), 2.0, radius=r, order=order, colours=cols, image=img[b:b + 1],
                                            return_vertex=True)
            assert torch.equal(r1[0], rgb[b]) and torch.equal(v1[0], vert[b]), (order, b)
        want = fo.scatter_vertex(p[127:].cpu().numpy(), H, W, 2.0, r, order)
        assert np.array_equal(vert[127:].cpu().numpy(), want)


def test_both_launches_replay_under_a_graph():
    """Neither launcher allocates or synchronises: captured once, the replay on new inputs gives the eager bits."""
    ns = torch_ops.load()
    B, V, H, W, r = 3, 6890, 96, 130, 3
    lib = _lib.load()
    p = [torch.from_numpy(fo.scatter_proj(B, V, H, W, r, 2.0, seed)).to(DEV) for seed in (1, 2)]
    s = [torch.from_numpy(fo.seg_scores(B, 48, 48, 32, seed)).to(DEV) for seed in (1, 2)]
    img = torch.from_numpy(fo.random_image(B, H, W, 5)).to(DEV)
    lut = figures.default_lut().to(DEV)
    eager = (figures.scatter_points(p[1], (W, H), 2.0, radius=r, order="depth", image=img, return_vertex=True),
             figures.seg_colour(s[1], (W, H), background=img))
    sp, ss = p[0].clone(), s[0].clone()
    rgb = torch.empty((B, H, W, 3), dtype=torch.uint8, device=DEV)
    vert = torch.empty((B, H, W), dtype=torch.int32, device=DEV)
    seg = torch.empty((B, H, W, 3), dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        st = _lib.stream()
        _lib.check(lib.smplr_scatter_points(_lib.ptr(sp), None, None, 0xb4771f, _lib.ptr(img), 230, 0xffffff, B, V, 2.0, r, 1, H,
                                            W, _lib.ptr(vert), _lib.ptr(rgb), st), "smplr_scatter_points")
        _lib.check(lib.smplr_seg_colour(_lib.ptr(ss), None, B, 48, 48, 32, _lib.ptr(lut), 32, 0, _lib.ptr(img), 128, H, W,
                                        _lib.ptr(seg), st), "smplr_seg_colour")
        op_rgb, op_vert = ns.scatter_points(sp, None, None, img, H, W, 2.0, r, 1)
    sp.copy_(p[1])
    ss.copy_(s[1])
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(rgb, eager[0][0]) and torch.equal(vert, eager[0][1]) and torch.equal(seg, eager[1])
    assert torch.equal(op_rgb, eager[0][0]) and torch.equal(op_vert, eager[0][1])


def test_empty_batch_and_missing_outputs():
    assert figures.scatter_points(torch.empty(0, 10, 3, device=DEV), 8, 1.0).shape == (0, 8, 8, 3)
    assert figures.seg_colour(torch.empty(0, 4, 4, 2, device=DEV), 8).shape == (0, 8, 8, 3)
    rgb, vert = torch_ops.load().scatter_points(torch.zeros(1, 10, 3, device=DEV), None, None, None, 8, 8, 1.0, return_vertex=False)
    assert vert.numel() == 0 and rgb[0, 7, 0].tolist() == list(figures.MPL_BLUE) and rgb[0, 0, 0].tolist() == [255, 255, 255]
    with pytest.raises(RuntimeError, match="lives on"):
        figures.scatter_points(torch.zeros(1, 10, 3, device=DEV), 8, 1.0, keep=torch.ones(1, 10, dtype=torch.uint8))


def test_prediction_figures_end_to_end(smpl_model, part_tables):
    """`prediction_figures` on `predict_batch`'s output of a small synthetic model, B = 2: the oracle applied to the same pred."""
    from ilps_amd.decoder import SMPLDecoder
    from ilps_amd.inference import predict_batch
    from ilps_amd.model import SMPLRegressor
    torch.manual_seed(0)
    W, S, N = 48, 64, 2
    net = SMPLRegressor(W, "enet", True).to(DEV)
    dec = SMPLDecoder(smpl_model, img_wh=W)
    images = torch.rand(N, 3, 256, 256, device=DEV)                           # (the ENet encoder takes 256 x 256 inputs)
    pred = predict_batch(net, dec, images)
    figs = figures.prediction_figures(pred, images, W, part_tables=part_tables[1], size=S, radius=1)
    proj = pred["projects"].cpu().numpy()
    scores = pred["segs"].cpu().numpy()
    pick = (np.arange(S) * 256) // S
    img = figures.as_uint8_images(images.cpu()).numpy()[:, pick][:, :, pick]
    cols = figures.part_colours(part_tables[1], proj.shape[1]).numpy()
    win = fo.scatter_vertex(proj, S, S, np.float32(S / W), 1, "index")
    assert (win >= 0).any()
    assert sorted(figs) == ["input", "projects", "seg", "seg_overlay", "verts_overlay"]
    assert np.array_equal(figs["input"].cpu().numpy(), img)
    assert np.array_equal(figs["seg"].cpu().numpy(), fo.seg_colour(scores, S, S))
    assert np.array_equal(figs["seg_overlay"].cpu().numpy(), fo.seg_colour(scores, S, S, background=img, alpha_q=128))
    assert np.array_equal(figs["projects"].cpu().numpy(), fo.scatter_rgb(win, cols))
    assert np.array_equal(figs["verts_overlay"].cpu().numpy(), fo.scatter_rgb(win, cols, image=img))
    panel = figures.prediction_panel(pred, images, W, part_tables=part_tables[1], size=S, radius=1)
    assert tuple(panel.shape) == (N, S, 5 * S, 3) and torch.equal(panel[:, :, 4 * S:], figs["seg_overlay"])
