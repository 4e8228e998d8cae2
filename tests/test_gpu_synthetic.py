"""csrc/proxy.hip through `ilps_amd.synthetic` on the GPU, against tests/_synthetic_oracle.py: seg channels and heat
decisions bit for bit, heat values within the exponential's error; row independence; the torch op; and the loop around it
(`SyntheticBatches`) feeding `SegTrainer.step`, `training.fit` and `evaluate_3d`.

Heat tolerance: the oracle reproduces the exponential's fp32 argument exactly, so only the device's expf differs from
float64's exp; HIP documents expf at 1-2 ulp, <= 2.4e-7 on values <= 1, and 1e-6 leaves 4x over that.
Measured on an MI355X (this file's cases): largest heat difference 4.5e-8."""
import numpy as np
import pytest
import torch

import _synthetic_oracle as so
from ilps_amd import synthetic as syn
from _synthetic_oracle import HEAT_TOL, as_tensors, compare

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def run(case, seg, out=None):
    return syn.proxy_inputs(**as_tensors(case, DEV), num_parts=case["P"], seg=seg, sigma=case["sigma"], out=out)


@pytest.mark.parametrize("seg", list(so.SEG_MODES))
@pytest.mark.parametrize("hw", so.SHAPES)
def test_kernel_equals_the_oracle(hw, seg):
    worst = 0.0
    for i, case in enumerate(so.case_grid(*hw)):
        if seg == "none" and case["joints"] is None:
            continue
        got = run(case, seg)
        assert got.is_contiguous() and got.device == DEV
        worst = max(worst, compare(got.cpu().numpy(), case, seg, "%s %s case %d" % (hw, seg, i)))
    print("proxy_inputs %s %s: largest heat difference %.3g (bound %.1g)" % (hw, seg, worst, HEAT_TOL))


@pytest.mark.parametrize("seg", list(so.SEG_MODES))
def test_one_column_path_at_W8_through_an_offset_view(seg):
    """W = 8 takes the 16-B path; an `out` that starts 4 B off a 16-B boundary must take the one-column path, and give the
    same bits."""
    for i, case in enumerate(so.case_grid(8, 8)):
        if seg == "none" and case["joints"] is None:
            continue
        want = run(case, seg)
        n = want.numel()
        flat = torch.full((n + 8,), -7.0, dtype=torch.float32, device=DEV)
        view = flat[1:1 + n].view(want.shape)
        assert view.data_ptr() % 16 == 4 and want.data_ptr() % 16 == 0
        got = run(case, seg, out=view)
        assert got.data_ptr() == view.data_ptr() and torch.equal(got.view(torch.int32), want.view(torch.int32)), i
        assert float(flat[0]) == -7.0 and (flat[1 + n:] == -7.0).all()                # nothing written around the view
        compare(got.cpu().numpy(), case, seg, "offset view, %s case %d" % (seg, i))


def test_joint_on_a_pixel_centre_is_bit_equal_to_one():
    part = torch.zeros((2, 9, 12), dtype=torch.uint8, device=DEV)
    joints = torch.tensor([[[5.0, 4.0], [0.0, 0.0]], [[11.0, 8.0], [2.5, 2.5]]], device=DEV)
    for sigma in (0.5, 4.0):
        out = syn.proxy_inputs(part, joints, seg="none", sigma=sigma).cpu()
        one = torch.tensor(1.0).view(torch.int32)
        assert out[0, 0, 4, 5].view(torch.int32) == one and out[0, 1, 0, 0].view(torch.int32) == one
        assert out[1, 0, 8, 11].view(torch.int32) == one and float(out[1, 1].max()) < 1.0


def test_rows_are_independent():
    """A hostile row (NaN joints, every class removed, a box over everything) leaves the other rows' bits alone."""
    H, W, B, J = 6, 12, 4, 5
    case = so.make_case(H, W, B, J, 31, 2, 1)
    case["keep"] = None
    case["remove"] = np.array([0, -1, 1 << 3, 0], np.int32)
    case["joints"][1] = np.nan
    case["boxes"][1] = (-10, -10, W + 10, H + 10)
    for seg in so.SEG_MODES:
        full = run(case, seg)
        hostile = full[1].cpu().numpy()
        cseg = syn.seg_channels(seg)                                     # all background, all heat off
        assert not hostile[cseg:].any() and not hostile[int(seg == "onehot"):cseg].any(), seg
        assert seg != "onehot" or (hostile[0] == 1).all()
        for b in (0, 2, 3):
            alone = {k: (v[b:b + 1] if isinstance(v, np.ndarray) else v) for k, v in case.items()}
            assert torch.equal(run(alone, seg)[0].view(torch.int32), full[b].view(torch.int32)), (seg, b)


def test_torch_op_equals_the_ctypes_path():
    from ilps_amd import torch_ops
    ns = torch_ops.load()
    for hw in ((8, 8), (5, 7)):
        for case in list(so.case_grid(*hw))[4::5]:
            t = as_tensors(case, DEV)
            J = 0 if t["joints"] is None else t["joints"].shape[1]
            for seg, mode in so.SEG_MODES.items():
                if seg == "none" and J == 0:
                    continue
                want = run(case, seg)
                out = torch.full_like(want, -3.0)
                inv2s2, cut2 = syn.heat_constants(case["sigma"])
                ns.proxy_inputs(t["part"], t["joints"], t["keep"], t["remove"], t["boxes"], out, case["P"], mode,
                                1.0 / case["P"], inv2s2, cut2)
                assert torch.equal(out.view(torch.int32), want.view(torch.int32)), (hw, seg)
    with pytest.raises(RuntimeError):
        ns.proxy_inputs(t["part"], None, None, None, None, torch.empty((1, 1, 2, 2), device=DEV), 31, 0, 1.0, 0.5, 36.0)


def test_device_torch_restatement_equals_the_kernel():
    """`proxy_inputs_torch` on the device (the timing baseline) computes the same thing: seg bits, heat within the bound."""
    case = so.make_case(9, 12, 3, 6, 31, 2, 3)
    t = as_tensors(case, DEV)
    for seg in so.SEG_MODES:
        a = run(case, seg)
        b = syn.proxy_inputs_torch(**t, num_parts=31, seg=seg, sigma=case["sigma"])
        cseg = syn.seg_channels(seg)
        assert torch.equal(a[:, :cseg], b[:, :cseg]) and torch.equal(a[:, cseg:] != 0, b[:, cseg:] != 0)
        assert float((a - b).abs().max()) <= HEAT_TOL


# ---- the loop ---------------------------------------------------------------------------------------------------------------
FILL = (0.6, 0.9)


@pytest.fixture(scope="module")
def setup(smpl_model):
    from ilps_amd.keras_smpl.batch_smpl import SMPLLayer
    from ilps_amd.keypoints import KeypointSpec
    layer = SMPLLayer(smpl_model)
    return {"layer": layer, "topo": syn.hull_topology(smpl_model), "spec": KeypointSpec.from_model(layer, "cocoplus")}


def batches_for(setup, B=4, input_wh=32, output_wh=16, **kw):
    kw.setdefault("spec", setup["spec"])
    kw.setdefault("sampler", syn.BodySampler(setup["layer"], fill=FILL))
    return syn.SyntheticBatches(setup["layer"], B, input_wh, output_wh, topology=setup["topo"], device=DEV, **kw)


def test_loop_clean_batch(setup):
    from ilps_amd.render import render_mesh
    bt = batches_for(setup, sigma=1.5)
    images, labels = next(bt)
    K = setup["spec"].K
    assert bt.in_channels == 1 + K and images.shape == (4, 1 + K, 32, 32) and images.dtype == torch.float32
    assert images.is_contiguous() and labels.shape == (4, 16, 16) and labels.dtype == torch.int32
    x, verts = bt.last["x"], bt.last["verts"]
    part32 = render_mesh(verts, setup["topo"], x[:, :4], mode="ortho", img_wh=32, scale=2.0)["part"]
    part16 = render_mesh(verts, setup["topo"], x[:, :4], mode="ortho", img_wh=16)["part"]
    rescale = torch.tensor(1.0 / 31, dtype=torch.float32, device=DEV)
    assert torch.equal(images[:, 0], part32.to(torch.float32) * rescale)              # bit for bit
    assert torch.equal(labels, part16.to(torch.int32)) and int((part32 > 0).sum()) > 0
    # every kept joint with a finite position inside the image has its channel's maximum at the rounded joint
    joints, heat = bt.last["joints"].cpu(), images[:, 1:].cpu()
    seen = 0
    for b in range(4):
        for k in range(K):
            jx, jy = joints[b, k].tolist()
            if np.isfinite([jx, jy]).all() and -0.5 < jx < 31.5 and -0.5 < jy < 31.5:
                at = int(heat[b, k].argmax())
                assert (at % 32, at // 32) == (int(np.floor(jx + 0.5)), int(np.floor(jy + 0.5))), (b, k, jx, jy)
                seen += 1
    assert seen >= 2 * K
    # the framing: the foreground's longer side lies in [fill_lo W - 2, fill_hi W + 2] (a pixel of rasterisation per side)
    fg = (part32 > 0).cpu().numpy()
    for b in range(4):
        ys, xs = np.nonzero(fg[b])
        side = max(np.ptp(xs), np.ptp(ys)) + 1
        print("sample %d: foreground %d px of 32 (fill %.1f .. %.1f)" % (b, side, *FILL))
        assert FILL[0] * 32 - 2 <= side <= FILL[1] * 32 + 2, (b, side)


def test_loop_repeats_from_its_seed_and_corrupts(setup):
    kw = dict(corruption=dict(remove_parts=(1, 2, 3, 4), remove_prob=0.5, swap_pairs=((0, 1),), box_prob=1.0), silh_wh=8,
              seg="onehot", seed=7)
    a, b = batches_for(setup, **kw), batches_for(setup, **kw)
    for _ in range(2):
        ba, bb = next(a), next(b)
        assert len(ba) == 3
        for ta, tb in zip(ba, bb):
            assert torch.equal(ta, tb)
    images, labels, silh = ba
    K = setup["spec"].K
    assert a.in_channels == 32 + K and images.shape == (4, 32 + K, 32, 32) and silh.shape == (4, 8, 8)
    assert set(silh.unique().tolist()) <= {0, 1} and torch.equal(images[:, :32].sum(1), torch.ones_like(images[:, 0]))
    d = a.last["draws"]
    assert set(d) == set(syn.DRAW_KEYS) and a.last["keep"] is d["keep"]
    # the occluder (present in every sample here) is background in the input and leaves the labels clean
    x0, y0, x1, y1 = d["boxes"][0, 0].tolist()
    assert x1 > x0 and y1 > y0 and bool((images[0, 0, y0:y1, x0:x1] == 1).all())
    c = batches_for(setup, seed=8, **{k: v for k, v in kw.items() if k != "seed"})
    assert not torch.equal(next(c)[0], ba[0])


def test_truth_and_eval_batches_feed_the_evaluators(setup, smpl_model):
    from ilps_amd.decoder import SMPLDecoder
    from ilps_amd.evaluation import evaluate_3d, evaluate_iou_and_acc
    from ilps_amd.model import SMPLRegressor
    torch.manual_seed(0)
    bt = batches_for(setup, B=2, input_wh=256, output_wh=16, corruption={})
    net = SMPLRegressor(16, "enet", True, in_channels=bt.in_channels).to(DEV)
    pairs = list(bt.truth_batches(2))
    assert len(pairs) == 2 and pairs[0][1][0].shape == (2, 72) and pairs[0][1][1].shape == (2, 10)
    assert bt.last["draws"] is None                                     # uncorrupted
    res = evaluate_3d(net, setup["layer"], pairs)
    assert np.isfinite(res["pve"]) and res["count"] == 4 and np.isfinite(res["pose_mse"])
    from ilps_amd.focal_loss import softmax_focal_loss
    dec = SMPLDecoder(smpl_model, img_wh=16, outputs=(), loss=softmax_focal_loss(2.0, True))
    acc = evaluate_iou_and_acc(net, dec, bt.eval_batches(1))
    assert 0.0 <= float(acc["accuracy"]) <= 1.0 and int(acc["total"]) == 2 * 16 * 16


def test_training_on_synthetic_batches(setup, smpl_model):
    from ilps_amd.training import SegTrainer, fit
    torch.manual_seed(0)
    bt = batches_for(setup, B=2, input_wh=256, output_wh=48, corruption={})
    tr = SegTrainer(smpl_model, input_wh=256, output_wh=48, in_channels=bt.in_channels, device=DEV)
    assert tr.smpl_model.backbone.enet.init_conv.weight.shape[1] == bt.in_channels
    w0 = tr.smpl_model.backbone.enet.init_conv.weight.detach().clone()
    loss = tr.step(*next(bt))
    assert np.isfinite(float(loss)) and not torch.equal(tr.smpl_model.backbone.enet.init_conv.weight.detach(), w0)
    hist = fit(tr, bt, trials=1, steps_per_trial=2)
    assert len(hist) == 1 and isinstance(hist[0], float) and np.isfinite(hist[0])
