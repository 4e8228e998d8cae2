"""Segmentation metrics on the GPU: the confusion kernel (csrc/metrics.hip) and the rasteriser's metrics epilogue
against a float64 NumPy restatement of evaluate.py's counts, bit for bit (integer counts), and their use through the
decoder, the trainer and evaluate_iou_and_acc."""
import numpy as np
import pytest
import torch

from _inputs import make_x
from test_gpu_parity import dev, t
from test_metrics_cpu import np_argmax

pytestmark = pytest.mark.gpu


def np_conf(gt, pred, C):
    """The (C + 1, C) counts restated: row = label (C for one outside [0, C)), column = prediction."""
    gt, pred = np.asarray(gt).reshape(-1).astype(np.int64), np.asarray(pred).reshape(-1).astype(np.int64)
    row = np.where((gt >= 0) & (gt < C), gt, C)
    out = np.zeros((C + 1, C), np.int64)
    np.add.at(out, (row, pred), 1)
    return out


def np_eval(conf_or_pair, C):
    gt, pred = conf_or_pair
    I = np.array([np.sum((gt == k) & (pred == k)) for k in range(1, C)], np.float64)
    U = np.array([np.sum((gt == k) | (pred == k)) for k in range(1, C)], np.float64)
    return I, U, float(np.sum(gt == pred)), gt.size


@pytest.mark.parametrize("C", [32, 2])
@pytest.mark.parametrize("B,W", [(1, 47), (128, 48), (1024, 64), (3, 33)])
def test_confusion_kernel_matches_the_restatement(B, W, C):
    from ilps_amd.metrics import SegConfusion
    rng = np.random.default_rng(B * 7 + W + C)
    scores = rng.random((B, W, W, C)).astype(np.float32)
    # planted ties, NaN, and values quantised so that ties occur everywhere
    scores[0, 0, 0, :] = 0.5
    scores[0, 0, 1, C - 1] = np.nan
    scores[0, 0, 2, :] = np.nan
    scores[0, 1, :, 1] = scores[0, 1, :, 0]
    if B > 1:
        scores[1] = np.round(scores[1] * 4) / 4
    gt = rng.integers(-2, C + 3, (B, W, W))
    m = SegConfusion(C, dev())
    m.update(t(scores), t(gt, torch.int32))
    pred = np_argmax(scores) if B * W * W <= 300000 else scores.argmax(-1)
    if B * W * W > 300000:                                 # (np.argmax is the restatement where no NaN was planted)
        pred[0] = np_argmax(scores[:1])[0]
    want = np_conf(gt, pred, C)
    got = m.counts.cpu().numpy()
    np.testing.assert_array_equal(got, want)
    assert got.sum() == B * W * W
    I, U, correct, total = np_eval((gt, pred), C)
    np.testing.assert_array_equal(m.intersections(), I)
    np.testing.assert_array_equal(m.unions(), U)
    assert m.correct() == correct and m.total() == total
    # the prediction-map form counts the same
    m2 = SegConfusion(C, dev()).update_maps(t(pred, torch.int32), t(gt, torch.int32))
    assert torch.equal(m2.counts, m.counts)
    # the torch op adds into its argument in place
    from ilps_amd import torch_ops
    if torch_ops.available():
        c3 = torch.zeros(C + 1, C, dtype=torch.int64, device=dev())
        torch_ops.load().seg_confusion(t(scores), t(gt, torch.int32), c3)
        assert torch.equal(c3, m.counts)


@pytest.mark.parametrize("C,offset", [(3, 0), (4, 0), (8, 0), (16, 0), (31, 0), (32, 1), (32, 2), (2, 1), (16, 3)])
@pytest.mark.parametrize("B,W", [(5, 33), (64, 48)])
def test_every_launch_form_matches_the_restatement(B, W, C, offset):
    """Each form of seg_confusion_kernel: the vector ones (C = 4, 8, 16, 32 with 16-B loads, C = 2 with 8-B loads) and
    the any-C one (C = 3, 31, and score tensors whose base is not aligned to the vector load: a view `offset` floats into
    its buffer)."""
    from ilps_amd.metrics import SegConfusion
    rng = np.random.default_rng(B + W + C + offset)
    scores = rng.random((B, W, W, C)).astype(np.float32)
    scores[0, 0, 0, :] = 0.5
    scores[0, 0, 1, C - 1] = np.nan
    scores[0, 0, 2, min(1, C - 1)] = scores[0, 0, 2, 0] = 2.0
    gt = rng.integers(-2, C + 3, (B, W, W))
    buf = torch.empty(B * W * W * C + offset, device=dev())
    view = buf[offset:].view(B, W, W, C)
    view.copy_(t(scores))
    assert (view.data_ptr() % 16 != 0) == (offset % 4 != 0)
    m = SegConfusion(C, dev()).update(view, t(gt, torch.int32))
    np.testing.assert_array_equal(m.counts.cpu().numpy(), np_conf(gt, np_argmax(scores), C))


@pytest.mark.parametrize("vs", [1, 5])
def test_fused_epilogue_counts_equal_the_kernel(smpl_model, vs):
    """B = 128, W = 48 through the decoder with the fused loss: vs = 1 takes the fused-skinning path, vs = 5 the two-call
    path.  The epilogue's counts equal the confusion kernel's on the keep_seg scores of the same call and the NumPy
    restatement; loss and gradient are bit-identical with and without counting (deterministic mode); 1 and 4 streams
    give the same counts."""
    from ilps_amd.decoder import SMPLDecoder
    from ilps_amd.focal_loss import softmax_focal_loss
    from ilps_amd.metrics import SegConfusion
    B, W = 128, 48
    x = make_x(B, W, seed=11 + vs)
    rng = np.random.default_rng(vs)
    lab_np = rng.integers(-1, 34, (B, W, W))
    lab = t(lab_np, torch.int64)
    res = {}
    for streams in (1, 4):
        dec = SMPLDecoder(smpl_model, img_wh=W, vertex_sampling=vs, outputs=(), loss=softmax_focal_loss(2.0, True),
                          keep_seg=True, deterministic=True, streams=streams)
        runs = []
        for with_m in (False, True):
            m = SegConfusion(32, dev()) if with_m else None
            xg = t(x).requires_grad_(True)
            out = dec(xg, lab, confusion=m)
            out["seg_loss"].sum().backward()
            torch.cuda.synchronize()
            runs.append((out, xg.grad.clone(), m))
        (o0, g0, _), (o1, g1, m) = runs
        assert torch.equal(o0["seg_loss"], o1["seg_loss"]) and torch.equal(g0, g1)
        assert torch.equal(o0["seg"], o1["seg"])
        k = SegConfusion(32, dev()).update(o1["seg"], lab)
        assert torch.equal(m.counts, k.counts), "epilogue counts differ from the kernel's (vs=%d, streams=%d)" % (vs, streams)
        want = np_conf(lab_np, o1["seg"].cpu().numpy().argmax(-1), 32)
        np.testing.assert_array_equal(m.counts.cpu().numpy(), want)
        assert int(m.counts.sum()) == B * W * W
        res[streams] = m.counts.clone()
    assert torch.equal(res[1], res[4])
    # without the scores written the counts are the same
    dec = SMPLDecoder(smpl_model, img_wh=W, vertex_sampling=vs, outputs=(), loss=softmax_focal_loss(2.0, True))
    m = SegConfusion(32, dev())
    with torch.no_grad():
        dec(t(x), lab, confusion=m)
    assert torch.equal(m.counts, res[1])


def test_decoder_without_fused_loss_uses_the_kernel(smpl_model):
    from ilps_amd.decoder import SMPLDecoder
    from ilps_amd.metrics import SegConfusion
    B, W = 4, 48
    dec = SMPLDecoder(smpl_model, img_wh=W)
    lab = torch.randint(0, 32, (B, W, W), device=dev())
    m = SegConfusion(32, dev())
    with torch.no_grad():
        out = dec(t(make_x(B, W, seed=5)), lab, confusion=m)
    want = np_conf(lab.cpu().numpy(), out["seg"].cpu().numpy().argmax(-1), 32)
    np.testing.assert_array_equal(m.counts.cpu().numpy(), want)


def test_legacy_rasteriser_refuses_counts():
    """SMPLR_RASTER=1 (the round-1 kernel, kept for A/B runs) has no metrics epilogue: a conf is refused - on the fused
    skinning path (vs = 1) before any launch, on the two-call path (vs = 5) after the binning - in a fresh process (the
    switch is read once).  Every operand is a real buffer of the decoder's own pass, so a missing refusal shows up as an
    assertion (counts left at zero), not as a launch on bad addresses."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = """
import sys, torch
sys.path.insert(0, "tests")
import ilps_amd
from _inputs import make_x
from ilps_amd.decoder import SMPLDecoder
from ilps_amd.focal_loss import softmax_focal_loss
from ilps_amd.metrics import SegConfusion
from ilps_amd.smpl_model import synthetic_smpl_model
dev = torch.device("cuda:0")
model = synthetic_smpl_model(1234)
for vs in (1, 5):
    dec = SMPLDecoder(model, img_wh=48, vertex_sampling=vs, outputs=(), loss=softmax_focal_loss(2.0, True))
    x = torch.as_tensor(make_x(2, 48, seed=vs), device=dev)
    lab = torch.randint(0, 32, (2, 48, 48), device=dev)
    m = SegConfusion(32, dev)
    try:
        with torch.no_grad():
            dec(x, lab, confusion=m)
        torch.cuda.synchronize()
        print("vs=%d accepted, counts %d" % (vs, m.total()))
    except RuntimeError as e:
        torch.cuda.synchronize()
        print("vs=%d refused %s counts %d" % (vs, "SMPLR_RASTER=1" in str(e), m.total()))
"""
    env = dict(os.environ, SMPLR_RASTER="1")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300, cwd=root)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "vs=1 refused True counts 0" in r.stdout and "vs=5 refused True counts 0" in r.stdout, r.stdout


def test_trainer_step_metrics(smpl_model):
    """Trainer.step(metrics=(seg, silhouette)) over two steps = the sum of the per-step counts; the silhouette head's
    counts match torch.argmax on out['silhouette'] (recomputed in eval mode on the monitor decoder)."""
    from ilps_amd.metrics import SegConfusion
    from ilps_amd.training import SegTrainer, fit
    B, W = 4, 48
    torch.manual_seed(3)
    images = torch.rand(B, 3, 256, 256, device=dev())
    labels = torch.randint(0, 32, (B, W, W), device=dev())
    silh_labels = torch.randint(0, 2, (B, W, W), device=dev())
    torch.manual_seed(0)
    tr = SegTrainer(smpl_model, output_wh=W, encoder_architecture="enet", use_IEF=True, device=dev(), with_silhouette=True)
    tr.smpl_model.eval()                                   # (fixed statistics: the recomputation below sees the same net)
    seg_m, silh_m = SegConfusion(32, dev()), SegConfusion(2, dev())
    per = []
    for _ in range(2):
        with torch.no_grad():
            o = tr.monitor(images)
        per.append((np_conf(labels.cpu().numpy(), o["seg"].cpu().numpy().argmax(-1), 32),
                    np_conf(silh_labels.cpu().numpy(), torch.argmax(o["silhouette"], -1).cpu().numpy(), 2)))
        tr.step(images, labels, silh_labels, metrics=(seg_m, silh_m))
    torch.cuda.synchronize()
    np.testing.assert_array_equal(seg_m.counts.cpu().numpy(), per[0][0] + per[1][0])
    np.testing.assert_array_equal(silh_m.counts.cpu().numpy(), per[0][1] + per[1][1])
    assert silh_m.total() == 2 * B * W * W
    # fit resets per trial and hands the metric to every step; its return keeps its form
    seen = []
    m = SegConfusion(32, dev())
    hist = fit(tr, iter([(images, labels)] * 4), trials=2, steps_per_trial=2, save_every=1,
               on_trial_end=lambda trial, trainer: seen.append(m.total()), metrics=m)
    assert len(hist) == 2 and all(isinstance(h, float) for h in hist)
    assert seen == [2 * B * W * W, 2 * B * W * W]


def test_evaluate_iou_and_acc_over_two_batches(smpl_model):
    from ilps_amd.decoder import SMPLDecoder
    from ilps_amd.evaluation import evaluate_iou_and_acc
    from ilps_amd.focal_loss import softmax_focal_loss
    from ilps_amd.model import SMPLRegressor
    W = 48
    torch.manual_seed(1)
    net = SMPLRegressor(W, "enet", True).to(dev())
    dec = SMPLDecoder(smpl_model, img_wh=W, outputs=(), loss=softmax_focal_loss(2.0, True))
    plain = SMPLDecoder(smpl_model, img_wh=W).share_constants(dec)
    batches = [(torch.rand(3, 3, 256, 256, device=dev()), torch.randint(0, 32, (3, W, W), device=dev())) for _ in range(2)]
    r = evaluate_iou_and_acc(net, dec, batches)
    net.eval()
    with torch.no_grad():
        preds = [plain(net(im))["seg"].cpu().numpy().argmax(-1) for im, _ in batches]
    gt = np.concatenate([g.cpu().numpy() for _, g in batches])
    pred = np.concatenate(preds)
    I, U, correct, total = np_eval((gt, pred), 32)
    np.testing.assert_array_equal(r["intersections"], I)
    np.testing.assert_array_equal(r["unions"], U)
    assert r["correct"] == correct and r["total"] == total == 6 * W * W
    assert r["accuracy"] == correct / total
    with np.errstate(invalid="ignore", divide="ignore"):
        np.testing.assert_equal(r["mean_iou"], np.mean(I / U))


def test_fused_loss_still_checks_class_weights(smpl_model):
    """DecoderOpts(loss=...) without confusion: a class-weight vector off the device, of another dtype or of the wrong
    length is refused before anything is launched (as before the metrics existed)."""
    from ilps_amd import ops
    B, W = 2, 48
    c = ops.SMPLConstants.from_model(smpl_model, dev())
    pt = ops.get_part_table(1, dev(), c.V)
    x = t(make_x(B, W, seed=1))
    lab = torch.randint(0, 32, (B, W, W), device=dev())
    for cw in (torch.ones(32), torch.ones(32, device=dev(), dtype=torch.float64), torch.ones(31, device=dev())):
        opts = ops.DecoderOpts(want_verts=False, want_proj=False, want_mask=False, want_seg=False, loss=(lab, cw, 2.0))
        with pytest.raises(RuntimeError, match="class_w"):
            ops.DecoderFn.apply(x, c, 4, W, 1, pt, 64, True, False, 1, False, opts)
