"""The fused silhouette loss head on the GPU (csrc/silh_loss.hip, silh_px_kernel's loss epilogue, ops.DecoderFn,
SMPLDecoder(silh_loss=...), SegTrainer(fused_silh_loss=True)): the stage against the float64 formula
(tests/_silh_loss_oracle.py) and the unfused head, the confusion counts against metrics.seg_confusion, the backward
against smplr_silh_bwd and the float64 VJP, hostile rows, the decoder, the trainer and the torch ops.  Every comparison
prints the worst error it met."""
import numpy as np
import pytest
import torch

import _silh_loss_oracle as slo
from _inputs import make_x
from test_gpu_parity import dev, grad_close, t
from test_gpu_silhouette import PARK, V, bodies, form, layer, pad, px_last, vjp_check  # noqa: F401  (layer: a fixture)

pytestmark = pytest.mark.gpu

PARAMS = [(0.0, False), (2.0, False), (2.0, True)]            # (gamma, weighted)
# name -> (B, W, VP): forms 0, 2, 3 and 1 of smplr_silh_fwd_form, then partial 8 x 8 tiles with four workgroups per mesh
SHAPES = {"W48": (3, 48, V), "W50": (3, 50, V), "W97": (3, 97, V), "W48-fused": (3, 48, "px_last+1"), "W5": (1, 5, V),
          "W7": (1, 7, V)}
LOSS_RTOL, LOSS_ATOL = 1e-4, 1e-7         # test_gpu_loss_fused.py's bar for the same fp32 softmax + log
K_RTOL, K_ATOL = 2e-5, 1e-9               # ... and its bar for the rasteriser's `stats`
E2E_RTOL, E2E_ATOL = 2e-3, 1e-6           # against the float64 rasteriser's scores
UNFUSED_RTOL = 1e-5                       # against SoftmaxFocalFn on the written silhouette


def weights(weighted):
    from ilps_amd.focal_loss import class_weights
    return class_weights(dev())[:2].contiguous() if weighted else None


def make_labels(silh, seed):
    """(B, W, W) int32 on the device: half random in {0, 1}, half s > 0.5, a few -1, 2 and 255."""
    s = silh[..., 1].cpu().numpy()
    rng = np.random.default_rng(seed)
    lab = np.where(rng.random(s.shape) < 0.5, rng.integers(0, 2, s.shape), s > 0.5).astype(np.int32)
    flat = lab.reshape(-1)
    n = 3 if flat.size < 100 else 12
    pos = rng.choice(flat.size, n, replace=False)
    flat[pos] = np.resize(np.array([-1, 2, 255], np.int32), n)
    return t(lab, torch.int32)


_STAGE = {}


def stage(layer, name):
    """Per shape, computed once: projections, the plain forward, labels and the float64 rasteriser's scores."""
    if name not in _STAGE:
        from ilps_amd import ops
        from oracle import np_oracle as o
        B, W, VP = SHAPES[name]
        proj = bodies(layer, B, W, 4000 + W)
        if VP == "px_last+1":
            proj = pad(proj, px_last() + 1)
        silh, arg = ops._silh_fwd(proj, W)
        s64 = o.projects_to_silhouette(proj.cpu().numpy().astype(np.float64), W)[..., 1]
        _STAGE[name] = dict(B=B, W=W, proj=proj, silh=silh, arg=arg, labels=make_labels(silh, W), s64=s64)
    return _STAGE[name]


def rel_excess(got, want, rtol, atol):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float((np.abs(got - want) / (rtol * np.abs(want) + atol)).max())


def test_the_shapes_reach_every_form():
    forms = [form(px_last() + 1 if vp == "px_last+1" else vp, W) for _, W, vp in SHAPES.values()]
    assert forms == [0, 2, 3, 1, 0, 0]


@pytest.mark.parametrize("gamma,weighted", PARAMS, ids=["ce", "focal", "focal-weighted"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_stage_parity(layer, monkeypatch, name, gamma, weighted):
    from ilps_amd import ops
    from ilps_amd.focal_loss import softmax_focal_loss
    st = stage(layer, name)
    W, proj, labels, cw = st["W"], st["proj"], st["labels"], weights(weighted)
    tag = "%s gamma=%g weighted=%s" % (name, gamma, weighted)
    monkeypatch.delenv("SMPLR_SILH_LOSS_EPILOGUE", raising=False)
    silh, arg, loss, k = ops._silh_fwd_loss(proj, W, labels, cw, gamma)
    assert torch.equal(silh, st["silh"]) and torch.equal(arg, st["arg"]), "%s: silh / arg differ from _silh_fwd" % tag
    loss1, k1 = ops._silh_loss_fwd(st["silh"], labels, cw, gamma)
    assert torch.equal(loss, loss1) and torch.equal(k, k1), "%s: smplr_silh_fwd_loss differs from smplr_silh_loss_fwd" % tag
    for env in ("0", "1"):
        monkeypatch.setenv("SMPLR_SILH_LOSS_EPILOGUE", env)
        s2, a2, l2, k2 = ops._silh_fwd_loss(proj, W, labels, cw, gamma)
        assert torch.equal(s2, silh) and torch.equal(a2, arg) and torch.equal(l2, loss) and torch.equal(k2, k), \
            "%s: SMPLR_SILH_LOSS_EPILOGUE=%s differs from the default" % (tag, env)
    monkeypatch.delenv("SMPLR_SILH_LOSS_EPILOGUE", raising=False)
    w2 = slo.FOCAL_W2 if weighted else None
    sn, lab = silh.cpu().numpy(), labels.cpu().numpy()
    L, K = loss.cpu().numpy().reshape(lab.shape), k.cpu().numpy().reshape(lab.shape)
    L64, K64 = slo.silh_loss(sn[..., 1], lab, gamma, w2, z0=sn[..., 0])
    e_l, e_k = rel_excess(L, L64, LOSS_RTOL, LOSS_ATOL), rel_excess(K, K64, K_RTOL, K_ATOL)
    Le, _ = slo.silh_loss(st["s64"], lab, gamma, w2)
    e_e = rel_excess(L, Le, E2E_RTOL, E2E_ATOL)
    unf = softmax_focal_loss(gamma, weighted)(labels, silh).cpu().numpy().reshape(lab.shape)
    d_u = np.abs(L - unf.astype(np.float64))
    e_u = float((d_u / np.maximum(UNFUSED_RTOL * np.abs(unf), 1e-300)).max()) if d_u.max() > 0 else 0.0
    print("%s: loss err/bar %.3g (1e-4 rel + 1e-7), k err/bar %.3g (2e-5 rel + 1e-9), end to end err/bar %.3g (2e-3 rel + "
          "1e-6), against the unfused head err/bar %.3g (1e-5 rel; max abs diff %.2e)" % (tag, e_l, e_k, e_e, e_u, d_u.max()))
    assert e_l <= 1.0 and e_k <= 1.0 and e_e <= 1.0 and e_u <= 1.0, tag
    out = (lab != 0) & (lab != 1)
    assert out.sum() >= 3 and np.all(L[out] == 0) and np.all(K[out] == 0), "%s: labels outside {0, 1} must give 0 / 0" % tag
    assert np.all(L[~out] > 0) and np.all(K[~out] != 0)


# ------------------------------------------------------------------------------------------------------- confusion
@pytest.mark.parametrize("B,W", [(1, 5), (3, 48), (130, 48), (256, 48)])
def test_confusion_counts_equal_the_metrics_kernel(layer, monkeypatch, B, W):
    """(3, 2) counts of both routes, after two accumulating calls, against metrics.seg_confusion on the written
    silhouette (exact); B = 130 / 256: two / one workgroups per mesh in silh_px_kernel."""
    from ilps_amd import ops
    from ilps_amd.metrics import SegConfusion, seg_confusion
    proj = bodies(layer, B, W, 900 + B)
    silh, _ = ops._silh_fwd(proj, W)
    labels = make_labels(silh, B)
    want = seg_confusion(silh, labels, SegConfusion(2, dev()).counts)
    assert int(want.sum()) == B * W * W and int(want[2].sum()) >= 3
    assert np.array_equal(want.cpu().numpy(), slo.confusion(silh.cpu().numpy(), labels.cpu().numpy()))
    for env in ("0", "1", None):
        if env is None:
            monkeypatch.delenv("SMPLR_SILH_LOSS_EPILOGUE", raising=False)
        else:
            monkeypatch.setenv("SMPLR_SILH_LOSS_EPILOGUE", env)
        m = SegConfusion(2, dev())
        ops._silh_fwd_loss(proj, W, labels, None, 0.0, conf=m.counts)
        assert torch.equal(m.counts, want), "epilogue=%s: %s != %s" % (env, m.counts.tolist(), want.tolist())
        ops._silh_fwd_loss(proj, W, labels, None, 0.0, conf=m.counts)
        assert torch.equal(m.counts, 2 * want), "epilogue=%s: second call does not accumulate" % env
    m = SegConfusion(2, dev())
    ops._silh_loss_fwd(silh, labels, None, 2.0, conf=m.counts)
    assert torch.equal(m.counts, want)
    print("B=%d W=%d: counts %s on both routes and the stand-alone kernel" % (B, W, want.tolist()))


def test_confusion_with_two_streams(smpl_model):
    from ilps_amd.decoder import SMPLDecoder
    from ilps_amd.focal_loss import softmax_focal_loss
    from ilps_amd.metrics import SegConfusion, seg_confusion
    B, W = 5, 48
    x = t(make_x(B, W, seed=61))
    dec = SMPLDecoder(smpl_model, img_wh=W, heads=("silhouette",), silh_loss=softmax_focal_loss(0.0, False), streams=2)
    silh = dec(x)["silhouette"]
    labels = make_labels(silh, 61)
    want = seg_confusion(silh, labels, SegConfusion(2, dev()).counts)
    m = SegConfusion(2, dev())
    out = dec(x, silh_labels=labels, silh_confusion=m)
    torch.cuda.synchronize()
    assert torch.equal(out["silhouette"], silh) and torch.equal(m.counts, want)
    dec(x, silh_labels=labels.long(), silh_confusion=m.counts)
    assert torch.equal(m.counts, 2 * want)


# -------------------------------------------------------------------------------------------------------- backward
@pytest.mark.parametrize("B,W", [(3, 48), (128, 48), (3, 50)])
def test_backward_equals_silh_bwd_and_the_float64_vjp(layer, B, W):
    from ilps_amd import ops
    proj = bodies(layer, B, W, 300 + B + W)
    silh, arg = ops._silh_fwd(proj, W)
    labels = make_labels(silh, B + W)
    loss, k = ops._silh_loss_fwd(silh, labels, weights(True), 2.0)
    dloss = torch.randn(B, W * W, generator=torch.Generator().manual_seed(B)).to(dev())
    g = (dloss * k).reshape(B, W, W)                                  # one fp32 multiply per pixel, as the kernel forms it
    dsilh = torch.stack([torch.zeros_like(g), g], dim=-1).contiguous()
    rows = sorted({0, B // 2, B - 1})
    p64, a = proj[rows].cpu().numpy().astype(np.float64), arg[rows].cpu().numpy()
    for det in (True, False):
        d = ops._silh_loss_bwd(dloss, k, silh, arg, proj, W, det)
        if det:
            want = ops._silh_bwd(dsilh, silh, arg, proj, W, True)
            assert torch.equal(d, want), "B=%d W=%d: deterministic _silh_loss_bwd differs from _silh_bwd on (0, dloss k)" % (B, W)
        # (vjp_check also asserts: z column 0, rows of vertices that win no pixel exactly 0)
        vjp_check(d[rows].cpu().numpy(), p64, dsilh[rows].cpu().numpy(), W, a, "loss bwd B=%d W=%d%s" % (B, W, " det" if det else ""),
                  det)


# ---------------------------------------------------------------------------------------------------- hostile rows
def test_hostile_rows_do_not_touch_their_neighbours(layer):
    from ilps_amd import ops
    B, W = 4, 48
    proj = bodies(layer, B, W, 77).clone()
    proj[1] = float("nan")
    proj[3] = PARK
    ref, _ = ops._silh_fwd(bodies(layer, B, W, 77), W)
    labels = make_labels(ref, 5)
    labels[1].clamp_(0, 1)
    dloss = torch.randn(B, W * W, generator=torch.Generator().manual_seed(4)).to(dev())
    silh, arg, loss, k = ops._silh_fwd_loss(proj, W, labels, None, 2.0)
    d = ops._silh_loss_bwd(dloss, k, silh, arg, proj, W, True)
    assert bool(torch.isnan(loss[1]).all()) and bool(torch.isnan(k[1]).all()), "the all-NaN mesh's loss and k are NaN"
    assert bool(torch.isfinite(loss[3]).all()) and float(silh[3, ..., 1].max()) == 0.0
    for r in (0, 2):
        p1, l1 = proj[r:r + 1].contiguous(), labels[r:r + 1].contiguous()
        s1, a1, loss1, k1 = ops._silh_fwd_loss(p1, W, l1, None, 2.0)
        assert torch.equal(loss1, loss[r:r + 1]) and torch.equal(k1, k[r:r + 1]), "row %d alone: loss / k differ" % r
        d1 = ops._silh_loss_bwd(dloss[r:r + 1].contiguous(), k1, s1, a1, p1, W, True)
        assert torch.equal(d1, d[r:r + 1]) and bool(torch.isfinite(d1).all()), "row %d alone: deterministic dproj differs" % r


# --------------------------------------------------------------------------------------------------------- decoder
@pytest.mark.parametrize("heads,WS,streams,det", [(("silhouette",), 48, 1, False), (("silhouette",), 32, 1, False),
                                                  (("seg", "silhouette"), 48, 1, False), (("seg", "silhouette"), 32, 2, True)],
                         ids=["silh-48", "silh-32", "both-48", "both-32-streams2-det"])
def test_decoder_gradient_equals_the_unfused_decoder(smpl_model, heads, WS, streams, det):
    from ilps_amd.decoder import SMPLDecoder
    from ilps_amd.focal_loss import softmax_focal_loss
    W, B = 48, 3
    ce, focal = softmax_focal_loss(0.0, False), softmax_focal_loss(2.0, True)
    kw = dict(img_wh=W, silh_wh=WS, heads=heads, streams=streams, deterministic=det, loss=focal if "seg" in heads else None)
    fused = SMPLDecoder(smpl_model, silh_loss=ce, **kw)
    plain = SMPLDecoder(smpl_model, **kw).share_constants(fused)
    x = make_x(B, W, seed=500 + WS)
    with torch.no_grad():
        silh0 = plain(t(x))["silhouette"]
    sl = make_labels(silh0, WS)
    lab = torch.randint(0, 32, (B, W, W), generator=torch.Generator().manual_seed(1)).to(dev()) if "seg" in heads else None
    grads, losses = [], []
    for dec in (fused, plain):
        xg = t(x).requires_grad_(True)
        if dec is fused:
            out = dec(xg, lab, silh_labels=sl)
            assert out["silh_loss"].shape == (B, WS * WS) and not out["silhouette"].requires_grad
            assert torch.equal(out["silhouette"], silh0)
            loss = out["silh_loss"].mean()
        else:
            out = dec(xg, lab)
            loss = ce(sl, out["silhouette"]).mean()
        if "seg" in heads:
            loss = loss + out["seg_loss"].mean()
        loss.backward()
        grads.append(xg.grad.cpu().numpy())
        losses.append(float(loss.detach()))
    err = float(np.abs(grads[0] - grads[1]).max() / np.abs(grads[1]).max())
    print("decoder %s silh_wh=%d: loss %.7f / %.7f, dx max|diff|/max|ref| %.2e = %.3g x the bar 2e-3"
          % ("+".join(heads), WS, losses[0], losses[1], err, err / 2e-3))
    assert abs(losses[0] - losses[1]) <= 1e-5 * abs(losses[1])
    grad_close(grads[0], grads[1], name="dx fused against unfused (%s, silh_wh=%d)" % ("+".join(heads), WS))


def test_decoder_without_silh_labels_is_unchanged(smpl_model):
    from ilps_amd import ops
    from ilps_amd.decoder import SMPLDecoder
    from ilps_amd.focal_loss import softmax_focal_loss
    W, B = 48, 3
    x = make_x(B, W, seed=9)
    new = SMPLDecoder(smpl_model, img_wh=W, heads=("seg", "silhouette"), deterministic=True, silh_loss=softmax_focal_loss(0.0, False))
    old = SMPLDecoder(smpl_model, img_wh=W, heads=("seg", "silhouette"), deterministic=True).share_constants(new)
    g = torch.randn(B, W, W, 2, generator=torch.Generator().manual_seed(2)).to(dev())
    res = []
    for dec in (new, old):
        xg = t(x).requires_grad_(True)
        out = dec(xg)
        assert "silh_loss" not in out and out["silhouette"].requires_grad
        ((out["silhouette"] * g).sum() + out["seg"].square().sum()).backward()
        res.append((out, xg.grad))
    for key in res[1][0]:
        assert torch.equal(res[0][0][key], res[1][0][key]), key
    assert torch.equal(res[0][1], res[1][1])
    c = new.constants(dev())
    pt = ops.get_part_table(1, dev(), c.V)
    outs = ops.DecoderFn.apply(t(x), c, 4, W, 1, pt, 64, True, True, 1, False, ops.DecoderOpts())
    assert len(outs) == 7
    outs = ops.DecoderFn.apply(t(x), c, 4, W, 1, pt, 64, True, True, 1, False,
                               ops.DecoderOpts(silh_loss=(torch.zeros(B, W, W, dtype=torch.int32, device=dev()), None, 0.0)))
    assert len(outs) == 8 and outs[7].shape == (B, W * W)
    with pytest.raises(RuntimeError, match="silh_labels"):
        new(t(x), silh_confusion=torch.zeros(3, 2, dtype=torch.int64, device=dev()))
    with pytest.raises(RuntimeError, match="silh_labels"):
        old(t(x), silh_labels=torch.zeros(B, W, W, dtype=torch.int32, device=dev()))


# --------------------------------------------------------------------------------------------------------- trainer
@pytest.mark.parametrize("kind", ["joint", "silhouette-only"])
def test_trainer_step_equals_the_unfused_trainer(smpl_model, kind):
    from ilps_amd.metrics import SegConfusion
    from ilps_amd.training import SegTrainer
    B, W = 2, 48
    g = torch.Generator().manual_seed(11)
    images = torch.rand(B, 3, 256, 256, generator=g).to(dev())
    labels = torch.randint(0, 32, (B, W, W), generator=g).to(dev()) if kind == "joint" else None
    sl = torch.randint(0, 2, (B, W, W), generator=g).to(dev())
    got = []
    for fused in (True, False):
        torch.manual_seed(0)
        tr = SegTrainer(smpl_model, output_wh=W, encoder_architecture="enet", use_IEF=True, device=dev(), with_silhouette=True,
                        fused_silh_loss=fused)
        tr.smpl_model.train()
        m = SegConfusion(2, dev())
        torch.manual_seed(1)                                            # the encoder's dropout draws
        loss = float(tr.step(images, labels, sl, metrics=(None, m)))
        got.append((loss, m.counts.clone(), tr.smpl_model.backbone.enet.init_conv.weight.grad.cpu().numpy()))
    (lf, cf, gf), (lu, cu, gu) = got
    err = float(np.abs(gf - gu).max() / np.abs(gu).max())
    print("%s step: loss %.7f fused / %.7f unfused, first-layer gradient max|diff|/max|ref| %.2e = %.3g x the bar 2e-3"
          % (kind, lf, lu, err, err / 2e-3))
    assert abs(lf - lu) <= 1e-5 * abs(lu)
    assert torch.equal(cf, cu) and int(cf.sum()) == B * W * W
    grad_close(gf, gu, name="first-layer gradient, %s step" % kind)


# ------------------------------------------------------------------------------------------------------- torch ops
def test_torch_ops_check_their_arguments_and_equal_the_ctypes_path(layer):
    from ilps_amd import ops, torch_ops
    ns = torch_ops.load()
    B, W = 2, 48
    proj = bodies(layer, B, W, 13)
    silh, arg = ops._silh_fwd(proj, W)
    labels = make_labels(silh, 13)
    cw = weights(True)
    conf_a = torch.zeros(3, 2, dtype=torch.int64, device=dev())
    conf_b = torch.zeros_like(conf_a)
    s1, a1, l1, k1 = ops._silh_fwd_loss(proj, W, labels, cw, 2.0, conf=conf_a)
    s2, a2, l2, k2 = ns.silh_fwd_loss(proj, None, labels, cw, 2.0, W, conf_b)
    assert all(torch.equal(p, q) for p, q in ((s1, s2), (a1, a2), (l1, l2), (k1, k2), (conf_a, conf_b)))
    l3, k3 = ns.silh_loss_fwd(silh, labels, cw, 2.0, conf_b)
    assert torch.equal(l3, l1) and torch.equal(k3, k1) and torch.equal(conf_b, 2 * conf_a)
    dloss = torch.randn(B, W * W, generator=torch.Generator().manual_seed(3)).to(dev())
    for det in (False, True):
        d = ns.silh_loss_bwd(dloss, k1, silh, arg, proj, det)
        if det:
            assert torch.equal(d, ops._silh_loss_bwd(dloss, k1, silh, arg, proj, W, True))
        assert d.shape == (B, V, 3) and bool(torch.isfinite(d).all())
    bad = [lambda: ns.silh_loss_fwd(silh, labels[:, :40].contiguous(), None, 0.0, None),          # labels' shape
           lambda: ns.silh_loss_fwd(silh, labels.long(), None, 0.0, None),                        # int64 labels
           lambda: ns.silh_loss_fwd(silh, labels.cpu(), None, 0.0, None),                         # a CPU operand
           lambda: ns.silh_loss_fwd(silh, labels, cw.cpu(), 0.0, None),
           lambda: ns.silh_loss_fwd(silh, labels, None, 0.0, torch.zeros(33, 32, dtype=torch.int64, device=dev())),
           lambda: ns.silh_loss_fwd(silh, labels, None, -1.0, None),
           lambda: ns.silh_fwd_loss(proj, None, labels, None, 0.0, 50, None),                     # W against the labels
           lambda: ns.silh_fwd_loss(proj, silh[..., 0].contiguous()[:, :40].contiguous(), labels, None, 0.0, W, None),
           lambda: ns.silh_loss_bwd(dloss[:, :100].contiguous(), k1, silh, arg, proj, False),
           lambda: ns.silh_loss_bwd(dloss, k1, silh, arg.long(), proj, False),
           lambda: ns.silh_loss_bwd(dloss.cpu(), k1, silh, arg, proj, False)]
    for i, fn in enumerate(bad):
        with pytest.raises((RuntimeError, NotImplementedError)):
            fn()
    with pytest.raises(RuntimeError):
        ops._silh_fwd_loss(proj, W, labels.long(), None, 0.0)
    with pytest.raises(RuntimeError):
        ops._silh_loss_fwd(silh, labels, None, 0.0, conf=torch.zeros(33, 32, dtype=torch.int64, device=dev()))
