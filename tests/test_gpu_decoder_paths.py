"""The host paths of ops.DecoderFn against each other, bit for bit: the binning workgroups skinning their own vertices
against the separate skinning call (SMPLR_FUSE_SKIN=0), one chunk against two, pose + blend in one launch against two
(ops.POSE_BLEND_SPLIT_B = 1) - for every option set a caller can ask for.  Between the runs of one option set every
returned tensor, the confusion counts and dx for one seeded cotangent per differentiable output are EQUAL: what the
docstrings of ops.py promise ("bit for bit what the two calls give", "results are identical for any nchunk",
"bit-identical either way").  Deterministic backward; B = 3, so that two chunks are 2 + 1 meshes; W = 16."""
import pytest
import torch

from _inputs import make_x

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, W = 3, 16
NAMES = ("verts", "proj", "mask", "seg", "silh", "J_transformed", "loss", "silh_loss")


def _seeded(shape, seed, kind="normal", high=2):
    g = torch.Generator().manual_seed(seed)
    if kind == "int":
        return torch.randint(0, high, shape, generator=g)
    return torch.randn(shape, generator=g)


def _loss_spec(B):
    class_w = (_seeded((32,), 11).abs() + 0.5).to(DEV)
    return (_seeded((B, W, W), 12, "int", 32).to(DEV), class_w, 2.0)


def _silh_loss_spec(B, Ws):
    return (_seeded((B, Ws, Ws), 13, "int", 2).to(torch.int32).to(DEV), (_seeded((2,), 14).abs() + 0.5).to(DEV), 2.0)


def _conf(classes):
    return torch.zeros(classes + 1, classes, dtype=torch.int64, device=DEV)


# name -> (vertex_sampling, with_silh, DecoderOpts keywords for a batch of B: a callable, confusion tensors are fresh per run)
OPTION_SETS = {
    "plain": (1, False, lambda B: {}),
    "loss": (1, False, lambda B: dict(loss=_loss_spec(B), want_seg=False)),
    "loss + confusion": (1, False, lambda B: dict(loss=_loss_spec(B), want_seg=False, confusion=_conf(32))),
    "loss + want_seg": (1, False, lambda B: dict(loss=_loss_spec(B), want_seg=True)),
    "seg + silhouette, one W (hint)": (1, True, lambda B: {}),
    "seg + silhouette at 24": (1, 24, lambda B: {}),
    "silhouette only": (1, True, lambda B: dict(seg=False)),
    "silhouette loss + confusion": (1, True, lambda B: dict(silh_loss=_silh_loss_spec(B, W), silh_confusion=_conf(2))),
    "no verts / proj / mask": (1, False, lambda B: dict(want_verts=False, want_proj=False, want_mask=False)),
    "loss, hint, nothing written": (1, True, lambda B: dict(loss=_loss_spec(B), want_seg=False, confusion=_conf(32),
                                                          want_verts=False, want_proj=False, want_mask=False)),
    "vs = 2": (2, False, lambda B: {}),
    "vs = 2, loss": (2, False, lambda B: dict(loss=_loss_spec(B), want_seg=False)),
}


@pytest.fixture(scope="module")
def setup(smpl_model):
    from ilps_amd import ops
    c = ops.SMPLConstants.from_model(smpl_model, torch.device(DEV))
    assert c.V == 6890 and c.blend3_fwd is not None and c.lbs_top4 is not None
    return c, torch.tensor(make_x(B, W, seed=5), device=DEV)


def _run(setup, name, nchunk=1):
    """One forward and the backwards -> {output name: tensor}, {output name: dx}, [confusion counts].
    setup: the constants and x (B, 86); tools/probes/decoder_hash.py hashes what this returns."""
    from ilps_amd import ops
    c, x0 = setup
    vs, with_silh, kw = OPTION_SETS[name]
    kw = kw(x0.shape[0])
    x = x0.clone().requires_grad_(True)
    pt = ops.get_part_table(vs, torch.device(DEV), c.V)
    res = ops.DecoderFn.apply(x, c, 4, W, vs, pt, 64, True, with_silh, nchunk, True, ops.DecoderOpts(**kw))
    outs, dxs = dict(zip(NAMES, res)), {}
    for i, (n, t) in enumerate(outs.items()):
        # (the mask has no gradient, compute_mask.py:30 - though autograd may call it differentiable: with a fused loss the
        # node's second mark_non_differentiable call replaces the first, and its cotangent is then ignored)
        if t.requires_grad and t.numel() and n != "mask":
            cot = _seeded(tuple(t.shape), 100 + i).to(DEV)
            dxs[n] = torch.autograd.grad(t, x, cot, retain_graph=True)[0]
    torch.cuda.synchronize()
    counts = [kw[k].clone() for k in ("confusion", "silh_confusion") if k in kw]
    return {n: t.detach() for n, t in outs.items()}, dxs, counts


def _same(a, b, what):
    (oa, da, ca), (ob, db, cb) = a, b
    assert oa.keys() == ob.keys() and da.keys() == db.keys() and len(ca) == len(cb), what
    for n in oa:
        assert oa[n].shape == ob[n].shape and torch.equal(oa[n], ob[n]), "%s: %s differs" % (what, n)
    for n in da:
        assert torch.equal(da[n], db[n]), "%s: dx through %s differs" % (what, n)
    for i, (p, q) in enumerate(zip(ca, cb)):
        assert torch.equal(p, q), "%s: confusion counts %d differ" % (what, i)


@pytest.mark.parametrize("name", list(OPTION_SETS))
def test_decoder_paths_agree_bit_for_bit(setup, monkeypatch, name):
    from ilps_amd import ops
    monkeypatch.delenv("SMPLR_FUSE_SKIN", raising=False)
    base = _run(setup, name)
    outs, dxs, counts = base
    # the run is not vacuous: what the option set asks for is there, finite, and drives a gradient
    vs, with_silh, kw = OPTION_SETS[name]
    kw = kw(B)
    assert outs["J_transformed"].shape == (B, 24, 3) and "J_transformed" in dxs
    assert (outs["seg"].numel() > 0) == (kw.get("seg", True) and kw.get("want_seg", True))
    assert (outs["loss"].numel() > 0) == ("loss" in kw) and (outs["silh"].numel() > 0) == bool(with_silh)
    assert (len(outs) == 8) == ("silh_loss" in kw)
    assert all(torch.isfinite(d).all() and float(d.abs().sum()) > 0 for d in dxs.values())
    assert all(int(cnt.sum()) == B * W * W for cnt in counts)
    with monkeypatch.context() as m:
        m.setenv("SMPLR_FUSE_SKIN", "0")
        _same(base, _run(setup, name), "separate skinning call")
    _same(base, _run(setup, name, nchunk=2), "two chunks")
    with monkeypatch.context() as m:
        m.setattr(ops, "POSE_BLEND_SPLIT_B", 1)
        _same(base, _run(setup, name), "pose + blend in two launches")
    with monkeypatch.context() as m:
        m.setenv("SMPLR_FUSE_SKIN", "0")
        _same(base, _run(setup, name, nchunk=2), "separate skinning call, two chunks")
