"""ops.decoder_plan and ops._decoder_operands without a device: the decisions of DecoderFn.forward (which outputs exist,
whether the binning workgroups skin their own vertices, whether the part rasteriser writes the silhouette's hint, pose +
blend as one launch or two) and every refusal it raises behind require_cuda(x), with its message.  Bounds are read from
the module's constants, never copied."""
import pytest
import torch

from ilps_amd import ops

V = 6890


def plan(B=128, W=48, Ws=0, vs=1, P=31, opts=None, bf16x3=True, sparse=True, fits=True):
    return ops.decoder_plan(B, W, Ws, V, vs, P, opts if opts is not None else ops.DecoderOpts(), bf16x3, sparse, fits)


@pytest.fixture(autouse=True)
def _default_environment(monkeypatch):
    for name in ("SMPLR_FUSE_SKIN", "SMPLR_SILH_HINT"):
        monkeypatch.delenv(name, raising=False)


def test_the_plan_is_frozen_plain_values():
    p = plan()
    assert all(isinstance(v, (bool, int)) for v in vars(p).values())
    with pytest.raises(Exception):
        p.fuse_skin = False
    assert p.VP == V and plan(vs=2).VP == (V + 1) // 2 and plan(vs=5).VP == (V + 4) // 5


def test_fuse_skin_by_batch():
    lo, hi = ops.FUSE_SKIN_BELOW_B, ops.FUSE_SKIN_FROM_B
    assert 1 < lo < hi
    for B, want in ((1, True), (lo - 1, True), (lo, False), ((lo + hi) // 2, False), (hi - 1, False), (hi, True),
                    (4 * hi, True)):
        assert plan(B=B).fuse_skin is want, B


def test_fuse_skin_follows_patched_thresholds(monkeypatch):
    monkeypatch.setattr(ops, "FUSE_SKIN_BELOW_B", 3)
    monkeypatch.setattr(ops, "FUSE_SKIN_FROM_B", 5)
    assert [plan(B=B).fuse_skin for B in (2, 3, 4, 5)] == [True, False, False, True]


def test_fuse_skin_needs_sparse_weights_every_vertex_a_fit_and_no_veto(monkeypatch):
    assert plan().fuse_skin
    assert not plan(vs=2).fuse_skin
    assert not plan(sparse=False).fuse_skin
    assert not plan(fits=False).fuse_skin
    assert not plan(Ws=48, opts=ops.DecoderOpts(seg=False)).fuse_skin
    monkeypatch.setenv("SMPLR_FUSE_SKIN", "0")
    assert not plan().fuse_skin
    monkeypatch.setenv("SMPLR_FUSE_SKIN", "1")
    assert plan().fuse_skin


def test_vmax_only_where_the_silhouette_rasteriser_reads_it(monkeypatch):
    top = ops.SILH_HINT_MAX_W
    assert plan(W=top, Ws=top).vmax and plan(W=16, Ws=16).vmax
    assert not plan(W=top).vmax                                              # no silhouette head
    assert not plan(W=top, Ws=top, opts=ops.DecoderOpts(seg=False)).vmax     # no part head
    assert not plan(W=top, Ws=top // 2).vmax and not plan(W=16, Ws=24).vmax   # two resolutions
    assert not plan(W=top + 1, Ws=top + 1).vmax
    assert not plan(W=top, Ws=top, P=17).vmax
    monkeypatch.setenv("SMPLR_SILH_HINT", "0")
    assert not plan(W=top, Ws=top).vmax
    monkeypatch.setenv("SMPLR_SILH_HINT", "1")
    assert plan(W=top, Ws=top).vmax


def test_pose_and_blend_in_one_launch(monkeypatch):
    cut = ops.POSE_BLEND_SPLIT_B
    assert cut > 1
    p = plan(B=2 * cut)
    assert p.pose_blend_one_launch(1) and p.pose_blend_one_launch(cut - 1)
    assert not p.pose_blend_one_launch(cut) and not p.pose_blend_one_launch(2 * cut)
    f32 = plan(bf16x3=False)
    assert not f32.pose_blend_one_launch(1) and not f32.pose_blend_one_launch(cut - 1)
    monkeypatch.setattr(ops, "POSE_BLEND_SPLIT_B", 1)
    assert not plan().pose_blend_one_launch(1)
    monkeypatch.setattr(ops, "POSE_BLEND_SPLIT_B", 2)
    assert plan().pose_blend_one_launch(1) and not plan().pose_blend_one_launch(2)


def test_outputs_that_exist():
    p = plan()
    assert p.seg and not p.silh and not p.loss and not p.silh_loss
    assert p.want_verts and p.want_proj and p.want_mask and p.want_seg
    off = ops.DecoderOpts(want_verts=False, want_proj=False, want_mask=False)
    p = plan(opts=off)
    assert not p.want_verts and not p.want_proj and not p.want_mask and p.want_seg
    assert plan(Ws=48, opts=off).want_proj and plan(Ws=24, opts=off).silh     # a silhouette head reads proj
    only = plan(Ws=48, opts=ops.DecoderOpts(seg=False))
    assert only.silh and not only.seg and not only.want_seg and not only.want_mask and only.want_proj
    spec = (torch.zeros(1, 48, 48, dtype=torch.int64), None, 2.0)
    assert plan(opts=ops.DecoderOpts(loss=spec)).loss and plan(opts=ops.DecoderOpts(loss=spec)).want_seg
    quiet = plan(opts=ops.DecoderOpts(loss=spec, want_seg=False))
    assert quiet.loss and not quiet.want_seg
    assert plan(opts=ops.DecoderOpts(want_seg=False)).want_seg                  # no loss: the scores are the output
    no_head = plan(Ws=48, opts=ops.DecoderOpts(seg=False, loss=spec))
    assert not no_head.loss                                                    # a loss without its head is no loss
    sl = (torch.zeros(1, 48, 48, dtype=torch.int32), None, 0.0)
    assert plan(Ws=48, opts=ops.DecoderOpts(silh_loss=sl)).silh_loss and not plan(Ws=48).silh_loss


# ---------------------------------------------------------------------------------------------------------- refusals
B, W = 2, 8


def operands(opts, P=31, Ws=0, num_cam=4, grid_wh=64):
    return ops._decoder_operands(opts, P, B, W, Ws, num_cam, grid_wh, torch.device("cpu"))


@pytest.fixture
def host_tensors(monkeypatch):
    """The refusals behind a loss head's labels lie behind their move to the device: let host tensors pass it."""
    def passes(t, name, dtype=torch.float32):
        assert isinstance(t, torch.Tensor) and t.dtype == dtype, name
        return t.contiguous()
    monkeypatch.setattr(ops, "require_cuda", passes)


def labels(dtype=torch.int64, n=B * W * W):
    return torch.zeros(n, dtype=dtype)


def test_accepted_operands(host_tensors):
    (lab, cw, gamma, conf), (sl, sw, sg, sconf) = operands(ops.DecoderOpts())
    assert lab is None and cw is None and conf is None and sl is None and sw is None and sconf is None
    for dt in (torch.int64, torch.int32, torch.int16, torch.uint8):
        (lab, cw, gamma, conf), _ = operands(ops.DecoderOpts(loss=(labels(dt), torch.ones(32), 2.0)))
        assert lab.dtype == torch.int32 and tuple(lab.shape) == (B, W, W) and cw.numel() == 32 and gamma == 2.0
    (lab, _, _, _), _ = operands(ops.DecoderOpts(seg=False, loss=(labels(), None, 2.0)), Ws=W)
    assert lab is None                                                          # the loss goes with its head


def test_refusals_without_tensors():
    with pytest.raises(RuntimeError, match=r"DecoderFn: no head asked for \(opts.seg = False needs a silhouette\)"):
        operands(ops.DecoderOpts(seg=False))
    for bad in (3, 17, 0):
        with pytest.raises(RuntimeError, match=r"the projection needs the 4 camera columns, num_cam must be in 4..16 \(got %d\)" % bad):
            operands(ops.DecoderOpts(), num_cam=bad)
    for bad in (0, -1, 129):
        with pytest.raises(RuntimeError, match=r"DecoderFn: grid_wh must be in 1..128 \(got %d\)" % bad):
            operands(ops.DecoderOpts(), grid_wh=bad)
    operands(ops.DecoderOpts(seg=False), Ws=W, grid_wh=0)                       # no part head, no grid
    with pytest.raises(RuntimeError, match=r"the fused loss head is the 32-class one \(P = 31\)"):
        operands(ops.DecoderOpts(loss=(labels(), None, 2.0)), P=17)
    with pytest.raises(RuntimeError, match="DecoderOpts.confusion rides on the fused loss: it needs DecoderOpts.loss"):
        operands(ops.DecoderOpts(confusion=torch.zeros(33, 32, dtype=torch.int64)))
    with pytest.raises(RuntimeError, match="DecoderOpts.silh_loss needs the silhouette head"):
        operands(ops.DecoderOpts(silh_loss=(torch.zeros(B, W, W, dtype=torch.int32), None, 0.0)))
    with pytest.raises(RuntimeError, match="DecoderOpts.silh_confusion rides on the fused silhouette loss: it needs "
                                           "DecoderOpts.silh_loss"):
        operands(ops.DecoderOpts(silh_confusion=torch.zeros(3, 2, dtype=torch.int64)), Ws=W)


def test_refusals_of_labels_weights_and_confusion(host_tensors):
    msg = "fused loss: labels must be an integer class map of %d x %d x %d entries" % (B, W, W)
    for bad in (labels(n=B * W * W - 1), labels(torch.float32), labels(torch.int8), labels(torch.bool)):
        with pytest.raises(RuntimeError, match=msg):
            operands(ops.DecoderOpts(loss=(bad, None, 2.0)))
    for n in (31, 33, 2):
        with pytest.raises(RuntimeError, match="class_w needs 32 entries"):
            operands(ops.DecoderOpts(loss=(labels(), torch.ones(n), 2.0)))
    spec = (labels(), None, 2.0)
    msg = r"DecoderOpts.confusion must be a contiguous \(33, 32\) int64 tensor on cpu"
    for bad in (torch.zeros(32, 32, dtype=torch.int64), torch.zeros(33, 32, dtype=torch.int32), torch.zeros(33, 32),
                torch.zeros(32, 33, dtype=torch.int64).t(),
                torch.zeros(33, 32, dtype=torch.int64)):        # (the last: right shape and type, but no device tensor)
        with pytest.raises(RuntimeError, match=msg):
            operands(ops.DecoderOpts(loss=spec, confusion=bad))
    sl = torch.zeros(B, W, W, dtype=torch.int32)
    with pytest.raises(RuntimeError, match=r"silhouette labels must be \(%d, %d, %d\) int32" % (B, W, W)):
        operands(ops.DecoderOpts(silh_loss=(sl.long(), None, 0.0)), Ws=W)
    with pytest.raises(RuntimeError, match="the silhouette loss takes 2 class weights, got 3"):
        operands(ops.DecoderOpts(silh_loss=(sl, torch.ones(3), 0.0)), Ws=W)
    msg = r"the silhouette confusion must be a contiguous \(3, 2\) int64 device tensor \(SegConfusion\(2\).counts\)"
    for bad in (torch.zeros(2, 2, dtype=torch.int64), torch.zeros(3, 2, dtype=torch.int32)):
        with pytest.raises(RuntimeError, match=msg):
            operands(ops.DecoderOpts(silh_loss=(sl, None, 0.0), silh_confusion=bad), Ws=W)


def test_the_shared_rules():
    for dt in (torch.int64, torch.int32, torch.int16, torch.uint8):
        assert ops._is_class_map(torch.zeros(6, dtype=dt)) and ops._is_class_map(torch.zeros(6, dtype=dt), 6)
        assert not ops._is_class_map(torch.zeros(6, dtype=dt), 5)
    for dt in (torch.float32, torch.int8, torch.bool, torch.float64):
        assert not ops._is_class_map(torch.zeros(6, dtype=dt))
    good = torch.zeros(33, 32, dtype=torch.int64)
    assert ops._is_confusion(good, 32) and not ops._is_confusion(good, 2)
    assert ops._is_confusion(torch.zeros(3, 2, dtype=torch.int64), 2)
    assert not ops._is_confusion(good.int(), 32) and not ops._is_confusion(good[:32], 32)
    assert not ops._is_confusion(good, 32, kernel_operand=True)                 # a host tensor is no kernel operand
