"""`SyntheticBatches(seg="edges")` on the GPU: the edge channel against tests/_edges_oracle.py's Canny of the batch's own
render, everything else against a `seg="silhouette"` loop from the same seed.  Fixtures as tests/test_gpu_synthetic.py:
B = 4, input 32, output 16."""
import numpy as np
import pytest
import torch

import _edges_oracle as eo
from ilps_amd import synthetic as syn

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
FILL = (0.6, 0.9)
EDGE = dict(low=40, high=80)
CORRUPTION = dict(box_prob=1.0, crop_prob=0.5, swap_pairs=((0, 1),))


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


def test_edge_channel_is_the_canny_of_the_batch_render(setup):
    from ilps_amd.render import render_mesh
    K = setup["spec"].K
    for corruption in (None, CORRUPTION):
        bt = batches_for(setup, seg="edges", edge=EDGE, corruption=corruption, seed=3)
        assert bt.in_channels == 1 + K
        images, labels = next(bt)
        assert images.shape == (4, 1 + K, 32, 32) and images.dtype == torch.float32 and images.is_contiguous()
        rgb = render_mesh(bt.last["verts"], setup["topo"], bt.last["x"][:, :4], mode="ortho", img_wh=32, scale=2.0)["rgb"]
        want = eo.canny(rgb.cpu().numpy(), "RGB_F32_HWC", **EDGE)[0].astype(np.float32)
        assert want.sum() >= 4 * 20                                       # an outline per body, at the least
        if corruption is not None:
            boxes = bt.last["draws"]["boxes"].cpu().numpy()
            hit = 0
            for b in range(4):
                for x0, y0, x1, y1 in boxes[b]:
                    if x1 > x0 and y1 > y0:
                        hit += int(want[b, max(y0, 0):y1, max(x0, 0):x1].sum())
                        want[b, max(y0, 0):y1, max(x0, 0):x1] = 0
            assert hit > 0                                                # the boxes removed something
        assert torch.equal(images[:, 0].cpu(), torch.from_numpy(want))


def test_everything_else_is_the_silhouette_loop_of_the_seed(setup):
    kw = dict(corruption=CORRUPTION, silh_wh=8, seed=7, sigma=2.0)
    a, s = batches_for(setup, seg="edges", edge=EDGE, **kw), batches_for(setup, seg="silhouette", **kw)
    again = batches_for(setup, seg="edges", edge=EDGE, **kw)
    for _ in range(2):
        ba, bs, bb = next(a), next(s), next(again)
        assert len(ba) == 3 and torch.equal(ba[1], bs[1]) and torch.equal(ba[2], bs[2])           # labels, silhouette labels
        assert torch.equal(ba[0][:, 1:].view(torch.int32), bs[0][:, 1:].view(torch.int32))          # heat channels
        assert not torch.equal(ba[0][:, 0], bs[0][:, 0])
        for k in ("x", "verts", "joints", "keep"):
            assert torch.equal(a.last[k], s.last[k]), k
        for ta, tb in zip(ba, bb):                                                                 # the same seed repeats the batch
            assert torch.equal(ta, tb)
    pairs_a, pairs_s = list(a.eval_batches(1)), list(s.eval_batches(1))
    assert torch.equal(pairs_a[0][1], pairs_s[0][1]) and a.last["draws"] is None


def test_edge_keywords(setup):
    with pytest.raises(ValueError):
        batches_for(setup, seg="edges", corruption=dict(remove_parts=(1, 2)))
    with pytest.raises(ValueError):
        batches_for(setup, seg="silhouette", edge=EDGE)
    with pytest.raises(ValueError):
        batches_for(setup, seg="edges", edge=dict(low=1, high=2, value=255))
    batches_for(setup, seg="edges", corruption=dict(remove_parts=()))
    flat = batches_for(setup, seg="edges", edge=dict(low=40, high=80, shading="parts", blur=False), corruption=None, seed=3)
    lam = batches_for(setup, seg="edges", corruption=None, seed=3)                                # the defaults
    assert lam.edge == syn.EDGE_DEFAULTS and flat.edge == dict(low=40, high=80, blur=False)
    fi, li = next(flat)[0], next(lam)[0]
    assert torch.equal(fi[:, 1:], li[:, 1:]) and not torch.equal(fi[:, 0], li[:, 0]) and fi[:, 0].any()


def test_one_training_step(setup, smpl_model):
    from ilps_amd.training import SegTrainer
    torch.manual_seed(0)
    bt = batches_for(setup, B=2, input_wh=256, output_wh=48, seg="edges", edge=EDGE, corruption={})
    tr = SegTrainer(smpl_model, input_wh=256, output_wh=48, in_channels=bt.in_channels, device=DEV)
    loss = tr.step(*next(bt))
    assert np.isfinite(float(loss))
