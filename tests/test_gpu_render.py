"""The HIP triangle renderer (csrc/render.hip through ilps_amd.render) against its NumPy restatement
(tests/_render_oracle.py): face and part maps bit for bit, depth and colour within float64 bars, on generated meshes
(an SMPL-sized sphere, a triangle soup, slivers across many tiles, planes on the sample grid) in both camera modes."""
import numpy as np
import pytest
import torch

import _render_oracle as ro
from ilps_amd import render
from ilps_amd.render import MeshTopology, render_mesh

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
DEPTH_BAR = 2e-5            # relative to max(1, |depth|)
RGB_BAR = 1e-4              # absolute, colours in [0, 1]
_topo = {}
_worst = {"depth": 0.0, "rgb": 0.0}


def mesh(kind, B, seed):
    """(B, V, 3) float32 vertices around the origin (about [-1, 1]) and (F, 3) faces."""
    rng = np.random.default_rng(seed)
    if kind == "sphere":
        return ro.posed_sphere(seed, B)
    if kind == "soup":
        v, f = ro.soup(seed)
    elif kind == "slivers":
        v, f = ro.slivers(seed)
    else:
        v, f = ro.grid_plane(12, 10, -0.9, -0.8, 0.15, z=0.2)
        v[:, 2] += 0.05 * v[:, 0]
    v = np.stack([v + np.r_[rng.uniform(-0.1, 0.1, 2), rng.uniform(-0.05, 0.05)].astype(np.float32) * (b > 0)
                  for b in range(B)])
    return v.astype(np.float32), f


def camera(mode, B, H, W):
    if mode == "ortho":
        return np.tile(np.array([0.4 * W, 0.4 * H, W / 2, H / 2], np.float32), (B, 1)), None
    return np.tile(np.array([1.2 * min(H, W), W / 2, H / 2], np.float32), (B, 1)), np.tile(np.float32([0, 0, 3]), (B, 1))


def topo_for(f, V):
    key = (f.tobytes(), V)
    if key not in _topo:
        _topo[key] = MeshTopology(f, V)
    return _topo[key]


def gpu(v, f, cam, mode, H, W, trans=None, **kw):
    t = topo_for(f, v.shape[1])
    out = render_mesh(torch.from_numpy(v).to(DEV), t, torch.from_numpy(cam).to(DEV), mode=mode, img_wh=(W, H),
                      trans=None if trans is None else torch.from_numpy(trans).to(DEV), **kw)
    return {k: x.cpu().numpy() for k, x in out.items()}, t


def check_against_oracle(got, t, v, f, cam, mode, H, W, trans=None, rows=None, bg=None, tag=""):
    for b in (range(v.shape[0]) if rows is None else rows):
        tb = None if trans is None else trans[b]
        col = ro.lambert_colors(v[b], f, render.COLORS["light_blue"], render.DEFAULT_LIGHTS, tb)
        want = ro.render(v[b], f, cam[b], mode, H, W, col, trans=tb, face_part=t.face_part,
                         bg=None if bg is None else bg[b])
        assert np.array_equal(got["face"][b], want["face"]), "%s row %d: %d face ids differ" % (
            tag, b, int((got["face"][b] != want["face"]).sum()))
        assert np.array_equal(got["part"][b], want["part"]), tag
        assert np.array_equal(got["alpha"][b], want["alpha"]), tag
        cov = want["alpha"]
        derr = np.abs(got["depth"][b] - want["depth"]) / np.maximum(1.0, np.abs(want["depth"]))
        rerr = np.abs(got["rgb"][b] - want["rgb"])
        assert (got["depth"][b][~cov] == 0).all()
        dm, rm = float(derr.max()), float(rerr.max())
        _worst["depth"], _worst["rgb"] = max(_worst["depth"], dm), max(_worst["rgb"], rm)
        assert dm <= DEPTH_BAR, "%s row %d: depth error %.3g" % (tag, b, dm)
        assert rm <= RGB_BAR, "%s row %d: rgb error %.3g" % (tag, b, rm)
    return cov


SIZES = [(48, 48), (64, 64), (224, 224), (256, 256), (512, 512), (200, 130), (100, 300)]


@pytest.mark.parametrize("mode", ["ortho", "perspective"])
@pytest.mark.parametrize("kind", ["sphere", "soup", "slivers", "plane"])
@pytest.mark.parametrize("H,W", SIZES)
def test_maps_match_the_oracle(kind, mode, H, W):
    B = 3
    v, f = mesh(kind, B, seed=H * 7 + W)
    cam, trans = camera(mode, B, H, W)
    got, t = gpu(v, f, cam, mode, H, W, trans)
    cov = check_against_oracle(got, t, v, f, cam, mode, H, W, trans, tag="%s %s %dx%d" % (kind, mode, H, W))
    assert cov.any()
    print("%s %s %dx%d: worst so far depth %.3g (rel), rgb %.3g" % (kind, mode, H, W, _worst["depth"], _worst["rgb"]))


@pytest.mark.parametrize("mode", ["ortho", "perspective"])
def test_plane_on_the_sample_grid(mode):
    """Vertices exactly on sample centres and edges along sample rows and columns: the top-left rule, bit for bit,
    and no sample inside the plane left uncovered."""
    H, W = 70, 90
    v, f = ro.grid_plane(20, 15, 3.0, 2.0, 4.0, z=0.5)
    if mode == "ortho":
        v[:, 1] = (H - 1) - v[:, 1]
        cam = np.float32([[1, 1, 0, 0]])
        trans = None
    else:
        v[:, 0], v[:, 1], v[:, 2] = (v[:, 0] - 40) * 2 / 64, (v[:, 1] - 30) * 2 / 64, 0.0
        cam, trans = np.float32([[64, 40, 30]]), np.float32([[0, 0, 2]])
    v = v[None].astype(np.float32)
    got, t = gpu(v, f, cam, mode, H, W, trans)
    check_against_oracle(got, t, v, f, cam, mode, H, W, trans, tag="grid " + mode)
    if mode == "ortho":
        assert (got["face"][0, 3:62, 4:83] >= 0).all()


def test_batch_of_128_and_each_mesh_alone():
    H = W = 64
    v, f = mesh("sphere", 128, seed=11)
    cam, _ = camera("ortho", 128, H, W)
    got, t = gpu(v, f, cam, "ortho", H, W)
    check_against_oracle(got, t, v, f, cam, "ortho", H, W, rows=(0, 1, 63, 100, 127), tag="B=128")
    again, _ = gpu(v, f, cam, "ortho", H, W)
    for k in got:
        assert np.array_equal(got[k].view(np.uint8), again[k].view(np.uint8)), k       # run to run, bit for bit
    for b in (0, 77, 127):
        alone, _ = gpu(v[b:b + 1], f, cam[b:b + 1], "ortho", H, W)
        for k in got:
            assert np.array_equal(alone[k][0].view(np.uint8), got[k][b].view(np.uint8)), (b, k)


def test_nan_rows_drop_exactly_their_faces():
    H = W = 96
    v, f = mesh("sphere", 2, seed=3)
    cam, trans = camera("perspective", 2, H, W)
    bad = np.array([5, 100, 2000, 3001, 6000])
    vn = v.copy()
    vn[1, bad] = np.nan
    got, t = gpu(vn, f, cam, "perspective", H, W, trans)
    # the same mesh with those faces made degenerate (zero area, zero normal contribution) and finite vertices
    f2 = f.copy()
    hit = np.isin(f, bad).any(1)
    f2[hit] = 0
    col = ro.lambert_colors(v[1], f2, render.COLORS["light_blue"], render.DEFAULT_LIGHTS, trans[1])
    want = ro.render(v[1], f2, cam[1], "perspective", H, W, col, trans=trans[1], face_part=t.face_part)
    assert hit.sum() > 20 and np.array_equal(got["face"][1], want["face"])
    assert np.abs(got["rgb"][1] - want["rgb"]).max() <= RGB_BAR
    assert not np.isin(got["face"][1], np.nonzero(hit)[0]).any()
    check_against_oracle(got, t, v, f, cam, "perspective", H, W, trans, rows=(0,), tag="nan row 0")


def test_meshes_off_screen_are_background():
    H, W = 80, 60
    v, f = mesh("sphere", 2, seed=4)
    cam, _ = camera("ortho", 2, H, W)
    cam[:, 2] += 1000.0                                    # far to the right
    cam[1, 2] -= 3000.0                                    # far to the left
    bg = np.random.default_rng(0).random((2, H, W, 3)).astype(np.float32)
    got, _ = gpu(v, f, cam, "ortho", H, W, background=torch.from_numpy(bg).to(DEV))
    assert (got["face"] == -1).all() and not got["alpha"].any() and (got["part"] == 0).all()
    assert (got["depth"] == 0).all() and np.array_equal(got["rgb"], bg)
    cam2, trans = camera("perspective", 2, H, W)
    trans[:, 2] = -5.0                                     # behind the camera
    got, _ = gpu(v, f, cam2, "perspective", H, W, trans)
    assert (got["face"] == -1).all() and (got["rgb"] == 1).all()


def test_background_images_are_composited():
    H, W = 100, 120
    v, f = mesh("sphere", 2, seed=6)
    cam, trans = camera("perspective", 2, H, W)
    rng = np.random.default_rng(1)
    img8 = rng.integers(0, 256, (2, H, W, 3), dtype=np.uint8)
    bg = img8.astype(np.float32) / 255.0
    got, t = gpu(v, f, cam, "perspective", H, W, trans, background=torch.from_numpy(img8).to(DEV))
    check_against_oracle(got, t, v, f, cam, "perspective", H, W, trans, bg=bg, tag="bg")
    # a float image above 1 is divided by 255 (renderer.py:235-236), one in [0, 1] is taken as it is; NCHW is accepted
    got2, _ = gpu(v, f, cam, "perspective", H, W, trans,
                  background=torch.from_numpy(img8.astype(np.float32)).permute(0, 3, 1, 2).to(DEV))
    got3, _ = gpu(v, f, cam, "perspective", H, W, trans, background=torch.from_numpy(bg).to(DEV))
    assert np.array_equal(got2["rgb"], got["rgb"])
    assert np.abs(got3["rgb"] - got["rgb"]).max() <= 1e-7       # (x / 255 on the host and on the device: 1 ulp)


def test_torch_op_equals_render_mesh():
    """torch.ops.smplraster.mesh_render runs the same two launches as render_mesh."""
    from ilps_amd import torch_ops
    ns = torch_ops.load()
    H, W = 72, 88
    v, f = mesh("sphere", 2, seed=12)
    cam, trans = camera("perspective", 2, H, W)
    t = topo_for(f, v.shape[1])
    d = t.on(DEV)
    vd, cd, td = (torch.from_numpy(a).to(DEV) for a in (v, cam, trans))
    want = render_mesh(vd, t, cd, mode="perspective", img_wh=(W, H), trans=td, near=0.5, far=100.0)
    light = list(render.COLORS["light_blue"]) + [x for pos, c in render.DEFAULT_LIGHTS for x in list(pos) + list(c)]
    outs = ns.mesh_render(vd, cd, td, d["faces"], d["face_part"], d["vf_off"], d["vf_face"], None, None, light, H, W, 1,
                          1.0, 0.5, 100.0)
    for k, o in zip(("face", "depth", "part", "alpha", "rgb"), outs):
        assert torch.equal(o, want[k]), k


def test_parts_and_vertex_shading():
    H = W = 128
    v, f = mesh("sphere", 2, seed=8)
    cam, _ = camera("ortho", 2, H, W)
    t = topo_for(f, v.shape[1])
    pal = np.random.default_rng(2).random((32, 3)).astype(np.float32)
    got, _ = gpu(v, f, cam, "ortho", H, W, shading="parts", palette=torch.from_numpy(pal).to(DEV))
    vc = np.random.default_rng(3).random((2, v.shape[1], 3)).astype(np.float32)
    got_v, _ = gpu(v, f, cam, "ortho", H, W, shading="vertex", vertex_colors=torch.from_numpy(vc).to(DEV))
    for b in range(2):
        want = ro.render(v[b], f, cam[b], "ortho", H, W, pal[t.vertex_part + 1], face_part=t.face_part)
        assert np.array_equal(got["face"][b], want["face"]) and np.array_equal(got["part"][b], want["part"])
        assert np.abs(got["rgb"][b] - want["rgb"]).max() <= RGB_BAR
        want = ro.render(v[b], f, cam[b], "ortho", H, W, vc[b])
        assert np.abs(got_v["rgb"][b] - want["rgb"]).max() <= RGB_BAR
    assert len(np.unique(got["part"])) > 10


def test_smpl_renderer_uint8_and_rgba():
    v, f = ro.uv_sphere()
    v = (v * 0.5).astype(np.float32)
    r = render.SMPLRenderer(img_size=96, flength=150., faces=f)
    trans = np.float32([0.1, 0, 2.5])
    im = r(v, trans=trans)
    assert im.shape == (96, 96, 3) and im.dtype == np.uint8
    out = render_mesh(torch.from_numpy(v[None]).to(DEV), r.topology(len(v)), [150., 48., 48.], mode="perspective",
                      img_wh=96, trans=trans)
    assert np.array_equal(im, np.floor(out["rgb"][0].cpu().numpy().astype(np.float64) * 255).astype(np.uint8))
    rgba = r(v, do_alpha=True, trans=trans)
    assert rgba.shape == (96, 96, 4)
    assert np.array_equal(rgba[..., 3], out["alpha"][0].cpu().numpy().astype(np.uint8) * 255)
    assert np.array_equal(rgba[..., :3], im)
    img = np.random.default_rng(0).integers(0, 256, (96, 96, 3), dtype=np.uint8)
    withbg = r(v, img=img, do_alpha=True, trans=trans)
    assert (withbg[..., 3] == 255).all()
    cov = out["alpha"][0].cpu().numpy()
    assert np.array_equal(withbg[~cov, :3], img[~cov])
    batch = r(np.stack([v, v * 0.8]), trans=trans)
    assert batch.shape == (2, 96, 96, 3) and np.array_equal(batch[0], im)
    seg = r(v, render_seg=True, trans=trans)
    assert seg.shape == (96, 96, 3) and not np.array_equal(seg, im)
    rot = r.rotated(v + trans, 90)
    assert rot.shape == (96, 96, 4)


def test_graph_capture_and_replay_equal_eager():
    H = W = 96
    v, f = mesh("sphere", 4, seed=9)
    cam, trans = camera("perspective", 4, H, W)
    t = topo_for(f, v.shape[1])
    vd, cd, td = (torch.from_numpy(a).to(DEV) for a in (v, cam, trans))
    eager = render_mesh(vd, t, cd, mode="perspective", img_wh=W, trans=td)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        static = render_mesh(vd, t, cd, mode="perspective", img_wh=W, trans=td)
    g.replay()
    torch.cuda.synchronize()
    for k in eager:
        assert torch.equal(eager[k], static[k]), k
    vd.copy_(torch.from_numpy(v[::-1].copy()))
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(static["face"][0], eager["face"][3])


def test_orientation_matches_the_silhouette_head():
    """A small triangle around projected (u, v) = (10, 30) at W = 48 covers pixel [17, 10]: where projects_to_silhouette
    peaks for a vertex at (10, 30)."""
    from oracle import np_oracle as o
    W = 48
    v = np.float32([[[9.6, 29.6, 0.5], [10.5, 29.7, 0.5], [9.9, 30.6, 0.5]]])
    got, _ = gpu(v, np.int32([[0, 1, 2]]), np.float32([[1, 1, 0, 0]]), "ortho", W, W)
    assert got["face"][0, 17, 10] == 0 and (got["face"][0] >= 0).sum() == 1
    silh = o.projects_to_silhouette(np.float64([[[10.0, 30.0, 0.0]]]), W)
    s = np.asarray(silh)[0, ..., 1]
    assert np.unravel_index(np.argmax(s), s.shape) == (17, 10)


def test_render_predictions_on_predict_batch(smpl_model):
    from ilps_amd.decoder import SMPLDecoder
    from ilps_amd.inference import predict_batch
    from ilps_amd.model import SMPLRegressor
    torch.manual_seed(0)
    reg = SMPLRegressor(48, "enet", True).to(DEV)
    dec = SMPLDecoder(smpl_model, img_wh=48)
    img = torch.rand(2, 3, 256, 256, device=DEV)
    pred = predict_batch(reg, dec, img)
    sv, sf = ro.uv_sphere()                                # stands in for SMPL's faces (V = 6 890 as well)
    t = MeshTopology(sf, 6890)
    out = render.render_predictions(pred, t, img, 48)
    assert out["rgb"].shape == (2, 256, 256, 3) and out["face"].shape == (2, 256, 256)
    verts = pred["verts"].cpu().numpy()
    cam = pred["smpl"][:, :4].float().cpu().numpy()
    bg = img.permute(0, 2, 3, 1).cpu().numpy()
    for b in range(2):
        col = ro.lambert_colors(verts[b], sf, render.COLORS["light_blue"], render.DEFAULT_LIGHTS)
        want = ro.render(verts[b], sf, cam[b], "ortho", 256, 256, col, scale=256 / 48, face_part=t.face_part, bg=bg[b])
        assert np.array_equal(out["face"][b].cpu().numpy(), want["face"])
        assert np.abs(out["rgb"][b].cpu().numpy() - want["rgb"]).max() <= RGB_BAR
