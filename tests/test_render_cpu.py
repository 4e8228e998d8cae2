"""The triangle renderer without a GPU: known answers and the partition property of the NumPy restatement
(tests/_render_oracle.py), normals and Lambert terms, the face-part rule, MeshTopology's checks, the pickle's faces,
the ABI entries' argument errors, the op's Meta kernel, SMPLRenderer's call surface and the kernels' resources."""
import inspect
import os
import pickle
import sys

import numpy as np
import pytest
import torch

import _render_oracle as ro
from ilps_amd import render
from ilps_amd.render import MeshTopology, face_parts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def ortho_id(H):
    """cam (k_u, k_v, u0, v0) = (1, 1, 0, 0): x = X and y = H - 1 - Y, so sample (j, i) is the point (j, H - 1 - i)."""
    return np.array([1, 1, 0, 0], np.float32)


def face_map(v, f, H, W, mode="ortho", cam=None, counts=False, **kw):
    cam = ortho_id(H) if cam is None else cam
    xi, yi, q, ok = ro.sample_space(v, cam, mode, H, **kw)
    return ro.raster(xi, yi, q, ok, f, H, W, counts=counts)


def img_tri(pts, z=0.5):
    """A triangle given in image (x = column, y = row) coordinates for ortho_id at H = 16."""
    return np.array([[x, 15 - y, z] for x, y in pts], np.float32)


def test_one_triangle_known_answer():
    v = img_tri([(2, 2), (10, 2), (2, 10)])
    face = face_map(v, np.array([[0, 1, 2]]), 16, 16)
    got = set(zip(*np.nonzero(face == 0)))
    # x >= 2, y >= 2, x + y <= 12, with the top-left rule on the three edges
    want = set()
    for r in range(16):
        for c in range(16):
            if 2 <= c and 2 <= r and c + r <= 12:
                want.add((r, c))
    # the edges the rule leaves out: which ones depends on their direction; each closed-edge sample is in or out as a whole
    assert got <= want and len(want - got) <= 9 + 9 + 8
    inner = {(r, c) for (r, c) in want if c > 2 and r > 2 and c + r < 12}
    assert inner <= got


def test_both_windings_cover_the_same_samples():
    v = img_tri([(1.3, 0.7), (12.6, 3.1), (4.2, 13.9)])
    a = face_map(v, np.array([[0, 1, 2]]), 16, 16)
    b = face_map(v, np.array([[0, 2, 1]]), 16, 16)
    assert (a >= 0).sum() > 40 and np.array_equal(a, b)


@pytest.mark.parametrize("mode", ["ortho", "perspective"])
def test_overlap_in_both_depth_orders(mode):
    """Two coincident triangles at different depths: the nearer one wins whichever face id it has (ortho: larger z
    nearer; perspective: smaller z nearer), equal depths go to the lower id."""
    t = [(1, 1), (14, 1), (1, 14)]
    for z0, z1 in ((0.3, 0.6), (0.6, 0.3), (0.5, 0.5)):
        if mode == "ortho":
            v = np.concatenate([img_tri(t, z0), img_tri(t, z1)])
            face = face_map(v, np.array([[0, 1, 2], [3, 4, 5]]), 16, 16)
            want = 0 if z0 >= z1 else 1
        else:
            zz = (2.0 + z0, 2.0 + z1)
            pts = [np.array([[(x - 8) * z / 10.0, (y - 8) * z / 10.0, z] for x, y in t], np.float32) for z in zz]
            v = np.concatenate(pts)
            face = face_map(v, np.array([[0, 1, 2], [3, 4, 5]]), 16, 16, mode="perspective",
                            cam=np.array([10, 8, 8], np.float32))
            want = 0 if zz[0] <= zz[1] else 1
        cov = face >= 0
        assert cov.sum() > 50 and (face[cov] == want).all(), (z0, z1)


def test_shared_edge_and_vertex_samples_belong_to_one_face():
    """Two triangles sharing a diagonal through sample centres, and a fan of eight around a sample centre."""
    v = img_tri([(2, 2), (12, 2), (12, 12), (2, 12)])
    face, cnt = face_map(v, np.array([[0, 1, 2], [0, 2, 3]]), 16, 16, counts=True)
    inside = np.zeros((16, 16), bool)
    inside[3:12, 3:12] = True                               # samples strictly inside the square
    assert (cnt[inside] == 1).all()
    diag = [(r, r) for r in range(3, 12)]                   # samples on the shared diagonal (x = 15 - y flips: rows)
    assert all(cnt[p] == 1 for p in diag)
    c = (7, 7)
    ang = np.arange(8) * np.pi / 4
    pts = [(c[0], c[1])] + [(c[0] + 4 * np.cos(a), c[1] + 4 * np.sin(a)) for a in ang]
    v = img_tri([(round(x * 256) / 256, round(y * 256) / 256) for x, y in pts])
    f = np.array([[0, 1 + k, 1 + (k + 1) % 8] for k in range(8)])
    face, cnt = face_map(v, f, 16, 16, counts=True)
    assert cnt[15 - 7, 7] == 1 and face[15 - 7, 7] >= 0     # the fan's centre: exactly one face
    assert cnt.max() == 1


def test_zero_area_offscreen_and_nonfinite_faces_cover_nothing():
    v = img_tri([(2, 2), (8, 2), (14, 2), (30, 30), (40, 30), (30, 40), (3, 3), (9, 3), (3, 9)])
    v[8, 0] = np.nan
    f = np.array([[0, 1, 2], [3, 4, 5], [6, 7, 8], [6, 7, 99]])
    assert (face_map(v, f, 16, 16) == -1).all()
    big = img_tri([(2, 2), (40000, 2), (2, 9)])             # outside the +-2^15 px guard band
    assert (face_map(big, np.array([[0, 1, 2]]), 16, 16) == -1).all()


def test_perspective_near_far_drop_whole_faces():
    v = np.array([[-1, -1, 2.0], [1, -1, 2.0], [0, 1, 5.0]], np.float32)
    cam = np.array([10, 8, 8], np.float32)
    f = np.array([[0, 1, 2]])
    assert (face_map(v, f, 16, 16, "perspective", cam) >= 0).any()
    assert (face_map(v, f, 16, 16, "perspective", cam, far=4.0) == -1).all()
    assert (face_map(v, f, 16, 16, "perspective", cam, near=2.5) == -1).all()
    v[2, 2] = -1.0
    assert (face_map(v, f, 16, 16, "perspective", cam) == -1).all()    # z <= 0: dropped, not clipped


def test_tiled_plane_is_a_partition():
    """Every interior sample of a planar tessellation with vertices and edges on sample centres is covered once."""
    v, f = ro.grid_plane(10, 9, 3.0, 2.0, 4.0)
    H = W = 48
    v[:, 1] = (H - 1) - v[:, 1]
    _, cnt = face_map(v, f, H, W, counts=True)
    interior = np.zeros((H, W), bool)
    interior[3:38, 4:43] = True                           # rows y = 2..38, columns x = 3..43
    assert (cnt[interior] == 1).all()
    assert cnt.max() == 1
    v2, f2 = ro.grid_plane(7, 7, 5.37, 4.11, 5.13, alt=False)      # off the sample grid
    _, cnt = face_map(v2, f2, H, W, counts=True)
    assert cnt.max() == 1 and (cnt == 1).sum() > 1000


def test_sphere_covers_inside_samples_exactly_twice():
    """A convex closed surface: every sample is covered by 0 or 2 faces (front and back), never 1 or 3."""
    v, f = ro.posed_sphere(5)
    assert v.shape == (1, 6890, 3) and f.shape == (13776, 3)
    H = W = 96
    cam = np.array([40, 40, 48, 48], np.float32)
    _, cnt = face_map(v[0], f, H, W, cam=cam, counts=True)
    assert set(np.unique(cnt)) == {0, 2}
    assert (cnt == 2).sum() > 2000


def test_cube_normals_and_lambert_terms():
    v = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], np.float64)
    # 12 outward triangles of the cube
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    f = np.array([t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))])
    n = ro.vertex_normals(v, f)
    # every corner sums two triangles per adjacent face or one: the corner direction, not necessarily normalised equally
    assert np.all(np.sign(n) == np.sign(v))
    col = ro.lambert_colors(v, f, (1, 1, 1), [((0, 0, 10), (1, 1, 1))])
    front = v[:, 2] > 0
    assert np.all(col[~front] >= 0) and np.all(col[front] > col[~front].max())
    # vertex (1, 1, 1): one light at (10, 0, 0) (left / right), colour = n . l
    c2 = ro.lambert_colors(v, f, (0.5, 1, 1), [((10, 0, 0), (1, 1, 1))])
    l = np.array([10, 0, 0.]) - v[7]
    want = np.clip(n[7] @ (l / np.linalg.norm(l)), 0, None) * np.array([0.5, 1, 1])
    np.testing.assert_allclose(c2[7], want, rtol=1e-12)
    # a vertex with no faces has the zero normal, so no light
    v3 = np.concatenate([v, [[5, 5, 5]]])
    assert np.all(ro.lambert_colors(v3, f, (1, 1, 1), [((0, 0, 10), (1, 1, 1))])[8] == 0)


def test_face_part_rule():
    vpart = np.array([3, 3, 7, -1, 7, 5, -1, -1])
    f = np.array([[0, 1, 2],       # two share 3          -> 4
                  [2, 4, 5],       # two share 7          -> 8
                  [5, 2, 0],       # all differ: lowest index 0 has 3 -> 4
                  [3, 5, 2],       # 3 has none: lowest with one is 2 (part 7) -> 8
                  [6, 7, 3],       # none -> 0
                  [6, 5, 3],       # only 5 -> 6
                  [1, 3, 0]])      # 1 and 0 share 3 (vertex 3 none) -> 4
    assert list(face_parts(f, vpart)) == [4, 8, 4, 8, 0, 6, 4]
    t = MeshTopology(f, 8, part_tables=(np.array([0, 1, 5, 2, 4]), np.array([0] * 4 + [2] * 2 + [3] * 2 + [5] * 25)))
    assert list(t.vertex_part) == [3, 3, 7, -1, 7, 5, -1, -1]
    assert list(t.face_part) == [4, 8, 4, 8, 0, 6, 4]
    t2 = MeshTopology(f, 8, face_part=np.arange(7))
    assert list(t2.face_part) == list(range(7))


def test_mesh_topology_csr_and_refusals():
    v, f = ro.uv_sphere()
    t = MeshTopology(f, 6890)
    assert t.vf_off[-1] == 3 * len(f) and len(t.vf_off) == 6891
    for vid in (0, 1, 500, 6889):
        inc = t.vf_face[t.vf_off[vid]:t.vf_off[vid + 1]]
        assert list(inc) == sorted(np.nonzero((f == vid).any(1))[0])
    assert t.face_part.max() <= 31
    for bad in (np.zeros((4, 2), np.int32), np.zeros((4, 3), np.float32), np.array([[0, 1, 8]]), np.array([[0, -1, 2]]),
                np.zeros(3, np.int32)):
        with pytest.raises(ValueError):
            MeshTopology(bad, 8)
    with pytest.raises(ValueError):
        MeshTopology(np.array([[0, 1, 2]]), 0)
    with pytest.raises(ValueError):
        MeshTopology(np.array([[0, 1, 2]]), 8, face_part=np.array([40]))


def test_pickle_faces_are_loaded(tmp_path):
    from ilps_amd.smpl_model import synthetic_smpl_model
    from ilps_amd.smpl_pkl import load_smpl_pkl
    m = synthetic_smpl_model(7)
    _, f = ro.uv_sphere()
    dd = {"v_template": m.v_template, "shapedirs": m.shapedirs, "posedirs": m.posedirs,
          "J_regressor": m.J_regressor, "weights": m.weights,
          "kintree_table": np.stack([np.where(m.parents < 0, 4294967295, m.parents), np.arange(24)]).astype(np.int64),
          "f": f.astype(np.uint32)}
    p = tmp_path / "smpl.pkl"
    p.write_bytes(pickle.dumps(dd, protocol=2))
    got = load_smpl_pkl(str(p))
    assert got.faces.dtype == np.int32 and np.array_equal(got.faces, f)
    assert synthetic_smpl_model(7).faces is None
    dd["f"] = np.array([[0, 1, 6890]])
    p.write_bytes(pickle.dumps(dd, protocol=2))
    with pytest.raises(ValueError):
        load_smpl_pkl(str(p))
    with pytest.raises(ValueError, match="faces"):
        render.SMPLRenderer(device="cpu")


def test_abi_entries_refuse_bad_arguments_without_a_gpu():
    from ilps_amd import _lib
    lib = _lib.load()
    one = 1

    def vtx(B=1, V=3, mode=0, H=16, W=16, shading=1, F=1, nl=0):
        return lib.smplr_mesh_vertex(one, one, None, B, V, mode, 1.0, H, W, 0.0, 1e30, shading, one, F, None, None, 0,
                                     None, nl, one, 0, one, None)

    def ras(B=1, V=3, F=1, H=16, W=16, mode=0):
        return lib.smplr_mesh_raster(one, one, None, B, V, F, H, W, mode, None, one, None, None, None, None, None)

    for kw, word in ((dict(H=0), b"image"), (dict(W=4097), b"image"), (dict(mode=2), b"mode"), (dict(V=0), b"sizes"),
                     (dict(V=(1 << 24) + 1), b"sizes"), (dict(F=(1 << 24) + 1), b"sizes"), (dict(B=-1), b"sizes")):
        assert vtx(**kw) == -1 and word in lib.smplr_last_error(), kw
        assert ras(**kw) == -1 and word in lib.smplr_last_error(), kw
    assert vtx(shading=3) == -1 and b"shading" in lib.smplr_last_error()
    assert vtx(nl=9, shading=0) == -1 and b"lights" in lib.smplr_last_error()
    assert vtx(shading=0) == -1 and b"lambert" in lib.smplr_last_error()      # no CSR, no light rig
    assert vtx(B=0) == 0 and ras(B=0) == 0                                    # an empty batch is a no-op
    assert lib.smplr_mesh_vbuf_bytes(128, 6890) == 128 * 6890 * 32 and lib.smplr_mesh_vbuf_bytes(0, 6890) == 0


def test_mesh_render_op_has_a_meta_kernel():
    from ilps_amd import torch_ops
    ns = torch_ops.load()
    assert str(ns.mesh_render.default._schema) == torch_ops.SCHEMAS["mesh_render"]
    m = lambda *s, dt=torch.float32: torch.empty(*s, dtype=dt, device="meta")
    light = [0.6, 0.7, 0.8] + [1.0] * 6
    outs = ns.mesh_render(m(2, 6890, 3), m(2, 4), None, m(13776, 3, dt=torch.int32), m(13776, dt=torch.uint8),
                          m(6891, dt=torch.int32), m(41328, dt=torch.int32), None, m(2, 200, 300, 3), light, 200, 300)
    assert [tuple(o.shape) for o in outs] == [(2, 200, 300), (2, 200, 300), (2, 200, 300), (2, 200, 300), (2, 200, 300, 3)]
    assert [o.dtype for o in outs] == [torch.int32, torch.float32, torch.uint8, torch.bool, torch.float32]
    outs = ns.mesh_render(m(3, 10, 3), m(3, 3), m(3, 3), m(4, 3, dt=torch.int32), None, None, None, m(10, 3), None, [],
                          64, 48, 1)
    assert tuple(outs[4].shape) == (3, 64, 48, 3)
    with pytest.raises(RuntimeError):                       # perspective takes (B, 3) cameras
        ns.mesh_render(m(3, 10, 3), m(3, 4), None, m(4, 3, dt=torch.int32), None, None, None, m(10, 3), None, [], 64, 48, 1)
    with pytest.raises(RuntimeError):
        ns.mesh_render(m(3, 10, 3), m(3, 4), None, m(4, 3, dt=torch.int32), None, None, None, m(10, 3), None, [], 0, 48)
    with pytest.raises(RuntimeError):
        ns.mesh_render(m(3, 10, 3), m(3, 4), None, m(4, 3, dt=torch.int32), None, None, None, None, None, [1.0], 8, 8)
    with pytest.raises((RuntimeError, NotImplementedError)):
        ns.mesh_render(torch.zeros(1, 3, 3), torch.zeros(1, 4), None, torch.zeros(1, 3, dtype=torch.int32), None, None,
                       None, torch.zeros(3, 3), None, [], 8, 8)


def test_render_mesh_refuses_cpu_and_bad_arguments():
    v, f = ro.uv_sphere()
    t = MeshTopology(f, 6890)
    with pytest.raises(RuntimeError):
        render.render_mesh(torch.zeros(1, 6890, 3), t, [1, 1, 0, 0], img_wh=32)
    with pytest.raises(ValueError):
        render.render_mesh(torch.zeros(1, 6890, 3), t, [1, 1, 0, 0], img_wh=32, mode="fisheye")


def test_smpl_renderer_call_surface_matches_the_reference():
    """renderer.py:33-43 and :86-96: the same parameters in the same order with the same defaults (plus trans)."""
    sig = inspect.signature(render.SMPLRenderer.__call__)
    want = [("verts", inspect._empty), ("cam", None), ("img", None), ("do_alpha", False), ("far", None), ("near", None),
            ("color_id", 0), ("img_size", None), ("render_seg", False)]
    got = [(n, p.default) for n, p in sig.parameters.items() if n != "self"]
    assert got[:len(want)] == want and got[len(want):] == [("trans", None)]
    rot = [(n, p.default) for n, p in inspect.signature(render.SMPLRenderer.rotated).parameters.items() if n != "self"]
    assert rot == [("verts", inspect._empty), ("deg", inspect._empty), ("cam", None), ("axis", "y"), ("img", None),
                   ("do_alpha", True), ("far", None), ("near", None), ("color_id", 0), ("img_size", None)]
    init = [(n, p.default) for n, p in inspect.signature(render.SMPLRenderer.__init__).parameters.items() if n != "self"]
    assert init[:2] == [("img_size", 224), ("flength", 500.)]
    np.testing.assert_allclose(render._rotation("y", 90), [[0, 0, 1], [0, 1, 0], [-1, 0, 0]], atol=1e-12)


def test_default_palette_is_distinct():
    p = render.default_palette()
    assert p.shape == (32, 3) and p.dtype == np.float32 and p.min() >= 0 and p.max() <= 1
    assert len({tuple(np.round(c, 4)) for c in p}) == 32


def test_render_kernels_fit_the_budget():
    """No scratch; the raster kernel's 32 KB z-buffer and registers leave four 256-thread workgroups per CU (the design
    counts on 4 x 32 KB of the CU's 160 KB), the vertex kernel full occupancy."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr
    ks = {n: k for n, k in kr.kernels().items() if "mesh_raster_kernel" in n or "mesh_vertex_kernel" in n}
    assert len(ks) == 2, sorted(ks)
    for name, k in ks.items():
        assert k["scratch"] == 0, name
        assert k["max_threads"] == 256, name
        if "raster" in name:
            assert k["lds"] == 64 * 64 * 8, name
            assert kr.waves_per_simd(k) >= 4, name          # 4 workgroups x 4 waves per CU = 4 waves per SIMD
        else:
            assert k["lds"] == 0 and kr.waves_per_simd(k) == 8, name
