"""seg_bin_own_kernel (the binning workgroup masks, classifies and places each vertex from the registers it skinned it in)
against seg_bin_kernel<true, true, true> (classification in table order, SMPLR_SEG_BIN_WALK=0) on one library in one process, and against
the float64 oracle.  Between the two forms: verts, proj, mask, the far-reaching section of rec with its header, goff,
lstart and seg bit for bit; the nearest-pixel records of each pixel as a set (either form takes their order inside a
pixel from an LDS atomic); x_grad within grad_close(2e-5) of each other, bit for bit in the deterministic mode."""
import types

import numpy as np
import pytest
import torch

from _inputs import make_x
from test_gpu_parity import SEG_ATOL, SEG_RTOL, VERT_ATOL, grad_close

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _ws_views(ws, B, W, P, K):
    """goff (B, P + 34), lstart (B, W^2 + 1), lrec (B, K, 2) of a binned workspace (raster_common.h: seg_ws_layout)."""
    raw = ws.view(torch.int32).cpu().numpy()
    up = lambda nbytes: (nbytes + 255) // 256 * 256
    gs, npix = P + 2 + 32, W * W
    o1 = up(B * gs * 4) // 4
    o2 = o1 + up(B * (npix + 1) * 4) // 4
    return (raw[:B * gs].reshape(B, gs), raw[o1:o1 + B * (npix + 1)].reshape(B, npix + 1),
            raw[o2:o2 + B * K * 2].reshape(B, K, 2))


def _bin(monkeypatch, on, v_posed, A, c, cam, W, pt, grid_wh=64, ref_compat=True):
    """One call of the skinning + binning + raster entry point -> every output and the workspace, on the host."""
    from ilps_amd import _lib, ops
    monkeypatch.setenv("SMPLR_SEG_BIN_WALK", "1" if on else "0")
    lib = _lib.load()
    B, V = v_posed.shape[0], c.V
    e = lambda shape, dt=torch.float32: torch.full(shape, -7, dtype=dt, device=v_posed.device)
    ws = ops._workspace(lib.smplr_seg_workspace(B, V, W, pt.P, pt.K), v_posed)
    o = dict(verts=e((B, V, 3)), proj=e((B, V, 3)), mask=e((B, V)), seg=e((B, W, W, pt.P + 1)),
             arg=e((B, W, W, 32), torch.int16), rec=e((B, lib.smplr_seg_slots(pt.P, pt.K), 4)),
             vslot=e((B, V), torch.int16))
    with torch.cuda.device(v_posed.device):
        ops._skin_vis_seg_call(v_posed, A, c, cam, W, pt, grid_wh, ref_compat, ws, **o)
        torch.cuda.synchronize()
    out = {k: t.cpu().numpy() for k, t in o.items()}
    out["goff"], out["lstart"], out["lrec"] = _ws_views(ws, B, W, pt.P, pt.K)
    out["goff"] = out["goff"][:, :2 * pt.P + 2]      # offsets [P + 1] | unit-weight flag | parts by size [P]; the rest is unused
    return out


def _same_binning(a, b, P, W):
    """The comparisons between the two forms (module docstring)."""
    for k in ("verts", "proj", "mask", "seg", "goff", "lstart"):
        assert np.array_equal(a[k].view(np.int32) if a[k].dtype == np.float32 else a[k],
                              b[k].view(np.int32) if b[k].dtype == np.float32 else b[k]), k
    ra, rb = a["rec"].view(np.int32), b["rec"].view(np.int32)
    npix = W * W
    for n in range(ra.shape[0]):
        far, L = int(a["goff"][n, P]), int(a["lstart"][n, npix])
        assert np.array_equal(ra[n, :far], rb[n, :far]), "far-reaching records of mesh %d" % n
        assert np.array_equal(ra[n, -1], rb[n, -1]), "header of mesh %d" % n
        # nearest-pixel records: (pixel, vertex) orders each list; fields, (x bits, part) and the vertex' slot range agree
        pix = np.repeat(np.arange(npix), np.diff(a["lstart"][n]))
        assert pix.size == L
        oa, ob = np.lexsort((ra[n, far:far + L, 3], pix)), np.lexsort((rb[n, far:far + L, 3], pix))
        assert np.array_equal(ra[n, far:far + L][oa], rb[n, far:far + L][ob]), "nearest-pixel records of mesh %d" % n
        assert np.array_equal(a["lrec"][n, :L][oa], b["lrec"][n, :L][ob]), "(x, part) of mesh %d" % n
        for o in (a, b):                               # the vertex -> slot map is inverse to its own records
            sl = o["vslot"][n].astype(np.int64)
            own = sl >= 0
            assert int(own.sum()) == int((o["rec"].view(np.int32)[n, :far + L, 3] >= 0).sum())
            assert np.array_equal(o["rec"].view(np.int32)[n, sl[own], 3], np.flatnonzero(own))
        fa = a["vslot"][n] < far
        assert np.array_equal(a["vslot"][n] >= 0, b["vslot"][n] >= 0)
        assert np.array_equal(a["vslot"][n][fa], b["vslot"][n][fa])


def _against_oracle(out, ids, off, W, grid_wh=64, ref_compat=True):
    from oracle import np_oracle as o
    proj = out["proj"].astype(np.float64)
    mask = o.compute_mask(proj, grid_wh, ref_compat)
    assert np.array_equal(mask, out["mask"])
    # (the oracle takes a maximum over each part's vertices: an empty part, whose channel is 0 everywhere, is left out
    # of its table and put back as zeros)
    full = [p for p in range(len(off) - 1) if off[p + 1] > off[p]]
    off_full = [off[p] for p in full] + [off[-1]]
    some = o.projects_to_seg(proj, mask, W, ids, off_full)
    want = np.zeros(some.shape[:3] + (len(off),), some.dtype)
    want[..., [0] + [1 + p for p in full]] = some
    assert out["seg"].shape == want.shape
    assert np.all(np.abs(out["seg"] - want) <= SEG_RTOL * np.abs(want) + SEG_ATOL)


@pytest.fixture(scope="module")
def ref_inputs(smpl_model):
    """B = 3 seeded rows through pose and blend, once: v_posed, A, x, the constants and the float64 vertices."""
    from ilps_amd import ops
    from oracle import np_oracle as o
    c = ops.SMPLConstants.from_model(smpl_model, torch.device(DEV))
    per_w = {}
    for W in (16, 48):
        xn = make_x(3, W, seed=77 + W)
        x = torch.tensor(xn, device=DEV)
        coef, Rs, J, A, Jt = ops._pose_fwd(x, 4, c)
        per_w[W] = (x, A, ops._blend_fwd(coef, c, 3), o.smpl_layer_call(xn.astype(np.float64), smpl_model))
    return c, per_w


@pytest.mark.parametrize("W", [16, 48])
def test_reference_topology(monkeypatch, ref_inputs, part_tables, W):
    from ilps_amd import ops
    c, per_w = ref_inputs
    x, A, vp, want_verts = per_w[W]
    pt = ops.get_part_table(1, torch.device(DEV), c.V)
    assert pt.inv is not None and pt.K == 6879 and c.V - pt.K == 11
    new, old = _bin(monkeypatch, True, vp, A, c, x, W, pt), _bin(monkeypatch, False, vp, A, c, x, W, pt)
    _same_binning(new, old, pt.P, W)
    assert np.abs(new["verts"] - np.asarray(want_verts, np.float64).reshape(new["verts"].shape)).max() <= VERT_ATOL
    _against_oracle(new, *part_tables[1], W)


@pytest.mark.parametrize("deterministic", [True, False])
def test_reference_topology_gradient(monkeypatch, smpl_model, deterministic):
    from ilps_amd.decoder import SMPLDecoder
    W, B = 48, 3
    x = torch.tensor(make_x(B, W, seed=125), device=DEV)
    dseg = torch.randn(B, W, W, 32, generator=torch.Generator().manual_seed(2)).to(DEV)
    dec = SMPLDecoder(smpl_model, img_wh=W, deterministic=deterministic)
    grads = []
    for on in ("1", "0"):
        monkeypatch.setenv("SMPLR_SEG_BIN_WALK", on)
        xg = x.clone().requires_grad_(True)
        out = dec(xg)
        out["seg"].backward(dseg)
        torch.cuda.synchronize()
        grads.append((out["seg"].detach().clone(), xg.grad.detach().cpu().numpy()))
    assert torch.equal(grads[0][0], grads[1][0])
    if deterministic:
        assert np.array_equal(grads[0][1], grads[1][1])
    else:
        grad_close(grads[0][1], grads[1][1], 2e-5, "dx (from registers) vs dx (table order)")


def _toy(V=300, B=2, W=8, seed=5, off=(0, 60, 60, 127, 200, 280)):
    """A mesh whose projection is chosen directly: one joint of weight 1 (or two of 1/2) per vertex, every joint matrix
    [I | t_j], camera (1, 1, 0, 0) -> proj = v_posed + t_j.  Parts 0..4 over a random order of the vertices: part 1
    empty, part 2 of 67 slots, 20 vertices in no part (`off`: another layout over the first off[-1] of that order).  In
    mesh 0 an un-owned vertex lies in front of an owned one in grid cell (3, 4), where the table leaves eleven un-owned
    (else b is None)."""
    rng = np.random.default_rng(seed)
    top4 = np.zeros((V, 8), np.float32)
    top4[:, 0] = 1.0
    top4[:, 4] = rng.integers(0, 24, V)
    two = rng.random(V) < 0.3
    top4[two, 0] = top4[two, 1] = 0.5
    top4[two, 5] = rng.integers(0, 24, int(two.sum()))
    tj = rng.integers(-2, 3, (24, 3)).astype(np.float32) * 0.25
    A = np.zeros((B, 24, 3, 4), np.float32)
    A[:, :, np.arange(3), np.arange(3)] = 1.0
    A[..., 3] = tj
    target = np.concatenate([rng.uniform(-1.0, W + 1.0, (B, V, 2)), rng.normal(0, 1, (B, V, 1))], axis=2).astype(np.float32)
    perm = rng.permutation(V)
    off = list(off)
    K = off[-1]
    ids = [int(v) for v in perm[:K]]
    a, b = int(perm[3]), (int(perm[K + 10]) if V > K + 10 else None)
    if b is not None:
        target[0, a] = [3.2, 4.1, 0.0]
        target[0, b] = [2.9, 3.8, 5.0]
    shift = top4[:, 0:1] * tj[top4[:, 4].astype(int)] + top4[:, 1:2] * tj[top4[:, 5].astype(int)]
    v_posed = target - shift[None]
    cam = np.tile(np.array([1.0, 1.0, 0.0, 0.0], np.float32), (B, 1))
    dense = np.zeros((V, 24), np.float32)                  # (the separate skinning launch wants the dense rows beside top4)
    np.add.at(dense, (np.arange(V), top4[:, 4].astype(int)), top4[:, 0])
    np.add.at(dense, (np.arange(V), top4[:, 5].astype(int)), top4[:, 1])
    c = types.SimpleNamespace(V=V, lbs_top4=torch.tensor(top4, device=DEV), lbs_weights=torch.tensor(dense, device=DEV))
    td = lambda x: torch.tensor(np.ascontiguousarray(x), device=DEV)
    return c, td(v_posed), td(A.reshape(B, 24, 12)), td(cam), ids, off, target, (a, b)


def test_small_mesh_with_unowned_vertices(monkeypatch):
    from ilps_amd import ops
    V, W = 300, 8
    c, vp, A, cam, ids, off, target, (a, b) = _toy(V=V, W=W)
    pt = ops.build_part_table(ids, off, None, V, torch.device(DEV))
    assert pt.inv is not None
    new, old = _bin(monkeypatch, True, vp, A, c, cam, W, pt), _bin(monkeypatch, False, vp, A, c, cam, W, pt)
    _same_binning(new, old, pt.P, W)
    assert np.abs(new["verts"] - target.astype(np.float64)).max() <= VERT_ATOL
    _against_oracle(new, ids, off, W)
    # the un-owned vertex b takes cell (3, 4) from the owned vertex a, and has no record
    assert new["mask"][0, b] == 1.0 and new["mask"][0, a] == 500.0 and new["vslot"][0, b] == -1
    assert new["goff"][0, 1] == new["goff"][0, 2]                       # the empty part


def test_duplicate_id_keeps_the_table_order_form(monkeypatch):
    """A table that lists a vertex twice gives no walk table and no table by vertex: the table-order form runs whatever the switch
    says (forward only: the backward keeps one slot per vertex, ops.build_part_table refuses such a table)."""
    from ilps_amd import ops
    V, W = 300, 8
    c, vp, A, cam, ids, off, _, _ = _toy(V=V, W=W, seed=6)
    ids[100] = ids[10]
    assert ops.build_walk_table(ids, V) is None and ops._part_inv(ids, off, V) is None
    dev = torch.device(DEV)
    pt = ops.PartTable(P=5, K=len(ids), part_pos=torch.tensor(ids, dtype=torch.int32, device=dev),
                       part_off=torch.tensor(off, dtype=torch.int32, device=dev), VP=V)
    new, old = _bin(monkeypatch, True, vp, A, c, cam, W, pt), _bin(monkeypatch, False, vp, A, c, cam, W, pt)
    for k in ("verts", "proj", "mask", "seg", "goff", "lstart"):
        assert np.array_equal(new[k], old[k]), k
    _against_oracle(new, ids, off, W)


def test_hostile_rows(monkeypatch, ref_inputs):
    """The row recipes of test_gpu_hostile_inputs.py: a NaN pose parameter, every vertex on one pixel, every vertex
    outside the image and the grid - beside two ordinary rows."""
    from ilps_amd import ops
    c, _ = ref_inputs
    W = 48
    xn = make_x(5, W, 4242)
    xn[1, 10] = np.nan
    xn[2, 0:4] = [0.0, 0.0, 24.0, 24.0]
    xn[3, 2:4] = [1e4, -1e4]
    x = torch.tensor(xn, device=DEV)
    coef, Rs, J, A, Jt = ops._pose_fwd(x, 4, c)
    vp = ops._blend_fwd(coef, c, 5)
    pt = ops.get_part_table(1, torch.device(DEV), c.V)
    new, old = _bin(monkeypatch, True, vp, A, c, x, W, pt), _bin(monkeypatch, False, vp, A, c, x, W, pt)
    _same_binning(new, old, pt.P, W)
    assert np.array_equal(new["arg"][..., 0], old["arg"][..., 0])
    assert int((new["mask"][2] == 1.0).sum()) == 2 and int((new["mask"][3] == 1.0).sum()) == 1
    assert int((new["mask"][1] == 1.0).sum()) == 1 and np.isnan(new["verts"][1]).all()
