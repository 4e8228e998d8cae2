"""SMPL+D through the SMPL layer on the GPU: `SMPLLayer(x, offsets=D)` (ops.BatchSMPLOffsetFn) against the float64 torch
restatement of oracle/torch_oracle.py with v_posed + D, on the `smpl_model` fixture (V = 6 890) with B = 2 and 3.

Bars, taken from the files that hold the same quantities without offsets:
  verts  1e-4 absolute (the README's; test_gpu_parity.VERT_ATOL);
  dD     is smplr_skin_bwd's dv_posed: tests/test_gpu_skin_small.py's 2 n 2^-24 mag with n = 27, against the float64
         skinning backward of _smpl_bwd_oracle.oracle fed the fp32 v_posed + D and A the forward saved;
  dx     tests/test_gpu_smpl_bwd_small.py's K 2^-24 mag_dx, K = _smpl_bwd_oracle.k_general(V, 0, gemm) + K_pose, against that
         file's staged float64 reference (stages S, G, P) linearised at the float64 forward with v_posed + D; K_pose is
         `_smpl_bwd_oracle.k_pose`'s recipe - 4 x the float32 pose stage's own error - measured on this file's rows.
Bit for bit: zero offsets give the verts of the layer without offsets; dx and dD equal smplr_skin_bwd -> smplr_blend3_bwd ->
smplr_pose_bwd called by hand on the saved forward; with only D requiring a gradient dD keeps its bits."""
import functools

import numpy as np
import pytest
import torch

import _smpl_bwd_oracle as so
from test_gpu_parity import VERT_ATOL, dev, t

pytestmark = pytest.mark.gpu

V = 6890
U = 2.0 ** -24


@functools.lru_cache(maxsize=None)
def inputs(B):
    rng = np.random.default_rng(77 + B)
    d = dict(x=np.array(so.x_rows(B)), D=rng.normal(0, 0.01, (B, V, 3)).astype(np.float32),
             dverts=rng.normal(0, 1, (B, V, 3)).astype(np.float32), dJt=rng.normal(0, 1, (B, 24, 3)).astype(np.float32))
    for a in d.values():
        a.setflags(write=False)
    return d


def same_constants(model):
    """The staged reference takes its blend shapes and joint regressor from _smpl_bwd_oracle.model(V): the fixture's."""
    m = so.model(V)
    for k in ("v_template", "shapedirs", "posedirs", "J_regressor"):
        assert np.array_equal(np.asarray(getattr(m, k)), np.asarray(getattr(model, k))), k


@functools.lru_cache(maxsize=None)
def staged(B, with_jt):
    """_smpl_bwd_oracle.staged with v_posed + D: float64 dx, mag_dx (B, 86), verts (B, V, 3)."""
    inp = inputs(B)
    w = WEIGHTS[0]
    fw = so.forward(V, B)
    c = dict(V=V, vs=1, vp=fw["vp"] + inp["D"].astype(np.float64), A=fw["A"], x=inp["x"])
    o = so.oracle(c, w, inp["dverts"], None)
    bt = so.blend_t(V)
    dcoef = o["dv_posed"].reshape(B, 3 * V) @ bt
    mag_dcoef = o["mag_dv_posed"].reshape(B, 3 * V) @ np.abs(bt)
    z = inp["dJt"].astype(np.float64).reshape(B, 72) if with_jt else np.zeros((B, 72))
    cot = np.concatenate([dcoef, o["dA"].reshape(B, 288), z], axis=1)
    mag = np.concatenate([mag_dcoef, o["mag_dA"].reshape(B, 288), np.abs(z)], axis=1)
    Jp = so.jacobian(V, B)
    dx = np.einsum("bko,bk->bo", Jp, cot)
    mag_dx = np.einsum("bko,bk->bo", np.abs(Jp), mag)
    dx32 = so.pose_vjp32(V, B, cot, np.zeros((B, 4)))
    lim = U * mag_dx
    k_pose = 4.0 * float((np.abs(dx32 - dx)[lim > 0] / lim[lim > 0]).max())
    return dict(dx=dx, mag_dx=mag_dx, verts=o["verts"], k_pose=k_pose)


WEIGHTS = [None]


def layer_and_consts(smpl_model):
    from ilps_amd.keras_smpl.batch_smpl import SMPLLayer
    same_constants(smpl_model)
    WEIGHTS[0] = np.asarray(smpl_model.weights, np.float32)
    layer = SMPLLayer(smpl_model)
    return layer, layer.constants(dev())


def run(layer, B, x_grad=True, with_jt=False):
    inp = inputs(B)
    x = t(np.array(inp["x"])).requires_grad_(x_grad)
    D = t(np.array(inp["D"])).requires_grad_(True)
    verts = layer(x, offsets=D)
    outs, cots = [verts], [t(np.array(inp["dverts"]))]
    if with_jt:
        outs, cots = outs + [layer.J_transformed], cots + [t(np.array(inp["dJt"]))]
    g = torch.autograd.grad(outs, [x, D] if x_grad else [D], cots)
    torch.cuda.synchronize()
    return verts.detach(), (g[0] if x_grad else None), g[-1]


def by_hand(c, B, with_jt):
    """The forward's launches and the three backward entry points, called here -> verts, dx, dv_posed, and the saved
    v_posed + D and A."""
    from ilps_amd import _lib, ops
    from ilps_amd._lib import check, ptr, stream
    lib = _lib.load()
    inp = inputs(B)
    d = dev()
    x, D, dverts = t(np.array(inp["x"])), t(np.array(inp["D"])), t(np.array(inp["dverts"]))
    dJt = t(np.array(inp["dJt"])) if with_jt else None
    Rs, J, A, Jt, vp = ops._pose_blend_fwd(x, 4, c)
    vp = vp + D
    verts, _ = ops._skin_fwd(vp, A, c)
    dvp, dA = torch.empty(B, V, 3, device=d), torch.empty(B, 24, 12, device=d)
    ws = torch.empty(lib.smplr_skin_bwd_workspace(B, V) // 4 + 1, device=d)
    check(lib.smplr_skin_bwd(ptr(dverts), None, ptr(vp), ptr(c.lbs_weights), ptr(c.lbs_top4), ptr(A), ptr(x), 86, B, V, 1,
                             ptr(dvp), ptr(dA), None, ptr(ws), stream()), "smplr_skin_bwd")
    dcoef = torch.empty(B, 220, device=d)
    ws2 = torch.empty(lib.smplr_blend3_bwd_workspace(B, 3 * V) // 4 + 1, device=d)
    check(lib.smplr_blend3_bwd(ptr(dvp), ptr(c.blend3_bwd), B, 3 * V, ptr(dcoef), ptr(ws2), stream()), "smplr_blend3_bwd")
    dx = torch.empty(B, 86, device=d)
    check(lib.smplr_pose_bwd(ptr(x), 86, 4, B, ptr(c.J_dirs), ptr(c.parents), ptr(Rs), ptr(J), ptr(A), ptr(dcoef), ptr(dA),
                             ptr(dJt), None, ptr(dx), stream()), "smplr_pose_bwd")
    torch.cuda.synchronize()
    return verts, dx, dvp, vp, A


def test_zero_offsets_change_nothing(smpl_model):
    layer, _ = layer_and_consts(smpl_model)
    x = t(np.array(inputs(3)["x"]))
    with torch.no_grad():
        plain = layer(x)
        jt = layer.J_transformed
        zero = layer(x, offsets=torch.zeros(3, V, 3, device=dev()))
        assert torch.equal(zero, plain) and torch.equal(layer.J_transformed, jt)
        moved = layer(x, offsets=t(np.array(inputs(3)["D"])))
        assert torch.equal(layer.J_transformed, jt), "the joints must not see D"
        assert not torch.equal(moved, plain)
    with pytest.raises(RuntimeError):
        layer(x, offsets=torch.zeros(3, V - 1, 3, device=dev()))


@pytest.mark.parametrize("B,with_jt", [(2, False), (3, True)])
def test_against_float64_and_the_chain(smpl_model, B, with_jt):
    layer, c = layer_and_consts(smpl_model)
    assert c.blend3_bwd is not None
    inp = inputs(B)
    verts, dx, dD = run(layer, B, True, with_jt)
    ref = staged(B, with_jt)
    ev = float(np.abs(verts.cpu().numpy() - ref["verts"]).max())
    print("VERTS B=%d: max |verts - float64| = %.3e" % (B, ev))
    assert ev <= VERT_ATOL
    # dx: test_gpu_smpl_bwd_small.py's bar
    K = so.k_general(V, 0, "bf16x3") + ref["k_pose"]
    r = so.ratio(dx.cpu().numpy(), ref, K)
    print("DX B=%d: K = %.1f (K_pose %.2f), error / bar %.4f" % (B, K, ref["k_pose"], r))
    assert r <= 1.0
    # the chain by hand: the same bits
    hv, hdx, hdvp, vp, A = by_hand(c, B, with_jt)
    assert torch.equal(hv, verts) and torch.equal(hdx, dx) and torch.equal(hdvp, dD)
    # dD: test_gpu_skin_small.py's bar for dv_posed, at the fp32 forward the backward was linearised at
    o = so.oracle(dict(V=V, vs=1, vp=vp.cpu().numpy(), A=A.cpu().numpy(), x=inp["x"]), WEIGHTS[0], inp["dverts"], None)
    err, bar = np.abs(dD.cpu().numpy().astype(np.float64) - o["dv_posed"]), 2 * 27 * U * o["mag_dv_posed"]
    print("DD B=%d: max err / bar %.4f" % (B, float((err / np.maximum(bar, 1e-300)).max())))
    assert np.all(err <= bar)
    # two runs: the same bits
    verts2, dx2, dD2 = run(layer, B, True, with_jt)
    assert torch.equal(verts2, verts) and torch.equal(dx2, dx) and torch.equal(dD2, dD)


def test_only_offsets_require_a_gradient(smpl_model):
    layer, c = layer_and_consts(smpl_model)
    verts, dx, dD = run(layer, 2, True, False)
    verts1, none, dD1 = run(layer, 2, False, False)
    assert none is None and torch.equal(verts1, verts) and torch.equal(dD1, dD)


def test_scan_fitter_passes_offsets_on(smpl_model):
    from ilps_amd.fitting import ScanFitter
    from test_gpu_scan import body_topology               # (the synthetic model carries no faces: a soup over its vertices)
    layer, _ = layer_and_consts(smpl_model)
    sf = ScanFitter(layer, body_topology()[0])
    inp = inputs(2)
    x, D = t(np.array(inp["x"])), t(np.array(inp["D"]))
    x[:, 0], x[:, 1:4] = 1.5, 0.25
    with torch.no_grad():
        placed = sf.place(x, D)
        assert torch.equal(placed, x[:, 0, None, None] * layer(x, offsets=D) + x[:, None, 1:4])
        assert torch.equal(sf.place(x, torch.zeros_like(D)), sf.place(x))
        pts = placed[:, ::7].contiguous()
        a = sf.terms(x, pts, None, offsets=D)
        b = sf.terms(x, pts, None, verts=placed)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
