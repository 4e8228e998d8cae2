"""Pose inputs by REGIME of the joint angle, and the bar each regime's gradient is held to.

`tests/_inputs.make_x` draws every joint at |theta| of 0.1 to 1.  Rodrigues' formula and its backward compute
`1 - cos`, `1 / angle` and `c dK - (dr . t) / angle^2`, which behave differently for |theta| <~ 1e-3, near pi, near
2 pi and beyond, and at a joint that is exactly 0.  `regime_batch` builds one batch of about 75 rows that visits all of
them; `reference` runs the float64 and the float32 oracle over it once and returns, per regime and column block, how
far the float32 ORACLE is from float64.  The HIP path is held to 4 x that figure (the margin
`test_blend3_matches_fp32_path` gives bf16x3 over the fp32 path), capped by `grad_close`'s 2e-3: the bar follows the
float32 reference regime by regime and is never taken from the HIP output.
"""
import numpy as np
import torch

from _inputs import make_x

W = 48
PI32, TWO_PI32 = float(np.float32(np.pi)), float(np.float32(2.0 * np.pi))
# (label, |theta_j|)
MAGNITUDES = (("0", 0.0), ("1e-7", 1e-7), ("1e-5", 1e-5), ("1e-4", 1e-4), ("1e-3", 1e-3), ("1e-2", 1e-2), ("1", 1.0),
              ("pi-1e-3", np.pi - 1e-3), ("pi", PI32), ("pi+1e-3", np.pi + 1e-3), ("2pi", TWO_PI32),
              ("2pi+1e-3", 2.0 * np.pi + 1e-3), ("7", 7.0), ("12", 12.0))
AXIS_MAGNITUDES = ("1e-4", "1", "pi")            # rows whose joints lie on a coordinate axis: two exact zeros per joint
SINGLE_JOINTS = (0, 9, 22)                       # root, a joint with three children, a leaf
TPOSE = "tpose"
REGIMES = tuple(l for l, _ in MAGNITUDES) + (TPOSE,)
SEEDS = (0, 1, 2)                                # cotangent seeds
FACTOR, CAP = 4.0, 2e-3
BLOCKS = ("theta", "beta")


def block_slice(block, num_cam=4):
    return slice(num_cam, num_cam + 72) if block == "theta" else slice(num_cam + 72, num_cam + 82)


def _unit(rng, n):
    d = rng.normal(size=(n, 3))
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def regime_batch(seed=2024):
    """-> x (B, 86) float32, rows: a list of (regime label, kind) with kind in 'all' | 'joint0' | 'joint9' | 'joint22' |
    'axis+x' ... 'axis-z' | 'tpose'.  Camera and beta of every row, and the joints a row does not set, are make_x's."""
    from ilps_amd.smpl_model import mean86
    rng = np.random.default_rng(seed)
    mags = dict(MAGNITUDES)
    thetas, rows = [], []                          # thetas: (24, 3) float64 with NaN = "keep make_x's"
    for label, m in MAGNITUDES:
        thetas.append(_unit(rng, 24) * m)
        rows.append((label, "all"))
        for j in SINGLE_JOINTS:
            th = np.full((24, 3), np.nan)
            th[j] = _unit(rng, 1)[0] * m
            thetas.append(th)
            rows.append((label, "joint%d" % j))
    for label in AXIS_MAGNITUDES:
        for ax in range(3):
            for sign in (1.0, -1.0):
                th = np.zeros((24, 3))
                th[:, ax] = sign * mags[label]
                thetas.append(th)
                rows.append((label, "axis%s%s" % ("+" if sign > 0 else "-", "xyz"[ax])))
    th = np.zeros((24, 3))
    th[0] = mean86(W)[4:7]
    thetas.append(th)
    rows.append((TPOSE, "tpose"))
    B = len(rows)
    x = make_x(B, W, seed=seed)
    for n, th in enumerate(thetas):
        keep = np.isnan(th)
        x[n, 4:76] = np.where(keep, x[n, 4:76].reshape(24, 3), th).astype(np.float32).reshape(72)
    # theta + 1e-8 is the zero vector in float32 where all three components are -1e-8: the reference formula divides by 0
    bad = (x[:, 4:76].reshape(B, 24, 3) == np.float32(-1e-8)).all(axis=2)
    assert not bad.any(), "a generated joint is (-1e-8, -1e-8, -1e-8): theta + 1e-8 = 0"
    return x, rows


def cotangents(B, seed):
    """gv (B, 6890, 3), gj (B, 24, 3): N(0, 1), float64 values that float32 holds exactly (every path gets the same)."""
    rng = np.random.default_rng(1000 + seed)
    f = lambda a: a.astype(np.float32).astype(np.float64)
    return f(rng.normal(0, 1, (B, 6890, 3))), f(rng.normal(0, 1, (B, 24, 3)))


def oracle_dx(model, x, dtype, num_cam=4, seeds=SEEDS, return_forward=False):
    """dx of (verts . gv + J_transformed . gj).sum() from TorchSMPL(model, dtype) autograd, per cotangent seed:
    (S, B, num_cam + 82) float64 [, verts, J_transformed as float64 arrays]."""
    from oracle.torch_oracle import TorchSMPL
    xo = torch.tensor(np.asarray(x), dtype=dtype, requires_grad=True)
    v, j, _ = TorchSMPL(model, dtype)(xo, num_cam=num_cam, return_all=True)
    out = []
    for s in seeds:
        gv, gj = cotangents(x.shape[0], s)
        loss = (v * torch.tensor(gv, dtype=dtype)).sum() + (j * torch.tensor(gj, dtype=dtype)).sum()
        out.append(torch.autograd.grad(loss, xo, retain_graph=True)[0].numpy().astype(np.float64))
    out = np.stack(out)
    if return_forward:
        return out, v.detach().numpy().astype(np.float64), j.detach().numpy().astype(np.float64)
    return out


def oracle_dx_proj(model, x, dtype, gv, gp, gj):
    """x (B, 86): dx of (verts . gv + projection . gp + J_transformed . gj).sum() from the oracle in `dtype`
    -> dx (B, 86), verts, projection (B, V, 3), float64 arrays."""
    from oracle import torch_oracle as to
    xo = torch.tensor(np.asarray(x), dtype=dtype, requires_grad=True)
    v, j, _ = to.TorchSMPL(model, dtype)(xo, return_all=True)
    p = to.orthographic_project(v, xo)
    c = lambda a: torch.tensor(a, dtype=dtype)
    ((v * c(gv)).sum() + (p * c(gp)).sum() + (j * c(gj)).sum()).backward()
    f = lambda a: a.detach().numpy().astype(np.float64)
    return f(xo.grad), f(v), f(p)


def block_errors(d, d64, num_cam=4):
    """err[block] (..., B): max|d - d64| / max|d64| within each row's column block."""
    out = {}
    for b in BLOCKS:
        sl = block_slice(b, num_cam)
        out[b] = np.abs(d[..., sl] - d64[..., sl]).max(axis=-1) / np.abs(d64[..., sl]).max(axis=-1)
    return out


def regime_max(err_rows, rows):
    """err_rows (..., B) -> {regime: max over the regime's rows and every leading axis}."""
    e = np.asarray(err_rows).reshape(-1, len(rows)).max(axis=0)
    return {r: max(float(e[n]) for n, (lab, _) in enumerate(rows) if lab == r) for r in REGIMES}


_cache = {}


def reference(model):
    """The regime batch through both oracles, once per process: dict(x, rows, d64 (S, B, 86), verts, J_transformed,
    Rs (B, 24, 3, 3) - all float64 -, ref_err {block: {regime: float}}, bar {block: {regime: float}})."""
    if "ref" not in _cache:
        from oracle import torch_oracle as to
        x, rows = regime_batch()
        d64, verts, jt = oracle_dx(model, x, torch.float64, return_forward=True)
        d32 = oracle_dx(model, x, torch.float32)
        err = block_errors(d32, d64)
        ref_err = {b: regime_max(err[b], rows) for b in BLOCKS}
        bar = {b: {r: min(FACTOR * e, CAP) for r, e in ref_err[b].items()} for b in BLOCKS}
        th = torch.tensor(x[:, 4:76].reshape(-1, 3), dtype=torch.float64)
        Rs = to.batch_rodrigues(th).numpy().reshape(len(rows), 24, 3, 3)
        _cache["ref"] = dict(x=x, rows=rows, d64=d64, d32=d32, verts=verts, J_transformed=jt, Rs=Rs, ref_err=ref_err,
                             bar=bar)
    return _cache["ref"]


def make_x_cam(B, num_cam, seed):
    """x (B, num_cam + 82) float32: make_x's theta and beta behind `num_cam` camera columns - make_x's own four where
    there is room for them, seeded filler behind."""
    x86 = make_x(B, W, seed=seed)
    cam = np.random.default_rng(seed + 7).normal(0, 10.0, (B, num_cam)).astype(np.float32)
    k = min(num_cam, 4)
    cam[:, :k] = x86[:, :k]
    return np.concatenate([cam, x86[:, 4:]], axis=1)
