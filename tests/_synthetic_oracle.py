"""NumPy restatement of `proxy_inputs` (include/smplraster.h, `ilps_amd.synthetic`): the label logic in integers, the heat
channels' d2 and the product d2 * inv2s2 in np.float32 arithmetic - IEEE, one rounding per operation, no FMA, hence bit-equal
to the contraction-off kernel, so the `d2 <= cut2` decision is the kernel's - and the exponential in float64 of that fp32
argument.

Test infrastructure only; nothing here is imported by the package."""
import numpy as np

SEG_MODES = {"index": 0, "onehot": 1, "silhouette": 2, "none": 3}


def heat_constants(sigma, cut=6.0):
    """(inv2s2, cut2) as np.float32: formed in double, rounded once."""
    return np.float32(1.0 / (2.0 * float(sigma) * float(sigma))), np.float32((float(cut) * float(sigma)) ** 2)


def corrupted_labels(part, P, remove=None, boxes=None):
    """l' (B, H, W) int64."""
    part = np.asarray(part)
    B, H, W = part.shape
    lab = part.astype(np.int64)
    out = lab.copy()
    out[lab > P] = 0
    ys, xs = np.arange(H)[:, None], np.arange(W)[None, :]
    for b in range(B):
        if remove is not None:
            r = int(np.asarray(remove)[b]) & 0xFFFFFFFF
            for p in range(1, 32):                      # bit 0 is ignored
                if (r >> p) & 1:
                    out[b][lab[b] == p] = 0
        if boxes is not None:
            for x0, y0, x1, y1 in np.asarray(boxes)[b].astype(np.int64):
                out[b][(xs >= x0) & (xs < x1) & (ys >= y0) & (ys < y1)] = 0
    return out


def proxy_inputs(part, joints=None, keep=None, remove=None, boxes=None, P=31, seg="index", rescale=None, sigma=4.0, cut=6.0):
    """-> (values (B, C, H, W) float64, on (B, J, H, W) bool: where a heat value is exp(...) and not the literal 0).
    Seg channels hold exactly representable fp32 numbers (the index mode's product is formed in np.float32)."""
    part = np.asarray(part)
    B, H, W = part.shape
    lab = corrupted_labels(part, P, remove, boxes)
    planes = []
    if seg == "index":
        rs = np.float32(1.0 / P if rescale is None else rescale)
        planes.append((lab.astype(np.float32) * rs).astype(np.float64)[:, None])
    elif seg == "onehot":
        planes.append((lab[:, None] == np.arange(P + 1)[None, :, None, None]).astype(np.float64))
    elif seg == "silhouette":
        planes.append((lab > 0).astype(np.float64)[:, None])
    elif seg != "none":
        raise ValueError(seg)
    J = 0 if joints is None else np.asarray(joints).shape[1]
    on = np.zeros((B, J, H, W), bool)
    if J:
        inv2s2, cut2 = heat_constants(sigma, cut)
        j = np.asarray(joints, np.float32)
        xs = np.arange(W, dtype=np.float32)[None, None, None, :]
        ys = np.arange(H, dtype=np.float32)[None, None, :, None]
        with np.errstate(invalid="ignore", over="ignore"):
            dx = xs - j[:, :, 0, None, None]
            dy = ys - j[:, :, 1, None, None]
            d2 = (dx * dx).astype(np.float32) + (dy * dy).astype(np.float32)
            assert d2.dtype == np.float32
            arg = (d2 * inv2s2).astype(np.float32)
            fin = np.isfinite(j).all(-1)[:, :, None, None]
            on = fin & (d2 <= cut2)
            if keep is not None:
                on = on & (np.asarray(keep) != 0)[:, :, None, None]
            heat = np.where(on, np.exp(-arg.astype(np.float64)), 0.0)
        planes.append(heat)
    return np.concatenate(planes, 1), on


# ---- the cases the CPU and the GPU tests share ------------------------------------------------------------------------------
SHAPES = ((8, 8), (6, 12), (5, 7), (9, 5))          # (H, W): 16-B path (W % 4 == 0), one-column path, non-square
SPECIAL_JOINTS = ((2.0, 3.0), (2.5, 1.5), (np.nan, 1.0), (np.inf, 2.0), (3.0, -np.inf), (1e30, 1.0), (-1000.0, 5000.0))


def box_kinds(H, W):
    """empty, inverted, partly outside, wholly outside, covering the image, and one ordinary box."""
    return np.array([(2, 1, 2, 4), (4, 3, 1, 1), (-3, -2, 3, 2), (W + 5, 1, W + 9, 3), (-10, -10, W + 10, H + 10),
                     (1, 2, W - 1, H - 1)], np.int32)


def make_case(H, W, B, J, P, NB, variant):
    """One operand set (numpy).  `variant` (an integer) rotates which special joint, box kind, remove mask and keep form a
    small case gets, so that the cases of a test cover all of them between them."""
    rng = np.random.default_rng(1000 * variant + 10 * H + W + B + J + P + NB)
    part = rng.integers(0, P + 1, (B, H, W)).astype(np.uint8)
    above = rng.uniform(size=part.shape) < 0.1
    part[above] = rng.integers(P + 1, 256, int(above.sum())).astype(np.uint8)      # labels above P
    joints = keep = None
    if J:
        joints = np.stack([rng.uniform(-1, W, (B, J)), rng.uniform(-1, H, (B, J))], -1).astype(np.float32)
        for b in range(B):
            for k in range(min(J, len(SPECIAL_JOINTS))):
                joints[b, k] = SPECIAL_JOINTS[(k + b + variant) % len(SPECIAL_JOINTS)]
        if variant % 2:
            keep = (rng.uniform(size=(B, J)) < 0.6).astype(np.uint8)
            keep[:, 0] = np.arange(B) % 2
    masks = (0, 1 << (1 + variant % P), -1, (1 << 31) - 1 if P < 31 else -(1 << 31))
    remove = None if variant % 3 == 2 else np.array([masks[(b + variant) % len(masks)] for b in range(B)], np.int32)
    boxes = None
    if NB:
        kinds = box_kinds(H, W)
        boxes = np.stack([[kinds[(b + i + variant) % len(kinds)] for i in range(NB)] for b in range(B)]).astype(np.int32)
    return {"part": part, "joints": joints, "keep": keep, "remove": remove, "boxes": boxes, "P": P,
            "sigma": (0.5, 4.0)[(variant // 2) % 2]}


def case_grid(H, W):
    """Every (B, J, P, NB) of {1, 3} x {0, 1, 64} x {1, 31} x {0, 4} with a running variant."""
    v = 0
    for B in (1, 3):
        for J in (0, 1, 64):
            for P in (1, 31):
                for NB in (0, 4):
                    yield make_case(H, W, B, J, P, NB, v)
                    v += 1


# ---- comparing a result with the oracle ---------------------------------------------------------------------------------------
HEAT_TOL = 1e-6          # fp32 exp against float64 exp of the same fp32 argument: 1-2 ulp of a value <= 1 is <= 2.4e-7


def as_tensors(case, device="cpu"):
    import torch
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(device)
    return {k: t(case[k]) for k in ("part", "joints", "keep", "remove", "boxes")}


def compare(got, case, seg, tag):
    """got (B, C, H, W) fp32 numpy against the oracle: seg channels and heat decisions exact, heat values within HEAT_TOL.
    -> the largest heat difference."""
    want, on = proxy_inputs(case["part"], case["joints"], case["keep"], case["remove"], case["boxes"], P=case["P"], seg=seg,
                               sigma=case["sigma"])
    assert got.shape == want.shape and got.dtype == np.float32, tag
    cseg = want.shape[1] - on.shape[1]
    assert np.array_equal(got[:, :cseg].astype(np.float64), want[:, :cseg]), tag + ": seg channels"
    heat = got[:, cseg:]
    assert np.array_equal(heat != 0, on & (want[:, cseg:] >= 1e-45)), tag + ": heat decisions"
    assert not (heat[~on].view(np.uint32) != 0).any(), tag + ": a heat value outside the window is not +0"
    err = float(np.abs(heat.astype(np.float64) - want[:, cseg:]).max()) if heat.size else 0.0
    assert err <= HEAT_TOL, "%s: heat differs by %.3g" % (tag, err)
    return err
