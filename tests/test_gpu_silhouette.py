"""The silhouette rasteriser, kernel form by kernel form, against the float64 oracle.

smplr_silh_fwd runs one of four kernels, chosen by smplr_silh_fwd_form(VP, W): 0 silh_px_kernel (W <= 48 while its LDS
layout holds the mesh), 1 silh_fused_kernel<true> (W <= 48, larger meshes up to 8 192 vertices), 2
silh_fused_kernel<false> (48 < W <= 96), 3 silh_prep + silh_fwd_kernel (brute force: W > 96 or VP > 8 192).  Each form
runs at and next to its edges against np_oracle.projects_to_silhouette (scores; arg-min vertex up to float64 near-ties)
and smplr_silh_bwd against np_oracle.silhouette_vjp evaluated at the HIP's own arg (both accumulation modes, 4 / 2 / 1
workgroups per mesh); the forms give the same bits on the same body; known answers on a few vertices; NaN positions; the
decoder with the silhouette at a resolution of its own.  Every comparison prints its worst error / bar."""
import numpy as np
import pytest
import torch

from _inputs import make_x, silh_argmin_disagreements
from test_gpu_parity import dev, grad_close, t

pytestmark = pytest.mark.gpu

V = 6890
# Bars about 3x the worst error measured on an MI355X (scores: 0.123 of 2e-5 |want| + 2e-7; gradients: 0.082 of
# 2^-16 sum|term|), so that a kernel that drifts by a few ulp more than today fails.
SCORE_RTOL, SCORE_ATOL = 8e-6, 8e-8   # |got - want| <= SCORE_RTOL |want| + SCORE_ATOL, both channels
VJP_C = 2.0 ** -18                    # |got - want| <= VJP_C * sum|term| per vertex and component ...
VJP_FLOOR = 1e-28                     # ... + this: pixels whose score is below ~1e-28 keep no relative precision in fp32
PARK = 1e6                            # padding vertices parked far outside every window: they never win a pixel
WIDTHS = (1, 7, 17, 33, 47, 48, 49, 64, 80, 96, 97, 128)
CASES = [(W, V) for W in WIDTHS] + [(48, "px_last"), (48, "px_last+1"), (48, 8192), (48, 8193)]


def form(VP, W):
    from ilps_amd import _lib
    return int(_lib.load().smplr_silh_fwd_form(VP, W))


def px_last(W=48):
    """The largest VP silh_px_kernel takes at W, from the query (bisection: its layout grows with VP)."""
    lo, hi = 1, 8193
    assert form(lo, W) == 0 and form(hi, W) != 0
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if form(mid, W) == 0 else (lo, mid)
    return lo


def resolve(VP):
    return {"px_last": px_last(), "px_last+1": px_last() + 1}.get(VP, VP)


@pytest.fixture(scope="module")
def layer(smpl_model):
    from ilps_amd.keras_smpl.batch_smpl import SMPLLayer
    return SMPLLayer(smpl_model)


def bodies(layer, B, W, seed):
    """(B, 6890, 3) fp32 projections of make_x's synthetic bodies at W, on the device."""
    from ilps_amd.keras_smpl.projection import orthographic_project
    x = t(make_x(B, W, seed=seed))
    with torch.no_grad():
        return orthographic_project([layer(x), x], None).detach().contiguous()


def pad(p, VP, value=PARK):
    out = torch.full((p.shape[0], VP, 3), value, device=p.device, dtype=torch.float32)
    out[:, :p.shape[1]] = p
    return out.contiguous()


def edge_points(W):
    """Vertices on the edges of the cell window (SM = 8 px of margin; -8.5 and W + 7.5 round half to even into it or out
    of it depending on parity) and outliers just outside it (9 .. 14.5 px beyond the image), whose exp(-d / 1.2) on the
    border pixels is still far above zero."""
    mid = (W - 1) / 2.0
    e = (-8.5, -7.5, W + 7.5, W + 8.5)
    pts = [(u, mid + k) for k, u in enumerate(e)] + [(mid - k, v) for k, v in enumerate(e)]
    for k in range(12):
        off = 9.0 + 0.5 * k
        pts += [(-off, (k * 7.3) % W), ((k * 5.1) % W, -off), (W - 1 + off, (k * 3.7) % W), ((k * 2.9) % W, W - 1 + off)]
    return np.array(pts, np.float32)


def matrix_meshes(layer, W, VP, seed):
    """(n, VP, 3) fp32 on the device.  VP = 6 890: the body as it is; the body centred on the window's lower-left corner
    and on its upper-right one, each with edge vertices and outliers (edge_points) in its first slots; for 48 < W <= 96
    a body centred on window column 64 (image column 56), where the row masks change words.  At most two meshes at
    W > 96 (the float64 reference is the cost).  Other VP: uniform random points over the window and beyond."""
    rng = np.random.default_rng(seed)
    if VP != V:
        return t(rng.uniform(-12.0, W + 12.0, (2, VP, 3)).astype(np.float32))
    b = bodies(layer, 4, W, seed).cpu().numpy()
    e = edge_points(W)
    ctr = b[:, :, :2].mean(axis=1)
    b[1, :, :2] += np.float32(-8.0) - ctr[1]
    b[2, :, :2] += np.float32(W + 8.0) - ctr[2]
    b[1, :len(e), :2] = e
    b[2, :len(e), :2] = e
    b[3, :, 0] += np.float32(56.0) - ctr[3, 0]
    keep = [1, 2] if W > 96 else ([0, 1, 2, 3] if 48 < W <= 96 else [0, 1, 2])
    return t(b[keep])


def score_check(got, want, name):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    err = np.abs(got - want)
    ratio = float((err / (SCORE_RTOL * np.abs(want) + SCORE_ATOL)).max())
    big = np.abs(want) > 1e-2
    print("%s: scores worst err/bar %.3g (max rel err %.2e where |want| > 1e-2, max abs err %.2e)"
          % (name, ratio, float((err[big] / np.abs(want[big])).max()) if big.any() else 0.0, float(err.max())))
    assert ratio <= 1.0, "%s: score error %.3g x the bar" % (name, ratio)


def arg_check(a, warg, p64, W, name):
    n, bad = silh_argmin_disagreements(a, warg, p64, W)
    print("%s: arg differs from float64 at %d pixels, %d not a float64 near-tie" % (name, n, bad))
    assert bad == 0, "%s: %d arg-min differences are not near-ties" % (name, bad)


def vjp_check(got, p64, g, W, arg, name, det):
    """got (n, VP, 3) from smplr_silh_bwd against silhouette_vjp at the HIP's own arg: |d| <= VJP_C sum|term| (+ floor)
    per vertex and component; the z column and the rows of vertices that win no pixel exactly 0.  det: the
    deterministic mode rounds every term to its fixed-point unit, 2^-(60 - e - t) with max|dsilh| < 2^e of the mesh and
    W^2 <= 2^t (silh_bwd_kernel), so a vertex's floor there also holds one unit per pixel it wins."""
    from oracle import np_oracle as o
    got = np.asarray(got, np.float64)
    g = np.asarray(g, np.float32)
    want, abs_sum = o.silhouette_vjp(p64, g, W, arg)
    assert np.all(got[..., 2] == 0), "%s: z column not 0" % name
    count = np.zeros(got.shape[:2])
    unit = np.zeros(got.shape[0])
    terms = 1
    while (1 << terms) < W * W:
        terms += 1
    for n in range(got.shape[0]):
        count[n] = np.bincount(arg[n][arg[n] >= 0], minlength=got.shape[1])
        if det:
            unit[n] = 2.0 ** -min(max(60 - int(np.frexp(np.abs(g[n]).max())[1]) - terms, -100), 100)
    assert np.all(got[count == 0] == 0), "%s: a vertex that wins no pixel has a gradient" % name
    bar = VJP_C * abs_sum + VJP_FLOOR + (count * unit[:, None])[..., None]
    ratio = float((np.abs(got[..., :2] - want[..., :2]) / bar).max())
    print("%s: dproj worst err/bar %.3g (bar 2^-18 sum|term|)" % (name, ratio))
    assert ratio <= 1.0, "%s: gradient error %.3g x the bar" % (name, ratio)


def test_the_matrix_reaches_every_form():
    assert sorted({form(resolve(VP), W) for W, VP in CASES}) == [0, 1, 2, 3]
    assert [form(V, W) for W in (48, 49, 96, 97)] == [0, 2, 2, 3]
    assert [form(resolve(VP), 48) for VP in ("px_last", "px_last+1", 8192, 8193)] == [0, 1, 1, 3]


@pytest.mark.parametrize("W,VP", CASES, ids=["W%d-VP%s" % c for c in CASES])
def test_form_against_float64(layer, W, VP):
    """(a) forward scores and arg, (c) backward in both accumulation modes, for one (W, VP) of the matrix."""
    from ilps_amd import ops
    from oracle import np_oracle as o
    VP = resolve(VP)
    name = "form %d W=%d VP=%d" % (form(VP, W), W, VP)
    proj = matrix_meshes(layer, W, VP, seed=1000 + W)
    silh, arg = ops._silh_fwd(proj, W)
    torch.cuda.synchronize()
    p64 = proj.cpu().numpy().astype(np.float64)
    want, warg = o.projects_to_silhouette(p64, W, return_argmin=True)
    a = arg.cpu().numpy()
    score_check(silh.cpu().numpy(), want, name)
    arg_check(a, warg, p64, W, name)
    g = np.random.default_rng(W + VP).normal(0.0, 1.0, want.shape).astype(np.float32)
    for det in (False, True):
        d = ops._silh_bwd(t(g), silh, arg, proj, W, det)
        vjp_check(d.cpu().numpy(), p64, g, W, a, name + (" det" if det else ""), det)


@pytest.mark.parametrize("B", [3, 128, 512])
def test_backward_workgroups_per_mesh(layer, B):
    """(c) nsplit = 4 / 2 / 1 workgroups per mesh at B = 3 / 128 / 512 (W = 48): rows {0, B/2, B-1} against the float64
    VJP, and - deterministic - the same bits as each row run alone (one mesh: 4 workgroups)."""
    from ilps_amd import ops
    from oracle import np_oracle as o
    W = 48
    proj = bodies(layer, B, W, 500 + B)
    silh, arg = ops._silh_fwd(proj, W)
    g = torch.randn(B, W, W, 2, generator=torch.Generator().manual_seed(B)).to(dev())
    rows = [0, B // 2, B - 1]
    p64 = proj[rows].cpu().numpy().astype(np.float64)
    want, warg = o.projects_to_silhouette(p64, W, return_argmin=True)
    a = arg[rows].cpu().numpy()
    score_check(silh[rows].cpu().numpy(), want, "B=%d rows %s" % (B, rows))
    arg_check(a, warg, p64, W, "B=%d" % B)
    for det in (False, True):
        d = ops._silh_bwd(g, silh, arg, proj, W, det)
        vjp_check(d[rows].cpu().numpy(), p64, g[rows].cpu().numpy(), W, a, "B=%d%s" % (B, " det" if det else ""), det)
        if det:
            for r in rows:
                p1 = proj[r:r + 1].contiguous()
                s1, a1 = ops._silh_fwd(p1, W)
                assert torch.equal(s1, silh[r:r + 1]) and torch.equal(a1, arg[r:r + 1]), "forward row %d alone" % r
                d1 = ops._silh_bwd(g[r:r + 1].contiguous(), s1, a1, p1, W, True)
                assert torch.equal(d1, d[r:r + 1]), "deterministic backward of row %d alone differs from B=%d" % (r, B)


def test_forms_are_bit_identical(layer):
    """(b) The same body as it is and padded with parked vertices into the other forms: silhouette and arg equal bit for
    bit; deterministic backward: the body's rows bit-identical, the parked rows exactly 0."""
    from ilps_amd import ops
    pl = px_last()
    for W, vps, forms in ((48, (V, pl + 1, 8193), [0, 1, 3]), (64, (V, 8193), [2, 3]), (96, (V, 8193), [2, 3])):
        assert [form(vp, W) for vp in vps] == forms
        body = bodies(layer, 2, W, 77 + W)
        g = t(np.random.default_rng(W).normal(0.0, 1.0, (2, W, W, 2)))
        ref = None
        for vp in vps:
            p = pad(body, vp)
            s, a = ops._silh_fwd(p, W)
            d = ops._silh_bwd(g, s, a, p, W, True)
            if ref is None:
                ref = (s, a, d)
                continue
            assert torch.equal(s, ref[0]) and torch.equal(a, ref[1]), "W=%d: VP=%d differs from VP=%d" % (W, vp, V)
            assert torch.equal(d[:, :V], ref[2]), "W=%d: backward at VP=%d differs" % (W, vp)
            assert float(d[:, V:].abs().max()) == 0.0
        print("W=%d: forms %s bit-identical (forward, deterministic backward)" % (W, forms))


# ------------------------------------------------------------------------------------------------ known answers
def kat_points(W):
    """Twelve vertices with known answers, for a W x W image, W >= 17 (dyadic coordinates: every d^2 is exact in fp32,
    so the float64 arg is the HIP's exactly, ties included)."""
    return np.array([
        (5.0, 7.0),                 # 0: on the centre of pixel (5, 7): score 1, background 0, no gradient from it
        (10.0, 11.25),              # 1: } pixel (10, 12) is 0.75 from both, in two cells: vertex 1 wins it
        (10.75, 12.0),              # 2: }
        (13.75, 3.0),               # 3: } pixel (14, 3) is 0.25 from both, one cell: vertex 3 wins it
        (14.25, 3.0),               # 4: }
        (2.5, 14.0),                # 5: 2.5 rounds to cell 2 (half to even): pixels (2, 14) and (3, 14) at 0.5
        (3.5, 16.0),                # 6: 3.5 rounds to cell 4: pixels (3, 16) and (4, 16) at 0.5
        (12.0, 5.5), (6.5, 1.5),    # 7, 8: half rows, a half corner
        (-9.5, 8.0),                # 9: outliers just outside the window
        (W + 9.25, 2.0),            # 10
        (15.0, W + 10.5),           # 11
    ], np.float32)


def all_outliers(W):
    return np.array([(-9.25, 3.0), (-12.5, 20.0), (W + 9.5, 7.0), (W + 14.75, 30.0), (5.0, -10.25), (25.0, -15.0),
                     (11.0, W + 8.5), (40.0, W + 11.75)], np.float32)


def w1_points(W):
    return np.array([(0.25, -0.5), (-3.0, 2.0), (4.5, 4.5), (-9.5, 0.0), (0.0, 9.75), (0.5, 0.0)], np.float32)


def runs(pts_fn, widths):
    """(form, W, proj (1, VP, 3)) of the points in every form that can take them: as they are, and padded with parked
    vertices into the fused<true> and brute-force forms."""
    out = []
    for W in widths:
        p = np.zeros((1, len(pts_fn(W)), 3), np.float32)
        p[0, :, :2] = pts_fn(W)
        p = t(p)
        out.append((form(p.shape[1], W), W, p))
        if W <= 48 and form(8192, W) == 1:
            out.append((1, W, pad(p, px_last(W) + 1)))
        out.append((3, W, pad(p, 8193)))
    return out


@pytest.mark.parametrize("kind", ["kat", "outliers", "w1"])
def test_known_answers_in_every_form(kind):
    """(d) A vertex on a pixel centre, exact ties across and inside a cell, k + 0.5 positions, every vertex an outlier,
    W = 1: in every form the oracle's scores, its arg exactly, and the gradient rules."""
    from ilps_amd import ops
    from oracle import np_oracle as o
    fn, widths = {"kat": (kat_points, (48, 64)), "outliers": (all_outliers, (48, 64)), "w1": (w1_points, (1,))}[kind]
    seen = set()
    for f, W, p in runs(fn, widths):
        assert form(p.shape[1], W) == f
        seen.add(f)
        name = "%s form %d W=%d VP=%d" % (kind, f, W, p.shape[1])
        s, a = ops._silh_fwd(p, W)
        p64 = p.cpu().numpy().astype(np.float64)
        want, warg = o.projects_to_silhouette(p64, W, return_argmin=True)
        sn, an = s.cpu().numpy(), a.cpu().numpy()
        score_check(sn, want, name)
        assert np.array_equal(an, warg), "%s: arg differs from the float64 arg-min" % name
        g = np.random.default_rng(f).normal(0.0, 1.0, want.shape).astype(np.float32)
        for det in (False, True):
            vjp_check(ops._silh_bwd(t(g), s, a, p, W, det).cpu().numpy(), p64, g, W, an, name, det)
        if kind == "outliers":
            assert float(sn[..., 1].max()) > 1e-6, "%s: the outliers reach the image" % name
        if kind != "kat":
            continue
        px = lambda c, r: (0, W - 1 - r, c)                          # output index of pixel (c, r)
        assert sn[px(5, 7)][1] == 1.0 and sn[px(5, 7)][0] == 0.0 and an[px(5, 7)] == 0
        assert an[px(10, 12)] == 1 and an[px(14, 3)] == 3
        assert an[px(2, 14)] == 5 and an[px(3, 14)] == 5 and sn[px(2, 14)][1] == sn[px(3, 14)][1]
        assert an[px(3, 16)] == 6 and an[px(4, 16)] == 6 and sn[px(3, 16)][1] == sn[px(4, 16)][1]
        for det in (False, True):
            # a cotangent at the pixel under vertex 0 only: d = 0 there, no gradient anywhere
            g1 = np.zeros(want.shape, np.float32)
            g1[px(5, 7)] = [0.5, -1.5]
            assert float(ops._silh_bwd(t(g1), s, a, p, W, det).abs().max()) == 0.0, name
            # at the tie pixel (10, 12) only: all of it to vertex 1, none to vertex 2
            g1[px(5, 7)] = 0.0
            g1[px(10, 12)] = [0.5, -1.5]
            d = ops._silh_bwd(t(g1), s, a, p, W, det).cpu().numpy()
            assert float(np.abs(d[0, 1]).sum()) > 0 and float(np.abs(d[0, 2]).sum()) == 0.0, name
            assert float(np.abs(d[0, [0] + list(range(3, d.shape[1]))]).sum()) == 0.0, name
    assert seen == ({0, 3} if kind == "w1" else {0, 1, 2, 3})


def test_deterministic_scale_scans_every_entry_of_dsilh():
    """A known answer for silh_bwd_kernel<true>'s scale rule, the one place where it differs from silh_loss_bwd_kernel on
    purpose: the maximum is taken over all 2 W^2 entries of |dsilh|, not over the pixels' g = dsilh[1] - dsilh[0].  One
    pixel holds (2^40, 2^40): its g is exactly 0 and it contributes nothing, but frexp(2^40) gives eg = 41, W^2 = 256
    gives terms = 8, so every term is rounded to 2^-(60 - 41 - 8) = 2^-11 (a scan of |g| would round to about 2^-49)."""
    from ilps_amd import ops
    from oracle import np_oracle as o
    W, VP = 16, 64
    rng = np.random.default_rng(41)
    p = np.zeros((1, VP, 3), np.float32)
    p[0, :, :2] = rng.uniform(0.0, W - 1.0, (VP, 2))
    g = rng.normal(0.0, 1.0, (1, W, W, 2)).astype(np.float32)
    g[0, 5, 9] = 2.0 ** 40
    proj = t(p)
    silh, arg = ops._silh_fwd(proj, W)
    got = ops._silh_bwd(t(g), silh, arg, proj, W, True).cpu().numpy().astype(np.float64)
    a = arg.cpu().numpy()
    assert np.all(got * 2.0 ** 11 == np.rint(got * 2.0 ** 11)), "an element is no multiple of 2^-11"
    assert np.any(got != 0)
    want, abs_sum = o.silhouette_vjp(p.astype(np.float64), g, W, a)
    count = np.bincount(a[0][a[0] >= 0], minlength=VP)
    bar = count[None, :, None] * 2.0 ** -12 + VJP_C * abs_sum + VJP_FLOOR
    ratio = float((np.abs(got[..., :2] - want[..., :2]) / bar).max())
    print("deterministic scale: %d vertices win pixels, dproj worst err/bar %.3g (bar: 2^-12 per pixel won + 2^-18 sum|term|)"
          % (int((count > 0).sum()), ratio))
    assert np.all(got[..., 2] == 0) and ratio <= 1.0, "gradient error %.3g x the bar" % ratio


# ------------------------------------------------------------------------------------------------ NaN positions
def nan_runs(p48, p64, fill):
    """The forms for a mesh given at W = 48 and at W = 64: px, fused<true> (padded), brute (padded), fused<false>,
    brute at W = 97 (the W = 64 mesh)."""
    pl = px_last()
    return [(0, 48, p48), (1, 48, pad(p48, pl + 1, fill)), (3, 48, pad(p48, 8193, fill)), (2, 64, p64), (3, 97, p64)]


def test_one_nan_vertex_is_ignored_by_every_form(layer):
    """(e) One NaN vertex among finite ones wins no pixel in any form: every form gives the silhouette of the mesh
    without it (the reference's reduce_max over exp(NaN) would be NaN everywhere - DESIGN.md's deviations), and the
    W = 48 forms give the same bits."""
    from ilps_amd import ops
    from oracle import np_oracle as o
    p48, p64 = bodies(layer, 1, 48, 31), bodies(layer, 1, 64, 32)
    for p in (p48, p64):
        p[0, 100, :2] = float("nan")
    first = None
    for f, W, p in nan_runs(p48, p64, PARK):
        assert form(p.shape[1], W) == f
        name = "one NaN vertex, form %d W=%d" % (f, W)
        s, a = ops._silh_fwd(p, W)
        assert torch.isfinite(s).all() and not bool((a == 100).any()), name
        ref = p.cpu().numpy().astype(np.float64)
        ref[0, 100, :2] = PARK                                          # the mesh without the NaN vertex
        want, warg = o.projects_to_silhouette(ref, W, return_argmin=True)
        score_check(s.cpu().numpy(), want, name)
        arg_check(a.cpu().numpy(), warg, ref, W, name)
        if W == 48:
            if first is None:
                first = (s, a)
            assert torch.equal(s, first[0]) and torch.equal(a, first[1]), name


def test_all_nan_mesh_gives_a_nan_silhouette_in_every_form():
    """(e) A mesh whose vertices are all NaN: the NaN silhouette DESIGN.md states, in every form (the brute-force kernel
    used to skip NaN keys and return an empty image there); the arg is a vertex of the mesh, the same in the W = 48
    forms, and the backward writes zeros (no finite distance)."""
    from ilps_amd import ops
    nan = float("nan")
    p48 = torch.full((1, V, 3), nan, device=dev())
    first = None
    for f, W, p in nan_runs(p48, p48, nan):
        assert form(p.shape[1], W) == f
        s, a = ops._silh_fwd(p, W)
        n_nan = int(torch.isnan(s).sum())
        print("all-NaN mesh, form %d W=%d: %d of %d silhouette values NaN, arg in [%d, %d]"
              % (f, W, n_nan, s.numel(), int(a.min()), int(a.max())))
        assert n_nan == s.numel(), "form %d W=%d: the silhouette of an all-NaN mesh is not NaN" % (f, W)
        assert int(a.min()) >= 0 and int(a.max()) < p.shape[1]
        if W == 48:
            if first is None:
                first = a
            assert torch.equal(a, first), "form %d: arg of the all-NaN mesh differs from the px form's" % f
        g = torch.randn(1, W, W, 2, device=dev())
        for det in (False, True):
            assert float(ops._silh_bwd(g, s, a, p, W, det).abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ the decoder
@pytest.mark.parametrize("heads,WS", [(("seg", "silhouette"), 64), (("seg", "silhouette"), 112), (("silhouette",), 64)],
                         ids=["both-64", "both-112", "silhouette-64"])
def test_decoder_silhouette_at_its_own_resolution(smpl_model, part_tables, heads, WS):
    """(f) SMPLDecoder(img_wh=48, silh_wh=WS) (train_stage2_silhouette.py:72-104): dx against float64 autograd of the
    SMPL layer + projection seeded with dproj = the seg part (torch_oracle.projects_to_seg autograd at 48, HIP mask) +
    the silhouette part (silhouette_vjp at the HIP's arg), at test_decoder_end_to_end's bars."""
    from ilps_amd import ops
    from ilps_amd.decoder import SMPLDecoder
    from oracle import np_oracle as o
    from oracle import torch_oracle as to
    W, B = 48, 2
    x = make_x(B, W, seed=7100 + WS)
    rng = np.random.default_rng(WS)
    gs = rng.normal(0, 1, (B, W, W, 32)).astype(np.float32)
    gl = rng.normal(0, 1, (B, WS, WS, 2)).astype(np.float32)
    dec = SMPLDecoder(smpl_model, img_wh=W, silh_wh=WS, heads=heads)
    xg = t(x).requires_grad_(True)
    out = dec(xg)
    assert out["silhouette"].shape == (B, WS, WS, 2)
    loss = (out["silhouette"] * t(gl)).sum()
    if "seg" in heads:
        loss = loss + (out["seg"] * t(gs)).sum()
    loss.backward()
    proj = out["projects"].detach()
    s2, sarg = ops._silh_fwd(proj, WS)
    assert torch.equal(s2, out["silhouette"].detach())
    xo = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    po = to.orthographic_project(to.TorchSMPL(smpl_model)(xo), xo)
    pd = po.detach()
    cot = torch.tensor(o.silhouette_vjp(pd.numpy(), gl, WS, sarg.cpu().numpy())[0])
    if "seg" in heads:
        ids, off = part_tables[1]
        mo = torch.tensor(out["mask"].cpu().numpy(), dtype=torch.float64)
        ps = pd.clone().requires_grad_(True)
        (to.projects_to_seg(ps, mo, W, ids, off) * torch.tensor(gs, dtype=torch.float64)).sum().backward()
        cot = cot + ps.grad
    po.backward(cot)
    got, want = xg.grad.cpu().numpy(), xo.grad.numpy()
    for sl, name in ((slice(0, 4), "dcam"), (slice(4, 76), "dtheta"), (slice(76, 86), "dbeta")):
        err = float(np.abs(got[:, sl] - want[:, sl]).max() / (np.abs(want[:, sl]).max() + 1e-30))
        print("decoder %s silh_wh=%d %s: max|diff|/max|ref| %.2e = %.3g x the bar 5e-3" % ("+".join(heads), WS, name, err,
                                                                                            err / 5e-3))
        grad_close(got[:, sl], want[:, sl], 5e-3, "%s (silh_wh=%d, %s)" % (name, WS, "+".join(heads)))
