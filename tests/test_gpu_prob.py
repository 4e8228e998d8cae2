"""csrc/prob.hip on the device against the float64 oracle (tests/_prob_oracle.py).  Every output is an fp64 result rounded to
fp32 once, so every bar is 2^-23 (one fp32 ulp: twice the rounding) relative to the sum of the magnitudes the oracle adds up
for that output; the achieved worst case is printed beside it.  Samples and likelihood with their gradients over strided rows,
masks and weights; the fusion over log-variances of +-200; the one-pass statistics on shifted data, odd rows and offset views;
hostile rows; determinism; the torch ops; the chain regressor -> samples -> SMPLLayer -> spread; the trainer."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _prob_oracle as o  # noqa: E402
from ilps_amd import prob  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
BAR = 2.0 ** -23
VERTEX_BAR = 1e-4            # the fp32 decoder's vertices against float64 (metres)
# (B, S, D, row stride of mu and s)
SHAPES = [(1, 1, 86, 86), (3, 2, 5, 5), (2, 33, 86, 86), (5, 65, 158, 158), (130, 4, 90, 93), (2, 3, 256, 256)]


def t(a, dtype=torch.float32):
    return torch.as_tensor(np.asarray(a), dtype=dtype).to(DEV)


def bits(a):
    return a.detach().contiguous().view(torch.int32).cpu()


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def strided(a, stride):
    """(B, D) numpy -> a device view whose rows lie `stride` floats apart (the gaps hold NaN)."""
    buf = torch.full((a.shape[0], stride), float("nan"), dtype=torch.float32, device=DEV)
    buf[:, :a.shape[1]] = t(a)
    return buf[:, :a.shape[1]]


def worst(got, want, mag, what):
    """|got - want| <= 2^-23 mag, beyond fp32's own floor: below 2^-126 its numbers lie 2^-149 apart, so a result down there
    (a mean weighted by exp(-400)) is off by up to that spacing however it was computed."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape and np.isfinite(got).all() and np.isfinite(want).all(), what
    rel = np.maximum(np.abs(got - want) - 2.0 ** -149, 0.0) / np.where(mag > 0, mag, 1.0)
    rel = np.where(mag > 0, rel, np.where(got == want, 0.0, np.inf))
    print("%s: worst %.3g of %.3g" % (what, rel.max() if rel.size else 0.0, BAR))
    assert (rel <= BAR).all(), what


# ---- samples --------------------------------------------------------------------------------------------------------------

def sample_case(B, S, D, seed, lo=-60.0, hi=60.0):
    rng = np.random.default_rng(seed)
    mu = rng.normal(0, 3, (B, D)).astype(np.float32)
    mu[0, min(5, D - 1)] = -0.0
    s = rng.uniform(lo, hi, (B, D)).astype(np.float32)
    eps = rng.normal(size=(B, S, D)).astype(np.float32)
    g = rng.normal(size=(B, S, D)).astype(np.float32)
    mask = np.ones(D, np.uint8)
    mask[:min(4, D - 1)] = 0                                  # the camera columns
    return mu, s, eps, g, mask


def run_samples(mu, s, eps, g, mask, mean_first, stride=None):
    stride = mu.shape[1] if stride is None else stride
    mt, st = strided(mu, stride).requires_grad_(True), strided(s, stride).requires_grad_(True)
    x, status = prob.gaussian_samples(mt, st, t(eps), mask, mean_first, return_status=True)
    assert x.is_contiguous() and x.dtype == torch.float32 and status.dtype == torch.int32 and not status.requires_grad
    dmu, ds = torch.autograd.grad(x, (mt, st), t(g))
    torch.cuda.synchronize()
    return x.detach(), status, dmu, ds


@pytest.mark.parametrize("mean_first", [False, True])
@pytest.mark.parametrize("B,S,D,stride", SHAPES)
def test_samples_and_their_gradients_against_the_oracle(B, S, D, stride, mean_first):
    mu, s, eps, g, mask = sample_case(B, S, D, B + S + D)
    x, status, dmu, ds = run_samples(mu, s, eps, g, mask, mean_first, stride)
    want, st, mag = o.samples(mu, s, eps, mask, mean_first)
    assert status.cpu().tolist() == st.tolist() == [0] * B and x.shape == (B, S, D)
    worst(x.cpu().numpy(), want, mag, "x (%d, %d, %d)" % (B, S, D))
    drawn = o.drawn_mask(S, D, mask, mean_first)
    ref = np.broadcast_to(mu[:, None], (B, S, D))
    assert np.array_equal(x.cpu().numpy().view(np.int32)[:, ~drawn], ref.view(np.int32)[:, ~drawn])          # bit copies
    dm, dsw, mag_mu, mag_s = o.samples_backward(s, eps, g, mask, mean_first)
    worst(dmu.cpu().numpy(), dm, mag_mu, "dmu")
    worst(ds.cpu().numpy(), dsw, mag_s, "ds")
    assert (bits(ds).numpy()[:, mask == 0] == 0).all()        # exactly +0
    # eps is never read where nothing is drawn: NaN planted there changes no bit
    eps2 = eps.copy()
    eps2[:, ~drawn] = np.nan
    x2, status2, dmu2, ds2 = run_samples(mu, s, eps2, g, mask, mean_first, stride)
    assert same_bits(x, x2) and same_bits(dmu, dmu2) and same_bits(ds, ds2) and status2.cpu().tolist() == [0] * B


def test_samples_without_a_mask_draw_every_column():
    mu, s, eps, g, _ = sample_case(3, 4, 86, 7, -6, 6)
    x, status, dmu, ds = run_samples(mu, s, eps, g, None, False)
    want, _, mag = o.samples(mu, s, eps)
    worst(x.cpu().numpy(), want, mag, "x, no mask")
    worst(ds.cpu().numpy(), o.samples_backward(s, eps, g)[1], o.samples_backward(s, eps, g)[3], "ds, no mask")


# ---- likelihood -----------------------------------------------------------------------------------------------------------

def nll_case(B, D, G, seed):
    rng = np.random.default_rng(seed)
    groups = rng.integers(0, G, D)
    if G >= 3:
        groups[groups == 1] = 0                               # an empty group
    groups[rng.random(D) < 0.2] = -1
    groups[0] = -1
    row_w = rng.uniform(0.5, 2.0, (B, G)).astype(np.float32)
    row_w[rng.random((B, G)) < 0.3] = 0.0
    mu, tt = rng.normal(0, 3, (B, D)).astype(np.float32), rng.normal(0, 3, (B, D)).astype(np.float32)
    s = rng.uniform(-20, 20, (B, D)).astype(np.float32)
    return mu, s, tt, groups, row_w, rng.normal(size=(B, G)).astype(np.float32)


def run_nll(mu, s, tt, groups, row_w, g, stride=None, G=None):
    stride = mu.shape[1] if stride is None else stride
    mt, st = strided(mu, stride).requires_grad_(True), strided(s, stride).requires_grad_(True)
    w = None if row_w is None else t(row_w)
    if w is None and G is not None and G > groups.max() + 1:
        w = torch.ones((mu.shape[0], G), device=DEV)
    nll, status = prob.gaussian_nll(mt, st, strided(tt, stride), groups, w, return_status=True)
    dmu, ds = torch.autograd.grad(nll, (mt, st), t(g))
    torch.cuda.synchronize()
    return nll.detach(), status, dmu, ds


@pytest.mark.parametrize("G", [1, 3, 8])
@pytest.mark.parametrize("B,S,D,stride", SHAPES)
def test_nll_and_its_gradients_against_the_oracle(B, S, D, stride, G):
    mu, s, tt, groups, row_w, g = nll_case(B, D, G, B + D + G)
    for w in (None, row_w):
        tt2 = tt.copy()
        if w is not None:
            w = w.copy()
            w[0, 0] = 0.0
            tt2[0, groups == 0] = np.nan                      # a NaN target under a zero weight: not read
        nll, status, dmu, ds = run_nll(mu, s, tt2, groups, w, g, stride, G)
        want, st, mag = o.nll(mu, s, tt2, groups, G, w)
        assert nll.shape == (B, G) and status.cpu().tolist() == st.tolist() == [0] * B
        worst(nll.cpu().numpy(), want, mag, "nll (%d, %d) G %d" % (B, D, G))
        dm, dsw, mag_mu, mag_s = o.nll_backward(mu, s, tt2, groups, G, g, w)
        worst(dmu.cpu().numpy(), dm, mag_mu, "dmu")
        worst(ds.cpu().numpy(), dsw, mag_s, "ds")
        assert (bits(dmu).numpy()[:, groups < 0] == 0).all() and (bits(ds).numpy()[:, groups < 0] == 0).all()
        if G >= 3:
            assert (nll[:, 1] == 0).all()                     # the empty group


# ---- fusion ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("G", [1, 2, 16])
@pytest.mark.parametrize("D,stride", [(5, 5), (86, 86), (90, 93), (256, 256)])
def test_fusion_against_the_oracle(G, D, stride):
    rng = np.random.default_rng(G + D)
    B = 3 * G
    mu = rng.normal(0, 3, (B, D)).astype(np.float32)
    s = rng.uniform(-200, 200, (B, D)).astype(np.float32)
    s[:G, 0] = np.linspace(-200, 200, G) if G > 1 else 200.0  # the whole span inside one group
    mu[0, 1] = -0.0
    mu_f, s_f, status = prob.fuse_gaussians(strided(mu, stride), strided(s, stride), G, return_status=True)
    wm, ws, st, mag_mu, mag_s = o.fuse(mu, s, G)
    assert mu_f.shape == s_f.shape == (3, D) and status.cpu().tolist() == st.tolist() == [0] * 3
    assert not mu_f.requires_grad and not s_f.requires_grad
    worst(mu_f.cpu().numpy(), wm, mag_mu, "mu_f G %d D %d" % (G, D))
    worst(s_f.cpu().numpy(), ws, mag_s, "s_f")
    if G == 1:
        assert same_bits(mu_f, t(mu)) and same_bits(s_f, t(s))


def test_fuse_shape_replaces_each_groups_beta():
    rng = np.random.default_rng(5)
    x, s = rng.normal(size=(6, 86)).astype(np.float32), rng.uniform(-4, 4, (6, 158)).astype(np.float32)
    out = prob.fuse_shape(t(x), t(s), 3)
    beta = o.fuse(x[:, -10:], s[:, -10:], 3)[0]
    assert same_bits(out[:, :76], t(x)[:, :76])
    assert np.abs(out[:, 76:].cpu().numpy() - np.repeat(beta, 3, 0)).max() <= 1e-6


# ---- spread ---------------------------------------------------------------------------------------------------------------

SPREADS = [(1, 1, 1), (2, 2, 7), (3, 5, 65), (2, 33, 1025), (1, 3, 6890), (3, 1, 259)]


def run_spread(p, S, offset=False):
    if offset:                                                # a view one float into its storage
        buf = torch.empty(p.size + 1, dtype=torch.float32, device=DEV)
        pt = buf[1:].view(p.shape)
        pt.copy_(t(p))
        assert pt.storage_offset() == 1 and pt.is_contiguous()
    else:
        pt = t(p)
    mean, rms, status = prob.sample_spread(pt, S, return_status=True)
    torch.cuda.synchronize()
    return mean, rms, status


@pytest.mark.parametrize("shifted", [False, True])
@pytest.mark.parametrize("B,S,N", SPREADS)
def test_spread_against_the_oracle(B, S, N, shifted):
    rng = np.random.default_rng(B + S + N)
    p = rng.normal(size=(B * S, N, 3))
    p = (1e3 + 1e-3 * p if shifted else p).astype(np.float32)       # (rows of N points lie 12 N bytes apart: odd rows of an
    wm, wr, st, mag = o.spread(p, S)                                # odd N are 4 or 8 bytes off the 16-byte grid)
    for offset in (False, True):
        mean, rms, status = run_spread(p, S, offset)
        assert mean.shape == (B, N, 3) and rms.shape == (B, N) and status.cpu().tolist() == st.tolist() == [0] * B
        worst(mean.cpu().numpy(), wm, mag, "mean (%d, %d, %d)%s" % (B, S, N, " shifted" if shifted else ""))
        if S == 1:
            assert (bits(rms) == 0).all() and same_bits(mean, t(p))
        else:
            worst(rms.cpu().numpy(), wr, wr, "rms, relative to rms")         # (on shifted data: 1e-3 against coordinates of 1e3)


def test_spread_keeps_negative_zero_at_one_sample():
    p = np.zeros((2, 5, 3), np.float32)
    p[0, 1] = -0.0
    mean, rms, _ = run_spread(p, 1)
    assert same_bits(mean, t(p)) and (bits(rms) == 0).all()


# ---- hostile rows ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("what", ["mu_nan", "s_inf", "eps_nan", "sigma_overflow"])
def test_a_hostile_row_of_samples_touches_nothing_else(what):
    B, S, D = 4, 5, 86
    mu, s, eps, g, mask = sample_case(B, S, D, 11, -6, 6)
    clean = run_samples(mu, s, eps, g, mask, True)
    if what == "mu_nan":
        mu[2, 1] = np.nan                                     # a column that is not stochastic counts too
    elif what == "s_inf":
        s[2, 40] = -np.inf
    elif what == "eps_nan":
        eps[2, 3, 40] = np.inf
    else:
        s[2, 40] = 200.0                                      # sigma = e^100: the sample overflows fp32
    x, status, dmu, ds = run_samples(mu, s, eps, g, mask, True)
    assert status.cpu().tolist() == [0, 0, prob.NONFINITE, 0] == o.samples(mu, s, eps, mask, True)[1].tolist()
    assert torch.isnan(x[2]).all() and torch.isnan(dmu[2]).all() and torch.isnan(ds[2]).all()
    keep = [0, 1, 3]
    for a, b in zip((x, dmu, ds), (clean[0], clean[2], clean[3])):
        assert same_bits(a[keep], b[keep])


def test_an_eps_that_is_not_drawn_may_be_anything():
    mu, s, eps, g, mask = sample_case(2, 3, 86, 12, -6, 6)
    eps[1, :, 2] = np.inf
    eps[1, 0, 50] = np.nan
    x, status, dmu, ds = run_samples(mu, s, eps, g, mask, True)
    assert status.cpu().tolist() == [0, 0] and torch.isfinite(x).all() and torch.isfinite(ds).all()


@pytest.mark.parametrize("what", ["mu_nan", "s_inf", "target_nan", "overflow"])
def test_a_hostile_row_of_the_likelihood_touches_nothing_else(what):
    B, D, G = 4, 86, 3
    mu, s, tt, groups, row_w, g = nll_case(B, D, G, 13)
    row_w[2] = 1.0
    d = int(np.flatnonzero(groups == 0)[0])
    clean = run_nll(mu, s, tt, groups, row_w, g)
    if what == "mu_nan":
        mu[2, d] = np.nan
    elif what == "s_inf":
        s[2, d] = np.inf
    elif what == "target_nan":
        tt[2, d] = np.nan
    else:
        s[2, d], tt[2, d] = -88.0, 3e5                        # r^2 exp(-s) = 1e11 e^88: finite in fp64, not in fp32
    nll, status, dmu, ds = run_nll(mu, s, tt, groups, row_w, g)
    assert status.cpu().tolist() == [0, 0, prob.NONFINITE, 0] == o.nll(mu, s, tt, groups, G, row_w)[1].tolist()
    assert torch.isnan(nll[2]).all() and torch.isnan(dmu[2]).all() and torch.isnan(ds[2]).all()
    keep = [0, 1, 3]
    for a, b in zip((nll, dmu, ds), (clean[0], clean[2], clean[3])):
        assert same_bits(a[keep], b[keep])


def test_a_hostile_column_of_the_fusion_and_point_of_the_spread():
    rng = np.random.default_rng(14)
    mu, s = rng.normal(size=(6, 86)).astype(np.float32), rng.uniform(-5, 5, (6, 86)).astype(np.float32)
    clean = prob.fuse_gaussians(t(mu), t(s), 3)
    mu[4, 7], s[5, 9] = np.nan, np.inf
    mu_f, s_f, status = prob.fuse_gaussians(t(mu), t(s), 3, return_status=True)
    assert status.cpu().tolist() == [0, prob.NONFINITE]
    hit = torch.zeros((2, 86), dtype=torch.bool)
    hit[1, 7] = hit[1, 9] = True
    for a, b in zip((mu_f, s_f), clean):
        assert torch.equal(torch.isnan(a).cpu(), hit) and torch.equal(bits(a)[~hit], bits(b)[~hit])
    p = rng.normal(size=(3 * 4, 300, 3)).astype(np.float32)
    cm, cr, _ = run_spread(p, 4)
    p[4 + 2, 17, 1], p[4 + 0, 299, 0] = np.nan, -np.inf       # row 1: a sample in the middle, sample 0 of the tail point
    mean, rms, status = run_spread(p, 4)
    assert status.cpu().tolist() == [0, prob.NONFINITE, 0] == o.spread(p, 4)[2].tolist()
    hit = torch.zeros((3, 300), dtype=torch.bool)
    hit[1, 17] = hit[1, 299] = True
    assert torch.equal(torch.isnan(rms).cpu(), hit) and torch.equal(torch.isnan(mean).all(2).cpu(), hit)
    assert torch.equal(torch.isnan(mean).any(2).cpu(), hit)
    assert torch.equal(bits(rms)[~hit], bits(cr)[~hit]) and torch.equal(bits(mean)[~hit], bits(cm)[~hit])


# ---- determinism and surfaces ---------------------------------------------------------------------------------------------

def test_two_runs_and_a_row_alone_give_the_same_bits():
    B, S, D = 130, 4, 90
    mu, s, eps, g, mask = sample_case(B, S, D, 15, -6, 6)
    a, b = run_samples(mu, s, eps, g, mask, True, 93), run_samples(mu, s, eps, g, mask, True, 93)
    r = slice(57, 58)
    one = run_samples(mu[r], s[r], eps[r], g[r], mask, True)
    for i in (0, 2, 3):
        assert same_bits(a[i], b[i]) and same_bits(a[i][r], one[i])
    mu, s, tt, groups, row_w, g = nll_case(B, D, 3, 16)
    a, b = run_nll(mu, s, tt, groups, row_w, g, 93), run_nll(mu, s, tt, groups, row_w, g, 93)
    one = run_nll(mu[r], s[r], tt[r], groups, row_w[r], g[r])
    for i in (0, 2, 3):
        assert same_bits(a[i], b[i]) and same_bits(a[i][r], one[i])
    rng = np.random.default_rng(17)
    mu, s = rng.normal(size=(B, D)).astype(np.float32), rng.uniform(-9, 9, (B, D)).astype(np.float32)
    a, b = prob.fuse_gaussians(t(mu), t(s), 2), prob.fuse_gaussians(t(mu), t(s), 2)
    one = prob.fuse_gaussians(t(mu[114:116]), t(s[114:116]), 2)
    for i in range(2):
        assert same_bits(a[i], b[i]) and same_bits(a[i][r], one[i])
    p = rng.normal(size=(B * 3, 70, 3)).astype(np.float32)
    a, b, one = run_spread(p, 3), run_spread(p, 3), run_spread(p[171:174], 3)
    for i in range(2):
        assert same_bits(a[i], b[i]) and same_bits(a[i][r], one[i])


def test_torch_ops_give_the_ctypes_bits():
    from ilps_amd import torch_ops
    ns = torch_ops.load()
    B, S, D = 5, 6, 90
    mu, s, eps, g, mask = sample_case(B, S, D, 18, -6, 6)
    x, status, dmu, ds = run_samples(mu, s, eps, g, mask, True, 93)
    mt, st = strided(mu, 93), strided(s, 93)
    x2, status2 = ns.prob_sample_fwd(mt, st, t(eps), mask.tolist(), True)
    dmu2, ds2 = ns.prob_sample_bwd(st, t(eps), mask.tolist(), True, status2, t(g))
    assert same_bits(x, x2) and torch.equal(status, status2) and same_bits(dmu, dmu2) and same_bits(ds, ds2)
    mu, s, tt, groups, row_w, g = nll_case(B, D, 3, 19)
    nll, status, dmu, ds = run_nll(mu, s, tt, groups, row_w, g, 93)
    nll2, status2 = ns.prob_nll_fwd(strided(mu, 93), strided(s, 93), strided(tt, 93), groups.tolist(), 3, t(row_w))
    dmu2, ds2 = ns.prob_nll_bwd(strided(mu, 93), strided(s, 93), strided(tt, 93), groups.tolist(), 3, t(row_w), status2, t(g))
    assert same_bits(nll, nll2) and torch.equal(status, status2) and same_bits(dmu, dmu2) and same_bits(ds, ds2)
    a, b = prob.fuse_gaussians(strided(mu[:4], 93), strided(s[:4], 93), 2), ns.prob_fuse(strided(mu[:4], 93), strided(s[:4], 93), 2)
    assert same_bits(a[0], b[0]) and same_bits(a[1], b[1]) and b[2].cpu().tolist() == [0, 0]
    p = np.random.default_rng(20).normal(size=(6, 259, 3)).astype(np.float32)
    a, b = run_spread(p, 3), ns.prob_spread(t(p), 3)
    assert same_bits(a[0], b[0]) and same_bits(a[1], b[1]) and torch.equal(a[2], b[2])


# ---- the chain and the trainer --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pose_repr", ["axis_angle", "rot6d"])
def test_chain_from_the_regressor_to_the_spread_of_sampled_meshes(smpl_model, pose_repr):
    """ENet + IEF on 256 x 256 images, B = 2, S = 5: the device chain sample -> SMPLLayer -> sample_spread against the float64
    chain from the regressor's own mean and log-variances (the oracle's samples rounded to fp32, the 6D head's oracle,
    oracle/torch_oracle.TorchSMPL in float64, the oracle's spread), to the decoder's vertex bar.  Then log-variances of -60:
    the samples collapse on the mean."""
    from oracle.torch_oracle import TorchSMPL
    from ilps_amd.decoder import SMPLDecoder
    from ilps_amd.evaluation import evaluate_uncertainty
    from ilps_amd.inference import predict_batch
    from ilps_amd.keras_smpl.batch_smpl import SMPLLayer
    from ilps_amd.model import SMPLRegressor
    torch.manual_seed(0)
    net = SMPLRegressor(48, "enet", True, pose_repr=pose_repr, probabilistic=True).to(DEV).eval()
    layer = SMPLLayer(smpl_model)
    gen = torch.Generator(device=DEV)
    gen.manual_seed(1)
    images = torch.randn((2, 3, 256, 256), generator=gen, device=DEV)
    S, D = 5, net.nout
    with torch.no_grad():
        out = net(images)
        assert out.shape == (2, 86) and net.mean.shape == net.log_var.shape == (2, D) and net.log_var.dtype == torch.float32
        assert torch.allclose(net.log_var, torch.full_like(net.log_var, 2 * np.log(0.1)), atol=1e-5)
        eps = torch.randn((2, S, D), generator=gen, device=DEV)
        xs = net.sample(eps, mean_first=True)
        assert xs.shape == (2 * S, 86) and same_bits(xs[::S], out)
        mean, rms = prob.sample_spread(layer(xs), S)
    y = o.samples(net.mean.cpu().numpy(), net.log_var.cpu().numpy(), eps.cpu().numpy(), net.stochastic, True)[0]
    y = y.astype(np.float32).astype(np.float64).reshape(2 * S, D)
    if pose_repr == "rot6d":
        import _rot6d_oracle as r6
        y = r6.forward(y)[0].astype(np.float32).astype(np.float64)
    verts = TorchSMPL(smpl_model, torch.float64)(torch.tensor(y)).detach().numpy()
    wm, wr, _, _ = o.spread(verts, S)
    print("chain %s: mean off by %.3g, rms by %.3g of %.3g; rms up to %.3g" % (
        pose_repr, np.abs(mean.cpu().numpy() - wm).max(), np.abs(rms.cpu().numpy() - wr).max(), VERTEX_BAR, wr.max()))
    assert np.abs(mean.cpu().numpy() - wm).max() <= VERTEX_BAR and np.abs(rms.cpu().numpy() - wr).max() <= VERTEX_BAR
    assert wr.max() > 1e-3                                    # (a sigma of 0.1 moves vertices by millimetres at the least)
    truth = {"x": out, "verts": layer(out)}
    res = evaluate_uncertainty(net, layer, [(images, truth)], S, gen)
    assert res["count"] == 2 and res["rms"].shape == (wr.shape[1],) and np.isfinite(res["nll"]).all() and res["error"].max() <= VERTEX_BAR
    with torch.no_grad():
        net.spread.bias.fill_(-60.0)
    pred = predict_batch(net, SMPLDecoder(smpl_model, img_wh=48), images, samples=S, generator=gen)
    assert pred["verts_mean"].shape == pred["verts"].shape and pred["verts_rms"].shape == pred["verts"].shape[:2]
    assert float(pred["verts_rms"].max()) < 1e-6 and float((pred["verts_mean"] - pred["verts"]).abs().max()) <= VERTEX_BAR
    assert "verts_rms" not in predict_batch(net, SMPLDecoder(smpl_model, img_wh=48), images)


@pytest.mark.parametrize("pose_repr", ["axis_angle", "rot6d"])
def test_three_steps_of_the_probabilistic_trainer_and_a_resume(smpl_model, pose_repr, tmp_path):
    """B = 4, S = 3, W = 48 on SyntheticBatches(truth=True)."""
    from ilps_amd import synthetic as syn
    from ilps_amd.keras_smpl.batch_smpl import SMPLLayer
    from ilps_amd.keypoints import KeypointSpec
    from ilps_amd.training import ProbabilisticTrainer
    layer = SMPLLayer(smpl_model)
    bt = syn.SyntheticBatches(layer, 4, 256, 48, topology=syn.hull_topology(smpl_model), device=DEV, truth=True, seed=3,
                              spec=KeypointSpec.from_model(layer, "cocoplus"), sampler=syn.BodySampler(layer, fill=(0.5, 0.8)))

    def trainer():
        torch.manual_seed(0)
        tr = ProbabilisticTrainer(smpl_model, output_wh=48, encoder_architecture="enet", use_IEF=True, device=DEV,
                                  in_channels=bt.in_channels, pose_repr=pose_repr, samples=3, spec=KeypointSpec.smpl_joints(), root=0)
        tr.smpl_model.train()
        return tr
    tr = trainer()
    assert tr.smpl_model.probabilistic and tr.groups.count(0) == tr.smpl_model.nout - 14 and tr.groups.count(1) == 10
    for i in range(3):
        images, _, _, truth = next(bt)
        loss = tr.step(images, truth=truth)
        assert torch.isfinite(loss), i
        assert float(tr.smpl_model.spread.bias.grad.abs().sum()) > 0
        assert torch.isfinite(tr.last_nll).all() and torch.isfinite(tr.last_sample_terms).all()
    path = str(tmp_path / "prob.pt")
    tr.save(path, trial=2)
    images, _, _, truth = next(bt)
    torch.manual_seed(5)                                      # (the encoder's dropout draws from the global generator)
    want = tr.step(images, truth=truth)
    tr2 = trainer()
    assert tr2.resume(path) == 3
    ck = torch.load(path, map_location=DEV)
    assert "spread.bias" in ck["smpl_model"] and "spread.weight" in ck["smpl_model"] and ck["generator"] is not None
    assert all(torch.equal(ck["smpl_model"][k], v) for k, v in tr2.smpl_model.state_dict().items())
    assert len(ck["optimizer"]["state"]) == len(tr2.opt.state_dict()["state"])
    torch.manual_seed(5)
    got = tr2.step(images, truth=truth)
    # the same weights, Adam state, images, dropout and sample draws: the loss is the same forward again; 1e-4 allows the
    # convolutions another solver (fp32, some forty layers deep) and nothing else
    print("%s: the step after the resume %.9g, without it %.9g" % (pose_repr, float(got), float(want)))
    assert torch.isfinite(got) and abs(float(got) - float(want)) <= 1e-4 * abs(float(want))
