"""Every row walk, row-block height and mode of seg_bwd_kernel (csrc/seg_bwd.hip) against the float64 restatement of the
operation in tests/_seg_bwd_oracle.py, at the smallest shapes that select them.  The reference reads the kernel's own arg:
every vertex and every component is compared, nothing is set aside.

CASES: name -> (W, B, part table, multi-window meshes, rows per block, the walk the launch takes).  Unless the table has
fewer than 31 parts each case runs plain and with the loss head, default and deterministic.  test_heights pins the
heights through smplr_seg_bwd_nsplit, so a change to seg_bwd_rows fails there instead of quietly testing another form.
(The multi-window meshes have every one of the 6 890 vertices visible: 6 890 records plus padding are two windows of
4 096 slots - one slot per vertex, so the real table cannot reach a third; their rows mix both and name the slots on
either side of the window's edge.)

The bar, per vertex component, from the documented accuracy of the kernel's arithmetic (never from its output):

    |got - want| <= 2^-23 (8 mag + 6 magx) + 2^-24 nterm mag + unit
    mag = sum |term|, magx = sum |term| x (x = m d), nterm = the number of non-zero terms

  * one term is -g score (m^2 r) (du, dv) with t = d^2 m^2, r = rsq(t), x = t r, score = exp(-x).  In units of 2^-23 =
    one float32 ulp: du, dv, d^2 and t are four roundings (half an ulp each; t carries 1), v_rsq is good to one ulp, so
    r carries 1/2 + 1 and x = t r 1 + 1.5 + 0.5 = 3; d score / score = -x dx / x, and fast_exp_neg adds 1e-7 (1 + x) =
    0.84 (1 + x) ulp (csrc/raster_common.h): the part that grows with x is 3.84 x <= 6 x -> 6 magx.
  * what does not grow with x: 0.84 (exp) + 0.5 (g, a difference of two cotangents) + 0.5 (g score) + 1.5 + 0.5 (m^2 r)
    + 0.5 (kk) + 0.5 (du or dv) + 0.5 (the fma into the run) = 5.3 <= 8 -> 8 mag.  With the loss head g = c1 - c2
    exp(score): c1, c2 and the product are three more roundings, __expf(score) another 0.84 (1 + score) ulp on a value
    <= e, and the score's own error enters exp(score) with a factor score x <= 1 / e; mag then takes |c1| + |c2|
    exp(score) for |g|, the sizes of the two parts whose difference g is.
  * the sum: a lane's run, the block's LDS accumulator, the block's partial and the merge over the blocks are float32
    additions, nterm of them at most, each half an ulp of a partial sum <= mag -> 2^-24 nterm mag.
  * unit, default form: the smallest positive float32 subnormal.  Deterministic form: the run sums are added as 64-bit
    fixed point with `scale` a power of two such that 2 max|g| max(m) rows W < 2^62 (the comment above `scale` in
    seg_bwd_kernel): one unit is at most 2^-57 gmax max(m_max, 1) rows W, rows <= 24, and each of at most nterm run
    sums rounds once -> unit = nterm 2^-57 gmax max(m_max, 1) 24 W, gmax = max|dseg| of the mesh, with the loss head
    2 max|dloss stats.z|.

The worst err / bar of every case is printed (run with -s); on the MI355X the figures are in the docstring of
test_forms_against_float64."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _seg_bwd_oracle as so
from test_gpu_blend_small import GUARD, guarded, intact
from test_gpu_parity import grad_close

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CASES = {
    "pipe48_b2": (48, 2, "p31", (), 8, "pipelined 48"),
    "pipe48_b128": (48, 128, "p31", (), 24, "pipelined 48"),
    "pipe64_b2": (64, 2, "p31", (), 8, "pipelined 64"),
    "pipe64_b64": (64, 64, "p31", (), 16, "pipelined 64"),
    "fast8_b1": (8, 1, "p31", (), 8, "FAST, one block, entry prefetch clamps at W - 1"),
    "fast16_b256": (16, 256, "p31", (), 16, "FAST"),
    "fast32_b3": (32, 3, "p31", (), 8, "FAST"),
    "fast96_b2": (96, 2, "p31", (), 8, "FAST"),
    "gen50_b3": (50, 3, "p31", (), 8, "general, last block 2 rows"),
    "gen50_b86": (50, 86, "p31", (), 24, "general, ragged last block"),
    "gen20_b300": (20, 300, "p31", (), 20, "general, one block"),
    "gen40_b128": (40, 128, "p31", (), 20, "general"),
    "gen24_p5": (24, 3, "p5", (), 8, "general, C = 6"),
    "gen24_p17": (24, 3, "p17", (), 8, "general, C = 18"),
    "mw48_b2": (48, 2, "real", (0,), 8, "multi-window (mesh 0) beside a single window"),
    "mw48_b128": (48, 128, "real", (3, 77), 24, "multi-window (meshes 3 and 77)"),
}
WAYS = [(False, False), (False, True), (True, False), (True, True)]            # (loss head, deterministic)
_small, _big = {}, {}


def case(name):
    """The case, built once: the small ones are all kept, of the tall ones only the latest (the tests run case by case)."""
    store = _small if CASES[name][1] <= 3 else _big
    if name not in store:
        _big.clear()
        W, B, table, multi, _, _ = CASES[name]
        k = so.build_case(W, B, table, multi, seed=sum(map(ord, name)))
        k.ref = {}
        store[name] = k
    return store[name]


def ref(k, loss):
    if loss not in k.ref:
        k.ref[loss] = (so.seg_loss_bwd_ref(k.dloss, k.stats, k.arg, k.rec, k.VP, k.W) if loss else
                       so.seg_bwd_ref(k.dseg, k.arg, k.rec, k.VP, k.W, k.C))
    return k.ref[loss]


def ways(name):
    return [w for w in WAYS if not w[0] or CASES[name][2] in ("p31", "real")]


def bits(t):
    return t.contiguous().view(torch.int32)


def test_heights():
    from ilps_amd import _lib
    lib = _lib.load()
    for name, (W, B, _, _, rows, _) in CASES.items():
        assert lib.smplr_seg_bwd_nsplit(B, W) == -(-W // rows), name
        assert rows == 8 or -(-W // 8) != -(-W // rows), name                 # (the count tells a tall launch from 8 rows)


FORMS = [(name, loss, det) for name in CASES for loss, det in ways(name)]


@pytest.mark.parametrize("name,loss,det", FORMS)
def test_forms_against_float64(name, loss, det):
    """Worst err / bar on the MI355X (first run of this file), plain | plain det | loss | loss det - all below one half,
    so no coefficient of the bar was touched:
        pipe48_b2 .16 .02 .13 .08    pipe48_b128 .24 .23 .23 .21    pipe64_b2 .13 .02 .13 .01    pipe64_b64 .19 .13 .20 .13
        fast8_b1 .16 .06 .17 .08     fast16_b256 .25 .22 .25 .23    fast32_b3 .18 .12 .14 .11    fast96_b2 .13 .00 .13 .00
        gen50_b3 .14 .06 .14 .05     gen50_b86 .22 .19 .20 .17      gen20_b300 .23 .20 .24 .23   gen40_b128 .24 .15 .24 .14
        gen24_p5 .21 .12             gen24_p17 .19 .13              mw48_b2 .22 .18 .22 .16      mw48_b128 .27 .40 .29 .29
    (the default form's worst vertices carry one or a few terms at x = 40 .. 80, where 6 magx is the bar; mw48_b128's
    deterministic .40 is fixed-point resolution on a vertex whose one term is 1e-13)."""
    k = case(name)
    W, B, _, multi, rows, walk = CASES[name]
    if name.startswith("mw"):
        assert all((k.nslots[n] > so.SB_SLOTS) == (n in multi) for n in range(B))
    else:
        assert k.nslots.max() <= so.SB_SLOTS
    r = ref(k, loss)
    got_t = so.run_case(k, loss, det)
    got = got_t.cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all()
    m_max = np.sqrt(np.array([k.rec[n, :k.nslots[n], 2].max() for n in range(B)], np.float64))
    if det:
        gmax = (2 * np.abs(k.dloss.astype(np.float64) * k.stats[..., 2]).max(1) if loss else
                np.abs(k.dseg).reshape(B, -1).max(1).astype(np.float64))
        unit = r.nterm * (2.0 ** -57 * gmax * np.maximum(m_max, 1.0) * 24 * W)[:, None, None]
    else:
        unit = 2.0 ** -149
    br = so.bar(r, unit)
    err = np.abs(got - r.dproj)
    ratio = np.where(err > 0, err / np.where(br > 0, br, 1e-300), 0.0)
    i = np.unravel_index(ratio.argmax(), ratio.shape)
    parts = (2.0 ** -23 * 8 * r.mag[i], 2.0 ** -23 * 6 * r.magx[i], 2.0 ** -24 * r.nterm[i] * r.mag[i],
             unit[i] if det else unit)
    print("\n[seg_bwd forms] %-12s W=%-2d B=%-3d rows=%-2d %-5s %-3s worst err/bar %.3f at %s: err %.3e want %.3e bar = "
          "%.2e (mag) + %.2e (magx) + %.2e (sum) + %.2e (unit), nterm %d  [%s]"
          % (name, W, B, rows, "loss" if loss else "plain", "det" if det else "fp32", ratio[i], tuple(int(v) for v in i),
             err[i], r.dproj[i], *parts, r.nterm[i], walk))
    assert (err <= br).all(), "%d of %d components outside the bar, worst err/bar %.3f at %s" % (
        int((err > br).sum()), err.size, ratio[i], i)
    # exactness: no third component, and a vertex without a live pixel is exactly 0.  (npair, not nterm: with the loss
    # head a pair's g = c1 - c2 exp(score) can cancel to exactly 0 in float64 - c1 = c2 where the background's score is 0
    # and the gate open, and exp(score) rounds to 1 below score = 1e-16 - where float32 keeps the rounding of c1, c2;
    # that is inside the bar, whose mag takes |c1| + |c2| exp(score), and not an exact zero.)
    assert not got[..., 2].any()
    assert not got[r.npair == 0].any()
    assert (r.npair[..., 0] > 0).any(1).all() and (r.npair[..., 0] == 0).any()
    if det:
        assert torch.equal(bits(so.run_case(k, loss, True)), bits(got_t))


NULL_CASES = ["pipe48_b2", "pipe64_b2", "fast8_b1", "fast96_b2", "gen50_b3", "mw48_b2"]


@pytest.mark.parametrize("loss", [False, True])
@pytest.mark.parametrize("name", NULL_CASES)
def test_dead_pixels_add_exactly_nothing(name, loss):
    """The pixel exactly on its record (d == 0) and the underflowed pair (m d > 104), taken out of arg: the same bits."""
    k = case(name)
    assert len(k.nulls) == 2
    a = k.arg.copy()
    for n, ro, c, ch in k.nulls:
        assert a[n, ro, c, ch] >= 0
        a[n, ro, c, ch] = -1
    assert torch.equal(bits(so.run_case(k, loss, True, arg=a)), bits(so.run_case(k, loss, True)))


@pytest.mark.parametrize("loss", [False, True])
@pytest.mark.parametrize("name", ["pipe48_b2", "pipe64_b2", "fast32_b3", "gen50_b3", "mw48_b2", "pipe48_b128", "pipe64_b64",
                                  "gen50_b86", "gen40_b128", "mw48_b128"])
def test_deterministic_mesh_does_not_depend_on_its_batch(name, loss):
    """8-row launches: each mesh alone (B = 1 takes 8 rows too).  Tall launches: the batch rotated by five meshes
    (the same B, hence the same height)."""
    k = case(name)
    W, B, _, _, rows, _ = CASES[name]
    full = bits(so.run_case(k, loss, True))
    if rows == 8:
        for n in range(B):
            assert torch.equal(bits(so.run_case(k, loss, True, sel=slice(n, n + 1))), full[n:n + 1]), n
    else:
        sel = [(n + 5) % B for n in range(B)]
        assert torch.equal(bits(so.run_case(k, loss, True, sel=sel)), full[sel])


@pytest.mark.parametrize("loss", [False, True])
@pytest.mark.parametrize("name", ["pipe64_b2", "gen50_b3"])
def test_deterministic_scales_with_the_cotangent(name, loss):
    k = case(name)
    a = so.run_case(k, loss, True).cpu().numpy()
    for c in (2.0 ** -60, 2.0 ** 40):
        b = so.run_case(k, loss, True, scale=c).cpu().numpy().astype(np.float64) / c
        grad_close(b, a, 1e-6, "%s %s cotangent x %g" % (name, "loss" if loss else "plain", c), per_column=False)


@pytest.mark.parametrize("loss", [False, True])
@pytest.mark.parametrize("name", ["gen50_b3", "mw48_b2"])
def test_memory_contract(name, loss):
    """dproj and the workspace as the front parts of NaN-filled buffers, both poisoned with NaN themselves: the guards
    stay, every dproj row was zeroed by some block, no partial is read that this launch did not write (the bits of a
    run on a zeroed workspace), and the partials of merge = False, summed over the row blocks in block order and
    scattered by the records' vertices, are the merged dproj bit for bit."""
    from ilps_amd import _lib
    from ilps_amd._lib import check, ptr, stream
    lib = _lib.load()
    k = case(name)
    W, B, VP, pt = k.W, k.B, k.VP, k.pt
    nws, nd = lib.smplr_seg_bwd_workspace(B, W) // 4, B * VP * 3
    nsplit = lib.smplr_seg_bwd_nsplit(B, W)
    assert nws == B * nsplit * so.SB_NWIN * so.SB_SLOTS * 2
    arg, rec = so.on_dev(k, "arg"), so.on_dev(k, "rec")
    cot = so.on_dev(k, "dloss" if loss else "dseg")
    stats = so.on_dev(k, "stats") if loss else None

    def call(ws, dp, det):
        if loss:
            check(lib.smplr_seg_loss_bwd(ptr(cot), ptr(stats), ptr(arg), ptr(rec), B, VP, W, pt.P, pt.K, ptr(dp), ptr(ws),
                                         det, stream()), "smplr_seg_loss_bwd")
        else:
            check(lib.smplr_seg_bwd(ptr(cot), ptr(arg), ptr(rec), B, VP, W, pt.P, pt.K, ptr(dp), ptr(ws), det, stream()),
                  "smplr_seg_bwd")
        torch.cuda.synchronize()

    results = []
    for det in (0, 1):
        ws, dp = guarded(nws), guarded(nd)
        call(ws, dp, det)
        assert intact(ws, nws) and intact(dp, nd), det
        assert bool(torch.isfinite(dp[:nd]).all()), det
        results.append(dp[:nd].clone())
    r = ref(k, loss)
    assert np.abs(results[0].cpu().numpy().reshape(B, VP, 3) - r.dproj).max() <= 1e-4 * np.abs(r.dproj).max()
    ws0, dp0 = torch.zeros(nws + GUARD, device=arg.device), guarded(nd)
    call(ws0, dp0, 1)
    assert torch.equal(bits(dp0[:nd]), bits(results[1]))
    # merge = False: no dproj, the partials alone
    wsp = guarded(nws)
    call(wsp, None, 1)
    assert intact(wsp, nws)
    part = wsp[:nws].cpu().numpy().reshape(B, nsplit, so.SB_NWIN * so.SB_SLOTS, 2)
    vert = k.rec.view(np.int32)[..., 3]
    want = np.zeros((B, VP, 3), np.float32)
    for n in range(B):
        nsl = int(k.nslots[n])
        acc = np.zeros((nsl, 2), np.float32)
        for s in range(nsplit):
            acc = acc + part[n, s, :nsl]
        assert np.isfinite(acc).all()
        ok = vert[n, :nsl] >= 0
        want[n, vert[n, :nsl][ok], :2] = acc[ok]
    assert np.array_equal(want.view(np.int32), results[1].cpu().numpy().reshape(B, VP, 3).view(np.int32))


def _hashes(env):
    e = dict(os.environ)
    e.pop("SMPLR_SEGBWD_PIPE", None)
    e.update(env)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_seg_bwd_oracle.py")], env=e, cwd=ROOT,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("W=")]
    assert len(lines) == 2 * len(so.HASH_CASES), r.stdout
    return lines


def test_pipelined_walk_equals_the_plain_walk():
    """`Same arithmetic, same order of flushes as seg_bwd_row` (csrc/seg_bwd.hip): the deterministic dproj of W = 48 and
    64, B = 2 and the tall batch, plain and loss, has the same sha256 with SMPLR_SEGBWD_PIPE=0."""
    want = _hashes({})
    assert len(set(l.split()[-1] for l in want)) == len(want)
    assert _hashes({"SMPLR_SEGBWD_PIPE": "0"}) == want
