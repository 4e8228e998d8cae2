"""The shifted-channel inputs and the bars of tests/_encoder_inputs.py are fair: torch's own CPU fp32 BatchNorm2d
(+ PReLU, and the bottleneck tail built from it), a sound fp32 implementation, stays inside every one of them against
float64.  The GPU tests (tests/test_gpu_encoder_kernels.py) hold the HIP kernels to the same bars.  No GPU needed."""
import os
import sys

import pytest
import torch

import _encoder_inputs as ei

SEED = ei.REGIME_SEED


def test_regime_tensor_follows_its_table():
    x, regimes = ei.regime_tensor(4, 64, 65, SEED)
    assert x.shape == (4, 8, 64, 65) and x.dtype == torch.float32 and regimes == ei.REGIMES
    assert regimes[0] == (0.5, 2.0) and regimes[ei.CONSTANT_CHANNEL] == (100.0, 0.0) and regimes[7] == (3000.0, 30.0)
    x64 = x.double()
    M = x[:, 0].numel()
    for c, (m, s) in enumerate(regimes):
        got_m, got_s = float(x64[:, c].mean()), float(x64[:, c].std())
        # a sample mean is within 6 sigma / sqrt(M), a sample std within 6 sigma / sqrt(2 M); fp32 storage adds an ulp of |m|
        assert abs(got_m - m) <= 6 * s / M ** 0.5 + abs(m) * ei.ULP, (c, got_m)
        assert abs(got_s - s) <= 6 * s / (2 * M) ** 0.5 + abs(m) * ei.ULP, (c, got_s)
    assert torch.equal(x[:, ei.CONSTANT_CHANNEL], torch.full_like(x[:, ei.CONSTANT_CHANNEL], 100.0))
    assert torch.equal(x, ei.regime_tensor(4, 64, 65, SEED)[0])
    assert not torch.equal(x, ei.regime_tensor(4, 64, 65, SEED + 1)[0])


@pytest.mark.parametrize("eps", [1e-3, 1e-5])
@pytest.mark.parametrize("form", ["bn", "bn_act", "bn_res"])
def test_torch_fp32_is_inside_every_bar(form, eps):
    x, p, gy, other, scale = ei.regime_case(form, SEED)
    kw = dict(with_act=form != "bn", other=other, plane_scale=scale)
    ref = ei.reference(x, p, gy, eps, 0.1, dtype=torch.float64, **kw)
    got = ei.reference(x, p, gy, eps, 0.1, dtype=torch.float32, **kw)
    ei.assert_finite(got)
    rep, left_out, total = ei.compare(got, ref, x, p, eps, plane_scale=scale)
    ei.assert_report(rep, left_out, total, exempt=(ei.CONSTANT_CHANNEL,), tag="torch fp32 %s eps=%g" % (form, eps))
    assert got["num_batches_tracked"] == ref["num_batches_tracked"] == 1


def test_encoder_kernels_use_no_scratch_and_keep_full_occupancy():
    """Every bn_* and prelu_* kernel of the built library (csrc/norm.hip, csrc/act.hip): no scratch, no spills (AGPRs),
    at most the 64 VGPRs that 8 waves per SIMD allow on gfx950, and 8 waves per SIMD by the SGPR count as well."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import kernel_resources as kr
    ks = {n: k for n, k in kr.kernels().items() if "smplr" in n and ("bn_" in n or "prelu_" in n)}
    for stem, count in (("bn_stats_kernel", 1), ("bn_finalize_kernel", 1), ("bn_apply_kernel", 3), ("bn_bwd_stats_kernel", 3),
                        ("bn_bwd_finalize_kernel", 1), ("bn_bwd_apply_kernel", 3), ("prelu_fwd_kernel", 1),
                        ("prelu_bwd_kernel", 1), ("prelu_bwd_reduce_kernel", 1)):
        assert sum(("%d%s" % (len(stem), stem)) in n for n in ks) == count, (stem, sorted(ks))
    assert len(ks) == 15, sorted(ks)
    for n, k in ks.items():
        assert k["scratch"] == 0 and k["agpr"] == 0, (n, k)
        assert k["vgpr"] <= 64, (n, k["vgpr"])
        assert kr.waves_per_simd(k) == 8, (n, k)
