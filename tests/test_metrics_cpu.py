"""Segmentation metrics without a GPU: the CPU path of metrics.SegConfusion against a float64 NumPy restatement of
evaluate.py's per-class intersections / unions and correct pixels, the counts' gloo all-reduce, the seg_confusion op's
Meta kernel and the register / LDS / scratch budget of the metrics kernels (read from the built library)."""
import os
import sys

import numpy as np
import pytest
import torch

from ilps_amd.metrics import SegConfusion, compute_intersection_and_union, count_correct_predicts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def np_argmax(scores):
    """np.argmax over the last axis with NaN above every number (the first NaN wins), ties to the first."""
    s = np.asarray(scores, np.float64)
    out = np.empty(s.shape[:-1], np.int64)
    flat, of = s.reshape(-1, s.shape[-1]), out.reshape(-1)
    for i, row in enumerate(flat):
        nan = np.flatnonzero(np.isnan(row))
        of[i] = nan[0] if nan.size else int(np.argmax(row))
    return out


def np_eval(gt, pred, C):
    """evaluate.py:22-59 restated: I_k, U_k over classes 1..C-1, correct pixels, every pixel."""
    gt, pred = np.asarray(gt).reshape(-1), np.asarray(pred).reshape(-1)
    I = np.array([np.sum((gt == k) & (pred == k)) for k in range(1, C)], np.float64)
    U = np.array([np.sum((gt == k) | (pred == k)) for k in range(1, C)], np.float64)
    return I, U, float(np.sum(gt == pred)), gt.size


def _check(m, gt, scores, C):
    I, U, correct, total = np_eval(gt, np_argmax(scores), C)
    np.testing.assert_array_equal(m.intersections(), I)
    np.testing.assert_array_equal(m.unions(), U)
    assert m.correct() == correct and m.total() == total
    assert m.pixel_accuracy() == correct / total
    with np.errstate(invalid="ignore", divide="ignore"):
        ref = np.mean(I / U)
    np.testing.assert_equal(m.mean_iou(), ref)


def test_random_maps_match_the_restatement():
    rng = np.random.default_rng(0)
    scores = rng.random((3, 13, 13, 32)).astype(np.float32)
    gt = rng.integers(0, 32, (3, 13, 13))
    m = SegConfusion(32)
    m.update(torch.from_numpy(scores[:2]), torch.from_numpy(gt[:2]))
    m.update(torch.from_numpy(scores[2:]), torch.from_numpy(gt[2:]))
    _check(m, gt, scores, 32)
    assert m.counts.shape == (33, 32) and m.counts.dtype == torch.int64 and int(m.counts.sum()) == gt.size
    I, U = compute_intersection_and_union(gt, np_argmax(scores), 32)
    np.testing.assert_array_equal(I, m.intersections())
    np.testing.assert_array_equal(U, m.unions())
    assert count_correct_predicts(gt, np_argmax(scores)) == m.correct()


def test_absent_class_makes_the_mean_nan():
    rng = np.random.default_rng(1)
    scores = rng.random((2, 9, 9, 32)).astype(np.float32)
    scores[..., 7] = -1.0                                  # never predicted ...
    gt = rng.integers(0, 32, (2, 9, 9))
    gt[gt == 7] = 8                                        # ... and never labelled
    m = SegConfusion(32).update(torch.from_numpy(scores), torch.from_numpy(gt))
    _check(m, gt, scores, 32)
    assert np.isnan(m.iou()[6]) and np.isnan(m.mean_iou())
    assert np.isfinite(np.nanmean(m.iou()))


def test_out_of_range_labels_keep_unions_exact():
    rng = np.random.default_rng(2)
    scores = rng.random((2, 11, 11, 32)).astype(np.float32)
    gt = rng.integers(-3, 40, (2, 11, 11))
    m = SegConfusion(32).update(torch.from_numpy(scores), torch.from_numpy(gt))
    _check(m, gt, scores, 32)
    bad = int(np.sum((gt < 0) | (gt >= 32)))
    assert bad > 0 and int(m.counts[32].sum()) == bad


def test_ties_and_nan_follow_argmax():
    rng = np.random.default_rng(3)
    scores = rng.random((1, 8, 8, 32)).astype(np.float32)
    scores[0, 0, 0, :] = 0.5                               # all equal: channel 0
    scores[0, 0, 1, [3, 9, 30]] = 2.0                      # a tie at the top: channel 3
    scores[0, 0, 2, 5] = np.nan                            # NaN wins
    scores[0, 0, 3, [4, 20]] = np.nan                      # the first NaN wins
    scores[0, 0, 4, 0], scores[0, 0, 4, 1] = -0.0, 0.0     # +-0 at the top: the lower channel
    scores[0, 0, 4, 2:] = -1.0
    gt = rng.integers(0, 32, (1, 8, 8))
    m = SegConfusion(32).update(torch.from_numpy(scores), torch.from_numpy(gt))
    _check(m, gt, scores, 32)
    pred = np_argmax(scores)
    assert list(pred[0, 0, :5]) == [0, 3, 5, 4, 0]


def test_two_classes_and_maps():
    rng = np.random.default_rng(4)
    scores = rng.random((4, 7, 7, 2)).astype(np.float32)
    scores[0, 0, 0] = [0.25, 0.25]
    gt = rng.integers(0, 2, (4, 7, 7))
    m = SegConfusion(2).update(torch.from_numpy(scores), torch.from_numpy(gt))
    _check(m, gt, scores, 2)
    m2 = SegConfusion(2).update_maps(torch.from_numpy(np_argmax(scores)), torch.from_numpy(gt))
    assert torch.equal(m.counts, m2.counts)
    m.reset()
    assert int(m.counts.abs().sum()) == 0


def _rank(rank, world, path, q):
    import torch.distributed as dist
    dist.init_process_group("gloo", init_method="file://" + path, rank=rank, world_size=world)
    try:
        m = SegConfusion(32)
        g = torch.Generator().manual_seed(rank)
        m.update(torch.rand(2, 6, 6, 32, generator=g), torch.randint(0, 32, (2, 6, 6), generator=g))
        mine = m.counts.clone()
        m.all_reduce()
        q.put((rank, mine.numpy(), m.counts.numpy()))
    finally:
        dist.destroy_process_group()


def test_all_reduce_over_two_gloo_ranks(tmp_path):
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    path = str(tmp_path / "rdv")
    ps = [ctx.Process(target=_rank, args=(r, 2, path, q)) for r in range(2)]
    for p in ps:
        p.start()
    res = sorted(q.get(timeout=120) for _ in ps)
    for p in ps:
        p.join(60)
        assert p.exitcode == 0
    total = res[0][1] + res[1][1]
    for _, _, got in res:
        np.testing.assert_array_equal(got, total)
    assert total.sum() == 2 * 2 * 36


def test_seg_confusion_op_has_a_meta_kernel():
    from ilps_amd import torch_ops
    ns = torch_ops.load()
    assert str(ns.seg_confusion.default._schema) == torch_ops.SCHEMAS["seg_confusion"]
    m = lambda *s, dt=torch.float32: torch.empty(*s, dtype=dt, device="meta")
    assert ns.seg_confusion(m(2, 48, 48, 32), m(2, 48, 48, dt=torch.int32), m(33, 32, dt=torch.int64)) is None
    assert ns.seg_confusion(m(5, 2), m(5, dt=torch.int32), m(3, 2, dt=torch.int64)) is None
    with pytest.raises(RuntimeError):
        ns.seg_confusion(m(2, 48, 48, 32), m(2, 48, 47, dt=torch.int32), m(33, 32, dt=torch.int64))
    with pytest.raises(RuntimeError):
        ns.seg_confusion(m(2, 48, 48, 32), m(2, 48, 48, dt=torch.int32), m(32, 32, dt=torch.int64))
    with pytest.raises((RuntimeError, NotImplementedError)):
        ns.seg_confusion(torch.zeros(4, 32), torch.zeros(4, dtype=torch.int32), torch.zeros(33, 32, dtype=torch.int64))


def test_seg_confusion_refuses_operands_off_the_device():
    """The ctypes path checks devices before anything is launched: CPU operands are refused."""
    from ilps_amd.metrics import seg_confusion
    with pytest.raises(RuntimeError):
        seg_confusion(torch.zeros(4, 32), torch.zeros(4, dtype=torch.int32), torch.zeros(33, 32, dtype=torch.int64))


def test_ctypes_entries_refuse_bad_arguments_without_a_gpu():
    from ilps_amd import _lib
    lib = _lib.load()
    assert lib.smplr_seg_confusion(None, None, None, 10, 32, None, None, None) == -1      # neither scores nor pred
    assert lib.smplr_seg_confusion(None, None, None, 10, 33, None, None, None) == -1      # C > 32
    assert lib.smplr_seg_confusion(None, 1, None, 0, 32, None, None, None) == 0           # nothing to count
    # conf without the loss epilogue
    rc = lib.smplr_seg_raster_ex_conf(1, 48, 31, 6879, 1, 1, None, None, 0.0, 1, 1, None, None, None, 1, None)
    assert rc == -1 and b"loss" in lib.smplr_last_error()


def test_metrics_kernels_fit_the_budget():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr
    ks = kr.kernels()
    met = {n: k for n, k in ks.items() if "raster2_fwd_kernel" in n and "ELb1EEEv" in n and n.startswith("_ZN5smplr18raster2_fwd_kernelILb1E")}
    assert len(met) == 3, sorted(met)
    for name, k in met.items():
        twin = name.replace("ELb1EEEv", "ELb0EEEv", 1)
        assert twin in ks, name
        assert k["scratch"] == 0, name
        assert kr.waves_per_simd(k) == kr.waves_per_simd(ks[twin]), name
        assert k["lds"] <= 80 * 1024, "%s: %d B of LDS" % (name, k["lds"])
        if k["max_threads"] > 512:                         # the shapes that run two blocks per CU (8 waves per SIMD)
            assert k["sgpr"] <= 80, "%s: %d SGPRs - 7 waves per SIMD, one block per CU" % (name, k["sgpr"])
    conf = {n: k for n, k in ks.items() if "seg_confusion" in n}
    assert len(conf) >= 2
    for name, k in conf.items():
        assert k["scratch"] == 0, name
        assert kr.waves_per_simd(k) == 8, name
