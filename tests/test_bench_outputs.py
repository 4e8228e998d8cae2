"""bench.py's plain run and `--dump-outputs DIR`: a run without `--full` times exactly --steps steps and prints the headline
line only; the dump holds what the last timed step returned, float32, at most 64 MB (a fixed seeded mesh sample above)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _run(args, timeout=300):
    e = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        e.pop(k, None)
    r = subprocess.run([sys.executable, BENCH] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=e,
                       timeout=timeout)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    lines = [ln for ln in r.stdout.decode().splitlines() if ln.strip()]
    assert len(lines) == 1, lines
    return json.loads(lines[0])


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d)) if f.endswith(".npy")}


def test_dump_outputs_keeps_everything_under_the_cap(tmp_path):
    import bench
    outs = {"a": torch.arange(24, dtype=torch.float32).reshape(4, 3, 2), "b": torch.ones(4, 5, dtype=torch.float64),
            "none": None, "empty": torch.empty(0)}
    info = bench.dump_outputs(str(tmp_path), outs)
    got = _load(str(tmp_path))
    assert sorted(got) == ["a", "b"] and info["meshes"] == 4 and info["mesh_sample_seed"] is None
    assert all(a.dtype == np.float32 for a in got.values())
    assert np.array_equal(got["a"], outs["a"].numpy()) and np.array_equal(got["b"], np.ones((4, 5), np.float32))


def test_dump_outputs_samples_the_same_meshes_in_every_array_above_64_MB(tmp_path):
    import bench
    B = 200                                             # 200 x (48*48*32 + 6890*3) floats = 75.5 MB
    idx = torch.arange(B, dtype=torch.float32)
    outs = {"seg": idx.reshape(B, 1, 1, 1).expand(B, 48, 48, 32).contiguous(),
            "verts": idx.reshape(B, 1, 1).expand(B, 6890, 3).contiguous()}
    info = bench.dump_outputs(str(tmp_path / "one"), outs)
    bench.dump_outputs(str(tmp_path / "two"), outs)
    one, two = _load(str(tmp_path / "one")), _load(str(tmp_path / "two"))
    n = info["meshes"]
    assert 0 < n < B and one["seg"].shape == (n, 48, 48, 32) and one["verts"].shape == (n, 6890, 3)
    files = [os.path.join(tmp_path, "one", f) for f in os.listdir(tmp_path / "one")]
    assert sum(os.path.getsize(f) for f in files) <= 64 * 10 ** 6
    rows = one["seg"][:, 0, 0, 0]
    assert np.array_equal(rows, one["verts"][:, 0, 0]) and len(np.unique(rows)) == n      # the same meshes in both
    assert all(np.array_equal(one[k], two[k]) for k in one)                                  # and the same every time


def test_plain_dry_run_line_has_no_train_leg():
    d = _run(["--steps", "3", "--warmup", "0", "--batch", "2", "--dry-run"])
    assert d["steps"] == 3 and d["train_step"] is None


@pytest.mark.gpu
def test_plain_run_times_steps_and_dumps_the_last_step(tmp_path):
    """A plain run: the headline keys, exactly --steps timed steps, none of the --full legs; the dump is the step's
    outputs and input gradient for all B meshes, and a second run with the same arguments gives the same forward."""
    B, K = 8, 7
    runs = []
    for name in ("one", "two"):
        out = str(tmp_path / name)
        d = _run(["--gpus", "1", "--steps", str(K), "--warmup", "2", "--batch", str(B), "--dump-outputs", out])
        runs.append((d, _load(out)))
    d, got = runs[0]
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in d
    assert d["steps"] == K and d["full"] is False and d["dtype"] == "f32" and d["higher_is_better"] is True
    assert abs(d["value"] - B / (d["ms_per_step"] * 1e-3)) <= 1e-3 * d["value"]
    for k in ("ms_per_step_windows", "train_step", "stages_us", "roofline", "aux", "cpu_baseline", "parity"):
        assert k not in d, k
    shapes = {"verts": (B, 6890, 3), "proj": (B, 6890, 3), "mask": (B, 6890), "seg": (B, 48, 48, 32),
              "joints": (B, 24, 3), "x_grad": (B, 86)}
    assert {k: v.shape for k, v in got.items()} == shapes
    assert all(v.dtype == np.float32 and np.isfinite(v).all() for v in got.values())
    assert float(np.abs(got["x_grad"]).sum()) > 0 and d["dump_outputs"]["meshes"] == B
    again = runs[1][1]
    for k in ("verts", "proj", "mask", "seg", "joints"):
        assert np.array_equal(got[k], again[k]), k
    np.testing.assert_allclose(again["x_grad"], got["x_grad"], rtol=1e-4, atol=1e-4 * float(np.abs(got["x_grad"]).max()))
