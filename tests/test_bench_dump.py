"""bench.py --dump-outputs: one step of the timed path from the seeded inputs, written as DIR/<name>.npy within 64 MB;
the inputs are the same on every run with the same arguments, so are the outputs up to rounding."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _sizes(d):
    return sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d))


def test_dump_outputs_keeps_its_budget_with_a_seeded_row_sample(tmp_path):
    rng = np.random.RandomState(3)
    arrays = {"loss": np.array(0.25, np.float32), "mean_loss": np.array(0.5), "w": rng.randn(30, 8).astype(np.float32),
              "big": rng.randn(5000, 16).astype(np.float32), "bigger": rng.randn(9000, 16)}
    budget = 200_000
    for run in ("a", "b"):
        bench.dump_outputs(arrays, str(tmp_path / run), budget=budget)
        assert _sizes(tmp_path / run) <= budget
    a, b = tmp_path / "a", tmp_path / "b"
    assert sorted(os.listdir(a)) == sorted(os.listdir(b))
    for f in os.listdir(a):
        x, y = np.load(a / f), np.load(b / f)
        assert x.dtype in (np.float32, np.float64) and np.array_equal(x, y), f
    # small arrays whole, large ones cut to a sample of their rows, the indices beside them
    for name in ("loss", "mean_loss", "w"):
        assert np.array_equal(np.load(a / (name + ".npy")), arrays[name])
        assert not (a / (name + ".rows.npy")).exists()
    for name in ("big", "bigger"):
        rows = np.load(a / (name + ".rows.npy"))
        assert 0 < len(rows) < len(arrays[name]) and np.all(np.diff(rows) > 0)
        assert np.array_equal(np.load(a / (name + ".npy")), arrays[name][rows.astype(np.int64)])


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_bench_dumps_the_same_step_on_every_run(tmp_path):
    import torch
    assert torch.cuda.is_available()
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--batch",
           "2048", "--profile-only"]
    runs = []
    for run in ("a", "b"):
        out = tmp_path / run
        done = subprocess.run(cmd + ["--dump-outputs", str(out)], capture_output=True, text=True, timeout=280)
        assert done.returncode == 0, done.stdout[-2000:] + done.stderr[-4000:]
        rec = json.loads([l for l in done.stdout.splitlines() if l.startswith("{")][-1])
        assert rec["steps"] == 3 and rec["ms_per_step"] > 0
        assert _sizes(out) <= 64 * 10**6
        runs.append({f[:-4]: np.load(out / f) for f in os.listdir(out)})
    a, b = runs
    assert sorted(a) == sorted(b)
    assert a["logits"].shape == (2048, 24) and a["fingerprint"].shape == (2048, 256)
    assert any(k.startswith("grad.") for k in a) and "param.dense.weight" in a
    for k in a:
        assert a[k].dtype in (np.float32, np.float64), k
        assert np.all(np.isfinite(a[k])), k
    # one step from the same seeded data, parameters and optimizer state: the two runs differ only by the order in
    # which the kernels' atomic sums round (Adam divides a near-zero gradient by its own magnitude, which moves a few
    # entries of barely trained biases by more, relative to their tiny scale)
    for k in a:
        d, scale = np.abs(a[k].astype(np.float64) - b[k]), max(float(np.abs(b[k]).max()), 1e-30)
        tol = 1e-5 * scale if k in ("loss", "mean_loss") else 1e-3 * scale + 1e-6 if k.startswith("param.") else 1e-4 * scale
        assert float(d.max()) <= tol, (k, float(d.max()), scale)
