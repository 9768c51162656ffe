"""bench.py without --full times the headline step and nothing else; --full adds every other leg to the same line."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

# what only --full measures: top-level keys of the line, keys of its config
FULL_ONLY = ("kernel_ms_per_step", "roofline_by_kernel", "head_gemm", "bf16_storage", "bf16_storage_and_gradient_streams",
             "cpu_baseline_large_batch")
FULL_ONLY_CONFIG = ("molecules_per_s_at_batch_100", "fit_molecules_per_s_batch_100", "pcba_shape",
                    "widths_128_128_dense_256", "value_exact_gemm_mode", "tox21_real")


def _parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py"] + list(argv))
    return bench.parse()


def test_only_full_runs_the_other_legs(monkeypatch):
    plain = _parse(monkeypatch, "--steps", "3")
    assert not plain.full and not plain.other_legs
    assert plain.small_batch == 0 and plain.fit_pipeline == 0 and plain.no_cpu_baseline
    full = _parse(monkeypatch, "--steps", "3", "--full")
    assert full.other_legs and full.small_batch == 100 and full.fit_pipeline == 1 and not full.no_cpu_baseline
    # --profile-only trims --full to the breakdown pass of the large-batch step
    prof = _parse(monkeypatch, "--full", "--profile-only")
    assert prof.full and not prof.other_legs and prof.fit_pipeline == 0 and prof.no_cpu_baseline


def _run(args, timeout):
    done = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True,
                          timeout=timeout)
    assert done.returncode == 0, done.stdout[-2000:] + done.stderr[-4000:]
    return json.loads([l for l in done.stdout.splitlines() if l.startswith("{")][-1])


@pytest.mark.gpu
@pytest.mark.timeout(900)
def test_bench_plain_run_is_the_headline_and_full_adds_the_rest():
    base = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "2048"]
    plain = _run(base, 280)
    assert plain["steps"] == 3 and plain["warmup"] == 1 and plain["value"] > 0 and plain["ms_per_step"] > 0
    assert plain["metric"] == "molecules/sec fwd+bwd GraphConvModel" and plain["dtype"] == "f32"
    assert plain["roofline"]["launches_per_step"] >= 2 and plain["roofline"]["achieved"] > 0
    assert plain["cpu_baseline"] is None
    assert not [k for k in FULL_ONLY if k in plain] and not [k for k in FULL_ONLY_CONFIG if k in plain["config"]]
    full = _run(base + ["--full", "--cpu-seconds", "2"], 600)
    assert full["steps"] == 3 and full["ms_per_step"] > 0
    assert [k for k in FULL_ONLY if k not in full] == [] and [k for k in FULL_ONLY_CONFIG if k not in full["config"]] == []
    assert full["cpu_baseline"]["value"] > 0
    assert set(full["kernel_ms_per_step"]) == set(full["roofline_by_kernel"]) and full["kernel_ms_per_step"]["gather_sum"] > 0
