"""Time ``Model.evaluate`` with ``[Metric(roc_auc_score, np.mean)]``: the device path against the host path of the
same commit and against what the commit before did (``predict`` + ``roc_auc_per_task``, one sklearn sort per task), on
a Tox21-validation-like (783 x 12) and a PCBA-validation-like (44 000 x 128) set of random scores, and the two metric
kernels alone.  Needs a GPU; prints one JSON line per shape ("Metrics on the device").

    python tools/eval_timing.py [--runs 20] [--out FILE]

Every figure is the median of ``--runs`` warmed-up runs, each between two device synchronisations.  The model is a
one-layer softmax head over random features, so that predict() costs little next to the scoring.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import deepchem_amd as dc  # noqa: E402
from deepchem_amd import _lib  # noqa: E402
from deepchem_amd.metrics import Metric, roc_auc_per_task, roc_auc_score  # noqa: E402
from deepchem_amd.models import device_metrics  # noqa: E402
from deepchem_amd.models.losses import SoftmaxCrossEntropy  # noqa: E402

SHAPES = {"tox21_valid": (783, 12), "pcba_valid": (44000, 128)}
FEATURES = 16


class Head(torch.nn.Module):

    def __init__(self, n_tasks):
        super().__init__()
        self.n_tasks = n_tasks
        self.linear = torch.nn.Linear(FEATURES, 2 * n_tasks)

    def forward(self, x):
        return torch.softmax(self.linear(x).reshape(-1, self.n_tasks, 2), dim=-1)


def median_ms(fn, runs):
    for _ in range(3):
        fn()
    times = []
    for _ in range(runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times)), float(np.min(times)), float(np.max(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("eval_timing.py measures on a GPU; none is visible")
    dev = torch.device("cuda")
    lines = []
    for name, (n, T) in SHAPES.items():
        rng = np.random.RandomState(0)
        X = rng.randn(n, FEATURES).astype(np.float32)
        y = (rng.rand(n, T) < 0.1).astype(np.float64)
        y[0], y[1] = 1.0, 0.0
        ds = dc.data.NumpyDataset(X, y, np.ones((n, T)))
        torch.manual_seed(0)
        model = dc.models.TorchModel(Head(T), SoftmaxCrossEntropy(), output_types=["prediction"], batch_size=4096,
                                     device=dev)
        metric = Metric(roc_auc_score, np.mean)
        res = {"shape": name, "n": n, "tasks": T, "runs": args.runs}

        device_metrics.MIN_ROWS = 0
        on_device = model.evaluate(ds, [metric])
        assert model.device_metric_passes == 1
        res["evaluate_device_ms"] = median_ms(lambda: model.evaluate(ds, [metric]), args.runs)
        device_metrics.MIN_ROWS = 1 << 62
        on_host = model.evaluate(ds, [metric])
        res["evaluate_host_ms"] = median_ms(lambda: model.evaluate(ds, [metric]), args.runs)
        device_metrics.MIN_ROWS = 0
        res["device_minus_host"] = abs(on_device[metric.name] - on_host[metric.name])
        res["predict_ms"] = median_ms(lambda: model.predict(ds), args.runs)
        w = np.ones((n, T))
        res["parent_predict_sklearn_ms"] = median_ms(lambda: roc_auc_per_task(y, model.predict(ds), w),
                                                     max(3, args.runs // 4))

        # the kernels alone, on a resident (n, T, 2) column
        prob = torch.as_tensor(model.predict(ds), device=dev).contiguous()
        y_dev = torch.as_tensor(y, device=dev)
        ws = torch.empty(int(_lib.load().gcmi_metrics_workspace_bytes(n, T)), dtype=torch.uint8, device=dev)
        res["rank_kernels_ms"] = median_ms(
            lambda: device_metrics.rank_scores(_lib.GCMI_METRIC_ROC_AUC, prob, 1, 2 * T, 2, y_dev, 1, None, ws),
            args.runs)
        res["moments_kernel_ms"] = median_ms(
            lambda: device_metrics.moment_sums(_lib.GCMI_METRIC_MOMENTS, prob, 2 * T, 2, 1, y_dev, None, None, None),
            args.runs)
        # what the sort has to move: 4 passes x (keys read for the histogram, keys + rows read and written to scatter)
        sort_bytes = 4 * (4 + 8 + 8) * n * T
        res["sort_algorithmic_bytes"] = sort_bytes
        res["rank_call_bytes_per_s_vs_sort_traffic"] = sort_bytes / (res["rank_kernels_ms"][0] * 1e-3)
        lines.append(json.dumps(res))
        print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
