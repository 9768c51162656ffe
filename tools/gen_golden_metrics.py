"""Generate tests/golden/metrics_ref.npz: inputs and THE REFERENCE's ``Metric.compute_metric`` results (mean and per
task) for the nine score functions ``deepchem_amd.metrics`` provides.

Run once where the reference tree and its dependencies (sklearn, scipy) are installed -- never on the GPU machine:

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_metrics.py

The reference is imported with the rdkit stub of ``oracle/gen_golden.py``.  Class probabilities are stored as the
(n, T, 2) float32 array [1 - s, s] that the reference's shape normalisation makes of a score s; every s is a multiple
of 2^-16 (or of 1/16) so that 1 - s is exact in float32.  Cases:

  a   n = 257, T = 3     scores quantised to 1/16 (many ties), labels Bernoulli(0.3), weights zero on ~20 % of rows,
                         otherwise in {0.5, 1, 1.5}
  b   n = 4097, T = 2    fine-grained scores with one block of 300 equal scores at sorted positions 3797..4096 (task 0:
                         across position 4096) and 1900..2199 (task 1: across position 2048)
  c   n = 65, T = 130    more tasks than a wave has lanes
  d   n = 24, T = 2      task 0: -0.0 and +0.0, a denormal, negative scores, duplicates; task 1: all scores equal
                         (infinite scores: the reference raises ValueError -- recorded as d_inf_raises)
  g2, g63, g64           n = 2, 63, 64, T = 1
  e   n = 1025, T = 3    regression, y float64 with mean -300 and standard deviation 2, predictions float32
  f   n = 513, T = 4     regression through a NormalizationTransformer-style per-task scale and shift: raw float32
                         predictions, the reference scores raw.astype(float64) * scale + shift

Classification results are recorded with ``use_sample_weights`` off and on (``_w``) where the reference's function
takes ``sample_weight`` (roc_auc_score, accuracy_score); prc_auc_score does not, so ``*_prc_sklearn_w`` holds sklearn's
``auc(precision_recall_curve(..., sample_weight=w))`` of class 1 directly.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
from gen_golden import import_reference  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "metrics_ref.npz")
CLASSIFICATION = ("roc_auc_score", "prc_auc_score", "accuracy_score")
WEIGHTED_CLASSIFICATION = ("roc_auc_score", "accuracy_score")
REGRESSION = ("pearson_r2_score", "r2_score", "mean_squared_error", "mean_absolute_error", "rms_score", "mae_score")
WEIGHTED_REGRESSION = ("r2_score", "mean_squared_error", "mean_absolute_error")


def weights_for(rng, shape):
    w = rng.choice([0.5, 1.0, 1.5], size=shape)
    w[rng.rand(*shape) < 0.2] = 0.0
    return w


def labels_for(rng, n, T, p=0.3):
    y = (rng.rand(n, T) < p).astype(np.float64)
    y[0, :], y[1, :] = 1.0, 0.0  # both classes in every task
    return y


def probs_of(scores):
    s = np.asarray(scores, np.float32)
    prob = np.stack([np.float32(1) - s, s], axis=-1)
    assert np.array_equal(prob[..., 0].astype(np.float64), 1.0 - s.astype(np.float64)), "1 - s must be exact"
    return prob


def classification_cases():
    rng = np.random.RandomState(20240607)
    cases = {}
    y = labels_for(rng, 257, 3)
    cases["a"] = (y, probs_of(rng.randint(0, 17, size=(257, 3)) / 16.0), weights_for(rng, (257, 3)))

    n = 4097
    s = np.stack([rng.permutation(60000)[:n] + 2000 for _ in range(2)], axis=1).astype(np.float64)
    for t, first in ((0, n - 300), (1, 1900)):  # positions in descending order
        order = np.argsort(-s[:, t], kind="stable")
        s[order[first:first + 300], t] = s[order[first], t]
    cases["b"] = (labels_for(rng, n, 2), probs_of(s / 65536.0), weights_for(rng, (n, 2)))

    cases["c"] = (labels_for(rng, 65, 130, 0.4), probs_of(rng.randint(0, 1 << 16, size=(65, 130)) / 65536.0),
                  weights_for(rng, (65, 130)))

    special = np.array([-0.0, 0.0, 1e-40, -1e-40, -1.5, -0.25, 2.0, 2.0, 0.5, 0.5, -0.25, 0.75] * 2, np.float32)
    d = np.stack([special, np.full(24, 0.375, np.float32)], axis=1)
    # (the class-0 column 1 - s is not exact for a denormal s: it is stored, and scored, as the reference rounds it)
    d_prob = np.stack([np.float32(1) - d, d], axis=-1).astype(np.float32)
    cases["d"] = (labels_for(rng, 24, 2, 0.5), d_prob, weights_for(rng, (24, 2)))

    for n in (2, 63, 64):
        cases["g%d" % n] = (labels_for(rng, n, 1, 0.5), probs_of(rng.randint(0, 9, size=(n, 1)) / 8.0),
                            np.where(np.arange(n)[:, None] < 2, 1.0, weights_for(rng, (n, 1))))
    return cases


def regression_cases():
    rng = np.random.RandomState(77)
    cases = {}
    y = -300.0 + 2.0 * rng.randn(1025, 3)
    cases["e"] = (y, (y + 0.7 * rng.randn(1025, 3)).astype(np.float32), None, None, weights_for(rng, (1025, 3)))
    scale = np.array([2.0, 0.37, 11.5, 1.0])
    shift = np.array([-300.0, 4.25, 1000.0, 0.0])
    z = rng.randn(513, 4)
    y = z * scale + shift
    cases["f"] = (y, (z + 0.3 * rng.randn(513, 4)).astype(np.float32), scale, shift, weights_for(rng, (513, 4)))
    return cases


def main():
    dc = import_reference()
    from sklearn.metrics import auc, precision_recall_curve
    out = {}

    def record(prefix, fn_name, y, pred, w, weighted):
        metric = dc.metrics.Metric(getattr(dc.metrics, fn_name), np.mean)
        mean, per_task = metric.compute_metric(y, pred, w, n_tasks=y.shape[1], per_task_metrics=True,
                                               use_sample_weights=weighted)
        tag = "%s_%s%s" % (prefix, fn_name, "_w" if weighted else "")
        out[tag + "_mean"] = np.float64(mean)
        out[tag + "_task"] = np.atleast_1d(np.asarray(per_task, np.float64))

    for name, (y, prob, w) in classification_cases().items():
        for t in range(y.shape[1]):
            assert 0 < y[:, t].sum() < y.shape[0], "both classes in every task"
            assert (w[y[:, t] == 1, t] > 0).any() and (w[y[:, t] == 0, t] > 0).any()
        out[name + "_y"], out[name + "_prob"], out[name + "_w"] = y, prob, w
        for fn_name in CLASSIFICATION:
            record(name, fn_name, y, prob, w, False)
        for fn_name in WEIGHTED_CLASSIFICATION:
            record(name, fn_name, y, prob, w, True)
        weighted_prc = []
        for t in range(y.shape[1]):
            precision, recall, _ = precision_recall_curve(y[:, t], prob[:, t, 1], sample_weight=w[:, t])
            weighted_prc.append(auc(recall, precision))
        out[name + "_prc_sklearn_w_task"] = np.asarray(weighted_prc, np.float64)

    # infinite scores: the reference does not score them
    y, prob, w = classification_cases()["d"]
    prob = prob.copy()
    prob[3, 0, :] = (-np.inf, np.inf)
    try:
        dc.metrics.Metric(dc.metrics.roc_auc_score, np.mean).compute_metric(y, prob, w, n_tasks=2)
        out["d_inf_raises"] = np.bool_(False)
    except ValueError:
        out["d_inf_raises"] = np.bool_(True)

    for name, (y, raw, scale, shift, w) in regression_cases().items():
        pred = raw if scale is None else raw.astype(np.float64) * scale + shift
        out[name + "_y"], out[name + "_pred_raw"], out[name + "_w"] = y, raw, w
        if scale is not None:
            out[name + "_scale"], out[name + "_shift"] = scale, shift
        for fn_name in REGRESSION:
            record(name, fn_name, y, pred, w, False)
        for fn_name in WEIGHTED_REGRESSION:
            record(name, fn_name, y, pred, w, True)

    np.savez_compressed(OUT, **out)
    print("wrote %s: %d arrays, %d bytes" % (OUT, len(out), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
