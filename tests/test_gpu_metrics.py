"""The metric kernels (deepchem_amd/csrc/metrics.hip) against results recorded from the reference
(tests/golden/metrics_ref.npz), and ``Model.evaluate`` / ``ValidationCallback`` scoring on the device end to end.

Tolerances.  Unweighted ROC-AUC is integer-exact on the GPU up to one fp64 division, and sklearn's trapezoid sum over
n <= 4097 fp64 terms of size <= 1 is within n * 2^-52 ~ 9e-13 of it: 1e-12.  Weighted ROC-AUC and PRC-AUC: fp64 sums
taken in another order, the same bound.  Moments: centred fp64 sums, relative 64 * n * 2^-53 < 1e-10 at n = 4097;
case e (labels around -300, spread 2) fails an implementation with raw uncentred sums.  Accuracy is exact."""
import io
import os

import numpy as np
import pytest
import torch

import deepchem_amd as dc
from deepchem_amd import _lib
from deepchem_amd import metrics as M
from deepchem_amd.models import device_metrics as DM
from tests.util import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda"
CLASSIFICATION_CASES = ("a", "b", "c", "d", "g2", "g63", "g64")
TOL = 1e-12
REL_TOL = 1e-10


@pytest.fixture(scope="module")
def gold():
    return load_golden("metrics_ref.npz")


def _workspace(n, T):
    n_bytes = int(_lib.load().gcmi_metrics_workspace_bytes(n, T))
    assert n_bytes >= 16 * n * T
    return torch.empty(n_bytes, dtype=torch.uint8, device=DEV)


def _rank(which, prob, column, y, positive, w):
    """One gcmi_metric_rank call on a strided view: column `column` of the (n, T, 2) probabilities."""
    n, T = y.shape
    out, status = DM.rank_scores(which, prob, column, 2 * T, 2, y, positive, w, _workspace(n, T))
    torch.cuda.synchronize()
    return out.cpu().numpy(), status.cpu().numpy()


def _on_device(gold, case):
    y = torch.as_tensor(gold[case + "_y"], device=DEV)
    prob = torch.as_tensor(gold[case + "_prob"], device=DEV).contiguous()
    w = torch.as_tensor(gold[case + "_w"].astype(np.float32), device=DEV)
    return y, prob, w


@pytest.mark.parametrize("case", CLASSIFICATION_CASES)
@pytest.mark.parametrize("weighted", [False, True])
def test_rank_kernel_reproduces_the_reference(gold, case, weighted):
    y, prob, w = _on_device(gold, case)
    w = w if weighted else None
    # ROC-AUC as the reference's Metric gets it: one-hot labels against both probability columns, averaged
    roc1, st1 = _rank(_lib.GCMI_METRIC_ROC_AUC, prob, 1, y, 1, w)
    roc0, st0 = _rank(_lib.GCMI_METRIC_ROC_AUC, prob, 0, y, 0, w)
    assert not st1.any() and not st0.any()
    want = gold["%s_roc_auc_score%s_task" % (case, "_w" if weighted else "")]
    diff = np.abs((roc1 + roc0) / 2 - want).max()
    print(case, "weighted" if weighted else "unweighted", "ROC-AUC max |diff|", diff)
    assert diff <= TOL
    prc, st = _rank(_lib.GCMI_METRIC_PRC_AUC, prob, 1, y, 1, w)
    assert not st.any()
    want = gold[case + ("_prc_sklearn_w_task" if weighted else "_prc_auc_score_task")]
    diff = np.abs(prc - want).max()
    print(case, "weighted" if weighted else "unweighted", "PRC-AUC max |diff|", diff)
    assert diff <= TOL


@pytest.mark.parametrize("case", CLASSIFICATION_CASES)
@pytest.mark.parametrize("weighted", [False, True])
def test_accuracy_is_exact(gold, case, weighted):
    y, prob, w = _on_device(gold, case)
    T = y.shape[1]
    s = DM.moment_sums(_lib.GCMI_METRIC_ACCURACY, prob, 2 * T, 2, 2, y, w if weighted else None, None, None)
    s = s.cpu().numpy()
    got = s[:, 10] / s[:, 0]
    want = gold["%s_accuracy_score%s_task" % (case, "_w" if weighted else "")]
    if weighted:
        assert np.abs(got - want).max() <= TOL
    else:
        assert np.array_equal(got, want)


def test_accuracy_takes_the_first_maximum_of_more_classes():
    prob = torch.tensor([[[.2, .4, .4]], [[.5, .5, 0.]], [[.1, .2, .7]], [[.3, .3, .3]]], device=DEV)
    y = torch.tensor([[1.], [1.], [2.], [0.]], dtype=torch.float64, device=DEV)
    s = DM.moment_sums(_lib.GCMI_METRIC_ACCURACY, prob, 3, 3, 3, y, None, None, None).cpu().numpy()
    assert s[0, 10] == 3.0 and s[0, 0] == 4.0  # np.argmax: 1, 0, 2, 0


@pytest.mark.parametrize("case", ["e", "f"])
@pytest.mark.parametrize("weighted", [False, True])
def test_moments_kernel_reproduces_the_reference(gold, case, weighted):
    y = torch.as_tensor(gold[case + "_y"], device=DEV)
    raw = torch.as_tensor(gold[case + "_pred_raw"], device=DEV)
    w = torch.as_tensor(gold[case + "_w"].astype(np.float32), device=DEV) if weighted else None
    scale = shift = None
    if case == "f":
        scale, shift = torch.as_tensor(gold["f_scale"], device=DEV), torch.as_tensor(gold["f_shift"], device=DEV)
    n, T = y.shape
    s = DM.moment_sums(_lib.GCMI_METRIC_MOMENTS, raw, T, 1, 1, y, w, scale, shift).cpu().numpy()
    names = ("r2_score", "mean_squared_error", "mean_absolute_error") if weighted else \
        ("pearson_r2_score", "r2_score", "mean_squared_error", "mean_absolute_error", "rms_score", "mae_score")
    for fn_name in names:
        got = np.array([DM.from_moments(getattr(M, fn_name), s[t]) for t in range(T)], np.float64)
        want = gold["%s_%s%s_task" % (case, fn_name, "_w" if weighted else "")]
        rel = np.abs(got - want) / np.abs(want)
        print(case, fn_name, "weighted" if weighted else "", "max relative diff", rel.max())
        assert rel.max() <= REL_TOL
    # the sums themselves against float64 numpy
    yh, wh = gold[case + "_y"], gold[case + "_w"] if weighted else np.ones((n, T))
    ph = gold[case + "_pred_raw"].astype(np.float64)
    if case == "f":
        ph = ph * gold["f_scale"] + gold["f_shift"]
    assert np.array_equal(s[:, 8], yh[0]) and np.array_equal(s[:, 9], ph[0])
    dy, dp = yh - yh[0], ph - ph[0]
    for k, want in enumerate([wh.sum(0), (wh * dy).sum(0), (wh * dp).sum(0), (wh * dy * dy).sum(0),
                              (wh * dp * dp).sum(0), (wh * dy * dp).sum(0), (wh * np.abs(yh - ph)).sum(0),
                              (wh * (yh - ph) ** 2).sum(0)]):
        scale_k = np.abs(want) if k not in (1, 2) else (wh * np.abs(dy if k == 1 else dp)).sum(0)
        assert (np.abs(s[:, k] - want) <= REL_TOL * scale_k).all(), k


def test_status_flags_leave_the_other_tasks_right(gold):
    y, prob, _ = _on_device(gold, "a")
    y, prob = y.clone(), prob.clone()
    y[:, 1] = 1.0              # task 1: one class only
    prob[5, 2, :] = float("nan")   # task 2: a NaN score
    for which, tag in ((_lib.GCMI_METRIC_ROC_AUC, "a_roc_auc_score_task"), (_lib.GCMI_METRIC_PRC_AUC, "a_prc_auc_score_task")):
        out1, st1 = _rank(which, prob, 1, y, 1, None)
        assert list(st1) == [0, 1, 2]
        if which == _lib.GCMI_METRIC_ROC_AUC:
            out0, st0 = _rank(which, prob, 0, y, 0, None)
            assert list(st0) == [0, 1, 2]
            out1 = (out1 + out0) / 2
        assert abs(out1[0] - gold[tag][0]) <= TOL
    # infinite scores are ranked, and reported (the reference refuses them: metrics_ref.npz, d_inf_raises)
    scores = torch.tensor([[0.5], [float("inf")], [0.25], [float("-inf")], [0.5]], device=DEV)
    labels = torch.tensor([[1.], [1.], [0.], [0.], [0.]], dtype=torch.float64, device=DEV)
    out, status = DM.rank_scores(_lib.GCMI_METRIC_ROC_AUC, scores, 0, 1, 1, labels, 1, None, _workspace(5, 1))
    assert status.cpu().tolist() == [4] and out.cpu().tolist() == [(2 * 5 + 1) / 12.0]


# ------------------------------------------------------------------------------------------------ end to end
def _molecules(n=40):
    here = os.path.dirname(os.path.abspath(__file__))
    with open(os.path.join(here, "golden", "smiles_sample.txt")) as f:
        smiles = [ln.strip() for ln in f if ln.strip() and not ln.startswith("#")]
    packed, _ = dc.feat.ConvMolFeaturizer().featurize_packed(smiles[:n])
    assert packed.n_mols == n
    return packed


def _model(mode, engine):
    model = dc.models.GraphConvModel(2, number_input_features=[75, 64], batch_size=16, mode=mode,
                                     device=torch.device(DEV))
    model.small_batch_engine = engine
    return model


def _classification_set():
    packed = _molecules()
    rng = np.random.RandomState(5)
    y = (rng.rand(40, 2) < 0.4).astype(np.float64)
    y[0], y[1] = 1.0, 0.0
    w = np.where(rng.rand(40, 2) < 0.2, 0.0, 1.0)
    return dc.data.PackedDataset(packed, y, w)


@pytest.mark.parametrize("engine", [False, True])
def test_evaluate_scores_classification_on_the_device(engine):
    ds = _classification_set()
    model = _model("classification", engine)
    model.fit(ds, nb_epoch=2, checkpoint_interval=0)
    metrics = [M.Metric(M.roc_auc_score, np.mean), M.Metric(M.prc_auc_score), M.Metric(M.accuracy_score)]
    before = model.device_metric_passes
    means, tasks = model.evaluate(ds, metrics, per_task_metrics=True)
    assert model.device_metric_passes == before + 1
    pred = model.predict(ds)
    assert pred.shape == (40, 2, 2)
    for metric in metrics:
        mean, per_task = metric.compute_metric(ds.y, pred, ds.w, per_task_metrics=True, n_tasks=2)
        print(metric.name, "device", tasks[metric.name], "host", per_task)
        assert np.abs(np.array(tasks[metric.name]) - np.array(per_task)).max() <= TOL
        assert abs(means[metric.name] - mean) <= TOL
    # weighted, and a single dictionary without per_task_metrics
    weighted = model.evaluate(ds, metrics[:1], use_sample_weights=True)
    assert model.device_metric_passes == before + 2
    host = metrics[0].compute_metric(ds.y, pred, ds.w, n_tasks=2, use_sample_weights=True)
    assert abs(weighted["mean-roc_auc_score"] - host) <= TOL
    # one class in a task: the host function's error
    one_class = dc.data.PackedDataset(ds.packed, np.ones((40, 2)), ds.w)
    with pytest.raises(ValueError, match="Only one class present"):
        model.evaluate(one_class, metrics[:1])
    # a metric function of the caller's, or another number of classes: the host path
    def half(y, p):
        return 0.5
    passes = model.device_metric_passes
    assert model.evaluate(ds, [M.Metric(half, mode="classification", classification_handling_mode="direct")]) == \
        {"half": 0.5}
    assert model.device_metric_passes == passes


def test_evaluate_scores_regression_through_a_normalization_transformer():
    packed = _molecules()
    rng = np.random.RandomState(6)
    y = rng.randn(40, 2) * np.array([4.0, 0.5]) + np.array([-300.0, 7.0])
    raw = dc.data.NumpyDataset(np.zeros((40, 1)), y, np.ones((40, 2)))
    norm = dc.trans.NormalizationTransformer(transform_y=True, dataset=raw)
    ds = dc.data.PackedDataset(packed, (y - norm.y_means) / norm.y_stds, np.ones((40, 2)))
    model = _model("regression", True)
    model.fit(ds, nb_epoch=2, checkpoint_interval=0)
    metrics = [M.Metric(M.pearson_r2_score, np.mean), M.Metric(M.rms_score, np.mean), M.Metric(M.r2_score),
               M.Metric(M.mae_score)]
    before = model.device_metric_passes
    means, tasks = model.evaluate(ds, metrics, [norm], per_task_metrics=True)
    assert model.device_metric_passes == before + 1
    pred = model.predict(ds, [norm])
    truth = dc.trans.undo_transforms(ds.y, [norm])
    for metric in metrics:
        mean, per_task = metric.compute_metric(truth, pred, ds.w, per_task_metrics=True, n_tasks=2)
        rel = np.abs(np.array(tasks[metric.name]) - np.array(per_task)) / np.abs(per_task)
        print(metric.name, "device", tasks[metric.name], "host", per_task)
        assert rel.max() <= REL_TOL and abs(means[metric.name] - mean) <= REL_TOL * abs(mean)
    # any other y-transformer: the host path, same numbers as scoring predict() by hand
    log = dc.trans.LogTransformer(transform_y=True)
    log_ds = dc.data.PackedDataset(packed, np.log1p(np.abs(y)), np.ones((40, 2)))
    passes = model.device_metric_passes
    got = model.evaluate(log_ds, metrics[1:2], [log])
    assert model.device_metric_passes == passes
    want = metrics[1].compute_metric(dc.trans.undo_transforms(log_ds.y, [log]), model.predict(log_ds, [log]), n_tasks=2)
    assert got == {"mean-rms_score": want}


@pytest.mark.parametrize("engine", [False, True])
def test_validation_callback_during_fit(engine):
    ds = _classification_set()
    model = _model("classification", engine)
    metric = M.Metric(M.roc_auc_score, np.mean)
    buf = io.StringIO()
    cb = dc.models.ValidationCallback(ds, 2, [metric], output_file=buf, save_on_minimum=False)
    before = model.device_metric_passes
    model.fit(ds, nb_epoch=3, checkpoint_interval=0, callbacks=[cb])  # 3 batches an epoch: 9 steps
    lines = buf.getvalue().splitlines()
    assert [ln.split(" validation:")[0] for ln in lines] == ["Step %d" % s for s in (2, 4, 6, 8)]
    assert model.device_metric_passes == before + 4
    printed = [float(ln.split("mean-roc_auc_score=")[1]) for ln in lines]
    assert float("%g" % cb.get_best_score()) == max(printed)
    assert model.get_global_step() == 9
