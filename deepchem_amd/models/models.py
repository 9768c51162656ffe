"""Abstract ``Model`` (deepchem/models/models.py:22-235): it owns the model directory, and ``evaluate`` scores
predictions with metric callables."""
import os
import shutil
import tempfile
from typing import Callable, Dict, List, Optional, Sequence

import numpy as np


class Model(object):

    def __init__(self, model=None, model_dir: Optional[str] = None, **kwargs) -> None:
        if type(self).__name__ == "Model":
            raise ValueError("This constructor is for an abstract class and should never be called directly.")
        # a directory of our own making is removed again with the object; a caller's directory is kept
        self.model_dir_is_temp = model_dir is None
        if model_dir is None:
            model_dir = tempfile.mkdtemp()
        os.makedirs(model_dir, exist_ok=True)
        self.model_dir = model_dir
        self.model = model
        self.model_class = type(model)

    def __del__(self):
        if getattr(self, "model_dir_is_temp", False):
            shutil.rmtree(self.model_dir, ignore_errors=True)

    def get_task_type(self) -> str:
        raise NotImplementedError

    def get_num_tasks(self) -> int:
        raise NotImplementedError

    def evaluate(self, dataset, metrics, transformers: List = [], per_task_metrics: bool = False,
                 use_sample_weights: bool = False, n_classes: int = 2):
        """Score ``predict(dataset)`` against ``dataset.y`` (models/models.py:162-223).  Labels and predictions
        both go back through the y-transformers before scoring, as in the reference's Evaluator
        (utils/evaluate.py:197-332).

        ``dc.metrics.Metric`` objects are scored as ``Evaluator.compute_model_performance`` scores them:
        ``{metric.name: averaged score}``, and with ``per_task_metrics`` a second dictionary of the per-task
        scores.  A model on a GPU scores them where the predictions sit when it can (``_device_scores``).

        Bare callables ``f(y_true, y_pred, w) -> float or per-task array`` keep this repository's older form:
        ``{name: score}``, the mean over tasks unless ``per_task_metrics``."""
        from deepchem_amd.metrics import Metric
        from deepchem_amd.trans.transformers import undo_transforms
        if isinstance(metrics, Metric) or callable(metrics):
            metrics = [metrics]
        on_labels = [t for t in transformers if t.transform_y]
        wrapped = [m for m in metrics if isinstance(m, Metric)]
        if not wrapped:
            truth = undo_transforms(dataset.y, on_labels)
            predicted = self.predict(dataset, on_labels)
            scores = {}
            for metric in metrics:
                value = metric(truth, predicted, dataset.w)
                label = getattr(metric, "name", None) or getattr(metric, "__name__", "metric")
                scores[label] = value if per_task_metrics else float(np.nanmean(value))
            return scores
        results = None
        if len(wrapped) == len(metrics):
            results = self._device_scores(dataset, wrapped, on_labels, use_sample_weights, n_classes)
        averaged, per_task = {}, {}
        if results is not None:
            for metric, values in zip(metrics, results):
                averaged[metric.name], per_task[metric.name] = metric._combine(list(values), len(values), True)
            return (averaged, per_task) if per_task_metrics else averaged
        truth = undo_transforms(dataset.y, on_labels)
        weights = dataset.w
        predicted = self.predict(dataset, on_labels)
        n_tasks = 1 if np.ndim(truth) < 2 else np.shape(truth)[1]
        for metric in metrics:
            if not isinstance(metric, Metric):
                value = metric(truth, predicted, weights)
                label = getattr(metric, "name", None) or getattr(metric, "__name__", "metric")
                averaged[label], per_task[label] = float(np.nanmean(value)), value
                continue
            averaged[metric.name], per_task[metric.name] = metric.compute_metric(
                truth, predicted, weights, per_task_metrics=True, n_tasks=n_tasks, n_classes=n_classes,
                use_sample_weights=use_sample_weights)
        return (averaged, per_task) if per_task_metrics else averaged

    def _device_scores(self, dataset, metrics, on_labels, use_sample_weights: bool, n_classes: int):
        """Per-task scores of every metric computed without moving the predictions to the host, as a list with one
        list of per-task values per metric, or None where this model cannot do that (then the host path runs)."""
        return None
