"""Callbacks for ``fit()`` (deepchem/models/callbacks.py)."""
import sys


class ValidationCallback(object):
    """Every ``interval`` training steps: score ``dataset`` with ``metrics``, write one line
    ``Step N validation: name=value ...`` to ``output_file`` and remember the best score of
    ``metrics[save_metric]`` (the lowest, or with ``save_on_minimum=False`` the highest).  With ``save_dir`` the
    model's parameters are checkpointed there whenever the score improves (callbacks.py:7-113; the TensorBoard
    and W&B hooks of the reference have no counterpart in this ``TorchModel``).

    ``fit()`` reads ``interval`` to know at which steps the callback needs the model: the small-batch engine
    ends its chunk of steps there instead of calling back after every step."""

    def __init__(self, dataset, interval, metrics, output_file=sys.stdout, save_dir=None, save_metric=0,
                 save_on_minimum=True, transformers=[]):
        self.dataset = dataset
        self.interval = interval
        self.metrics = metrics
        self.output_file = output_file
        self.save_dir = save_dir
        self.save_metric = save_metric
        self.save_on_minimum = save_on_minimum
        self._best_score = None
        self.transformers = transformers

    def __call__(self, model, step):
        if step % self.interval != 0:
            return
        module = getattr(model, "model", None)
        was_training = bool(getattr(module, "training", False))
        scores = model.evaluate(self.dataset, self.metrics, self.transformers)
        if was_training:  # evaluate() predicts in eval mode; the fit that called us goes on in training mode
            module.train()
        message = 'Step %d validation:' % step
        for key in scores:
            message += ' %s=%g' % (key, scores[key])
        print(message, file=self.output_file)
        score = scores[self.metrics[self.save_metric].name]
        if not self.save_on_minimum:
            score = -score
        if self._best_score is None or score < self._best_score:
            self._best_score = score
            if self.save_dir is not None:
                model.save_checkpoint(model_dir=self.save_dir)

    def get_best_score(self):
        """The best score seen so far on the validation set."""
        return self._best_score if self.save_on_minimum else -self._best_score
