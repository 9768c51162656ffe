"""Optimizer and learning-rate-schedule front-ends with the reference's interface
(deepchem/models/optimizers.py).

``_create_pytorch_optimizer`` of ``Adam``, ``AdamW``, ``AdaGrad``, ``RMSProp``, ``GradientDescent`` and ``Lamb``
returns, for CUDA parameters, a ``FlatOptimizer``: a ``torch.optim.Optimizer`` whose ``step()`` runs the HIP kernels of
csrc/optim.hip (csrc/loss.hip for plain Adam) on every parameter that has a gradient, and whose ``step_flat()`` updates
a contiguous range of a flat parameter arena with one launch (two for Lamb).  The per-parameter state has the key
names and shapes of the torch counterpart (``torch.optim.Adam`` / ``AdamW`` / ``Adagrad`` / ``RMSprop`` / ``SGD``; for
Lamb the reference's ``LambOptimizer``, utils/optimizer_utils.py), so checkpoints are interchangeable.  CPU parameters,
``AdamW(amsgrad=True)`` and a ``weight_decay`` given as a schedule get torch's own optimizer.

The schedules build the same ``torch.optim.lr_scheduler`` objects the reference builds.

Not covered natively: ``SparseAdam`` (torch's own), ``KFAC`` (not implemented), amsgrad.
"""
import math
from functools import partial
from typing import Dict, Optional, Union

import torch

from deepchem_amd import ops


class LearningRateSchedule(object):
    """A schedule for the learning rate (optimizers.py:66-112); subclasses build a torch scheduler."""

    def _create_pytorch_schedule(self, optimizer):
        raise NotImplementedError("Subclasses must implement this")


class Optimizer(object):

    def __init__(self, learning_rate: Union[float, LearningRateSchedule]):
        self.learning_rate = learning_rate

    def _create_pytorch_optimizer(self, params):
        raise NotImplementedError("Subclasses must implement this")

    def _initial_lr(self) -> float:
        lr = self.learning_rate
        return lr.initial_rate if isinstance(lr, LearningRateSchedule) else lr


def _all_cuda(params) -> bool:
    return bool(params) and all(p.is_cuda for p in params)


# ---------------------------------------------------------------------------------------------- native optimizers
class FlatOptimizer(torch.optim.Optimizer):
    """What the native optimizers share: the per-tensor ``step()``, and the flat step over a parameter arena
    (``attach_flat`` / ``step_flat``) with the state kept as views of flat buffers.

    A subclass names its per-element state tensors (``_state_names``, in the order of the kernel's state arenas), what
    they start at (``_state_fill``) and how one range is updated (``_update``)."""

    _has_step = True  # torch keeps a step count in the state (SGD does not)
    _small_engine_rule = True  # an elementwise rule: the small-batch engine (deepchem_amd/small.py) can run it

    def __init__(self, params, defaults):
        super().__init__(params, defaults)
        self._flat = None

    # ------------------------------------------------------------------ what a rule defines
    def _state_names(self, group):
        return ()

    def _state_fill(self, group):
        return tuple(0.0 for _ in self._state_names(group))

    def _desc(self, group):
        raise NotImplementedError

    def _update(self, group, p, g, states, step: int, where=None):
        """One step on the flat float32 tensors ``p``, ``g`` and the state tensors; ``where`` names the flat range
        (None: one parameter tensor)."""
        s = list(states) + [None, None]
        ops.opt_step_(self._desc(group), p, g, s[0], s[1], group["lr"], step)

    # ------------------------------------------------------------------ the flat step
    def attach_flat(self, param_flat: torch.Tensor, grad_flat: torch.Tensor, slices):
        """All parameters (in order) are views of ``param_flat`` and their gradients views of ``grad_flat``
        (``slices``: (offset, numel) per parameter): ``step_flat`` then updates any contiguous range with ONE launch
        (Lamb: two).  The state tensors become views of flat buffers, so ``state_dict()`` keeps the per-parameter
        layout of the torch counterpart."""
        params = [p for g in self.param_groups for p in g["params"]]
        if len(params) != len(slices):
            raise ValueError("attach_flat: %d parameters, %d slices" % (len(params), len(slices)))
        group = self.param_groups[0]
        names = self._state_names(group)
        bufs = [torch.full_like(param_flat, fill) for fill in self._state_fill(group)]
        # carry over any state that already exists (restore() before the first native step)
        for p, (off, n) in zip(params, slices):
            st = self.state.get(p)
            if st:
                for name, buf in zip(names, bufs):
                    if name in st:
                        buf[off:off + n].copy_(st[name].reshape(-1))
        self._flat = dict(p=param_flat, g=grad_flat, names=names, bufs=bufs, slices=list(slices), params=params)
        if len(bufs) == 2:  # (the small-batch engine and older callers read the two Adam moments by these names)
            self._flat["m"], self._flat["v"] = bufs

    def _setup_flat_range(self, lo: int, hi: int):
        """State entries (views of the flat buffers) for every parameter inside [lo, hi); all of them share ONE step
        tensor, so a step costs one increment instead of a loop."""
        f = self._flat
        step_t = None
        inside = []
        for p, (off, n) in zip(f["params"], f["slices"]):
            if lo <= off and off + n <= hi:
                st = self.state[p]
                if "step" in st:
                    s = float(st["step"])
                    if step_t is None:
                        step_t = torch.tensor(s, dtype=torch.float32)
                    elif float(step_t) != s:
                        raise RuntimeError("parameters of one flat range have different optimizer step counts")
                inside.append((p, off, n))
        if step_t is None:
            step_t = torch.tensor(0.0, dtype=torch.float32)
        for p, off, n in inside:
            st = self.state[p]
            if self._has_step:
                st["step"] = step_t
            for name, buf in zip(f["names"], f["bufs"]):
                st[name] = buf[off:off + n].view(p.shape)
        f["range"] = (lo, hi)
        f["step_t"] = step_t
        f["n_inside"] = len(inside)
        f["inside"] = inside

    @torch.no_grad()
    def step_flat(self, lo: int, hi: int):
        """The rule on the flat range [lo, hi) (floats)."""
        f = self._flat
        if f.get("range") != (lo, hi):
            self._setup_flat_range(lo, hi)
        if f["n_inside"] == 0:
            return
        f["step_t"] += 1
        self._opt_called = True  # what torch's schedulers look at before they warn about the order of the two steps
        self._update(self.param_groups[0], f["p"][lo:hi], f["g"][lo:hi], [b[lo:hi] for b in f["bufs"]],
                     int(f["step_t"].item()), where=(lo, hi))

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        if self._flat is not None:  # re-home the loaded state into the flat buffers
            f = self._flat
            for p, (off, n) in zip(f["params"], f["slices"]):
                st = self.state.get(p)
                if not st:
                    continue
                for name, buf in zip(f["names"], f["bufs"]):
                    if name in st:
                        buf[off:off + n].copy_(st[name].reshape(-1))
                        st[name] = buf[off:off + n].view(p.shape)
                if "step" in st:
                    st["step"] = torch.as_tensor(st["step"], dtype=torch.float32).cpu()
            f.pop("range", None)  # re-derive the shared step tensor on the next flat step

    # ------------------------------------------------------------------ the per-tensor step
    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        # after a flat (native) step the parameters of the trained range share ONE step tensor: it advances once
        # per call here, not once per parameter that points at it
        bumped = set()
        for group in self.param_groups:
            names = self._state_names(group)
            for p in group["params"]:
                if p.grad is None:
                    continue  # torch skips parameters without a gradient
                if not p.is_cuda:
                    raise RuntimeError("%s: parameters must be CUDA tensors" % type(self).__name__)
                state = self.state[p]
                if not all(name in state for name in names) or (self._has_step and "step" not in state):
                    if self._has_step:
                        state["step"] = torch.tensor(0.0, dtype=torch.float32)
                    for name, fill in zip(names, self._state_fill(group)):
                        state[name] = torch.full_like(p, fill, memory_format=torch.preserve_format)
                step = 1
                if self._has_step:
                    if not isinstance(state["step"], torch.Tensor):
                        state["step"] = torch.tensor(float(state["step"]), dtype=torch.float32)
                    if id(state["step"]) not in bumped:
                        bumped.add(id(state["step"]))
                        state["step"] += 1
                    step = int(state["step"].item())
                grad = p.grad.data if p.grad.is_contiguous() else p.grad.contiguous()
                self._update(group, p.data.view(-1), grad.view(-1), [state[name].view(-1) for name in names], step,
                             where=p)
        return loss


class GcmiAdam(FlatOptimizer):
    """torch.optim.Adam semantics (no amsgrad; ``weight_decay`` is its L2 term) on the HIP kernels."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0):
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False,
                        maximize=False, foreach=None, capturable=False, differentiable=False,
                        fused=None)
        super().__init__(params, defaults)

    def _state_names(self, group):
        return ("exp_avg", "exp_avg_sq")

    _rule = "adam_l2"

    def _desc(self, group):
        return ops.opt_desc(self._rule, beta1=group["betas"][0], beta2=group["betas"][1], eps=group["eps"],
                            weight_decay=group["weight_decay"])

    def _update(self, group, p, g, states, step, where=None):
        if self._rule == "adam_l2" and group["weight_decay"] == 0:
            beta1, beta2 = group["betas"]
            ops.adam_step_(p, g, states[0], states[1], group["lr"], beta1, beta2, group["eps"], step)
        else:
            super()._update(group, p, g, states, step, where)


class GcmiAdamW(GcmiAdam):
    """torch.optim.AdamW semantics (decoupled weight decay, no amsgrad)."""

    _rule = "adamw"

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2):
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)


class GcmiSGD(FlatOptimizer):
    """torch.optim.SGD(params, lr): no momentum, no state."""

    _has_step = False

    def __init__(self, params, lr=1e-3):
        defaults = dict(lr=lr, momentum=0, dampening=0, weight_decay=0, nesterov=False, maximize=False, foreach=None,
                        differentiable=False, fused=None)
        super().__init__(params, defaults)

    def _desc(self, group):
        return ops.opt_desc("sgd")


class GcmiAdagrad(FlatOptimizer):
    """torch.optim.Adagrad(params, lr, initial_accumulator_value=..., eps=...): state ``step``, ``sum``."""

    def __init__(self, params, lr=1e-2, initial_accumulator_value=0, eps=1e-10):
        defaults = dict(lr=lr, lr_decay=0, eps=eps, weight_decay=0, initial_accumulator_value=initial_accumulator_value,
                        foreach=None, maximize=False, differentiable=False, fused=None)
        super().__init__(params, defaults)

    def _state_names(self, group):
        return ("sum",)

    def _state_fill(self, group):
        return (float(group["initial_accumulator_value"]),)

    def _desc(self, group):
        return ops.opt_desc("adagrad", eps=group["eps"])


class GcmiRMSprop(FlatOptimizer):
    """torch.optim.RMSprop(params, lr, alpha=..., eps=..., momentum=...), not centered: state ``step``,
    ``square_avg`` and, with momentum, ``momentum_buffer``."""

    def __init__(self, params, lr=1e-2, alpha=0.99, eps=1e-8, momentum=0):
        defaults = dict(lr=lr, momentum=momentum, alpha=alpha, eps=eps, centered=False, weight_decay=0,
                        capturable=False, foreach=None, maximize=False, differentiable=False)
        super().__init__(params, defaults)

    def _state_names(self, group):
        return ("square_avg", "momentum_buffer") if group["momentum"] > 0 else ("square_avg",)

    def _desc(self, group):
        return ops.opt_desc("rmsprop", eps=group["eps"], alpha=group["alpha"], momentum=group["momentum"])


class GcmiLamb(FlatOptimizer):
    """The reference's ``LambOptimizer`` (utils/optimizer_utils.py:11-163) as ``Lamb`` configures it (no debiasing,
    weight norm clamped to 10) on the two Lamb kernels: state ``step``, ``exp_avg``, ``exp_avg_sq`` and this step's
    ``weight_norm``, ``adam_norm``, ``trust_ratio`` as 0-dim views of a device buffer (never read by the host)."""

    _small_engine_rule = False  # per-tensor norms: the per-batch native step

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=0):
        if lr <= 0.0 or eps < 0.0 or not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0 or weight_decay < 0:
            raise ValueError("Lamb: invalid lr / eps / betas / weight_decay")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        self.clamp_value, self.adam, self.debias = 10, False, False
        self._work = {}

    def _state_names(self, group):
        return ("exp_avg", "exp_avg_sq")

    def _desc(self, group):
        return ops.opt_desc("lamb", beta1=group["betas"][0], beta2=group["betas"][1], eps=group["eps"],
                            weight_decay=group["weight_decay"])

    def _plan(self, where, p):
        """Segment table, scratch and norms buffer of one flat range (or of one parameter tensor), made once."""
        key = where if isinstance(where, tuple) else id(where)
        w = self._work.get(key)
        if w is not None and w["n"] == p.numel() and w["segs"].device == p.device:
            return w
        if isinstance(where, tuple):
            lo = where[0]
            members = [(q, off - lo, n) for q, off, n in self._flat["inside"]]
        else:
            members = [(where, 0, p.numel())]
        segs = torch.tensor([[off, n] for _, off, n in members], dtype=torch.int64).reshape(-1, 2).to(p.device)
        scratch = torch.empty(ops.lamb_scratch_floats(p.numel(), len(members)), dtype=torch.float32, device=p.device)
        norms = torch.zeros((len(members), 3), dtype=torch.float32, device=p.device)
        for k, (q, _, _) in enumerate(members):
            st = self.state[q]
            st["weight_norm"], st["adam_norm"], st["trust_ratio"] = norms[k, 0], norms[k, 1], norms[k, 2]
        w = dict(n=p.numel(), segs=segs, scratch=scratch, norms=norms)
        self._work[key] = w
        return w

    def _setup_flat_range(self, lo, hi):
        super()._setup_flat_range(lo, hi)
        self._work.pop((lo, hi), None)  # the members' state entries are new: point them at the norms again

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._work.clear()

    def _update(self, group, p, g, states, step, where=None):
        w = self._plan(where, p)
        ops.lamb_step_(self._desc(group), p, g, states[0], states[1], w["scratch"], w["segs"], w["norms"], group["lr"])


class _TorchLamb(torch.optim.Optimizer):
    """Lamb in torch ops, for parameters the kernels do not cover (CPU): the algorithm of the reference's
    ``LambOptimizer`` with ``debias=False``, ``adam=False``, ``clamp_value=10`` and its state layout."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=0):
        if lr <= 0.0 or eps < 0.0 or not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0 or weight_decay < 0:
            raise ValueError("Lamb: invalid lr / eps / betas / weight_decay")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        self.clamp_value, self.adam, self.debias = 10, False, False

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for group in self.param_groups:
            b1, b2 = group["betas"]
            for p in group["params"]:
                if p.grad is None:
                    continue
                if p.grad.is_sparse:
                    raise RuntimeError("Lamb does not support sparse gradients")
                st = self.state[p]
                if not st:
                    st["step"] = 0
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["step"] += 1
                m, v = st["exp_avg"], st["exp_avg_sq"]
                m.mul_(b1).add_(p.grad, alpha=1 - b1)
                v.mul_(b2).addcmul_(p.grad, p.grad, value=1 - b2)
                update = m / v.sqrt().add(group["eps"])
                if group["weight_decay"] != 0:
                    update.add_(p, alpha=group["weight_decay"])
                w_norm = torch.norm(p).clamp(0, self.clamp_value)
                u_norm = torch.norm(update)
                trust = 1 if (w_norm == 0 or u_norm == 0) else w_norm / u_norm
                st["weight_norm"], st["adam_norm"], st["trust_ratio"] = w_norm, u_norm, trust
                p.add_(update, alpha=-group["lr"] * trust)
        return loss


# ---------------------------------------------------------------------------------------------- front-ends
class AdaGrad(Optimizer):
    """AdaGrad (optimizers.py:115-170)."""

    def __init__(self, learning_rate: Union[float, LearningRateSchedule] = 0.001,
                 initial_accumulator_value: float = 0.1, epsilon: float = 1e-07):
        super(AdaGrad, self).__init__(learning_rate)
        self.initial_accumulator_value = initial_accumulator_value
        self.epsilon = epsilon

    def _create_pytorch_optimizer(self, params):
        params = list(params)
        cls = GcmiAdagrad if _all_cuda(params) else torch.optim.Adagrad
        return cls(params, self._initial_lr(), initial_accumulator_value=self.initial_accumulator_value,
                   eps=self.epsilon)


class Adam(Optimizer):
    """Adam (optimizers.py:190-241)."""

    def __init__(self, learning_rate: Union[float, LearningRateSchedule] = 0.001,
                 beta1: float = 0.9, beta2: float = 0.999, epsilon: float = 1e-08,
                 weight_decay: float = 0):
        super(Adam, self).__init__(learning_rate)
        self.beta1 = beta1
        self.beta2 = beta2
        self.epsilon = epsilon
        self.weight_decay = weight_decay

    def _create_pytorch_optimizer(self, params):
        params = list(params)
        # host-side / exotic configurations: torch's own optimizer
        native = _all_cuda(params) and isinstance(self.weight_decay, (int, float))
        cls = GcmiAdam if native else torch.optim.Adam
        return cls(params, lr=self._initial_lr(), betas=(self.beta1, self.beta2), eps=self.epsilon,
                   weight_decay=self.weight_decay)


class SparseAdam(Optimizer):
    """Sparse (lazy) Adam (optimizers.py:260-307): torch's own optimizer, nothing native."""

    def __init__(self, learning_rate: Union[float, LearningRateSchedule] = 0.001,
                 beta1: float = 0.9, beta2: float = 0.999, epsilon: float = 1e-08):
        super(SparseAdam, self).__init__(learning_rate)
        self.beta1 = beta1
        self.beta2 = beta2
        self.epsilon = epsilon

    def _create_pytorch_optimizer(self, params):
        return torch.optim.SparseAdam(params, self._initial_lr(), (self.beta1, self.beta2), self.epsilon)


class AdamW(Optimizer):
    """AdamW (optimizers.py:310-367)."""

    def __init__(self, learning_rate: Union[float, LearningRateSchedule] = 0.001,
                 weight_decay: Union[float, LearningRateSchedule] = 0.01, beta1: float = 0.9,
                 beta2: float = 0.999, epsilon: float = 1e-08, amsgrad: bool = False):
        super(AdamW, self).__init__(learning_rate)
        self.weight_decay = weight_decay
        self.beta1 = beta1
        self.beta2 = beta2
        self.epsilon = epsilon
        self.amsgrad = amsgrad

    def _create_pytorch_optimizer(self, params):
        params = list(params)
        if _all_cuda(params) and not self.amsgrad and isinstance(self.weight_decay, (int, float)):
            return GcmiAdamW(params, self._initial_lr(), (self.beta1, self.beta2), self.epsilon, self.weight_decay)
        return torch.optim.AdamW(params, self._initial_lr(), (self.beta1, self.beta2), self.epsilon,
                                 self.weight_decay, self.amsgrad)


class RMSProp(Optimizer):
    """RMSProp (optimizers.py:390-437)."""

    def __init__(self, learning_rate: Union[float, LearningRateSchedule] = 0.001, momentum: float = 0.0,
                 decay: float = 0.9, epsilon: float = 1e-10):
        super(RMSProp, self).__init__(learning_rate)
        self.momentum = momentum
        self.decay = decay
        self.epsilon = epsilon

    def _create_pytorch_optimizer(self, params):
        params = list(params)
        cls = GcmiRMSprop if _all_cuda(params) else torch.optim.RMSprop
        return cls(params, self._initial_lr(), alpha=self.decay, eps=self.epsilon, momentum=self.momentum)


class GradientDescent(Optimizer):
    """Plain gradient descent (optimizers.py:460-488)."""

    def __init__(self, learning_rate: Union[float, LearningRateSchedule] = 0.001):
        super(GradientDescent, self).__init__(learning_rate)

    def _create_pytorch_optimizer(self, params):
        params = list(params)
        cls = GcmiSGD if _all_cuda(params) else torch.optim.SGD
        return cls(params, self._initial_lr())


class KFAC(Optimizer):
    """KFAC (optimizers.py:776-814): the constructor only; the second-order optimizer itself is not implemented."""

    def __init__(self, **kwargs):
        self.kwargs = kwargs

    def _create_pytorch_optimizer(self):
        raise NotImplementedError("KFAC is not implemented in deepchem_amd")


class Lamb(Optimizer):
    """Lamb (optimizers.py:817-881; You et al., arXiv:1904.00962)."""

    def __init__(self, learning_rate: Union[float, LearningRateSchedule] = 0.001, beta1: float = 0.9,
                 beta2: float = 0.999, epsilon: float = 1e-08, weight_decay: float = 0):
        super(Lamb, self).__init__(learning_rate)
        self.beta1 = beta1
        self.beta2 = beta2
        self.epsilon = epsilon
        self.weight_decay = weight_decay

    def _create_pytorch_optimizer(self, params):
        params = list(params)
        cls = GcmiLamb if _all_cuda(params) else _TorchLamb
        return cls(params, lr=self._initial_lr(), betas=(self.beta1, self.beta2), eps=self.epsilon,
                   weight_decay=self.weight_decay)


# ---------------------------------------------------------------------------------------------- schedules
class ExponentialDecay(LearningRateSchedule):
    """initial_rate * decay_rate ** (step / decay_steps), in jumps every decay_steps when ``staircase``
    (optimizers.py:504-547)."""

    def __init__(self, initial_rate: float, decay_rate: float, decay_steps: int, staircase: bool = True):
        self.initial_rate = initial_rate
        self.decay_rate = decay_rate
        self.decay_steps = decay_steps
        self.staircase = staircase

    def _create_pytorch_schedule(self, optimizer):
        if self.staircase:
            return torch.optim.lr_scheduler.StepLR(optimizer, self.decay_steps, self.decay_rate)
        return torch.optim.lr_scheduler.ExponentialLR(optimizer, math.pow(self.decay_rate, 1 / self.decay_steps))


def _warmup_then_linear(step: int, *, num_warmup_steps: int, num_training_steps: int):
    if step < num_warmup_steps:
        return float(step) / float(max(1, num_warmup_steps))
    return max(0.0, float(num_training_steps - step) / float(max(1, num_training_steps - num_warmup_steps)))


def _warmup_then_constant(step: int, *, num_warmup_steps: int):
    if step < num_warmup_steps:
        return float(step) / float(max(1.0, num_warmup_steps))
    return 1.0


class LambdaLRWithWarmup(LearningRateSchedule):
    """Linear warm-up to the optimizer's rate, then a linear decay to 0 at ``num_training_steps``
    (``warmup_type='linear'``) or a constant rate (``'constant'``) (optimizers.py:557-636)."""

    def __init__(self, initial_rate: float, num_warmup_steps: int, num_training_steps: Optional[int] = None,
                 warmup_type: str = 'linear'):
        self.initial_rate = initial_rate
        self.num_warmup_steps = num_warmup_steps
        self.num_training_steps = num_training_steps
        self.warmup_type = warmup_type

    def _create_pytorch_schedule(self, optimizer):
        if self.warmup_type == 'linear':
            f = partial(_warmup_then_linear, num_warmup_steps=self.num_warmup_steps,
                        num_training_steps=self.num_training_steps)
        elif self.warmup_type == 'constant':
            f = partial(_warmup_then_constant, num_warmup_steps=self.num_warmup_steps)
        else:
            raise ValueError("Warmup type %s is not supported." % self.warmup_type)
        return torch.optim.lr_scheduler.LambdaLR(optimizer, f)


class PolynomialDecay(LearningRateSchedule):
    """From initial_rate to final_rate over decay_steps as (1 - step / decay_steps) ** power (optimizers.py:639-685).
    As in the reference, the torch schedule is a ``LambdaLR`` whose factor is that rate itself."""

    def __init__(self, initial_rate: float, final_rate: float, decay_steps: int, power: float = 1.0):
        self.initial_rate = initial_rate
        self.final_rate = final_rate
        self.decay_steps = decay_steps
        self.power = power

    def _create_pytorch_schedule(self, optimizer):

        def f(step):
            t = min(step, self.decay_steps) / self.decay_steps
            return ((self.initial_rate - self.final_rate) * (1 - t)**self.power) + self.final_rate

        return torch.optim.lr_scheduler.LambdaLR(optimizer, f)


class LinearCosineDecay(LearningRateSchedule):
    """Linear cosine decay (optimizers.py:695-741); as in the reference, a ``LambdaLR`` whose factor is the rate."""

    def __init__(self, initial_rate: float, decay_steps: int, alpha: float = 0.0, beta: float = 0.001,
                 num_periods: float = 0.5):
        self.initial_rate = initial_rate
        self.decay_steps = decay_steps
        self.alpha = alpha
        self.beta = beta
        self.num_periods = num_periods

    def _create_pytorch_schedule(self, optimizer):

        def f(step):
            t = min(step, self.decay_steps) / self.decay_steps
            cosine = 0.5 * (1 + math.cos(math.pi * 2 * self.num_periods * t))
            return self.initial_rate * ((self.alpha + (1 - t)) * cosine + self.beta)

        return torch.optim.lr_scheduler.LambdaLR(optimizer, f)


class PiecewiseConstantSchedule(LearningRateSchedule):
    """Rate scaled by a constant factor at each boundary (optimizers.py:750-773).  The reference gives it no torch
    schedule; neither does this one."""

    def __init__(self, initial_rate: float, boundaries_and_scales: Optional[Dict[int, float]] = None):
        self.initial_rate = initial_rate
        self.boundaries_and_scales = boundaries_and_scales
