"""Optimizers and learning-rate schedules on GraphConvModel's training paths: the small-batch engine, the per-batch
native step and the autograd path with torch's own optimizer and scheduler give the same trajectory; checkpoints
resume; the optimizer state interchanges with the torch counterpart.

16 synthetic molecules, batches of 8, [64, 64] / 128, six steps, exact-fp32 products.  Bounds on the per-step losses:
  engine vs per-batch step   first loss 1e-5 relative, all rtol 2e-3 + 1e-6 -- what tests/test_gpu_small.py
                             (test_small_engine_other_widths) holds plain Adam to for the same comparison;
  per-batch vs autograd      rtol 1e-4 + 1e-6 -- what tests/test_gpu_model.py (test_native_step_equals_autograd_step)
                             holds plain Adam to.
Plain Adam runs as the control; each case prints its figures beside the control's."""
import copy
import warnings

import numpy as np
import pytest
import torch

import deepchem_amd as dc
from deepchem_amd.feat.mol_graphs import convmols_from_packed
from deepchem_amd.utils.synthetic import synthetic_labels, synthetic_molecules
from oracle import graphconv_oracle as GO

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
O = dc.models.optimizers
N, T, B, STEPS = 16, 3, 8, 6

CASES = {
    "Adam": lambda: O.Adam(1e-3),
    "GradientDescent": lambda: O.GradientDescent(1e-3),
    "AdaGrad": lambda: O.AdaGrad(1e-3),
    "RMSProp": lambda: O.RMSProp(1e-3),
    "RMSProp_momentum": lambda: O.RMSProp(1e-3, momentum=0.9),
    "Adam_l2": lambda: O.Adam(1e-3, weight_decay=0.1),
    "AdamW": lambda: O.AdamW(1e-3),
    "Adam_ExponentialDecay_staircase": lambda: O.Adam(O.ExponentialDecay(1e-3, 0.5, 4)),
    # (the reference's torch schedule multiplies the initial rate by the decayed rate: 9e-4 falling to 3e-4)
    "Adam_PolynomialDecay": lambda: O.Adam(O.PolynomialDecay(0.03, 0.01, 4)),
    "Lamb": lambda: O.Lamb(1e-3),
}


@pytest.fixture(scope="module")
def data():
    packed = synthetic_molecules(N, seed=3, max_atoms=30)
    y, w = synthetic_labels(N, T, "classification", 3, pos_rate=0.4)
    state = GO.init_state(GO.ModelConfig(T, batch_size=B), 1)
    return dc.data.NumpyDataset(convmols_from_packed(packed), y, w), state


@pytest.fixture(autouse=True)
def exact_products():
    dc.set_gemm_mode("exact")
    yield
    dc.set_gemm_mode("fast")


class Spy:
    """Counts the calls that tell the three paths apart."""

    def __init__(self, monkeypatch):
        from deepchem_amd.native import NativeNet
        from deepchem_amd.small import SmallBatchEngine
        self.engine = self.native = 0
        fit, lb = SmallBatchEngine.fit, NativeNet.loss_backward

        def spy_fit(eng, descs, *a, **k):
            self.engine += len(descs)
            return fit(eng, descs, *a, **k)

        def spy_lb(net, *a, **k):
            self.native += 1
            return lb(net, *a, **k)

        monkeypatch.setattr(SmallBatchEngine, "fit", spy_fit)
        monkeypatch.setattr(NativeNet, "loss_backward", spy_lb)

    def take(self):
        out = (self.engine, self.native)
        self.engine = self.native = 0
        return out


def _model(case, grad_mode, state, model_dir=None):
    model = dc.models.torch_models.GraphConvModel(T, number_input_features=[75, 64], batch_size=B, grad_mode=grad_mode,
                                                  optimizer=CASES[case](), device=torch.device(DEV), log_frequency=1,
                                                  model_dir=model_dir)
    model.model.load_state_dict({k: v.clone() for k, v in state.items()})
    return model


def _leg(case, grad_mode, data, leg, monkeypatch):
    """One of the three paths from the common initial state: per-step losses, final state, step and scheduler counts."""
    ds, state = data
    model = _model(case, grad_mode, state)
    kwargs = {}
    if leg == "per_batch":
        model.small_batch_engine = False
    if leg == "autograd":
        model._ensure_built()
        with monkeypatch.context() as mp:  # torch's own optimizer (for Lamb: the torch-op restatement) and scheduler
            mp.setattr(O, "_all_cuda", lambda params: False)
            model._pytorch_optimizer = model.optimizer._create_pytorch_optimizer(model.model.parameters())
        assert not isinstance(model._pytorch_optimizer, O.FlatOptimizer)
        model._lr_schedule = model._new_schedule(model._pytorch_optimizer)
        kwargs["loss"] = lambda outputs, labels, weights: model._loss_fn(outputs, labels, weights)
    losses = []
    with warnings.catch_warnings():
        warnings.filterwarnings("error", message=".*lr_scheduler.step.*")  # torch's complaint about the order of the steps
        model.fit(ds, nb_epoch=STEPS * B // N, deterministic=True, checkpoint_interval=0, all_losses=losses, **kwargs)
    sched = model._lr_schedule
    return dict(losses=np.array(losses), step=model.get_global_step(), epoch=None if sched is None else sched.last_epoch,
                lr=model._pytorch_optimizer.param_groups[0]["lr"],
                state={k: v.detach().cpu() for k, v in model.model.state_dict().items()})


def _rel(a, b):
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-12)))


_CONTROL = {}


def _figures(runs):
    out = {}
    if "engine" in runs:
        out["engine_vs_per_batch"] = _rel(runs["engine"]["losses"], runs["per_batch"]["losses"])
    out["per_batch_vs_autograd"] = _rel(runs["per_batch"]["losses"], runs["autograd"]["losses"])
    return out


@pytest.mark.parametrize("grad_mode", ["reference", "full"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_three_paths_one_trajectory(case, grad_mode, data, monkeypatch):
    spy = Spy(monkeypatch)
    runs, calls = {}, {}
    legs = ("per_batch", "autograd") if case == "Lamb" else ("engine", "per_batch", "autograd")
    for leg in legs:
        runs[leg] = _leg(case, grad_mode, data, leg, monkeypatch)
        calls[leg] = spy.take()
    # which path ran
    if case == "Lamb":
        assert calls["per_batch"] == (0, STEPS)  # the model's default path for Lamb IS the per-batch native step
        lamb_default = _leg(case, grad_mode, data, "engine", monkeypatch)  # (small_batch_engine left on)
        assert spy.take() == (0, STEPS) and np.array_equal(lamb_default["losses"], runs["per_batch"]["losses"])
    else:
        assert calls["engine"] == (STEPS, 0), calls
        assert calls["per_batch"] == (0, STEPS), calls
    assert calls["autograd"] == (0, 0), calls
    for leg in legs:
        assert runs[leg]["step"] == STEPS and len(runs[leg]["losses"]) == STEPS
        assert runs[leg]["epoch"] == (STEPS if "Decay" in case else None), (leg, runs[leg]["epoch"])
        assert runs[leg]["lr"] == runs["autograd"]["lr"], (leg, runs[leg]["lr"], runs["autograd"]["lr"])
    figures = _figures(runs)
    if case == "Adam":
        _CONTROL[grad_mode] = figures
    elif grad_mode not in _CONTROL:  # the control: plain Adam through the same three legs
        _CONTROL[grad_mode] = _figures({leg: _leg("Adam", grad_mode, data, leg, monkeypatch)
                                        for leg in ("engine", "per_batch", "autograd")})
    control = _CONTROL[grad_mode]
    print("%s / %s: max relative difference of the per-step losses %s; plain Adam (control) %s"
          % (case, grad_mode, figures, control))
    for k, v in figures.items():
        if v > 2 * max(control[k], 1e-7):
            print("FINDING: %s / %s: %s = %.3g is more than twice the control's %.3g" % (case, grad_mode, k, v, control[k]))
    if "engine" in runs:
        a, b = runs["engine"]["losses"], runs["per_batch"]["losses"]
        assert abs(a[0] - b[0]) <= 1e-5 * abs(b[0]), (a, b)
        assert np.allclose(a, b, rtol=2e-3, atol=1e-6), (a, b)
    a, b = runs["per_batch"]["losses"], runs["autograd"]["losses"]
    assert np.allclose(a, b, rtol=1e-4, atol=1e-6), (a, b)
    # the parameters moved, and by the same amount on every path
    moved = sum(int(not torch.equal(runs["per_batch"]["state"][k], data[1][k])) for k in data[1])
    assert moved >= 4


@pytest.mark.parametrize("case", ["RMSProp_momentum", "Lamb"])
def test_checkpoint_resumes_the_trajectory_and_state_interchanges_with_torch(case, tmp_path, monkeypatch):
    """Three steps, save, a fresh model restores, three more: the parameters of an uninterrupted six-step run, under
    a smooth ExponentialDecay (as far as two executions of the same steps agree: see the bound below)."""
    packed = synthetic_molecules(24, seed=4, max_atoms=30)
    y, w = synthetic_labels(24, T, "classification", 4, pos_rate=0.4)
    ds = dc.data.NumpyDataset(convmols_from_packed(packed), y, w)
    state = GO.init_state(GO.ModelConfig(T, batch_size=B), 2)
    sched = lambda: O.ExponentialDecay(1e-3, 0.5, 4, staircase=False)
    make = {"RMSProp_momentum": lambda: O.RMSProp(sched(), momentum=0.9), "Lamb": lambda: O.Lamb(sched())}[case]
    monkeypatch.setitem(CASES, case, make)
    whole = _model(case, "full", state, str(tmp_path / "whole"))
    whole.fit(ds, nb_epoch=2, deterministic=True, checkpoint_interval=0)
    first = _model(case, "full", state, str(tmp_path / "cut"))
    first.fit(ds, nb_epoch=1, deterministic=True, checkpoint_interval=0)
    first.save_checkpoint()
    second = _model(case, "full", GO.init_state(GO.ModelConfig(T, batch_size=B), 9), str(tmp_path / "cut"))
    second.restore()
    assert second.get_global_step() == 3
    second.fit(ds, nb_epoch=1, deterministic=True, checkpoint_interval=0)
    assert whole.get_global_step() == second.get_global_step() == 6
    assert whole._pytorch_optimizer.param_groups[0]["lr"] == pytest.approx(second._pytorch_optimizer.param_groups[0]["lr"], rel=1e-12)
    # Both runs execute the same six steps, but the backward kernels sum with float atomics, so a gradient differs
    # between two executions at rounding level (1e-7 of its largest term).  A rule of the form lr g / (sqrt(v) + eps)
    # turns an entry whose gradient IS at that level into a step of either sign, amp lr at most per step (amp =
    # 1 / sqrt(1 - alpha) = 3.2 for RMSProp's first steps, times 1 + mu + mu^2 = 2.7 with momentum; Lamb's trust ratio
    # only shrinks it), so single entries may differ by 2 amp lr per step -- the form of tests/test_gpu_small.py's
    # _same_after_adam, whose bounds on the typical entry (median 2e-4, mean 1e-3 of the tensor's scale) and on
    # buffers (2e-4) are taken as they are.  A lost momentum buffer, step count or learning rate moves EVERY entry by
    # about amp lr per step, two orders above the median bound.
    amp = 3.2 * 2.7 if case == "RMSProp_momentum" else 1.0
    sw, s2 = whole.model.state_dict(), second.model.state_dict()
    params = {k for k, _ in whole.model.named_parameters()}
    worst = 0.0
    for k in sw:
        if not sw[k].is_floating_point():
            assert torch.equal(sw[k], s2[k]), k
            continue
        err = (sw[k].double() - s2[k].double()).abs().cpu().numpy()
        scale = max(float(sw[k].abs().max()), 1e-3)
        worst = max(worst, float(err.max()))
        if k in params:
            assert err.max() <= 2.2 * amp * 1e-3 * 6, (k, float(err.max()))
            assert np.median(err) <= 2e-4 * scale and np.mean(err) <= 1e-3 * scale, (k, float(np.median(err)), float(np.mean(err)))
        else:
            assert err.max() <= 2e-4 * scale, (k, float(err.max()), scale)
    print("%s: largest difference between the resumed and the uninterrupted run %.3g" % (case, worst))
    # the optimizer state in the torch counterpart's layout: into it and back
    opt = second._pytorch_optimizer
    sd = opt.state_dict()
    keys = {"RMSProp_momentum": {"step", "square_avg", "momentum_buffer"},
            "Lamb": {"step", "exp_avg", "exp_avg_sq", "weight_norm", "adam_norm", "trust_ratio"}}[case]
    trained = [st for st in sd["state"].values() if st]
    assert trained and all(set(st) == keys for st in trained)
    with monkeypatch.context() as mp:
        mp.setattr(O, "_all_cuda", lambda params: False)
        plain = second.optimizer._create_pytorch_optimizer(second.model.parameters())
    assert not isinstance(plain, O.FlatOptimizer)
    before = {i: {k: (v.clone() if torch.is_tensor(v) else v) for k, v in st.items()} for i, st in sd["state"].items()}
    plain.load_state_dict(sd)
    back = copy.deepcopy(plain.state_dict())
    for p in second.model.parameters():
        p.grad = torch.zeros_like(p)
    plain.step()  # torch's optimizer runs on the loaded state
    opt.load_state_dict(back)
    after = opt.state_dict()["state"]
    for i, st in before.items():
        for k in ("square_avg", "momentum_buffer", "exp_avg", "exp_avg_sq"):
            if k in st:
                assert torch.equal(st[k], after[i][k]), (i, k)
        if "step" in st:
            assert float(st["step"]) == float(after[i]["step"]) == 6
