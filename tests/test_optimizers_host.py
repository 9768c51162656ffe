"""dc.models.optimizers against the fixture recorded from the reference (tools/gen_golden_optim.py): constructor
signatures and defaults, and -- on CPU parameters, where the front-ends hand out torch's own optimizers -- the
parameters after each of five steps and the learning rate of every schedule over 12 steps."""
import inspect
import json

import numpy as np
import pytest
import torch

import deepchem_amd as dc
from tests.util import load_golden

O = dc.models.optimizers
GOLD = load_golden("optim_ref.npz")
SIGNATURES = json.loads(str(GOLD["signatures"]))
OPTIMIZERS = json.loads(str(GOLD["optimizers"]))
SCHEDULES = json.loads(str(GOLD["schedules"]))


@pytest.mark.parametrize("name", sorted(SIGNATURES))
def test_constructor_signature_and_defaults(name):
    cls = getattr(O, name)
    got = [[p.name, None if p.default is inspect.Parameter.empty else repr(p.default), int(p.kind)]
           for p in list(inspect.signature(cls.__init__).parameters.values())[1:]]
    assert got == SIGNATURES[name]


def test_class_tree():
    for name in SIGNATURES:
        base = O.LearningRateSchedule if "Decay" in name or "Schedule" in name or "Warmup" in name else O.Optimizer
        assert issubclass(getattr(O, name), base), name
    assert issubclass(O.GcmiAdam, O.FlatOptimizer)


@pytest.mark.parametrize("name", sorted(OPTIMIZERS))
def test_cpu_optimizer_reproduces_the_reference(name):
    cls, kw = OPTIMIZERS[name]
    ps = [torch.nn.Parameter(torch.tensor(GOLD["%s/p0/%d" % (name, i)])) for i in range(4)]
    opt = getattr(O, cls)(learning_rate=1e-3, **kw)._create_pytorch_optimizer(ps)
    assert not isinstance(opt, O.FlatOptimizer)  # CPU parameters: torch's own
    for s in range(5):
        for i, p in enumerate(ps):
            p.grad = torch.tensor(GOLD["%s/g%d/%d" % (name, s, i)])
        opt.step()
        for i, p in enumerate(ps):
            err = np.abs(p.detach().numpy() - GOLD["%s/p%d/%d" % (name, s + 1, i)]).max()
            assert err <= 1e-6, (name, s, i, err)
        if cls == "Lamb":
            trust = np.array([float(opt.state[p]["trust_ratio"]) for p in ps])
            assert np.allclose(trust, GOLD["%s/trust%d" % (name, s + 1)], rtol=1e-5, atol=0), (name, s, trust)
    if cls == "Lamb":
        assert set(opt.state[ps[0]]) == {"step", "exp_avg", "exp_avg_sq", "weight_norm", "adam_norm", "trust_ratio"}


@pytest.mark.parametrize("name", sorted(SCHEDULES))
def test_schedule_reproduces_the_reference(name):
    cls, kw = SCHEDULES[name]
    p = torch.nn.Parameter(torch.zeros(1))
    sched = getattr(O, cls)(**kw)
    opt = O.GradientDescent(learning_rate=sched)._create_pytorch_optimizer([p])
    s = sched._create_pytorch_schedule(opt)
    rates = []
    for _ in range(12):
        rates.append(opt.param_groups[0]["lr"])
        p.grad = torch.zeros(1)
        opt.step()
        s.step()
    want = GOLD["lr/%s" % name]
    assert np.allclose(rates, want, rtol=1e-12, atol=0), (rates, want)


def test_schedule_objects_are_torchs():
    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.SGD([p], 1e-3)
    L = torch.optim.lr_scheduler
    assert type(O.ExponentialDecay(1e-3, 0.9, 1000)._create_pytorch_schedule(opt)) is L.StepLR
    assert type(O.ExponentialDecay(1e-3, 0.9, 1000, staircase=False)._create_pytorch_schedule(opt)) is L.ExponentialLR
    for s in (O.PolynomialDecay(1e-3, 1e-4, 10), O.LinearCosineDecay(1e-3, 10), O.LambdaLRWithWarmup(1e-3, 2, 10)):
        assert type(s._create_pytorch_schedule(opt)) is L.LambdaLR
    with pytest.raises(NotImplementedError):
        O.PiecewiseConstantSchedule(1e-3, {2: 0.5})._create_pytorch_schedule(opt)


def test_fallbacks_are_torchs_own():
    p = [torch.nn.Parameter(torch.zeros(3))]
    assert type(O.AdamW(amsgrad=True)._create_pytorch_optimizer(p)) is torch.optim.AdamW
    assert type(O.Adam(weight_decay=0.1)._create_pytorch_optimizer(p)) is torch.optim.Adam
    assert type(O.AdaGrad()._create_pytorch_optimizer(p)) is torch.optim.Adagrad
    assert type(O.RMSProp()._create_pytorch_optimizer(p)) is torch.optim.RMSprop
    assert type(O.GradientDescent()._create_pytorch_optimizer(p)) is torch.optim.SGD
    assert type(O.SparseAdam()._create_pytorch_optimizer(p)) is torch.optim.SparseAdam


def test_cabi_rejects_bad_optimizer_arguments():
    """Argument checks run before any launch: no GPU needed."""
    from deepchem_amd import _lib, ops
    import ctypes
    for rule in (-1, 5, 99):  # (5 = Lamb: not an elementwise rule)
        with pytest.raises(_lib.GcmiError):
            _lib.call("gcmi_opt_step", ctypes.byref(ops.opt_desc(rule)), None, None, None, None, 0, 1e-3, 1, None)
    with pytest.raises(_lib.GcmiError):  # step 0
        _lib.call("gcmi_opt_step", ctypes.byref(ops.opt_desc("sgd")), None, None, None, None, 0, 1e-3, 0, None)
    with pytest.raises(_lib.GcmiError):  # NULL buffers with n > 0
        _lib.call("gcmi_opt_step", ctypes.byref(ops.opt_desc("sgd")), None, None, None, None, 8, 1e-3, 1, None)
    with pytest.raises(_lib.GcmiError):  # NULL description
        _lib.call("gcmi_opt_step", None, None, None, None, None, 8, 1e-3, 1, None)
    with pytest.raises(_lib.GcmiError):  # a rule that is not Lamb
        _lib.call("gcmi_lamb_step", ctypes.byref(ops.opt_desc("adamw")), None, None, None, None, None, None, 1, 8, None,
                  1e-3, None)
    with pytest.raises(_lib.GcmiError):  # NULL buffers
        _lib.call("gcmi_lamb_step", ctypes.byref(ops.opt_desc("lamb", beta1=0.9, beta2=0.999)), None, None, None, None,
                  None, None, 1, 8, None, 1e-3, None)
    assert _lib.load().gcmi_lamb_scratch_floats(-1, 0) < 0
    assert _lib.load().gcmi_lamb_scratch_floats(1000, 3) >= 1000
