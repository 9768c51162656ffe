"""Writes tests/golden/optim_ref.npz: what the reference's optimizers and learning-rate schedules compute.

Run with the reference checkout where oracle/gen_golden.py expects it.  For every optimizer front-end of
deepchem/models/optimizers.py that this project runs natively the file holds the constructor defaults, NumPy-seeded
parameters of shapes (1,), (3,), (8, 8), (1000,), five seeded gradients per parameter and the parameters after each of
five steps of the reference's own ``_create_pytorch_optimizer`` object (``LambOptimizer`` for ``Lamb``); for Lamb also
the recorded trust ratios.  One Lamb tensor is all zeros (trust ratio 1) and one has a norm above 10 (the clamp binds).
For every schedule it holds the learning rate over 12 steps with decay_steps = 4.
"""
import inspect
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(1,), (3,), (8, 8), (1000,)]
STEPS = 5
LR_STEPS = 12

# name -> constructor arguments beyond the defaults (the defaults are what a script gets; the extra cases turn on
# the terms the defaults leave out)
OPTIMIZERS = {
    "GradientDescent": ("GradientDescent", {}),
    "AdaGrad": ("AdaGrad", {}),
    "RMSProp": ("RMSProp", {}),
    "RMSProp_momentum": ("RMSProp", {"momentum": 0.9}),
    "Adam": ("Adam", {}),
    "Adam_l2": ("Adam", {"weight_decay": 0.1}),
    "AdamW": ("AdamW", {}),
    "Lamb": ("Lamb", {}),
    "Lamb_l2": ("Lamb", {"weight_decay": 0.1}),
}
SCHEDULES = {
    "ExponentialDecay_staircase": ("ExponentialDecay", dict(initial_rate=1e-3, decay_rate=0.5, decay_steps=4)),
    "ExponentialDecay_smooth": ("ExponentialDecay", dict(initial_rate=1e-3, decay_rate=0.5, decay_steps=4,
                                                         staircase=False)),
    "PolynomialDecay": ("PolynomialDecay", dict(initial_rate=1e-3, final_rate=1e-4, decay_steps=4, power=2.0)),
    "LinearCosineDecay": ("LinearCosineDecay", dict(initial_rate=1e-3, decay_steps=4)),
    "LambdaLRWithWarmup_linear": ("LambdaLRWithWarmup", dict(initial_rate=1e-3, num_warmup_steps=4,
                                                             num_training_steps=10)),
    "LambdaLRWithWarmup_constant": ("LambdaLRWithWarmup", dict(initial_rate=1e-3, num_warmup_steps=4,
                                                               warmup_type="constant")),
}
CLASSES = ["AdaGrad", "Adam", "SparseAdam", "AdamW", "RMSProp", "GradientDescent", "KFAC", "Lamb", "ExponentialDecay",
           "LambdaLRWithWarmup", "PolynomialDecay", "LinearCosineDecay", "PiecewiseConstantSchedule"]


def inputs(name):
    rng = np.random.RandomState(sum(map(ord, name)))
    params = [rng.randn(*s).astype(np.float32) for s in SHAPES]
    if name.startswith("Lamb"):
        params[1][:] = 0.0          # zero weight norm: trust ratio 1
        params[3] *= 2.0            # norm ~ 63: the clamp at 10 binds
    grads = [[rng.randn(*s).astype(np.float32) for s in SHAPES] for _ in range(STEPS)]
    return params, grads


def signature(cls):
    return [[p.name, None if p.default is inspect.Parameter.empty else repr(p.default), int(p.kind)]
            for p in list(inspect.signature(cls.__init__).parameters.values())[1:]]


def main():
    import torch
    from oracle.gen_golden import import_reference
    import_reference()
    from deepchem.models import optimizers as R
    out = {"signatures": np.array(json.dumps({c: signature(getattr(R, c)) for c in CLASSES})),
           "optimizers": np.array(json.dumps({k: [c, kw] for k, (c, kw) in OPTIMIZERS.items()})),
           "schedules": np.array(json.dumps({k: [c, kw] for k, (c, kw) in SCHEDULES.items()}))}
    for name, (cls, kw) in OPTIMIZERS.items():
        params, grads = inputs(name)
        ps = [torch.nn.Parameter(torch.tensor(p)) for p in params]
        opt = getattr(R, cls)(learning_rate=1e-3, **kw)._create_pytorch_optimizer(ps)
        for i, p in enumerate(params):
            out["%s/p0/%d" % (name, i)] = p
        for s in range(STEPS):
            for i, p in enumerate(ps):
                p.grad = torch.tensor(grads[s][i])
                out["%s/g%d/%d" % (name, s, i)] = grads[s][i]
            opt.step()
            for i, p in enumerate(ps):
                out["%s/p%d/%d" % (name, s + 1, i)] = p.detach().numpy().copy()
            if cls == "Lamb":
                out["%s/trust%d" % (name, s + 1)] = np.array([float(opt.state[p]["trust_ratio"]) for p in ps], np.float64)
    for name, (cls, kw) in SCHEDULES.items():
        p = torch.nn.Parameter(torch.zeros(1))
        sched = getattr(R, cls)(**kw)
        opt = R.GradientDescent(learning_rate=sched)._create_pytorch_optimizer([p])
        s = sched._create_pytorch_schedule(opt)
        rates = []
        for _ in range(LR_STEPS):
            rates.append(opt.param_groups[0]["lr"])
            p.grad = torch.zeros(1)
            opt.step()
            s.step()
        out["lr/%s" % name] = np.array(rates, np.float64)
    path = os.path.join(ROOT, "tests", "golden", "optim_ref.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
