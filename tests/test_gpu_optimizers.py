"""The optimizer kernels (csrc/optim.hip) through ``ops`` and through the ``FlatOptimizer`` classes: against the
fixture recorded from the reference (tools/gen_golden_optim.py) and against ``torch.optim`` on the CPU for random data.

Bound: max abs error < 2e-6 after five steps at lr = 1e-3, the bound ``test_adam_matches_torch``
(tests/test_gpu_kernels.py) holds the Adam kernel to: the rules do the same few fp32 operations per element.  Every
figure is printed before it is asserted."""
import json

import numpy as np
import pytest
import torch

import deepchem_amd as dc
from deepchem_amd import ops
from deepchem_amd._lib import GcmiError
from tests.util import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
O = dc.models.optimizers
GOLD = load_golden("optim_ref.npz")
OPTIMIZERS = json.loads(str(GOLD["optimizers"]))
BOUND = 2e-6
LR = 1e-3

# rule -> (description arguments, torch counterpart on the CPU, the state tensors of that counterpart in kernel order)
RULES = {
    "sgd": (dict(), lambda p: torch.optim.SGD(p, LR), ()),
    "adagrad": (dict(eps=1e-7), lambda p: torch.optim.Adagrad(p, LR, initial_accumulator_value=0.1, eps=1e-7), ("sum",)),
    "rmsprop": (dict(eps=1e-10, alpha=0.9), lambda p: torch.optim.RMSprop(p, LR, alpha=0.9, eps=1e-10), ("square_avg",)),
    "rmsprop_momentum": (dict(eps=1e-10, alpha=0.9, momentum=0.9),
                         lambda p: torch.optim.RMSprop(p, LR, alpha=0.9, eps=1e-10, momentum=0.9),
                         ("square_avg", "momentum_buffer")),
    "adam_l2": (dict(beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.1),
                lambda p: torch.optim.Adam(p, LR, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.1), ("exp_avg", "exp_avg_sq")),
    "adamw": (dict(beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.01),
              lambda p: torch.optim.AdamW(p, LR, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01), ("exp_avg", "exp_avg_sq")),
}
# 1: the scalar tail alone; 7: one vector + tail; 1000: whole vectors; 4099: several workgroups + tail; the last: more
# floats than the capped grid covers at once (1024 workgroups x 256 threads x 4), so the grid strides
SIZES = [1, 7, 1000, 4099, 1024 * 256 * 4 + 5]


def _desc(rule):
    return ops.opt_desc(rule.split("_momentum")[0], **RULES[rule][0])


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("rule", sorted(RULES))
def test_elementwise_rule_matches_torch_cpu(rule, n):
    rng = np.random.RandomState(n % 1000 + len(rule))
    p0 = torch.tensor(rng.randn(n).astype(np.float32))
    grads = [torch.tensor(rng.randn(n).astype(np.float32)) for _ in range(5)]
    ref_p = torch.nn.Parameter(p0.clone())
    ref = RULES[rule][1]([ref_p])
    names = RULES[rule][2]
    p = p0.to(DEV)
    fill = 0.1 if rule == "adagrad" else 0.0
    states = [torch.full((n,), fill, device=DEV) for _ in names] + [None, None]
    for step, g in enumerate(grads, 1):
        ref_p.grad = g.clone()
        ref.step()
        ops.opt_step_(_desc(rule), p, g.to(DEV), states[0], states[1], LR, step)
    err = float((p.cpu() - ref_p.detach()).abs().max())
    print("%s n=%d: max abs error of the parameters %.3g" % (rule, n, err))
    assert err < BOUND
    for name, s in zip(names, states):
        serr = float((s.cpu() - ref.state[ref_p][name]).abs().max())
        scale = max(1.0, float(ref.state[ref_p][name].abs().max()))
        print("%s n=%d: max abs error of %s %.3g (scale %.3g)" % (rule, n, name, serr, scale))
        assert serr < BOUND * scale


def test_unaligned_pointers_take_the_scalar_path():
    rng = np.random.RandomState(3)
    n = 1001
    base = [torch.tensor(rng.randn(n + 1).astype(np.float32)) for _ in range(4)]
    ref_p = torch.nn.Parameter(base[0][1:].clone())
    ref = torch.optim.Adam([ref_p], LR, weight_decay=0.1)
    ref_p.grad = base[1][1:].clone()
    ref.step()
    dev = [b.to(DEV) for b in base]
    dev[2].zero_()
    dev[3].zero_()
    ops.opt_step_(_desc("adam_l2"), dev[0][1:], dev[1][1:], dev[2][1:], dev[3][1:], LR, 1)  # 4 bytes off 16-byte alignment
    assert float((dev[0][1:].cpu() - ref_p.detach()).abs().max()) < BOUND
    assert float(dev[0][0].cpu()) == float(base[0][0])  # the float in front is not touched


@pytest.mark.parametrize("n", [1, 7, 1000, 4099])
def test_adam_l2_without_weight_decay_is_the_adam_kernel(n):
    rng = np.random.RandomState(n)
    p0, g = (torch.tensor(rng.randn(n).astype(np.float32)).to(DEV) for _ in range(2))
    a = [p0.clone(), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)]
    b = [p0.clone(), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)]
    for step in (1, 2, 3):
        ops.adam_step_(a[0], g, a[1], a[2], LR, 0.9, 0.999, 1e-8, step)
        ops.opt_step_(ops.opt_desc("adam_l2", beta1=0.9, beta2=0.999, eps=1e-8), b[0], g, b[1], b[2], LR, step)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


@pytest.mark.parametrize("name", sorted(k for k in OPTIMIZERS if not k.startswith("Lamb")))
def test_native_optimizer_reproduces_the_reference_fixture(name):
    """The front-end's CUDA optimizer, per-tensor ``step()``, on the fixture's parameters and gradients."""
    cls, kw = OPTIMIZERS[name]
    ps = [torch.nn.Parameter(torch.tensor(GOLD["%s/p0/%d" % (name, i)]).to(DEV)) for i in range(4)]
    opt = getattr(O, cls)(learning_rate=LR, **kw)._create_pytorch_optimizer(ps)
    assert isinstance(opt, O.FlatOptimizer)
    for s in range(5):
        for i, p in enumerate(ps):
            p.grad = torch.tensor(GOLD["%s/g%d/%d" % (name, s, i)]).to(DEV)
        opt.step()
    for i, p in enumerate(ps):
        err = float(np.abs(p.detach().cpu().numpy() - GOLD["%s/p5/%d" % (name, i)]).max())
        print("%s tensor %d: max abs error %.3g" % (name, i, err))
        assert err < BOUND


# ---------------------------------------------------------------------------------------------------------- Lamb
SEG_SIZES = [1, 3, 64, 1000, 5000]


def _lamb_case(weight_decay, seed=5):
    """Arena with gaps in front of, between and behind the segments; segment 1 all zeros (trust ratio 1), segment 4
    with a norm above 10 (the clamp binds)."""
    rng = np.random.RandomState(seed)
    gaps = [2, 1, 5, 3, 7, 4]
    offs, off = [], 0
    for gap, n in zip(gaps, SEG_SIZES):
        off += gap
        offs.append(off)
        off += n
    total = off + gaps[-1]
    p = rng.randn(total).astype(np.float32)
    p[offs[1]:offs[1] + 3] = 0.0
    p[offs[4]:offs[4] + 5000] *= 2.0
    grads = [rng.randn(total).astype(np.float32) for _ in range(5)]
    return offs, total, p, grads


def _lamb_run(offs, total, p0, grads, weight_decay):
    desc = ops.opt_desc("lamb", beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=weight_decay)
    p = torch.tensor(p0).to(DEV)
    m, v = torch.zeros(total, device=DEV), torch.zeros(total, device=DEV)
    segs = torch.tensor([[o, n] for o, n in zip(offs, SEG_SIZES)], dtype=torch.int64, device=DEV)
    scratch = torch.empty(ops.lamb_scratch_floats(total, len(offs)), device=DEV)
    norms = torch.zeros((len(offs), 3), device=DEV)
    trust = []
    for g in grads:
        ops.lamb_step_(desc, p, torch.tensor(g).to(DEV), m, v, scratch, segs, norms, LR)
        trust.append(norms[:, 2].cpu().numpy().copy())
    return p.cpu(), m.cpu(), v.cpu(), np.array(trust), norms.cpu()


@pytest.mark.parametrize("weight_decay", [0.0, 0.1])
def test_lamb_matches_the_torch_restatement_on_a_segment_table(weight_decay):
    offs, total, p0, grads = _lamb_case(weight_decay)
    ps = [torch.nn.Parameter(torch.tensor(p0[o:o + n].copy())) for o, n in zip(offs, SEG_SIZES)]
    ref = O._TorchLamb(ps, lr=LR, betas=(0.9, 0.999), eps=1e-8, weight_decay=weight_decay)
    ref_trust = []
    for g in grads:
        for q, o, n in zip(ps, offs, SEG_SIZES):
            q.grad = torch.tensor(g[o:o + n].copy())
        ref.step()
        ref_trust.append([float(ref.state[q]["trust_ratio"]) for q in ps])
    p, m, v, trust, norms = _lamb_run(offs, total, p0, grads, weight_decay)
    assert ref_trust[0][1] == 1.0 and trust[0][1] == 1.0            # the zero segment
    assert float(ref.state[ps[4]]["weight_norm"]) == 10.0 and float(norms[4, 0]) == 10.0  # the clamp binds
    for k, (q, o, n) in enumerate(zip(ps, offs, SEG_SIZES)):
        err = float((p[o:o + n] - q.detach()).abs().max())
        print("lamb wd=%g segment of %d: max abs error %.3g" % (weight_decay, n, err))
        assert err < BOUND
    rel = np.abs(trust - np.array(ref_trust)) / np.abs(np.array(ref_trust))
    print("lamb wd=%g: max relative error of the trust ratios %.3g" % (weight_decay, rel.max()))
    assert rel.max() < 1e-5
    # floats that belong to no segment: untouched, in every arena
    inside = np.zeros(total, bool)
    for o, n in zip(offs, SEG_SIZES):
        inside[o:o + n] = True
    assert np.array_equal(p.numpy()[~inside], p0[~inside])
    assert not m.numpy()[~inside].any() and not v.numpy()[~inside].any()
    # the same inputs again: the same bits
    p2, m2, v2, trust2, _ = _lamb_run(offs, total, p0, grads, weight_decay)
    assert torch.equal(p, p2) and torch.equal(m, m2) and torch.equal(v, v2) and np.array_equal(trust, trust2)


@pytest.mark.parametrize("name", ["Lamb", "Lamb_l2"])
def test_native_lamb_reproduces_the_reference_fixture(name):
    cls, kw = OPTIMIZERS[name]
    ps = [torch.nn.Parameter(torch.tensor(GOLD["%s/p0/%d" % (name, i)]).to(DEV)) for i in range(4)]
    opt = O.Lamb(learning_rate=LR, **kw)._create_pytorch_optimizer(ps)
    assert isinstance(opt, O.GcmiLamb)
    for s in range(5):
        for i, p in enumerate(ps):
            p.grad = torch.tensor(GOLD["%s/g%d/%d" % (name, s, i)]).to(DEV)
        opt.step()
        trust = np.array([float(opt.state[p]["trust_ratio"]) for p in ps])
        want = GOLD["%s/trust%d" % (name, s + 1)]
        rel = np.abs(trust - want) / np.abs(want)
        print("%s step %d: trust ratios %s, max relative error %.3g" % (name, s + 1, trust, rel.max()))
        assert rel.max() < 1e-5
        for i, p in enumerate(ps):
            err = float(np.abs(p.detach().cpu().numpy() - GOLD["%s/p%d/%d" % (name, s + 1, i)]).max())
            assert err < BOUND, (name, s, i, err)
    st = opt.state[ps[2]]
    assert set(st) == {"step", "exp_avg", "exp_avg_sq", "weight_norm", "adam_norm", "trust_ratio"}
    assert st["trust_ratio"].is_cuda and st["trust_ratio"].dim() == 0 and float(st["step"]) == 5


def test_bad_arguments_raise():
    p = torch.zeros(8, device=DEV)
    with pytest.raises(GcmiError):
        ops.opt_step_(ops.opt_desc(7), p, p, p, p, LR, 1)            # no such rule
    with pytest.raises(GcmiError):
        ops.opt_step_(ops.opt_desc("lamb"), p, p, p, p, LR, 1)       # Lamb is not elementwise
    with pytest.raises(GcmiError):
        ops.opt_step_(ops.opt_desc("adamw", beta1=0.9, beta2=0.999), p, p, p, p, LR, 0)   # step 0
    with pytest.raises(GcmiError):
        ops.opt_step_(ops.opt_desc("adamw", beta1=0.9, beta2=0.999), p, p, None, None, LR, 1)  # missing state
    with pytest.raises(GcmiError):
        ops.opt_step_(ops.opt_desc("adamw", beta1=1.5, beta2=0.999), p, p, p, p, LR, 1)   # beta outside [0, 1)
    with pytest.raises(ValueError):
        ops.opt_step_(ops.opt_desc("sgd"), p, p.cpu(), None, None, LR, 1)
    segs = torch.tensor([[0, 8]], dtype=torch.int64, device=DEV)
    with pytest.raises(ValueError):
        ops.lamb_step_(ops.opt_desc("lamb", beta1=0.9, beta2=0.999), p, p, p, p, torch.empty(4, device=DEV), segs, None, LR)
    with pytest.raises(GcmiError):
        ops.lamb_step_(ops.opt_desc("adamw", beta1=0.9, beta2=0.999), p, p, p, p,
                       torch.empty(ops.lamb_scratch_floats(8, 1), device=DEV), segs, None, LR)
    # a segment that does not lie inside the arena is skipped, not followed
    q, m, v = torch.ones(8, device=DEV), torch.zeros(8, device=DEV), torch.zeros(8, device=DEV)
    wild = torch.tensor([[4, 100], [-3, 2], [0, 4]], dtype=torch.int64, device=DEV)
    ops.lamb_step_(ops.opt_desc("lamb", beta1=0.9, beta2=0.999, eps=1e-8), q, torch.ones(8, device=DEV), m, v,
                   torch.empty(ops.lamb_scratch_floats(8, 3), device=DEV), wild, None, LR)
    assert float(q[4:].min()) == 1.0 and float(q[:4].max()) < 1.0
