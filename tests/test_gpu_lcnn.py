"""csrc/lcnn.hip and the native route of LCNNBlock / LCNNModel on the GPU against float64.

The accuracy bar is the project's (tests/test_gpu_mat.py): the error against the float64 restatement is at most 4 times
the float32 restatement's, with a floor of one float32 ulp of the tensor's largest entry.  Here ``e32`` is the LARGEST
error among three float32 restatements that differ in summation order alone (concatenated, split, split with the slots
reversed): a BatchNorm over P rows multiplies the rounding of X by up to 1 / sqrt(eps) = 316 wherever a site's
permutations nearly coincide, how much of that shows depends on the order, and one sample with a margin of 4 would be a
coin toss.  The gradient of the convolution bias in training mode is exactly zero in exact arithmetic (a site's centred rows
sum to zero); it goes through the same bar, where both sides are rounding alone.

Every case below was run on the CPU first: the three restatements' errors (output, dx, dW, dgamma, dbeta, the running
statistics) lie within 4 times of each other; below, per case, the largest ratio between two of them over those tensors
(cases further apart than 4 were given another seed, ``RESEED``):
* training / eval: 1x1 3.8 / 4.0; 2x2 2.2 / 3.6; 3x3 3.3 / 3.6; 5x5 2.2 / 2.9; 7x9 2.2 / 4.0; mixed 2.8 / 3.3; hub 2.5 / 1.5;
  lonely 2.6 / 2.2; rows12 1.0 / 2.5; rows13 1.0 / 1.4; rows14 1.0 / 2.2; O1 1.0 / 1.1; O19 2.7 / 2.8; O32 2.5 / 2.5;
  O33 1.1 / 1.9; O44 2.1 / 2.5; O51 1.9 / 2.0; O52 2.4 / 2.6; O64 2.2 / 3.2
* special masks (all sites / the kept site's cotangent alone): 3x3 3.6 / 2.6; mixed 2.8 / 2.8; O44 1.8 / 2.4
* three steps: 5x5 2.2; mixed 3.3; O44 2.1
At their first seeds 2x2 (52.8 in training), 7x9 (8.5 in eval), lonely (8.5), O51 (9.9) and O52 (5.7) lay further apart.
"""
import numpy as np
import pytest
import torch

from deepchem_amd import ops
from deepchem_amd.models.torch_models import LCNNBlock, LcnnBatch
from tests import lcnn_refs as R
from tests.yardstick import f32_threads

DEV = "cuda"
ORDERS = ("concat", "split", "split_rev")
NAMES = ("out", "dx", "dW", "db", "dgamma", "dbeta", "rm", "rv")

# name -> (graphs builder, P, K, F, O, seed)
TORI = {"1x1": (1, 1), "2x2": (2, 2), "3x3": (3, 3), "5x5": (5, 5), "7x9": (7, 9)}
MIXED = ((1, 1), (3, 3), (1, 1), (2, 2), (5, 5), (1, 1))
SHAPES = {"O1": (1, 1, 1, 2), "O19": (19, 3, 19, 6), "O32": (32, 44, 32, 8), "O33": (33, 3, 1, 8), "O44": (44, 44, 19, 6),
          "O51": (51, 1, 32, 2), "O52": (52, 3, 19, 2), "O64": (64, 44, 32, 8)}  # (O, F, K, P); 256 // O steps at 33, 43, 52


def build(name):
    """(graphs, P, K, F, O, seed) of a case."""
    if name in TORI:
        seed = {"1x1": 1, "2x2": 2, "3x3": 3, "5x5": 5, "7x9": 7}[name]
        rng = np.random.RandomState(seed)
        return [R.torus(rng, *TORI[name], 3, 6, 19, lambda r, n, f: r.normal(0, 1, (n, f)))], 6, 19, 3, 19, seed
    if name == "mixed":
        rng = np.random.RandomState(11)
        return [R.torus(rng, a, b, 3, 6, 19, lambda r, n, f: r.normal(0, 1, (n, f))) for a, b in MIXED], 6, 19, 3, 19, 11
    if name == "hub":
        rng = np.random.RandomState(12)
        return [R.hub_sites(rng, 129, 6, 3, 3)], 6, 3, 3, 8, 12
    if name == "lonely":
        rng = np.random.RandomState(13)
        return [R.random_sites(rng, 9, 6, 3, 3, lonely=True)], 6, 3, 3, 8, 13
    if name.startswith("rows"):  # 256 // 19 = 13 sites per workgroup
        n = int(name[4:])
        rng = np.random.RandomState(n)
        return [R.random_sites(rng, n, 2, 1, 1)], 2, 1, 1, 19, n
    o, f, k, p = SHAPES[name]
    rng = np.random.RandomState(o)
    return [R.random_sites(rng, 20, p, k, f)], p, k, f, o, o


# cases whose three restatements lay more than 4 times apart at the first seed: the seed of their parameters moved on
RESEED = {'2x2': 2000, '7x9': 1000, 'lonely': 2000, 'O51': 2000, 'O52': 6000}
CASES = list(TORI) + ["mixed", "hub", "lonely", "rows12", "rows13", "rows14"] + list(SHAPES)


def make_inputs(name, training, mask_kind="random"):
    graphs, P, K, F, O, seed = build(name)
    x, nbr, ptr = R.pack(graphs, P, K)
    rng = np.random.RandomState(100 + seed + RESEED.get(name, 0))
    N = x.shape[0]
    c = dict(P=P, K=K, F=F, O=O, N=N, graphs=graphs, nbr=nbr, x=x.astype(np.float32), training=training,
             W=rng.normal(0, 1 / np.sqrt(K * F), (O, K * F)).astype(np.float32), b=rng.normal(0, 0.3, O).astype(np.float32),
             gamma=rng.uniform(0.5, 1.5, O).astype(np.float32), beta=rng.normal(0, 0.3, O).astype(np.float32),
             rm=rng.normal(0, 0.3, O).astype(np.float32), rv=rng.uniform(0.5, 2, O).astype(np.float32),
             cot=rng.normal(0, 1, (N, O)).astype(np.float32))
    mask = (rng.rand(N, P) >= 0.2).astype(np.float32) / 0.8 if training else np.ones((N, P), np.float32)
    if mask_kind == "special":  # site 0 keeps all rows, site 1 drops all
        mask[0], mask[1 % N] = 1.25, 0.0
    c["mask"] = mask
    return c


def restate(c, dtype, order, steps=1):
    t = {k: torch.tensor(c[k], dtype=dtype, requires_grad=True) for k in ("x", "W", "b", "gamma", "beta")}
    st = R.BNState(0, dtype, c["rm"], c["rv"])
    for _ in range(steps):
        out = R.block(t["x"], c["nbr"], t["W"], t["b"], t["gamma"], t["beta"], c["mask"], st, c["training"], order)
    g = torch.autograd.grad((out * torch.tensor(c["cot"], dtype=dtype)).sum(), list(t.values()), allow_unused=True)
    g = [torch.zeros_like(v) if gi is None else gi for gi, v in zip(g, t.values())]
    vals = [out.detach()] + g + [st.mean, st.var]
    return {n: v.numpy().astype(np.float64) for n, v in zip(NAMES, vals)}, st.tracked


def references(c, steps=1):
    """(float64 values by name, e32 by name: the largest error of the three float32 restatements, their spread)."""
    want, tracked = restate(c, torch.float64, "concat", steps)
    errs = {n: [] for n in NAMES}
    for order in ORDERS:
        with f32_threads(1):  # (the O = 64 case is repeatable at one thread only)
            got, _ = restate(c, torch.float32, order, steps)
        for n in NAMES:
            errs[n].append(float(np.max(np.abs(got[n] - want[n]))))
    spread = max(max(e) / max(min(e), 1e-300) for n, e in errs.items() if max(e) > 0)
    return want, {n: max(e) for n, e in errs.items()}, spread, tracked


def bar(got, want64, e32, name):
    """The accuracy bar of the module docstring; returns the ratio error / e32 (0 below the floor)."""
    want64 = np.asarray(want64, np.float64)
    e = float(np.max(np.abs(np.asarray(got, np.float64) - want64)))
    floor = float(np.spacing(np.float32(np.max(np.abs(want64)))))
    ratio = e / max(e32, 1e-300)
    print("%s: error %.3g, fp32 restatements %.3g, ratio %.2f, floor %.3g" % (name, e, e32, ratio, floor))
    assert np.all(np.isfinite(np.asarray(got))), name
    assert e <= max(4 * e32, floor), (name, e, e32, floor)
    return ratio if e > floor else 0.0


def native(c, steps=1, route="auto"):
    layer = LCNNBlock(c["K"] * c["F"], c["O"], c["P"]).to(DEV).train(c["training"])
    layer.route = route
    bn = layer.batch_norm
    with torch.no_grad():
        for p, k in ((layer.conv_weights.weight, "W"), (layer.conv_weights.bias, "b"), (bn.weight, "gamma"), (bn.bias, "beta"),
                     (bn.running_mean, "rm"), (bn.running_var, "rv")):
            p.copy_(torch.as_tensor(c[k]))
    b = LcnnBatch(c["graphs"], DEV, c["P"], c["K"])
    x = b.x.clone().requires_grad_(True)
    mask = torch.as_tensor(c["mask"], device=DEV)
    for _ in range(steps):
        out = layer(b.sites, x, mask)
    (out * torch.as_tensor(c["cot"], device=DEV)).sum().backward()
    vals = [out.detach(), x.grad, layer.conv_weights.weight.grad, layer.conv_weights.bias.grad, bn.weight.grad, bn.bias.grad,
            bn.running_mean, bn.running_var]
    return {n: v.detach().cpu().numpy() for n, v in zip(NAMES, vals)}, int(bn.num_batches_tracked), layer


@pytest.mark.gpu
@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("name", CASES)
def test_native_block_against_float64(name, training):
    c = make_inputs(name, training)
    want, e32, spread, tracked = references(c)
    got, got_tracked, layer = native(c)
    assert layer.last_route == "native" and layer.last_reason is None
    worst = max(bar(got[n], want[n], e32[n], "%s %s" % (name, n)) for n in NAMES)
    print("%s %s: worst ratio %.2f, restatement spread %.2f" % (name, "train" if training else "eval", worst, spread))
    assert got_tracked == tracked == (c["N"] if training else 0)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["3x3", "mixed", "O44"])
def test_special_masks(name):
    """A site that keeps all P rows outputs P * beta and gives the weights no gradient; a site that drops all rows
    outputs a zero row and gives nothing any gradient, exactly."""
    c = make_inputs(name, True, "special")
    keep_cot, drop_cot = np.zeros_like(c["cot"]), np.zeros_like(c["cot"])
    keep_cot[0], drop_cot[1] = c["cot"][0], c["cot"][1]
    want, e32, _, _ = references(c)
    got, _, _ = native(c)
    for n in NAMES:
        bar(got[n], want[n], e32[n], "%s %s" % (name, n))
    bar(got["out"][0], c["P"] * 1.25 * c["beta"].astype(np.float64), e32["out"], "site 0 = P * beta / (1 - p)")
    assert np.all(got["out"][1] == 0)
    c["cot"] = keep_cot
    want, e32, _, _ = references(c)
    got, _, _ = native(c)
    assert float(np.max(np.abs(want["dW"]))) < 1e-12  # the float64 weight gradient from that site alone: zero
    for n in ("dW", "dx", "db", "dgamma", "dbeta"):
        bar(got[n], want[n], e32[n], "%s kept site only, %s" % (name, n))
    c["cot"] = drop_cot
    got, _, _ = native(c)
    for n in ("dW", "dx", "db", "dgamma", "dbeta"):
        assert np.all(got[n] == 0), n


@pytest.mark.gpu
def test_reverse_lists_long_and_empty():
    """lc_rev_sum alone: the hub's list of 129 * P rows, and a node that is nobody's neighbour (exact zero rows)."""
    for name, O in (("hub", 19), ("lonely", 44)):
        graphs, P, K, F, _, seed = build(name)
        b = LcnnBatch(graphs, DEV, P, K)
        N = b.sites.n_sites
        rng = np.random.RandomState(seed)
        dx = rng.normal(0, 1, (N, P, O)).astype(np.float32)
        dy = ops.lc_rev_sum(b.sites, torch.as_tensor(dx, device=DEV)).cpu().numpy().reshape(N, K, O)
        nbr = b.sites.nbr.cpu().numpy().reshape(N, P, K)
        want, f32 = np.zeros((N, K, O)), np.zeros((N, K, O), np.float32)
        for j in range(K):
            np.add.at(want[:, j], nbr[:, :, j].reshape(-1), dx.reshape(N * P, O).astype(np.float64))
            np.add.at(f32[:, j], nbr[:, :, j].reshape(-1), dx.reshape(N * P, O))
        bar(dy, want, float(np.max(np.abs(f32 - want))), name + " dY")
        if name == "lonely":
            assert not np.any(nbr == N - 1) and np.all(dy[N - 1] == 0)
        else:
            assert np.diff(b.sites.rev_ptr.cpu().numpy())[0] == N * P


@pytest.mark.gpu
def test_running_statistics_after_three_steps():
    for name in ("5x5", "mixed", "O44"):
        c = make_inputs(name, True)
        want, e32, _, tracked = references(c, steps=3)
        got, got_tracked, _ = native(c, steps=3)
        assert got_tracked == tracked == 3 * c["N"]
        for n in ("rm", "rv", "out"):
            bar(got[n], want[n], e32[n], "%s after three steps, %s" % (name, n))


@pytest.mark.gpu
def test_two_runs_agree_bit_for_bit():
    for name in ("7x9", "hub", "O64"):
        c = make_inputs(name, True)
        a, _, _ = native(c)
        b, _, _ = native(c)
        for n in NAMES:
            assert np.array_equal(a[n], b[n]), (name, n)


@pytest.mark.gpu
def test_last_route_for_each_fallback_reason():
    c = make_inputs("3x3", True)
    got, _, layer = native(c, route="torch")
    assert layer.last_route == "torch" and layer.last_reason == "route='torch'"
    want, e32, _, _ = references(c)
    for n in NAMES:  # the torch route on the GPU computes the same thing
        bar(got[n], want[n], e32[n], "torch route " + n)
    rng = np.random.RandomState(0)
    for P, K, O, dtype, dev, reason in ((6, 3, 65, torch.float32, DEV, "shape outside"), (9, 3, 8, torch.float32, DEV, "shape outside"),
                                         (6, 33, 8, torch.float32, DEV, "shape outside"), (6, 3, 8, torch.float64, DEV, "not float32"),
                                         (6, 3, 8, torch.float32, "cpu", "not on the GPU")):
        b = LcnnBatch([R.random_sites(rng, 7, P, K, 2)], dev, P, K)
        layer = LCNNBlock(K * 2, O, P).to(device=dev, dtype=dtype)
        out = layer(b.sites, b.x.to(dtype))
        assert layer.last_route == "torch" and layer.last_reason.startswith(reason) and out.shape == (7, O)
    b = LcnnBatch([R.random_sites(rng, 7, 6, 3, 2)], DEV, 6, 3)
    layer = LCNNBlock(6, 8, 6).to(DEV)
    layer.batch_norm.momentum = 0.01
    layer(b.sites, b.x)
    assert layer.last_route == "torch" and "momentum" in layer.last_reason
    layer.batch_norm.momentum = 0.1
    layer(b.sites, b.x)
    assert layer.last_route == "native"


# ------------------------------------------------------------------------------------------------ reference fixtures
@pytest.mark.gpu
def test_native_layer_and_model_against_the_reference_fixtures():
    from tests import test_lcnn_host as H
    for case in range(int(H.LAYERS["n_cases"])):
        c = H.layer_case(case)
        layer = H.make_block(c, training=bool(c["training"])).to(DEV)
        b = H.sites_of(c, DEV)
        x = b.x.clone().requires_grad_(True)
        out = layer(b.sites, x, torch.as_tensor(c["mask"], device=DEV))
        assert layer.last_route == "native"
        (out * torch.as_tensor(c["cot"], device=DEV)).sum().backward()
        grads = {"x": x.grad.cpu()}
        grads.update({k: v.grad.cpu() for k, v in layer.named_parameters() if k in H.PARAMS})
        bn = layer.batch_norm
        H.check_against_fixture(c, out.detach().cpu(), grads, bn.running_mean.cpu(), bn.running_var.cpu(), bn.num_batches_tracked,
                                "native %d" % case)
    ds, model = H.fixture_dataset(), H.fixture_model(torch.device(DEV))
    H.check_first_batch(model, ds)
    assert model.last_route == "native"
    worst64 = H.check_fit(model, ds, bar64=True)
    print("fit: worst distance to the float64 losses, in units of the bound: %.2f" % worst64)
