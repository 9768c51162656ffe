"""Batches, oracle steps and the qualification rule for the per-step gradient tests of the small-batch engine
(tests/test_small_refs_host.py on the CPU, tests/test_gpu_small_grads.py on the device) and of the large-batch step
(tests/test_large_refs_host.py, tests/test_gpu_large_grads.py).  No test is collected here.

Why batches are qualified.  The gradient of this model is only piecewise smooth: a ReLU gate, a GraphPool route or a
GraphGather route flips when two numbers come within rounding of each other, and away from flips the backward amplifies
a relative input perturbation 10 to several hundred times.  On an arbitrary batch torch's own float32 run of the oracle
is, in one configuration in thirteen, further than 1e-4 of a tensor's scale from its float64 run (DESIGN section 43,
which has the figures).  A per-step gradient bound of 1e-4 can therefore only be asked on a batch on which, on the
CPU, (q1) the float32 oracle stays within a quarter of the bound of the float64 oracle, and (q2) input perturbations
at float32 rounding level move the float64 gradient by at most half the bound.  Both are conditions on the INPUTS;
neither looks at the code under test, and a seed is never chosen by what the GPU says."""
import collections
import contextlib
import functools

import numpy as np
import torch

from deepchem_amd.utils.synthetic import (PackedMols, concat_packed, single_atom_and_edge_cases, synthetic_labels,
                                          synthetic_molecules)
from oracle import graphconv_oracle as O
from oracle import mol_graphs_oracle as MO
from tests.yardstick import f32_threads

BOUND = 1e-4          # the project's per-tensor gradient bound (tests/test_gpu_fused_bwd.py holds the large step to it)
Q1_MAX = 2.5e-5       # float32 oracle against float64 oracle: a quarter of the bound
Q2_MAX = 5e-5         # float64 gradient under 2^-21 relative input perturbations: half the bound
Q2_MAG = 2.0 ** -21
Q2_DRAWS = 4
PAD = 5

# ---------------------------------------------------------------------------------------------- batches
_ATOM = [[]]
_PAIR = [[1], [0]]
_RING4 = [[1, 3], [0, 2], [1, 3], [2, 0]]


def _star(leaves):
    return [list(range(1, leaves + 1))] + [[0] for _ in range(leaves)]


SHAPED_KINDS = [("atom", _ATOM, 17), ("ring4", _RING4, 8), ("star3", _star(3), 11), ("star10", _star(10), 1),
                ("pair", _PAIR, 11)]
# rows per degree: 16-row tiles and 32-row slabs of the engine
SHAPED_HISTOGRAM = {0: 17, 1: 65, 2: 32, 3: 11, 4: 0, 5: 0, 6: 0, 7: 0, 8: 0, 9: 0, 10: 1}


def degree_histogram(packed):
    deg = np.diff(packed.adj_ptr)
    return {d: int((deg == d).sum()) for d in range(O.MAX_DEG + 1)}


def shaped_molecules(seed, pad=0):
    """48 molecules, 126 atoms, degree blocks on the engine's tile (16 rows) and slab (32 rows) edges:
    degree 0: 17 rows (a full tile + 1), degree 1: 65 (two slabs + 1, four tiles + 1), degree 2: 32 (one slab, two
    tiles), degree 3: 11 (a ragged tile), degrees 4..9 empty, degree 10: one row.  Molecule order shuffled by
    ``RandomState(seed)``.  ``pad``: the last ``pad`` molecules ARE the first ``pad`` (same graph, same features), the
    padded tail of a short last batch (``idx[np.arange(B) % n_real]``); the batch keeps the histogram because the
    shuffle is arranged so that each tail molecule is of the kind it repeats."""
    rng = np.random.RandomState(seed)
    kinds = [(name, adj) for name, adj, count in SHAPED_KINDS for _ in range(count)]
    order = [kinds[i] for i in rng.permutation(len(kinds))]
    n = len(order)
    if pad:
        assert 0 < pad <= 8
        for i in range(pad):  # the one star of degree 10 cannot be repeated without a second one
            if order[i][0] == "star10":
                j = next(k for k in range(pad, n - pad) if order[k][0] != "star10")
                order[i], order[j] = order[j], order[i]
        for i in range(pad):
            t = n - pad + i
            if order[t][0] != order[i][0]:
                j = next(k for k in range(pad, n - pad) if order[k][0] == order[i][0])
                order[t], order[j] = order[j], order[t]
    adjs = [adj for _, adj in order]
    sizes = np.array([len(a) for a in adjs], np.int64)
    atom_ptr = np.zeros(n + 1, np.int64)
    np.cumsum(sizes, out=atom_ptr[1:])
    deg = np.array([len(nb) for a in adjs for nb in a], np.int64)
    adj_ptr = np.zeros(deg.shape[0] + 1, np.int64)
    np.cumsum(deg, out=adj_ptr[1:])
    adj_idx = np.array([j for a in adjs for nb in a for j in nb], np.int32)
    A = int(atom_ptr[-1])
    feats = (rng.random_sample((A, 75)) < 0.1).astype(np.float32)
    for i in range(pad):
        t = n - pad + i
        feats[atom_ptr[t]:atom_ptr[t + 1]] = feats[atom_ptr[i]:atom_ptr[i + 1]]
    packed = PackedMols(feats, atom_ptr, adj_ptr, adj_idx)
    assert packed.n_mols == 48 and packed.n_atoms == 126
    assert degree_histogram(packed) == SHAPED_HISTOGRAM, degree_histogram(packed)
    return packed


_K4 = [[1, 2, 3], [0, 2, 3], [0, 1, 3], [0, 1, 2]]
TILED_KINDS = [("atom", _ATOM, 7), ("ring4", _RING4, 16), ("k4", _K4, 15), ("star3", _star(3), 3), ("star10", _star(10), 1),
               ("pair", _PAIR, 55)]
# rows per degree: the 64-row tiles (kFRows) and 128-row slabs (kS3Rows) of the large-batch step
TILED_HISTOGRAM = {0: 7, 1: 129, 2: 64, 3: 63, 4: 0, 5: 0, 6: 0, 7: 0, 8: 0, 9: 0, 10: 1}


def tiled_molecules(seed):
    """97 molecules (three head rounds of kHM = 32, plus one), 264 atoms, degree blocks on the tile edges of the
    large-batch step: degree 0: 7 rows, degree 1: 129 (a 128-row slab + 1, two 64-row tiles + 1), degree 2: 64 (exactly
    one tile), degree 3: 63 (a tile less one row), degrees 4..9 empty, degree 10: one row.  Molecule order shuffled by
    ``RandomState(seed)``; features as in ``shaped_molecules``: 0/1 at density 0.1, 75 columns."""
    rng = np.random.RandomState(seed)
    kinds = [adj for _, adj, count in TILED_KINDS for _ in range(count)]
    adjs = [kinds[i] for i in rng.permutation(len(kinds))]
    sizes = np.array([len(a) for a in adjs], np.int64)
    atom_ptr = np.zeros(len(adjs) + 1, np.int64)
    np.cumsum(sizes, out=atom_ptr[1:])
    deg = np.array([len(nb) for a in adjs for nb in a], np.int64)
    adj_ptr = np.zeros(deg.shape[0] + 1, np.int64)
    np.cumsum(deg, out=adj_ptr[1:])
    adj_idx = np.array([j for a in adjs for nb in a for j in nb], np.int32)
    feats = (rng.random_sample((int(atom_ptr[-1]), 75)) < 0.1).astype(np.float32)
    packed = PackedMols(feats, atom_ptr, adj_ptr, adj_idx)
    assert packed.n_mols == 97 and packed.n_atoms == 264
    assert degree_histogram(packed) == TILED_HISTOGRAM, degree_histogram(packed)
    return packed


def ordinary_molecules(seed):
    """34 molecules, about 500 atoms: 28 Tox21-like ones and the six edge cases; some degree blocks span many tiles."""
    return concat_packed([synthetic_molecules(28, seed=seed, max_atoms=40), single_atom_and_edge_cases(75, seed)])


# ---------------------------------------------------------------------------------------------- cases
Model = collections.namedtuple("Model", "mode T widths dense bn")
MODELS = {
    "A": Model("classification", 3, (64, 64), 128, True),        # the default; T C = 6 is not a multiple of 4
    "B": Model("regression", 2, (192, 256), 64, True),           # conv fwd <3,false> <4,true>; dense bwd <4>; readout <16>
    "C": Model("classification", 5, (256, 192), 128, True),      # conv fwd <4,false> <3,true>; dense bwd <3>
    "D": Model("regression", 1, (128, 128), 256, True),          # two-tile forms; readout <64>; pool+dense <4>; T C = 1
    "E": Model("classification", 12, (64, 128, 64, 64), 64, False),  # four layers, no BatchNorm, 24 head blocks
    "F": Model("classification", 1, (256,), 256, True),          # one layer: no pool-in conv
    # large-batch step only (LARGE_NEW): the dense block and GraphConv 1 run as separate launches, GraphConv 0 in one
    # pass below them, with BatchNorm -- the one order in which a stale `have_psums` of the walk would be consumed
    "G": Model("classification", 3, (64, 128), 128, True),
}
GRAD_MODES = ("full", "reference")
KINDS = ("shaped", "padded", "ordinary")

# (model, batch kind, seed, gradient modes).  One seed drives molecules, labels and the initial state.  Every entry met
# q1 and q2 on the CPU (tests/test_small_refs_host.py re-checks all of them); they were found by scanning seeds upward
# on the CPU, before any device run.
Case = collections.namedtuple("Case", "model kind seed modes")


def case_id(case, grad_mode):
    return "%s-%s-seed%d-%s" % (case.model, case.kind, case.seed, grad_mode)


def model_cfg(model_id, batch_size):
    m = MODELS[model_id]
    return O.ModelConfig(m.T, graph_conv_layers=m.widths, number_input_features=(75,) + tuple(m.widths[:-1]),
                         dense_layer_size=m.dense, mode=m.mode, batch_normalize=m.bn, batch_size=batch_size)


@functools.lru_cache(maxsize=None)
def batch_of(kind, seed):
    """(packed, n_real): the molecules of one batch in batch order and how many of them are real."""
    if kind == "shaped":
        p = shaped_molecules(seed)
        return p, p.n_mols
    if kind == "padded":
        p = shaped_molecules(seed, pad=PAD)
        return p, p.n_mols - PAD
    if kind == "tiled":
        p = tiled_molecules(seed)
        return p, p.n_mols
    assert kind == "ordinary"
    p = ordinary_molecules(seed)
    return p, p.n_mols


@functools.lru_cache(maxsize=None)
def case_inputs(model_id, kind, seed):
    """packed, y, w (float64, whole batch), cfg, state, n_real.  Rows from n_real on repeat the first rows; their weights
    are zeroed where the batch is formed (``oracle_step`` / the device batches), as pad_batch does."""
    if kind.startswith("width"):
        assert model_id == "A"
        return width_inputs(int(kind[len("width"):]), seed)
    m = MODELS[model_id]
    packed, n_real = batch_of(kind, seed)
    n = packed.n_mols
    y, w = synthetic_labels(n, m.T, m.mode, seed, pos_rate=0.4)
    if n_real < n:
        y[n_real:] = y[:n - n_real]
    cfg = model_cfg(model_id, n)
    state = O.init_state(cfg, seed)
    return packed, y, w, cfg, state, n_real


WIDTHS = (33, 64, 65, 96, 97)  # layer-0 input columns on the K-chunk edges of the large step's one-pass backward


def width_inputs(k, seed):
    """``case_inputs`` of model A at ``k`` input columns: the topology of ``shaped_molecules(seed)``, features
    continuous (uniform in [-1, 1]) so that a column dropped, swapped or read from the padding moves the result."""
    t = shaped_molecules(seed)
    feats = np.random.RandomState(7000 + 100 * seed + k).uniform(-1, 1, (t.n_atoms, k)).astype(np.float32)
    packed = PackedMols(feats, t.atom_ptr, t.adj_ptr, t.adj_idx)
    m = MODELS["A"]
    n = packed.n_mols
    y, w = synthetic_labels(n, m.T, m.mode, seed, pos_rate=0.4)
    cfg = O.ModelConfig(m.T, graph_conv_layers=m.widths, number_input_features=(k,) + tuple(m.widths[:-1]),
                        dense_layer_size=m.dense, mode=m.mode, batch_normalize=m.bn, batch_size=n)
    return packed, y, w, cfg, O.init_state(cfg, seed), n


# ---------------------------------------------------------------------------------------------- the oracle
def _convmols(packed):
    return [MO.conv_mol(*packed.molecule(m)) for m in range(packed.n_mols)]


def oracle_inputs(packed, y, w, cfg, n_real, double=False, predict=False):
    """The whole of ``packed`` as ONE batch of the oracle (tests/util.py::oracle_batch), weights zero from ``n_real``
    on.  ``double``: features, labels and weights in float64 (features that already are float64 are not rounded)."""
    n = packed.n_mols
    multi = MO.agglomerate(_convmols(packed))
    w_b = None
    if w is not None:
        w_b = w.copy()
        w_b[n_real:] = 0
    inputs, labels, weights = O.batch_tensors(multi, n, y, w_b, cfg, predict=predict)
    if double:
        inputs = [torch.as_tensor(np.asarray(multi["atom_features"], np.float64))] + list(inputs[1:])
        labels = None if labels is None else labels.double()
        weights = None if weights is None else weights.double()
    return inputs, labels, weights


def _double_state(state):
    return {k: (v.double() if v.is_floating_point() else v) for k, v in state.items()}


def oracle_step(packed, y, w, cfg, state, grad_mode, n_real, double=False):
    """One training-mode forward + loss + backward of the oracle (``faithful=False``: values and gradients equal to the
    faithful loop bit for bit, tests/test_oracle_golden.py).  ``double``: the same op sequence in float64 (the
    yardstick).  Returns the loss, the outputs, the gradients by parameter name (None where none arrives) and the
    trainer, whose state holds the running statistics after this step."""
    inputs, labels, weights = oracle_inputs(packed, y, w, cfg, n_real, double)
    if double:
        state = _double_state(state)
    tr = O.OracleTrainer(cfg, state, grad_mode=grad_mode, faithful=False)
    with (O.precision(torch.float64) if double else contextlib.nullcontext()):
        ref, outs = tr.loss(inputs, labels, weights)
        ref.backward()
    return float(ref.detach()), [o.detach() for o in outs], tr.grads(), tr


def oracle_predict64(packed, cfg, state):
    """The eval-mode forward of the oracle in float64."""
    inputs, _, _ = oracle_inputs(packed, None, None, cfg, packed.n_mols, double=True, predict=True)
    tr = O.OracleTrainer(cfg, _double_state(state), grad_mode="reference", faithful=False)
    with O.precision(torch.float64):
        return tr.predict(inputs)


def tensor_distance(a, b):
    """max|a - b| in units of b's scale, max(max|b|, 1e-6)."""
    a, b = np.asarray(a, np.float64).reshape(-1), np.asarray(b, np.float64).reshape(-1)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-6)) if b.size else 0.0


def perturbed(packed, state, rng, mag):
    """Every atom feature and every floating-point state tensor (running statistics included) times 1 + mag u, u fresh
    and uniform in [-1, 1], in float64."""
    def jitter(x):
        x = np.asarray(x, np.float64)
        return x * (1.0 + mag * rng.uniform(-1.0, 1.0, size=x.shape))
    p = PackedMols(jitter(packed.atom_features), packed.atom_ptr, packed.adj_ptr, packed.adj_idx)
    st = {k: (torch.from_numpy(jitter(v.numpy())).reshape(v.shape) if v.is_floating_point() else v.clone())
          for k, v in state.items()}
    return p, st


Reference = collections.namedtuple("Reference", "loss outs grads state")

# The float32 yardstick is torch's float32 arithmetic AT A FIXED THREAD COUNT.  The order of torch's float32 reductions
# (BatchNorm sums over the atom rows, products) follows the number of threads: with one thread the sums are sequential,
# the forward is about five times further from float64 (fingerprint 5e-5 against 1e-5 on the 500-atom batches), and a
# GraphGather route whose two candidates lie 3e-6 apart goes the other way; from two threads up it does not.  q1 is a
# statement about the batch, so it is taken under one arithmetic wherever the file runs.
F32_THREADS = 8




def _reference(step):
    loss, outs, grads, tr = step
    return Reference(loss, outs, grads, {k: v.detach().clone() for k, v in tr.state.items()})


@functools.lru_cache(maxsize=None)
def references(model_id, kind, seed, grad_mode):
    """(float64, float32) oracle steps of one case; computed once per process, shared, never modified."""
    packed, y, w, cfg, state, n_real = case_inputs(model_id, kind, seed)
    r64 = _reference(oracle_step(packed, y, w, cfg, state, grad_mode, n_real, double=True))
    with f32_threads(F32_THREADS):
        r32 = _reference(oracle_step(packed, y, w, cfg, state, grad_mode, n_real, double=False))
    return r64, r32


def worst_distance(got, want):
    """The largest tensor_distance over the tensors that have a gradient in ``want`` (and the tensor's name)."""
    worst, name = 0.0, None
    for k, b in want.items():
        if b is None:
            assert got[k] is None, k
            continue
        d = tensor_distance(got[k], b)
        if d >= worst:
            worst, name = d, k
    return worst, name


def qualify_inputs(packed, y, w, cfg, state, n_real, grad_mode, draw_seed=0, refs=None):
    """The rule itself, on any batch and model: (q1, q2) of one step.  q1: the worst tensor_distance of the float32
    oracle's gradient from the float64 oracle's.  q2: the worst tensor_distance, over ``Q2_DRAWS`` draws of
    ``perturbed(mag=2^-21)`` from ``RandomState(1000 + draw_seed)``, of the perturbed float64 gradient from the
    unperturbed one.  ``refs``: the (float64, float32) oracle steps where the caller already has them."""
    if refs is None:
        r64 = _reference(oracle_step(packed, y, w, cfg, state, grad_mode, n_real, double=True))
        with f32_threads(F32_THREADS):
            r32 = _reference(oracle_step(packed, y, w, cfg, state, grad_mode, n_real, double=False))
    else:
        r64, r32 = refs
    q1 = worst_distance(r32.grads, r64.grads)[0]
    rng = np.random.RandomState(1000 + draw_seed)
    q2 = 0.0
    for _ in range(Q2_DRAWS):
        p, st = perturbed(packed, state, rng, Q2_MAG)
        g = oracle_step(p, y, w, cfg, st, grad_mode, n_real, double=True)[2]
        q2 = max(q2, worst_distance(g, r64.grads)[0])
    return q1, q2


def qualify(model_id, kind, seed, grad_mode):
    """(q1, q2) of one case and gradient mode: ``qualify_inputs`` on ``case_inputs``, the perturbations drawn from
    ``RandomState(1000 + seed)``."""
    return qualify_inputs(*case_inputs(model_id, kind, seed), grad_mode, draw_seed=seed,
                          refs=references(model_id, kind, seed, grad_mode))


def qualifies(q1, q2):
    return q1 <= Q1_MAX and q2 <= Q2_MAX


CASES = [
    Case("A", "shaped", 5, GRAD_MODES),
    Case("B", "shaped", 5, GRAD_MODES),
    Case("C", "shaped", 5, GRAD_MODES),
    Case("D", "shaped", 5, GRAD_MODES),
    Case("E", "shaped", 10, GRAD_MODES),
    Case("F", "shaped", 5, GRAD_MODES),
    Case("A", "padded", 2, GRAD_MODES),
    Case("B", "padded", 10, GRAD_MODES),
    Case("A", "ordinary", 5, GRAD_MODES),
    Case("B", "ordinary", 7, GRAD_MODES),
    Case("C", "ordinary", 6, GRAD_MODES),
    # the sequence test runs one model on all three batch kinds from ONE state, so one seed has to qualify on all three:
    # 64 is the first such seed of model A (about one seed in three qualifies per kind), 7 qualifies for model B
    Case("A", "ordinary", 64, GRAD_MODES),
    Case("A", "shaped", 64, GRAD_MODES),
    Case("A", "padded", 64, GRAD_MODES),
    Case("B", "shaped", 7, GRAD_MODES),
    Case("B", "padded", 7, GRAD_MODES),
]
# what the one-step device test runs: the first case listed of each (model, kind)
ONE_STEP = [next(c for c in CASES if (c.model, c.kind) == mk) for mk in
            [(m, "shaped") for m in "ABCDEF"] + [("A", "padded"), ("B", "padded")] +
            [("A", "ordinary"), ("B", "ordinary"), ("C", "ordinary")]]
SEQUENCE = {"A": 64, "B": 7}   # model -> the seed whose three batch kinds all qualify
SEQUENCE_KINDS = ("ordinary", "shaped", "padded")

# What the per-route gradient tests of the large-batch step run (tests/test_gpu_large_grads.py):
# every one-step case above, the tiled batch on the default model, on the four-layer one without BatchNorm and on model
# G, and the five layer-0 widths.  The seed of each new entry is the first of 1, 2, ... that met q1 and q2 in both gradient modes
# on the CPU (tests/test_large_refs_host.py re-checks them).
LARGE_NEW = [
    Case("A", "tiled", 2, GRAD_MODES),
    Case("E", "tiled", 3, GRAD_MODES),
    Case("G", "tiled", 1, GRAD_MODES),
    Case("A", "width33", 1, GRAD_MODES),
    Case("A", "width64", 2, GRAD_MODES),
    Case("A", "width65", 4, GRAD_MODES),
    Case("A", "width96", 2, GRAD_MODES),
    Case("A", "width97", 1, GRAD_MODES),
]
LARGE_CASES = list(ONE_STEP) + LARGE_NEW
