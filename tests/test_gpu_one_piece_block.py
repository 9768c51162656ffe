"""The first GraphConv block on one-piece bf16 operands (small-integer atom features, fp32 storage, fast product mode:
csrc/model.hip one_piece_block0) against the split-fp32 kernels it replaces ON THE SAME INPUTS -- the batch is
collated twice, once with the property withdrawn.  The operands hold identical values and every product keeps its
fp32-level terms (the dropped operand pieces are zero), so the two differ in summation order only: the bound is the
one tests/test_gpu_fused_bwd.py uses for that, 2e-5 of a tensor's scale.  And against the oracle at the repository's
1e-4."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _one_piece_launches():
    from deepchem_amd import _lib
    v = ctypes.c_int32(0)
    _lib.call("gcmi_get_option", _lib.GCMI_OPT_ONE_PIECE_LAUNCHES, ctypes.byref(v))
    return v.value


def _integer_set(n_mols, seed=5):
    """The recipe of tests/test_gpu_fused_bwd.py -- ragged tiles, single atoms, degrees 0..6 and 10, molecules above
    the window cap of 96 atoms -- with small-integer features everywhere: 0 / 1 columns, and counts in [-3, 25] in a
    few columns (the edge-case set's own features are Gaussian)."""
    from deepchem_amd.utils.synthetic import (PackedMols, concat_packed, single_atom_and_edge_cases,
                                              synthetic_molecules)
    parts = [synthetic_molecules(n_mols, seed=seed, max_atoms=40), single_atom_and_edge_cases(75, seed=2)]
    if n_mols > 100:
        parts.append(synthetic_molecules(6, seed=3, mean_atoms=118, max_atoms=132, min_atoms=100))
    packed = concat_packed(parts)
    rng = np.random.RandomState(seed)
    f = (rng.random_sample(packed.atom_features.shape) < 0.12).astype(np.float32)
    f[:, 62] = rng.randint(-3, 4, f.shape[0])
    f[:, 63] = rng.randint(0, 26, f.shape[0])
    f[:, 7] = rng.randint(-25, 26, f.shape[0])
    deg = np.diff(packed.adj_ptr)
    assert deg.min() == 0 and deg.max() == 10 and 6 in deg
    return PackedMols(f, packed.atom_ptr, packed.adj_ptr, packed.adj_idx)


def _step(packed, y, w, tasks, grad_mode="full", promise=True, exact=False, state=None):
    """One training step (forward, loss, backward) of the whole-model entry points.  promise=False: the same collated
    batch with the small-integer property withdrawn -- the split-fp32 kernels."""
    import deepchem_amd as dc
    from deepchem_amd import _lib
    from deepchem_amd.data.collate import collate_to_device
    from deepchem_amd.metrics import to_one_hot
    n = packed.n_mols
    dbatch = collate_to_device(packed, None, DEV)
    g = dbatch.graph
    if not promise:
        g.note_small_int_features(None)
    labels = torch.as_tensor(to_one_hot(y.flatten(), 2).reshape(-1, tasks, 2).astype(np.float32), device=DEV)
    weights = torch.as_tensor(w.astype(np.float32), device=DEV)
    torch.manual_seed(11)
    model = dc.models.torch_models.GraphConvModel(tasks, graph_conv_layers=[64, 64], dense_layer_size=128,
                                                  number_input_features=[75, 64], batch_size=n, mode="classification",
                                                  grad_mode=grad_mode, device=DEV)
    if state is not None:
        model.model.load_state_dict({k: v.clone() for k, v in state.items()})
    native = model.model._native_net()
    assert native is not None
    g.set_mols(n)
    _lib.call("gcmi_set_option", _lib.GCMI_OPT_GEMM_EXACT, 1 if exact else 0)
    try:
        model.model.train()
        before = _one_piece_launches()
        logits, _, fp = native.forward(dbatch.atom_features, g, True, want_probs=False)
        loss = native.loss_backward(labels, weights, n)
        torch.cuda.synchronize()
        ran = _one_piece_launches() - before
    finally:
        _lib.call("gcmi_set_option", _lib.GCMI_OPT_GEMM_EXACT, 0)
    names = [k for k, _ in model.model.named_parameters()]
    return {"loss": float(loss), "grads": native.grad_flat.clone(), "slices": list(zip(names, native._slices)),
            "range": native.grad_range, "logits": logits.clone(), "fp": fp.clone(), "ran": ran,
            "bn": [(bn.running_mean.clone(), bn.running_var.clone(), int(bn.num_batches_tracked))
                   for bn in model.model.batch_norms],
            "dbatch": dbatch, "native": native}


def _compare_grads(a, b, tol):
    assert a["range"] == b["range"]
    lo, hi = a["range"]
    worst, checked = (0.0, None), 0
    for name, (off, n) in a["slices"]:
        if not (lo <= off and off + n <= hi):
            continue
        x = a["grads"][off:off + n].double().cpu().numpy()
        r = b["grads"][off:off + n].double().cpu().numpy()
        assert np.isfinite(x).all() and np.isfinite(r).all(), name
        err = np.abs(x - r).max() / max(np.abs(r).max(), 1e-6)
        if err > worst[0]:
            worst = (err, name)
        checked += 1
    print("worst relative gradient difference", worst, "over", checked, "tensors")
    assert worst[0] <= tol, worst
    return checked


@pytest.mark.parametrize("n_mols", [37, 1500])
def test_one_piece_block_equals_the_fp32_path(n_mols):
    from deepchem_amd.utils.synthetic import synthetic_labels
    packed = _integer_set(n_mols)
    tasks = 3
    y, w = synthetic_labels(packed.n_mols, tasks, "classification", 5, pos_rate=0.4)
    new = _step(packed, y, w, tasks, promise=True)
    old = _step(packed, y, w, tasks, promise=False)
    assert new["dbatch"].small_int_features and old["dbatch"].small_int_features  # what the collation found, both times
    # the one-piece forward product and the one-piece backward ran once each / not at all
    assert new["ran"] == 2 and old["ran"] == 0
    print("loss", new["loss"], old["loss"])
    assert abs(new["loss"] - old["loss"]) <= 2e-5 * max(abs(old["loss"]), 1.0)
    d_logits = float((new["logits"] - old["logits"]).abs().max())
    d_fp = float((new["fp"] - old["fp"]).abs().max())
    print("logits", d_logits, "of", float(old["logits"].abs().max()), "| fingerprints", d_fp)
    assert d_logits <= 2e-5 * max(float(old["logits"].abs().max()), 1.0)
    assert d_fp <= 2e-5  # tanh outputs: scale 1
    assert _compare_grads(new, old, 2e-5) > 40  # every parameter of the model (full mode)
    for i, ((rm1, rv1, k1), (rm0, rv0, k0)) in enumerate(zip(new["bn"], old["bn"])):
        dm = float((rm1 - rm0).abs().max()) / max(float(rm0.abs().max()), 1e-3)
        dv = float((rv1 - rv0).abs().max()) / max(float(rv0.abs().max()), 1e-3)
        print("BatchNorm", i, "running mean", dm, "running var", dv)
        assert dm <= 2e-5 and dv <= 2e-5 and k1 == k0 == 1


def test_one_piece_operands_are_exact():
    """The bf16 S0 and Xb rows the window pass leaves in the workspace (csrc/model.hip carve: S[0] is the first block,
    N x 76 floats, the copy of the features follows it; both as rows of 80 bf16), widened, against the fp32 neighbour
    sums and the features themselves: integers below 256, so not one bit differs."""
    from deepchem_amd import ops
    from deepchem_amd.utils.synthetic import synthetic_labels
    packed = _integer_set(1500)
    y, w = synthetic_labels(packed.n_mols, 2, "classification", 5, pos_rate=0.4)
    r = _step(packed, y, w, 2, promise=True)
    assert r["ran"] == 2
    x = r["dbatch"].atom_features
    g = r["dbatch"].graph
    n = g.n_atoms
    assert x.shape[1] == 76
    ws = r["native"]._ws
    s0 = ws[:n * 40].view(torch.bfloat16).view(n, 80).float()
    xb = ws[n * 76:n * 76 + n * 40].view(torch.bfloat16).view(n, 80).float()
    s_ref = ops.gather_sum(g, x)
    assert float(s_ref.abs().max()) > 25  # sums really exceed a single feature's range
    assert torch.equal(xb[:, :76], x) and torch.equal(s0[:, :76], s_ref)
    assert not xb[:, 76:].any() and not s0[:, 76:].any()  # the pad columns the products read are zero
    # ... and the device-side checker agrees with the collation about this matrix
    from deepchem_amd import _lib
    count = torch.zeros(1, dtype=torch.int64, device=DEV)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.call("gcmi_count_not_small_int", x.data_ptr(), int(x.stride(0)), n, 76, 10, count.data_ptr(), stream)
    assert int(count.item()) == 0
    bad = x.clone()
    bad[3, 5], bad[n - 1, 75], bad[n // 2, 0], bad[7, 7] = 0.5, 26.0, float("nan"), float("inf")
    _lib.call("gcmi_count_not_small_int", bad.data_ptr(), int(bad.stride(0)), n, 76, 10, count.data_ptr(), stream)
    assert int(count.item()) == 4


def test_one_piece_block_is_not_taken_without_the_property_or_in_exact_mode():
    from deepchem_amd.utils.synthetic import PackedMols, synthetic_labels
    packed = _integer_set(300)
    y, w = synthetic_labels(packed.n_mols, 2, "classification", 5, pos_rate=0.4)
    # exact product mode: the current sequence, whatever the features are
    assert _step(packed, y, w, 2, promise=True, exact=True)["ran"] == 0
    # reference gradient mode: the forward product alone (nothing in front of a GraphConv output trains)
    assert _step(packed, y, w, 2, grad_mode="reference", promise=True)["ran"] == 1
    # one non-integer feature in the batch: the collation withdraws the property
    f = packed.atom_features.copy()
    f[f.shape[0] // 2, 9] = 0.5
    r = _step(PackedMols(f, packed.atom_ptr, packed.adj_ptr, packed.adj_idx), y, w, 2, promise=True)
    assert not r["dbatch"].small_int_features and r["ran"] == 0
    # the promise is tied to the collated matrix: a copy of it run over the same graph makes none
    r = _step(packed, y, w, 2, promise=True)
    g, native = r["dbatch"].graph, r["native"]
    before = _one_piece_launches()
    native.forward(r["dbatch"].atom_features.clone(), g, False, want_probs=False)
    torch.cuda.synchronize()
    assert _one_piece_launches() == before


def test_one_piece_block_against_the_oracle():
    """1e-4 of each tensor's scale against the torch-CPU oracle's autograd (`full` mode) from the same state on the same
    batch of small-integer features."""
    from oracle import graphconv_oracle as O
    from tests.util import oracle_batch, oracle_convmols
    from deepchem_amd.utils.synthetic import PackedMols, synthetic_labels, synthetic_molecules
    n, tasks = 200, 4
    base = synthetic_molecules(n, seed=21, max_atoms=35)
    rng = np.random.RandomState(21)
    f = np.array(base.atom_features, np.float32, copy=True)
    f[:, 62] = rng.randint(-3, 4, f.shape[0])
    f[:, 63] = rng.randint(0, 26, f.shape[0])
    packed = PackedMols(f, base.atom_ptr, base.adj_ptr, base.adj_idx)
    y, w = synthetic_labels(n, tasks, "classification", 21, pos_rate=0.4)
    cfg = O.ModelConfig(tasks, batch_size=n)
    state = O.init_state(cfg, 21)
    r = _step(packed, y, w, tasks, promise=True, state=state)
    assert r["ran"] == 2
    tr = O.OracleTrainer(cfg, state, grad_mode="full")
    inputs, labels, weights = oracle_batch(cfg, oracle_convmols(packed), y, w, np.arange(n), n, True)
    ref, _ = tr.loss(inputs, labels, weights)
    ref.backward()
    ref_grads = tr.grads()
    print("loss", r["loss"], float(ref))
    assert abs(r["loss"] - float(ref)) <= 1e-4 * max(abs(float(ref)), 1.0)
    checked, worst = 0, (0.0, None)
    for name, (off, cnt) in r["slices"]:
        if ref_grads.get(name) is None:
            continue
        a = r["grads"][off:off + cnt].cpu().numpy()
        b = np.asarray(ref_grads[name], np.float32).reshape(-1)
        scale = max(np.abs(b).max(), 1e-6)
        err = np.abs(a - b).max() / scale
        if err > worst[0]:
            worst = (err, name)
        assert np.abs(a - b).max() <= 1e-4 * scale + 1e-7, (name, np.abs(a - b).max(), scale)
        checked += 1
    print("worst relative gradient error against the oracle", worst)
    assert checked > 40
