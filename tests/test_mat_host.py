"""MAT without a GPU: the float32 restatement (tests/mat_refs.py) against the reference's recorded outputs, gradients
and fit trajectory (tests/golden/mat_model.npz, tools/gen_golden_mat.py), the state dict with its shared modules, the
batch generator and the pad-free batch against the reference's padded arrays, and the SMILES featurizer against
hand-derived expectations.

Bar of the restatement: 1e-4 of each tensor's largest entry (mat_refs.rel_err), as tests/test_dmpnn_host.py.
"""
import os

import numpy as np
import pytest
import torch

import deepchem_amd as dc
from deepchem_amd import ops
from deepchem_amd.feat import MATEncoding, MATFeaturizer
from deepchem_amd.models.torch_models import MAT, MATModel, MatBatch, layers
from tests import mat_refs as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MODEL = np.load(os.path.join(GOLDEN, "mat_model.npz"))
KEYS = [str(k) for k in MODEL["keys"]]
TOL = 1e-4
WIDTH = dict(sa_hsize=32, d_input=32, d_hidden=32, d_output=32, encoder_hsize=32)
CPU = torch.device("cpu")


def state0():
    return {k: MODEL["param0_" + k] for k in KEYS}


def packed_batches(pad=True):
    ds = R.fixture_dataset(dc, MODEL)
    return [(R.pack(list(X_b)), y_b, w_b) for X_b, y_b, w_b, _ in ds.iterbatches(batch_size=8, deterministic=True,
                                                                                 pad_batches=pad)]


def test_fixture_molecules_are_the_recorded_ones():
    mols = R.fixture_molecules()
    assert [m.node_features.shape[0] for m in mols] == list(MODEL["n_atoms"]) == [n + 1 for n in R.FIXTURE_SIZES]
    assert all(np.abs(m.node_features).sum(1).min() > 0 for m in mols)


@pytest.mark.parametrize("kind", ["softmax", "exp"])
def test_float32_restatement_reproduces_the_reference(kind):
    pre = "" if kind == "softmax" else "exp_"
    batches = packed_batches()
    ref = R.MATRef(state0(), torch.float32, dist_kernel=kind, h=4)
    out = ref(batches[0][0])
    loss = R.l2_loss(out, batches[0][1], batches[0][2])
    loss.backward()
    errs = {"out0": R.rel_err(out.detach().numpy(), MODEL[pre + "out0"]),
            "loss0": abs(float(loss.detach()) - float(MODEL[pre + "loss0"])) / abs(float(MODEL[pre + "loss0"]))}
    for k, p in ref.table().items():
        errs["grad_" + k] = R.rel_err(p.grad.numpy(), MODEL[pre + "grad_" + k])
    print(kind, errs)
    assert len(errs) == 2 + 4 + 2 * 8 and max(errs.values()) <= TOL, errs


@pytest.mark.parametrize("kind", ["softmax", "exp"])
def test_float32_restatement_follows_the_reference_fit(kind):
    pre = "" if kind == "softmax" else "exp_"
    ref = R.MATRef(state0(), torch.float32, dist_kernel=kind, h=4)
    losses = R.fit(ref, packed_batches() * 2, 0.001)
    want = MODEL[pre + "fit_losses"]
    errs = np.abs(np.asarray(losses) - want) / np.abs(want)
    print(kind, "fit", errs)
    assert len(losses) == 6 and errs.max() <= TOL
    with torch.no_grad():
        pred = np.concatenate([ref(b[0]).numpy() for b in packed_batches(pad=False)])
    e = R.rel_err(pred, MODEL[pre + "predict"])
    print(kind, "predict", e)
    assert e <= TOL
    if kind == "softmax":
        for k, p in ref.table().items():
            assert R.rel_err(p.detach().numpy(), MODEL["final_" + k]) <= TOL, k


def test_padded_restatement_equals_the_pad_free_one():
    ref = R.MATRef(state0(), torch.float64, h=4)
    with torch.no_grad():
        a = ref(packed_batches()[0][0]).numpy()
        b = ref.padded_forward(MODEL["gen_node"], MODEL["gen_adj"], MODEL["gen_dist"]).numpy()
    assert R.rel_err(a, b) <= 1e-12


def test_state_dict_keys_aliases_and_loading():
    net = MAT(n_encoders=2, h=4, **WIDTH)
    sd = net.state_dict()
    assert list(sd) == KEYS and len(KEYS) == 2 * 14 + 4
    for k in KEYS:
        assert tuple(sd[k].shape) == MODEL["param0_" + k].shape, k
    for i in range(2):
        att, enc = net.encoder[i].self_attn, net.encoder[i]
        assert att.linear_layers[0] is att.linear_layers[1] is att.linear_layers[2]
        assert enc.sublayer[0] is enc.sublayer[1]
        pre = "encoder.%d." % i
        ptrs = {sd[pre + "self_attn.linear_layers.%d.weight" % j].data_ptr() for j in range(3)}
        assert len(ptrs) == 1
        assert sd[pre + "sublayer.0.norm.weight"].data_ptr() == sd[pre + "sublayer.1.norm.weight"].data_ptr()
    assert len(list(net.parameters())) == 4 + 2 * 8  # each shared parameter once
    net.load_state_dict({k: torch.as_tensor(v) for k, v in state0().items()})  # a reference-format dict loads
    assert np.array_equal(net.encoder[1].self_attn.linear_layers[2].weight.detach().numpy(),
                          MODEL["param0_encoder.1.self_attn.linear_layers.0.weight"])
    # the default model: the reference's 14 keys per encoder layer plus 4
    assert len(MAT().state_dict()) == 8 * 14 + 4
    for name in ("MATEmbedding", "MultiHeadedMATAttention", "MATEncoderLayer", "SublayerConnection", "MATGenerator",
                 "PositionwiseFeedForward"):
        assert hasattr(layers, name), name


def test_padded_forward_of_the_module_reproduces_the_reference_on_the_cpu():
    net = MAT(n_encoders=2, h=4, **WIDTH)
    net.load_state_dict({k: torch.as_tensor(v) for k, v in state0().items()})
    out = net([MODEL["gen_node"], MODEL["gen_adj"], MODEL["gen_dist"]])
    assert net.last_route == "torch"
    assert R.rel_err(out.detach().numpy(), MODEL["out0"]) <= TOL


def test_default_generator_and_matbatch_reproduce_the_padded_arrays():
    m = MATModel(n_encoders=2, h=4, batch_size=8, device=CPU, **WIDTH)
    ds = R.fixture_dataset(dc, MODEL)
    batches = list(m.default_generator(ds, deterministic=True))
    assert len(batches) == 3
    inputs, labels, weights = batches[0]
    for got, key in zip(inputs, ("gen_node", "gen_adj", "gen_dist")):
        assert got.shape == MODEL[key].shape and np.array_equal(got.astype(np.float32), MODEL[key]), key
    assert np.array_equal(labels[0], MODEL["y"][:8]) and np.array_equal(weights[0], MODEL["w"][:8])
    assert m.pad_array(np.ones((2, 2)), (3, 4)).tolist() == [[1, 1, 0, 0], [1, 1, 0, 0], [0, 0, 0, 0]]
    # the pad-free batch of the same molecules expands to exactly those arrays
    b = m.host_set(ds.X).batch(np.arange(8), CPU)
    assert m.host_set(ds.X) is m.host_set(ds.X)
    assert b.n_mols == 8 and not b.has_zero_atom and b.offs.n_max == 31
    for got, key in zip(b.to_padded(), ("gen_node", "gen_adj", "gen_dist")):
        assert np.array_equal(got.numpy(), MODEL[key]), key
    assert np.array_equal(b.pad_mask.numpy(), np.abs(MODEL["gen_node"]).sum(-1) != 0)
    assert np.array_equal(b.offs.atom_off, np.concatenate([[0], np.cumsum(MODEL["n_atoms"][:8])]))
    # the last, short batch is padded by the dataset; without a GPU the model walks the default generator
    assert [bt[0][0].shape[0] for bt in batches] == [8, 8, 8]
    assert isinstance(next(iter(m._batch_generator(ds)))[0], list)


def test_zero_feature_atom_and_large_molecule_are_flagged_for_the_torch_route():
    mols = R.fixture_molecules()[:3]
    bad = R.Encoding(mols[1].node_features.copy(), mols[1].adjacency_matrix, mols[1].distance_matrix)
    bad.node_features[2] = 0.0
    assert MatBatch.from_encodings(mols + [bad], CPU).has_zero_atom
    assert not MatBatch.from_encodings(mols, CPU).has_zero_atom
    net = MAT(n_encoders=1, h=4, **WIDTH)
    big = MatBatch.from_encodings([R.synthetic_molecule(ops.MAT_MAX_ATOMS, np.random.RandomState(0))], CPU)
    assert big.offs.n_max == ops.MAT_MAX_ATOMS + 1 and not net.native_covers(big)
    with pytest.raises(ValueError, match="MATEncoding-like"):
        MatBatch.from_encodings([np.zeros(3)], CPU)
    with pytest.raises(ValueError, match="dist_kernel"):
        MAT(dist_kernel="gauss")


# ------------------------------------------------------------------------------------------------ featurizer
def node_row(z_index, neighbours, hydrogens, charge, ring, aromatic):
    row = np.zeros(36)
    if z_index is not None:
        row[1 + z_index] = 1
    row[12 + neighbours] = 1
    row[18 + hydrogens] = 1
    row[23 + charge + 5] = 1
    row[34], row[35] = ring, aromatic
    return row


DUMMY = np.eye(1, 36)[0]
C, N, O = 1, 2, 3  # positions in [5, 6, 7, 8, 9, 15, 16, 17, 35, 53, 999]


def check_encoding(e, rows, bonds, dist):
    n = len(rows)
    assert isinstance(e, MATEncoding)
    assert np.array_equal(e.node_features, np.vstack([DUMMY] + rows))
    adj = np.zeros((n + 1, n + 1))
    for a, b in bonds:
        adj[a + 1, b + 1] = adj[b + 1, a + 1] = 1
    assert np.array_equal(e.adjacency_matrix, adj)
    want = np.full((n + 1, n + 1), 1e6)
    want[1:, 1:] = np.asarray(dist, float).reshape(n, n)
    assert np.array_equal(e.distance_matrix, want)
    assert np.all(e.distance_matrix[0] == 1e6) and np.all(e.distance_matrix[:, 0] == 1e6)
    assert np.all(e.adjacency_matrix[0] == 0) and np.all(e.adjacency_matrix[:, 0] == 0)


def test_featurizer_hand_derived_expectations():
    f = MATFeaturizer()
    cc, phenol, nh4, acetate, naph = f.featurize(["CC", "c1ccccc1O", "[NH4+]", "CC(=O)[O-]", "c1ccc2ccccc2c1"])
    check_encoding(cc, [node_row(C, 1, 3, 0, 0, 0)] * 2, [(0, 1)], [[0, 1], [1, 0]])
    ring6 = [[min(abs(i - j), 6 - abs(i - j)) for j in range(6)] for i in range(6)]
    d = np.zeros((7, 7))
    d[:6, :6] = ring6
    d[6, :6] = d[:6, 6] = np.asarray(ring6[5]) + 1
    check_encoding(phenol, [node_row(C, 2, 1, 0, 1, 1)] * 5 + [node_row(C, 3, 0, 0, 1, 1), node_row(O, 1, 1, 0, 0, 0)],
                   [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (0, 5), (5, 6)], d)
    check_encoding(nh4, [node_row(N, 0, 4, 1, 0, 0)], [], [[0]])
    check_encoding(acetate, [node_row(C, 1, 3, 0, 0, 0), node_row(C, 3, 0, 0, 0, 0), node_row(O, 1, 0, 0, 0, 0),
                             node_row(O, 1, 0, -1, 0, 0)], [(0, 1), (1, 2), (1, 3)],
                   [[0, 1, 2, 2], [1, 0, 1, 1], [2, 1, 0, 2], [2, 1, 2, 0]])
    # naphthalene, atoms in SMILES order: 0-1-2-3(-4-5-6-7-8)-9-0 with the fusion bond 3-8
    bonds = [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (5, 6), (6, 7), (7, 8), (3, 8), (8, 9), (0, 9)]
    rows = [node_row(C, 3 if a in (3, 8) else 2, 0 if a in (3, 8) else 1, 0, 1, 1) for a in range(10)]
    dist = np.full((10, 10), np.inf)
    np.fill_diagonal(dist, 0)
    for a, b in bonds:
        dist[a, b] = dist[b, a] = 1
    for k in range(10):  # Floyd-Warshall: an independent derivation of the bond counts
        dist = np.minimum(dist, dist[:, k:k + 1] + dist[k:k + 1, :])
    assert dist.max() == 5 and dist[0, 5] == 5 and dist[3, 8] == 1
    check_encoding(naph, rows, bonds, dist)
    assert f.featurize(["not a smiles ("])[0].size == 0
    # an element outside the list: an all-zero atomic-number block, as one_hot_encode gives
    si = f.featurize(["[SiH4]"])[0]
    assert si.node_features[1, 1:12].sum() == 0 and si.node_features[1].sum() > 0
