"""gcmi_gn_collate on the device: the batch buffer gathered from a resident graph set is, word for word, the buffer
MegnetBatch uploads from the graphs themselves (tests/test_megnet_collate_host.py holds the host routine to the same
words); the MegnetBatch around it; a training step, fit, predict and evaluate over either collation, and MEGNetModel's
routing between the two."""
import numpy as np
import pytest
import torch

import deepchem_amd as dc
from deepchem_amd import _lib, ops
from deepchem_amd.models.torch_models import MEGNetModel, MegnetBatch, ResidentMegnetSet
from deepchem_amd.models.torch_models import megnet as M
from tests import megnet_collate_cases as C

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GRID = [(w, u) for w in C.WIDTHS for u in C.MODES]
_SETS = {}


def grid_id(p):
    return "%s-%s" % (C.ids(p[0]), C.ids(p[1]))


def resident(widths, undirected):
    if (widths, undirected) not in _SETS:
        _SETS[widths, undirected] = ResidentMegnetSet(C.graph_set(widths, undirected), DEV)
    return _SETS[widths, undirected]


@pytest.mark.parametrize("name", sorted(C.SELECTIONS))
@pytest.mark.parametrize("case", GRID, ids=grid_id)
def test_device_buffer_equals_the_uploaded_host_buffer(case, name):
    widths, undirected = case
    rs, sel = resident(widths, undirected), C.SELECTIONS[name]
    host_batch, want = C.reference(widths, undirected, name)
    expect = torch.from_numpy(want.copy()).to(DEV)
    plan, n_nodes, n_edges = rs.plan(sel, pinned=True)
    out = torch.full((want.size,), -1, dtype=torch.int32, device=DEV)  # 0xFF bytes: an unwritten word, pads included, shows
    words = ops.gn_collate(rs.arrays, undirected, plan.to(DEV), len(sel), n_nodes, n_edges, out=out)
    assert words is out and torch.equal(words, expect)
    got = rs.batch(sel)
    assert torch.equal(got.graph._packed.view(torch.int32), expect)
    g, h = got.graph, host_batch.graph
    assert isinstance(got, MegnetBatch) and g._host is None and g.ref is not None and g.device == DEV
    assert (got.n_graphs, g.n_nodes, g.n_edges, g.n_inc, g.undirected) == (len(sel), h.n_nodes, h.n_edges, h.n_inc, undirected)
    assert list(g.host) == list(h.host)  # downloaded and split on first use
    for k, v in h.host.items():
        assert g.host[k].dtype == np.int32 and np.array_equal(g.host[k], v), k
        assert getattr(g, k).data_ptr() % 16 == 0 and np.array_equal(getattr(g, k).cpu().numpy(), v), k
    for k in ("x", "edge_attr", "global_features"):
        assert got[k].shape == host_batch[k].shape and got[k].data_ptr() % 16 == 0
        assert torch.equal(got[k].cpu(), host_batch[k]), k


def test_wrapper_refuses_what_the_kernel_assumes():
    rs = resident((5, 3, 1), True)
    sel = C.SELECTIONS["five_times"]
    plan, n_nodes, n_edges = rs.plan(sel)
    with pytest.raises(_lib.GcmiError, match="plan"):  # a plan on the host
        ops.gn_collate(rs.arrays, True, plan, len(sel), n_nodes, n_edges)
    with pytest.raises(_lib.GcmiError, match="plan"):  # a plan of another batch size
        ops.gn_collate(rs.arrays, True, plan.to(DEV), len(sel) + 1, n_nodes, n_edges)
    with pytest.raises(_lib.GcmiError, match="src"):
        ops.gn_collate(dict(rs.arrays, src=rs.arrays["src"].to(torch.int64)), True, plan.to(DEV), len(sel), n_nodes, n_edges)
    with pytest.raises(ValueError, match="outside the graph set"):
        rs.batch([0, C.N_GRAPHS])
    with pytest.raises(ValueError, match="no graphs"):
        rs.batch([])


# ------------------------------------------------------------------------------------------------ one training step
@pytest.mark.parametrize("undirected", C.MODES, ids=C.ids)
def test_a_training_step_is_bit_identical_on_either_batch(undirected):
    """The same bytes through the same kernels, none of which uses atomics: predictions and every parameter gradient
    are equal bit for bit.  The selection is the whole set, edge-free graphs included."""
    widths = (32, 32, 32)
    sel = C.SELECTIONS["whole_set"]
    X = C.graphs(widths)
    torch.manual_seed(5)
    model = MEGNetModel(n_blocks=2, is_undirected=undirected, batch_size=len(sel), device=DEV)
    model._ensure_built()
    model.model.train()
    rng = np.random.RandomState(1)
    y = torch.as_tensor(rng.normal(0, 1, (len(sel), 1)), dtype=torch.float32, device=DEV)
    results = []
    for batch in (MegnetBatch([X[i] for i in sel], undirected, DEV), resident(widths, undirected).batch(sel)):
        model.model.zero_grad(set_to_none=True)
        out = model.model(batch)
        assert model.last_route == "native"
        torch.square(out - y).mean().backward()
        results.append((out.detach().clone(), [p.grad.clone() for p in model.model.parameters()]))
    (out_h, grads_h), (out_d, grads_d) = results
    assert torch.equal(out_h, out_d)
    assert len(grads_h) == len(grads_d) > 10 and all(float(g.abs().max()) > 0 for g in grads_h)
    for (name, _), a, b in zip(model.model.named_parameters(), grads_h, grads_d):
        assert torch.equal(a, b), name


# ------------------------------------------------------------------------------------------------ fit, predict, evaluate
@pytest.fixture(scope="module")
def dataset96():
    rng = np.random.RandomState(5)
    X = np.empty(96, dtype=object)
    X[:] = [C.R.make_graph(*C.molecule(rng), rng, 32, 32, 32) for _ in range(96)]
    return dc.data.NumpyDataset(X, rng.normal(0, 1, (96, 1)), np.ones((96, 1)))


def test_fit_over_the_resident_set_equals_fit_over_host_collation(dataset96):
    """Three runs of the same seeds over 96 graphs in shuffled batches of 32: host, host again, device.  Before
    training the predictions are identical bit for bit.  After one epoch the device run must agree with a host run to
    the level the two host runs reach between themselves: identical if they are, and otherwise within 4 x their
    difference (the difference of two draws of the same noise exceeds one given draw by a factor of 2 often enough that a
    bound below that would fail on the noise alone) -- while the predictions have moved by far more.  Measured on an
    MI355X: host against host 0, device against host 0, moved 1.7e-1."""
    first, after = [], []
    for collate in ("host", "host", "device"):
        torch.manual_seed(11)
        np.random.seed(11)
        m = MEGNetModel(n_blocks=3, batch_size=32, device=DEV, collate=collate, learning_rate=1e-3)
        first.append(m.predict(dataset96))
        m.fit(dataset96, nb_epoch=1, deterministic=False, checkpoint_interval=0)
        assert m.last_route == "native"
        after.append(m.predict(dataset96))
        assert (m._resident is not None) == (collate == "device")
    assert np.array_equal(first[0], first[1]) and np.array_equal(first[0], first[2])
    noise = float(np.abs(after[0] - after[1]).max())
    apart = float(np.abs(after[2] - after[0]).max())
    moved = float(np.abs(after[0] - first[0]).max())
    print("host-host %.3e device-host %.3e moved %.3e" % (noise, apart, moved))
    assert apart <= 4 * noise
    assert moved > 10 * max(4 * noise, 1e-6)


def test_predict_and_evaluate_agree_under_both_settings(dataset96):
    metric = dc.metrics.Metric(dc.metrics.mean_absolute_error)
    got = []
    for collate in ("host", "device"):
        torch.manual_seed(7)
        m = MEGNetModel(n_blocks=1, batch_size=40, device=DEV, collate=collate)  # (a short last batch of 16)
        got.append((m.predict(dataset96), m.evaluate(dataset96, [metric])))
        assert m.last_route == "native"
    assert np.array_equal(got[0][0], got[1][0])
    assert got[0][1] == got[1][1] and len(got[0][1]) == 1


# ------------------------------------------------------------------------------------------------ routing
def routes(model, ds):
    """'device' / 'host' per batch of one pass."""
    return ["device" if b[0].graph._host is None else "host" for b in model._batch_generator(ds, deterministic=True)]


def test_auto_switches_to_the_device_at_the_threshold(dataset96, monkeypatch):
    at = M.MEGNET_DEVICE_COLLATE_MIN
    assert at >= 32
    monkeypatch.delenv("GCMI_RESIDENT_SET", raising=False)
    below = MEGNetModel(batch_size=at - 1, device=DEV)
    assert set(routes(below, dataset96)) == {"host"} and below._resident is None
    m = MEGNetModel(batch_size=at, device=DEV)
    got = routes(m, dataset96)
    assert got == ["device"] * len(got) and len(got) == -(-96 // at)
    assert isinstance(m._resident[1], ResidentMegnetSet) and m.resident_set(dataset96.X) is m._resident[1]
    assert set(routes(MEGNetModel(batch_size=at, device=DEV, collate="host"), dataset96)) == {"host"}
    assert set(routes(MEGNetModel(batch_size=at, device=DEV, route="torch"), dataset96)) == {"host"}
    assert set(routes(MEGNetModel(batch_size=8, device=DEV, collate="device"), dataset96)) == {"device"}  # below, on request
    with pytest.raises(ValueError, match="MEGNetModel\\(collate='device'\\): route='torch'"):
        routes(MEGNetModel(batch_size=at, device=DEV, collate="device", route="torch"), dataset96)
    monkeypatch.setenv("GCMI_RESIDENT_SET", "0")
    assert set(routes(MEGNetModel(batch_size=at, device=DEV), dataset96)) == {"host"}
    with pytest.raises(ValueError, match="MEGNetModel\\(collate='device'\\): GCMI_RESIDENT_SET=0"):
        routes(MEGNetModel(batch_size=at, device=DEV, collate="device"), dataset96)
    monkeypatch.delenv("GCMI_RESIDENT_SET")
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda *a: (1024, 1 << 30))  # 1 KiB free: the set does not fit
    with pytest.raises(ValueError, match="more than a quarter"):
        routes(MEGNetModel(batch_size=at, device=DEV, collate="device"), dataset96)
    auto = MEGNetModel(batch_size=at, device=DEV)
    assert set(routes(auto, dataset96)) == {"host"} and isinstance(auto._resident[1], str)


def test_the_set_is_built_once(dataset96, monkeypatch):
    monkeypatch.delenv("GCMI_RESIDENT_SET", raising=False)
    built = []
    real = ResidentMegnetSet.__init__
    monkeypatch.setattr(ResidentMegnetSet, "__init__", lambda self, *a: (built.append(1), real(self, *a))[1])
    m = MEGNetModel(n_blocks=1, batch_size=48, device=DEV, collate="device")
    m.fit(dataset96, nb_epoch=2, checkpoint_interval=0)
    m.predict(dataset96)
    assert len(built) == 1
