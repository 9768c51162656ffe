"""gcmi_gn_collate_host: the index routine of the MEGNet device collation (the same __host__ __device__ code as the kernel
of gcmi_gn_collate) run by host loops, and MegnetGraphSet.batch, the numpy route over the same flat arrays.  Both must
give, word for word, the buffer MegnetBatch packs from the graphs themselves -- no arithmetic is involved, so every
comparison is equality.  Then the plan and argument errors, the set's errors and MEGNetModel's routing on the CPU."""
import ctypes

import numpy as np
import pytest
import torch

import deepchem_amd as dc
from deepchem_amd import _lib, ops
from deepchem_amd.models.torch_models import MEGNetModel, MegnetBatch, MegnetGraphSet
from deepchem_amd.models.torch_models import megnet as M
from tests import megnet_collate_cases as C
from tests import megnet_refs as R

CPU = torch.device("cpu")
GRID = [(w, u) for w in C.WIDTHS for u in C.MODES]


def grid_id(p):
    return "%s-%s" % (C.ids(p[0]), C.ids(p[1]))


def repack(batch):
    """The buffer by the rule GnGraph has always packed with, restated: the int32 lists in GnGraph's order, then the
    float arrays, each padded with zero words to 16 bytes."""
    pad = lambda a: np.concatenate([a.reshape(-1).view(np.int32), np.zeros(-a.size % 4, np.int32)])  # noqa: E731
    g = batch.graph
    names = [k for k in ("src", "dst", "node_graph", "node_ptr", "edge_ptr", "inc_ptr", "inc_edge", "inc_other", "out_ptr",
                         "out_edge", "out_other") if k in g.host]
    return np.concatenate([pad(g.host[k]) for k in names] + [pad(np.ascontiguousarray(f.numpy())) for f in g.floats])


@pytest.mark.parametrize("case", GRID, ids=grid_id)
def test_gngraph_still_uploads_the_same_bytes(case):
    """The layout routine changed hands (Python loop -> gcmi_gn_collate_words), the bytes did not."""
    widths, undirected = case
    for name in ("whole_set", "pads", "edge_free"):
        batch, words = C.reference(widths, undirected, name)
        assert np.array_equal(words, repack(batch)), name
        total, layout = ops.gn_batch_layout(batch.n_graphs, batch.graph.n_nodes, batch.graph.n_edges, undirected, *widths)
        assert total == words.size and all(o % 4 == 0 for o, _ in layout.values())
        assert ("out_ptr" in layout) == (not undirected) and list(layout) == [k for k in ops.GN_BATCH_BLOCKS if k in layout]
    # arrays that are not the three feature blocks still travel behind the lists (tests/test_megnet_host.py)
    g = ops.GnGraph([[0, 1], [1, 0]], [0, 0], 1, undirected, CPU, floats=(np.arange(6.).reshape(2, 3), np.ones(5)))
    assert g.floats[0].shape == (2, 3) and g.floats[1].tolist() == [1.0] * 5
    assert all(f.data_ptr() % 16 == 0 for f in g.floats)


def test_pad_words_exist_behind_every_block_of_the_pads_case():
    for widths in C.WIDTHS[1:]:
        for undirected in C.MODES:
            batch, words = C.reference(widths, undirected, "pads")
            _, layout = ops.gn_batch_layout(5, batch.graph.n_nodes, batch.graph.n_edges, undirected, *widths)
            assert (batch.graph.n_nodes, batch.graph.n_edges) == (41, 39)
            assert all(int(np.prod(shape)) % 4 for _, shape in layout.values()), layout
    _, layout = ops.gn_batch_layout(5, 41, 39, True, 32, 32, 32)  # (rows of 32 floats leave no pad word)
    assert all(int(np.prod(layout[k][1])) % 4 for k in ops.GN_INT_BLOCKS if k in layout)


@pytest.mark.parametrize("name", sorted(C.SELECTIONS))
@pytest.mark.parametrize("case", GRID, ids=grid_id)
def test_host_routine_and_set_batch_write_the_words_megnetbatch_packs(case, name):
    widths, undirected = case
    sel = C.SELECTIONS[name]
    rs = C.resident_host(widths, undirected)
    batch, want = C.reference(widths, undirected, name)
    plan, n_nodes, n_edges = rs.plan(sel)
    assert (n_nodes, n_edges) == (batch.graph.n_nodes, batch.graph.n_edges)
    assert plan.dtype == torch.int32 and plan.numel() == 3 * len(sel) + 2
    out = C.unwritten(want.size)
    got = ops.gn_collate_host(rs.host_arrays, undirected, plan.numpy(), len(sel), n_nodes, n_edges, out=out)
    assert got is out
    assert np.array_equal(got, want)
    made = C.graph_set(widths, undirected).batch(sel)
    assert np.array_equal(C.packed_words(made), want)
    # the batch around either buffer has the attributes of the host-built one
    wrapped = MegnetBatch.from_device(torch.from_numpy(got), len(sel), n_nodes, n_edges, undirected, widths)
    assert wrapped.graph._host is None and wrapped.graph.ref is None
    for b in (made, wrapped):
        assert (b.n_graphs, b.graph.n_nodes, b.graph.n_edges, b.graph.n_inc, b.graph.undirected) == \
            (batch.n_graphs, batch.graph.n_nodes, batch.graph.n_edges, batch.graph.n_inc, undirected)
        assert list(b.graph.host) == list(batch.graph.host)
        for k, v in batch.graph.host.items():
            assert b.graph.host[k].dtype == np.int32 and np.array_equal(b.graph.host[k], v), k
            assert torch.equal(getattr(b.graph, k), getattr(batch.graph, k)), k
        for k in ("x", "edge_attr", "global_features", "edge_index", "batch"):
            assert b[k].shape == batch[k].shape and torch.equal(b[k], batch[k]), k
            assert k in ("edge_index", "batch") or b[k].data_ptr() % 16 == 0
    _lib.call("gcmi_gn_graph_check", ctypes.byref(wrapped.graph._host_ref))  # (lazy, from the downloaded lists)


def test_the_local_lists_are_the_batch_lists_of_each_graph_alone():
    widths = (5, 3, 1)
    for undirected in C.MODES:
        gs = C.graph_set(widths, undirected)
        k = 2 if undirected else 1
        for m, g in enumerate(C.graphs(widths)):
            L = R.lists(g.edge_index, np.zeros(g.num_nodes, np.int64), 1, undirected)
            v0, v1, e0, e1 = gs.node_ptr[m], gs.node_ptr[m + 1], gs.edge_ptr[m], gs.edge_ptr[m + 1]
            assert np.array_equal(gs.inc_start[v0:v1], L["inc_ptr"][:-1]), m
            assert np.array_equal(gs.inc_edge[k * e0:k * e1], L["inc_edge"]), m
            assert np.array_equal(gs.inc_other[k * e0:k * e1], L["inc_other"]), m
            if not undirected:
                assert np.array_equal(gs.out_start[v0:v1], L["out_ptr"][:-1]), m
                assert np.array_equal(gs.out_edge[e0:e1], L["out_edge"]) and np.array_equal(gs.out_other[e0:e1], L["out_other"])
        assert gs.node_ptr.dtype == np.int64 and gs.src.dtype == np.int32 and gs.n_graphs == C.N_GRAPHS
        assert hasattr(gs, "out_start") == (not undirected)


# ------------------------------------------------------------------------------------------------ plan and arguments
def test_a_plan_outside_the_set_or_without_graphs_is_refused_before_anything_runs():
    rs = C.resident_host((5, 3, 1), True)
    for bad in ([0, C.N_GRAPHS], [-1]):
        with pytest.raises(ValueError, match="outside the graph set"):
            rs.plan(bad)
        with pytest.raises(ValueError, match="outside the graph set"):
            rs.graphs.batch(bad)
    with pytest.raises(ValueError, match="no graphs"):
        rs.plan([])
    with pytest.raises(ValueError, match="no graphs"):
        rs.graphs.batch([])
    with pytest.raises(ValueError, match="not on a GPU"):
        rs.batch([0])


@pytest.mark.parametrize("undirected", C.MODES, ids=C.ids)
def test_bad_arguments_are_refused_with_a_message(undirected):
    lib = _lib.load()
    widths = (5, 3, 1)
    rs = C.resident_host(widths, undirected)
    sel = C.SELECTIONS["pads"]
    plan, n_nodes, n_edges = rs.plan(sel)
    words, _ = ops.gn_batch_layout(len(sel), n_nodes, n_edges, undirected, *widths)
    out = C.unwritten(words + 4)

    def desc(**change):
        d = _lib.GcmiGnSet(n_graphs=C.N_GRAPHS, undirected=1 if undirected else 0, fn=5, fe=3, fg=1)
        for k, a in rs.host_arrays.items():
            setattr(d, k, a.ctypes.data)
        for k, v in change.items():
            setattr(d, k, v)
        return ctypes.byref(d)

    def call(d=None, plan_ptr=plan.numpy().ctypes.data, n=len(sel), n_nodes=n_nodes, n_edges=n_edges,
             out_ptr=out.ctypes.data, out_words=words, entry="gcmi_gn_collate_host"):
        tail = (None,) if entry == "gcmi_gn_collate" else ()
        return getattr(lib, entry)(d or desc(), plan_ptr, n, n_nodes, n_edges, out_ptr, out_words, *tail)

    # the device entry makes the same checks before any launch (no pointer is followed there)
    for entry in ("gcmi_gn_collate_host", "gcmi_gn_collate"):
        for off in (-1, 1, 4):
            assert call(out_words=words + off, entry=entry) == -1 and b"output buffer holds" in lib.gcmi_last_error()
        assert call(out_ptr=out.ctypes.data + 4, entry=entry) == -1 and b"16-byte aligned" in lib.gcmi_last_error()
        assert call(out_ptr=None, entry=entry) == -1 and b"NULL" in lib.gcmi_last_error()
        assert call(plan_ptr=None, entry=entry) == -1 and b"NULL" in lib.gcmi_last_error()
        assert getattr(lib, entry)(None, *([0] * (7 if entry.endswith("collate") else 6))) == -1
        assert b"NULL set" in lib.gcmi_last_error()
        for k in rs.host_arrays:
            assert call(desc(**{k: None}), entry=entry) == -1 and b"NULL" in lib.gcmi_last_error(), k
        for n in (0, -1):
            assert call(n=n, entry=entry) == -1 and b"at least one graph" in lib.gcmi_last_error()
        for bad in (dict(n_nodes=-1), dict(n_edges=-1), dict(d=desc(fn=-1)), dict(d=desc(n_graphs=-1))):
            assert call(entry=entry, **bad) == -1 and b"negative" in lib.gcmi_last_error(), bad
        assert call(n_nodes=len(sel) - 1, entry=entry) == -1 and b"every graph holds a node" in lib.gcmi_last_error()
    assert np.all(out == -1)  # nothing was written by a refused call
    assert call() == 0 and np.all(out[words:] == -1)
    assert lib.gcmi_gn_collate_words(-1, 0, 0, 1, 5, 3, 1, None) == -1
    with pytest.raises(ValueError, match="3 \\* n_graphs \\+ 2"):
        ops.gn_collate_host(rs.host_arrays, undirected, plan.numpy()[:-1], len(sel), n_nodes, n_edges)
    with pytest.raises(_lib.GcmiError, match="output buffer holds"):
        ops.gn_collate_host(rs.host_arrays, undirected, plan.numpy(), len(sel), n_nodes, n_edges, out=out)
    with pytest.raises(ValueError, match="inc_edge needs"):
        ops.gn_collate_host(dict(rs.host_arrays, inc_edge=rs.host_arrays["inc_edge"][:-1].copy()), undirected, plan.numpy(),
                            len(sel), n_nodes, n_edges)
    with pytest.raises(ValueError, match="the set of a"):
        ops.gn_collate_host(rs.host_arrays, not undirected, plan.numpy(), len(sel), n_nodes, n_edges)
    with pytest.raises(ValueError, match="int32 words of the layout"):
        MegnetBatch.from_device(torch.zeros(words - 4, dtype=torch.int32), len(sel), n_nodes, n_edges, undirected, widths)


@pytest.mark.parametrize("undirected", C.MODES, ids=C.ids)
def test_the_routine_skips_a_bad_entry_and_does_not_read_through_it(undirected):
    """Defence in depth under the Python check: entry 1 of the plan names graph M + 7, then a graph larger than the
    room the plan gives it.  The words that graph would own stay as they were, every other graph's are written."""
    widths = (5, 3, 1)
    rs = C.resident_host(widths, undirected)
    sel = np.array([C.STAR31, C.RND_A, C.BARE])
    X = C.graphs(widths)
    batch = MegnetBatch([X[i] for i in sel], undirected, CPU)
    want = C.packed_words(batch)
    plan, n_nodes, n_edges = rs.plan(sel)
    _, layout = ops.gn_batch_layout(3, n_nodes, n_edges, undirected, *widths)
    v0, v1 = batch.graph.host["node_ptr"][1:3]
    e0, e1 = batch.graph.host["edge_ptr"][1:3]
    k = 2 if undirected else 1
    rows = {"src": (e0, e1), "dst": (e0, e1), "node_graph": (v0, v1), "inc_ptr": (v0, v1), "inc_edge": (k * e0, k * e1),
            "inc_other": (k * e0, k * e1), "out_ptr": (v0, v1), "out_edge": (e0, e1), "out_other": (e0, e1),
            "x": (5 * v0, 5 * v1), "edge_attr": (3 * e0, 3 * e1)}
    for bad in (C.N_GRAPHS + 7, -3, C.RING300):
        words = plan.numpy().copy()
        words[1] = bad
        out = C.unwritten(want.size)
        ops.gn_collate_host(rs.host_arrays, undirected, words, 3, n_nodes, n_edges, out=out)
        expect = want.copy()
        for name, (a, b) in rows.items():
            if name in layout:
                expect[layout[name][0] + a:layout[name][0] + b] = -1
        expect[layout["global_features"][0] + 1] = 0  # (the global row of a skipped graph is cleared)
        assert np.array_equal(out, expect), bad


# ------------------------------------------------------------------------------------------------ the set's errors
def test_the_set_raises_what_megnetbatch_raises():
    rng = np.random.RandomState(0)
    good = [R.make_graph([[0, 1], [1, 0]], 2, rng) for _ in range(3)]

    def both(graphs, match):
        for make in (lambda: MegnetBatch(graphs, True, CPU), lambda: MegnetGraphSet(graphs, True),
                     lambda: MegnetGraphSet(graphs, False)):
            with pytest.raises(ValueError, match=match):
                make()

    empty = R.make_graph(np.zeros((2, 0)), 1, rng)
    empty.node_features = np.zeros((0, 5))
    both(good[:1] + [empty] + good[1:], "give every graph of range\\(4\\) a node")
    no_global = R.make_graph([[0], [1]], 2, rng)
    no_global.global_features = None
    both(good + [no_global], "graph 3 has no global_features")
    flat_global = R.make_graph([[0], [1]], 2, rng)
    flat_global.global_features = np.zeros(4)
    both(good + [flat_global], "global_features of graph 3 must have shape \\(1, n_global_features\\)")
    no_edge_features = R.make_graph([[0], [1]], 2, rng)
    no_edge_features.edge_features = None
    both([no_edge_features], "graph 0 has no edge_features")
    both(good + [R.make_graph([[0], [1]], 2, rng, Fn=6)], "the node_features of a batch must be 2-D with one width")
    both(good + [R.make_graph([[0], [1]], 2, rng, Fe=2)], "the edge_features of a batch must be 2-D with one width")
    both(good + [R.make_graph([[0], [1]], 2, rng, Fg=3)], "the global_features of a batch must be 2-D with one width")
    both([], "no graphs")
    both([object()], "takes GraphData objects")
    outside = R.make_graph([[0], [2]], 2, rng)
    for mode in C.MODES:
        with pytest.raises(ValueError, match="every edge inside one graph"):
            MegnetGraphSet(good + [outside], mode)


# ------------------------------------------------------------------------------------------------ routing on the CPU
def cpu_model(batch_size, widths=(5, 3, 1), **kwargs):
    return MEGNetModel(n_node_features=widths[0], n_edge_features=widths[1], n_global_features=widths[2], n_blocks=1,
                       batch_size=batch_size, device=CPU, **kwargs)


@pytest.fixture(scope="module")
def dataset():
    widths = (5, 3, 1)
    rng = np.random.RandomState(9)
    X = C.graphs(widths)
    return dc.data.NumpyDataset(X, rng.normal(0, 1, (len(X), 1)), np.ones((len(X), 1)))


def test_collate_argument_of_the_model(dataset):
    with pytest.raises(ValueError, match="collate must be"):
        cpu_model(4, collate="gpu")
    with pytest.raises(ValueError, match="MEGNetModel\\(collate='device'\\): the model is on cpu, not on a GPU"):
        next(cpu_model(4, collate="device")._batch_generator(dataset))
    with pytest.raises(ValueError, match="not a NumpyDataset of GraphData"):
        next(cpu_model(4, collate="device")._batch_generator(dc.data.NumpyDataset(np.zeros((4, 3)), np.zeros((4, 1)))))
    assert M.MEGNET_DEVICE_COLLATE_MIN >= 32
    m = cpu_model(M.MEGNET_DEVICE_COLLATE_MIN)  # "auto" on a CPU model: host batches, no resident set
    made = list(m._batch_generator(dataset, deterministic=True))
    assert all(isinstance(b[0], MegnetBatch) and b[0].graph._host is not None for b in made) and m._resident is None
    assert m.graph_set(dataset.X) is m.graph_set(dataset.X)  # built once
    with pytest.raises(ValueError, match="widths \\(5, 3, 1\\), the model was built for \\(5, 3, 2\\)"):
        next(cpu_model(4, widths=(5, 3, 2))._batch_generator(dataset))


@pytest.mark.parametrize("undirected", C.MODES, ids=C.ids)
@pytest.mark.parametrize("deterministic", [True, False])
def test_batch_generator_follows_default_generator(dataset, deterministic, undirected):
    """Same walk, same shuffles, same padding of the last batch, same bytes, labels and weights."""
    for mode, pad in (("fit", True), ("predict", False)):
        m = cpu_model(4, is_undirected=undirected)
        np.random.seed(21)
        want = [m._prepare_batch(b) for b in m.default_generator(dataset, epochs=2, mode=mode, deterministic=deterministic,
                                                                 pad_batches=pad)]
        np.random.seed(21)
        got = [m._prepare_batch(b) for b in m._batch_generator(dataset, epochs=2, mode=mode, deterministic=deterministic,
                                                               pad_batches=pad)]
        assert len(got) == len(want) == 2 * 4
        for (gb, gy, gw), (wb, wy, ww) in zip(got, want):
            assert np.array_equal(C.packed_words(gb), C.packed_words(wb))
            assert torch.equal(gy[0], wy[0]) and torch.equal(gw[0], ww[0])
        if not deterministic:  # the walk was shuffled: the first batch is not the first four graphs
            first = MegnetBatch(list(dataset.X[:4]), undirected, CPU)
            assert not np.array_equal(C.packed_words(got[0][0]), C.packed_words(first))


def test_fit_and_predict_on_the_cpu_take_the_set_route(dataset):
    outs = []
    for collate in ("host", "auto"):
        torch.manual_seed(3)
        np.random.seed(3)
        m = cpu_model(4, collate=collate)
        m.fit(dataset, nb_epoch=1, deterministic=False, checkpoint_interval=0)
        assert m._graph_set is not None and m.last_route == "torch"
        outs.append(m.predict(dataset))
    assert np.array_equal(outs[0], outs[1])
