"""Restatements of CGCNN for the tests and for tools/gen_golden_cgcnn.py, on the CPU in a chosen precision (torch
tensors, so float64 gradients come from autograd; nothing here touches the package under test).

* ``layer_direct``  one CGCNNLayer in the reference's own order: the concatenated row per edge, Linear, BatchNorm over
                    the E rows, gate, sum at the destination, softplus.
* ``layer_split``   the same layer by the split algebra of csrc/cgcnn.hip: ``projections`` (Ps | Pd, Q) and ``conv_pass``.
* ``conv_pass``     everything between the products, from P, Q and h: what the kernels compute.
* ``CGCNNRef``      the model on a state dict; ``loss_fn`` / ``fit`` are those of tests/megnet_refs.py.
* ``edge_case_graphs``, ``sized_graph``, ``fixture_graphs``, ``random_graph``: the graphs the tests and the fixtures use.

A node without an arriving edge gets a ZERO row (DGL's ``update_all`` does not call the reduce function for a node of
in-degree zero and fills its new feature with zeros).  BatchNorm is ``F.batch_norm`` in the chosen precision: batch
statistics with the biased variance in training, running statistics updated with momentum 0.1 and the unbiased
variance; the running statistics in eval.
"""
import numpy as np
import torch
import torch.nn.functional as F

from tests.megnet_refs import _t, fit, loss_fn, rel_err  # noqa: F401  (fit, loss_fn and rel_err are used by the tests)

EPS, MOMENTUM = 1e-5, 0.1


class BNState:
    """running_mean, running_var, num_batches_tracked of one BatchNorm1d, in ``dtype``."""

    def __init__(self, width, dtype, mean=None, var=None, tracked=0):
        self.mean = torch.zeros(width, dtype=dtype) if mean is None else _t(mean, dtype).clone()
        self.var = torch.ones(width, dtype=dtype) if var is None else _t(var, dtype).clone()
        self.tracked = int(tracked)


def batch_norm(z, gamma, beta, state, training):
    if training:
        if z.shape[0] < 2:
            raise ValueError("Expected more than 1 value per channel when training, got input size %s" % (z.shape,))
        state.tracked += 1
    return F.batch_norm(z, state.mean, state.var, gamma, beta, training, MOMENTUM, EPS)


def gate_and_sum(zh, h, dst):
    """m = sigmoid(gate half) * softplus(message half), summed at the destination; softplus(h + sum), zero rows for
    nodes nothing arrives at."""
    H = h.shape[1]
    m = torch.sigmoid(zh[:, :H]) * F.softplus(zh[:, H:])
    S = torch.zeros_like(h).index_add(0, dst, m)
    arrives = (torch.bincount(dst, minlength=h.shape[0]) > 0).to(h.dtype).unsqueeze(1)
    return F.softplus(h + S) * arrives


def layer_direct(W, b, gamma, beta, h, ei, e, state, training):
    """``W`` (2H, 2H + Fe), ``b`` (2H,); ``gamma`` / ``beta`` None: no BatchNorm; ``ei`` (2, E) int64."""
    s, d = ei[0], ei[1]
    z = torch.cat((h[s], h[d], e), 1) @ W.t() + b
    if gamma is not None:
        z = batch_norm(z, gamma, beta, state, training)
    return gate_and_sum(z, h, d)


def projections(W, b, h, e):
    """(P = [Ps | Pd] (N, 4H), Q (E, 2H)) of the split form."""
    H = h.shape[1]
    return torch.cat((h @ W[:, :H].t(), h @ W[:, H:2 * H].t()), 1), e @ W[:, 2 * H:].t() + b


def conv_pass(P, Q, h, gamma, beta, ei, state, training):
    H = h.shape[1]
    z = (P[:, :2 * H][ei[0]] + P[:, 2 * H:][ei[1]]) + Q
    if gamma is not None:
        z = batch_norm(z, gamma, beta, state, training)
    return gate_and_sum(z, h, ei[1])


def layer_split(W, b, gamma, beta, h, ei, e, state, training):
    P, Q = projections(W, b, h, e)
    return conv_pass(P, Q, h, gamma, beta, ei, state, training)


# ------------------------------------------------------------------------------------------------ the model
class CGCNNRef(torch.nn.Module):
    """CGCNN on a state dict (numpy arrays or tensors by key), in ``dtype``; ``form``: 'direct' or 'split'.  The
    BatchNorm buffers live in ``self.bn`` (one ``BNState`` per layer) and move with every training forward."""

    def __init__(self, state, dtype, num_conv, mode="regression", n_tasks=1, n_classes=2, form="direct"):
        super().__init__()
        buffers = ("running_mean", "running_var", "num_batches_tracked")
        self.keys = [k for k in state if not k.endswith(buffers)]
        self.params = torch.nn.ParameterList([torch.nn.Parameter(_t(state[k], dtype).clone()) for k in self.keys])
        self.bn = []
        for i in range(num_conv):
            pre = "conv_layers.%d.batch_norm." % i
            self.bn.append(BNState(0, dtype, state[pre + "running_mean"], state[pre + "running_var"],
                                   int(np.asarray(state[pre + "num_batches_tracked"]))))
        self.dtype, self.num_conv, self.mode, self.n_tasks, self.n_classes, self.form = dtype, num_conv, mode, n_tasks, n_classes, form

    def p(self):
        return dict(zip(self.keys, self.params))

    def forward(self, inputs):
        """``inputs``: (x, edge_index, edge_attr, batch) as arrays."""
        x, ei, e, batch = inputs
        x, e = _t(x, self.dtype), _t(e, self.dtype)
        ei, batch = torch.as_tensor(np.asarray(ei), dtype=torch.int64), torch.as_tensor(np.asarray(batch), dtype=torch.int64)
        p, G = self.p(), int(batch.max()) + 1
        layer = layer_direct if self.form == "direct" else layer_split
        h = x @ p["embedding.weight"].t() + p["embedding.bias"]
        for i in range(self.num_conv):
            pre = "conv_layers.%d." % i
            h = layer(p[pre + "linear.weight"], p[pre + "linear.bias"], p[pre + "batch_norm.weight"], p[pre + "batch_norm.bias"],
                      h, ei, e, self.bn[i], self.training)
        mean = torch.zeros((G, h.shape[1]), dtype=self.dtype).index_add(0, batch, h) / \
            torch.bincount(batch, minlength=G).to(self.dtype).unsqueeze(1)
        gf = F.softplus(mean)
        gf = F.softplus(gf @ p["fc.weight"].t() + p["fc.bias"])
        out = gf @ p["out.weight"].t() + p["out.bias"]
        if self.mode == "classification":
            return out.view(-1, self.n_classes) if self.n_tasks == 1 else out.view(-1, self.n_tasks, self.n_classes)
        return out


# ------------------------------------------------------------------------------------------------ graphs
class Graph:
    """A GraphData stand-in: node_features, edge_index, edge_features."""

    def __init__(self, node_features, edge_index, edge_features):
        self.node_features, self.edge_index, self.edge_features = node_features, edge_index, edge_features
        self.num_nodes, self.num_edges = node_features.shape[0], edge_index.shape[1]


def make_graph(edge_index, n_nodes, rng, Fn=5, Fe=3):
    ei = np.asarray(edge_index, np.int64).reshape(2, -1)
    return Graph(rng.normal(0, 1, (n_nodes, Fn)), ei, rng.normal(0, 1, (ei.shape[1], Fe)))


def random_graph(rng, n_nodes, n_extra, Fn=5, Fe=3, extras=True):
    """Every node has an arriving edge (a random cycle), ``n_extra`` random edges on top, and with ``extras`` one
    duplicated edge and one self-loop."""
    perm = rng.permutation(n_nodes)
    src, dst = list(perm), list(np.roll(perm, -1))
    for _ in range(n_extra):
        src.append(int(rng.randint(n_nodes))), dst.append(int(rng.randint(n_nodes)))
    if extras:
        src += [src[0], int(perm[0])]
        dst += [dst[0], int(perm[0])]
    order = rng.permutation(len(src))
    return make_graph(np.asarray([src, dst])[:, order], n_nodes, rng, Fn, Fe)


FIXTURE_NODES = [10, 7, 12, 9, 11, 8, 10, 13, 6, 10, 9, 12, 11, 7, 10, 8, 14, 9, 10, 11]


def fixture_graphs(Fn=5, Fe=3):
    """The 20 graphs of tests/golden/cgcnn_model.npz (about 10 nodes, 4 arriving edges per node on average; graph 4
    has a node nothing arrives at), regenerated from their seed."""
    rng = np.random.RandomState(2026)
    gs = [random_graph(rng, n, 3 * n - 2, Fn, Fe, extras=(k % 3 == 0)) for k, n in enumerate(FIXTURE_NODES)]
    g = gs[4]
    gs[4] = Graph(np.concatenate([g.node_features, rng.normal(0, 1, (1, Fn))]), g.edge_index, g.edge_features)
    return gs


def pack(graphs):
    """(x, edge_index, edge_attr, batch) of a list of graphs, float64 / int64."""
    at, idx = 0, []
    for g in graphs:
        idx.append(np.asarray(g.edge_index, np.int64).reshape(2, -1) + at)
        at += g.node_features.shape[0]
    return (np.concatenate([np.asarray(g.node_features, np.float64) for g in graphs]), np.concatenate(idx, 1),
            np.concatenate([np.asarray(g.edge_features, np.float64) for g in graphs]),
            np.repeat(np.arange(len(graphs)), [g.node_features.shape[0] for g in graphs]))


STAR_ARMS = (1, 2, 12, 13, 63, 64, 65, 129)


def edge_case_graphs(rng, Fn=5, Fe=3):
    """One batch: a 1-node graph without an edge first, in the middle and last; a node without an arriving edge at the
    highest index of its graph; a self-loop; a triple edge; stars whose centres have 1 .. 129 ARRIVING edges and the same
    stars reversed (the centres' LEAVING lists have those lengths, and nothing arrives at them); a 300-node ring."""
    lone = lambda: make_graph(np.zeros((2, 0)), 1, rng, Fn, Fe)  # noqa: E731
    gs = [lone()]
    gs.append(make_graph([[0, 1, 1, 1, 2, 2], [1, 0, 0, 0, 2, 1]], 4, rng, Fn, Fe))  # triple edge, self-loop, node 3 bare
    for arms in STAR_ARMS:
        spokes = np.arange(1, arms + 1)
        gs.append(make_graph([spokes, np.zeros_like(spokes)], arms + 1, rng, Fn, Fe))
        gs.append(make_graph([np.zeros_like(spokes), spokes], arms + 1, rng, Fn, Fe))
        if arms == 13:
            gs.append(lone())
    ring = np.arange(300)
    gs.append(make_graph([ring, np.roll(ring, -1)], 300, rng, Fn, Fe))
    gs.append(lone())
    return gs


def sized_graph(rng, n_nodes, n_edges, Fn=5, Fe=3):
    """One graph (G = 1) with exactly these counts: a cycle through every node, random edges on top."""
    assert n_edges >= n_nodes
    g = random_graph(rng, n_nodes, n_edges - n_nodes, Fn, Fe, extras=False)
    assert g.num_nodes == n_nodes and g.num_edges == n_edges
    return g


def case_graphs(name, Fn=5, Fe=3):
    """The graph batches of the kernel and layer tests by name: 'edge' (``edge_case_graphs``), 'g1' (one small graph),
    'below' / 'above' (one graph with node and edge counts one below / one above a multiple of 64), 'cap' (8200 nodes
    and 8300 edges: at H = 128, 8 rows per workgroup, 1025 node groups and 1038 edge groups, past the 1024 partial rows
    of csrc/cgcnn.hip), 'tile' (2731 nodes, 4099 edges: the graph the tiling test repeats) and 'pair' (two nodes, the
    edges 0 -> 1 and 1 -> 0: the smallest batch the statistics accept)."""
    rng = np.random.RandomState(17)
    if name == "edge":
        return edge_case_graphs(rng, Fn, Fe)
    if name == "g1":
        return [random_graph(rng, 10, 28, Fn, Fe)]
    if name == "pair":
        return [make_graph([[0, 1], [1, 0]], 2, rng, Fn, Fe)]
    n, e = {"below": (127, 191), "above": (129, 193), "cap": (8200, 8300), "tile": (2731, 4099)}[name]
    return [sized_graph(rng, n, e, Fn, Fe)]
