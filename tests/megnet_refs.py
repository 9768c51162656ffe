"""Restatements of MEGNet for the tests and for tools/gen_golden_megnet.py, on the CPU in a chosen precision (torch
tensors, so float64 gradients come from autograd; nothing here touches the package under test).

* ``block_direct``   one GraphNetwork block in the reference's own order: doubled edges, concatenated rows, scatter-means.
* ``block_split``    the same block by the split algebra of csrc/megnet.hip: ``edge_pass``, ``node_pass``, ``seg_mean``
                     on the projections Ps, Pd, Q, R and the incidence lists of ``lists``.
* ``lists``          the incidence lists of a batch, built entry by entry (what ``ops.GnGraph`` must reproduce).
* ``set2set``        torch_geometric's Set2Set from its published definition, on explicit LSTM weights (gates i, f, g, o).
* ``MEGNetRef``      the model on a state dict; ``loss_fn``, ``fit``: the reference's losses and Adam steps.
* ``edge_case_graphs``, ``fixture_graphs``, ``random_graph``: the graphs the tests and the fixtures use.

A node without an arriving edge and a graph without an edge get a ZERO mean row (torch_geometric's ``scatter`` gives
that row in the middle of its result and a shorter result at its end).
"""
import numpy as np
import torch


def _t(a, dtype):
    return a.detach().to(dtype) if torch.is_tensor(a) else torch.as_tensor(np.asarray(a), dtype=dtype)


def scatter_mean(src, index, n):
    out = src.new_zeros((n, src.shape[1])).index_add(0, index, src)
    cnt = src.new_zeros(n).index_add(0, index, src.new_ones(index.shape[0]))
    return out / cnt.clamp(min=1).unsqueeze(1)


def linear(p, name, x):
    return x @ p[name + ".weight"].t() + p[name + ".bias"]


# ------------------------------------------------------------------------------------------------ the block, directly
def block_direct(p, pre, x, ei, e, u, batch, undirected, residual):
    """``p``: tensors by state-dict key, ``pre``: the block's prefix ('' or 'megnet_blocks.0.'); ``ei`` (2, E) int64."""
    src, dst = ei[0], ei[1]
    x0, e0, u0, E = x, e, u, e.shape[0]
    if undirected:
        src, dst = torch.cat((src, dst)), torch.cat((dst, src))
        e = torch.cat((e, e))
    eg = batch[src]
    e = linear(p, pre + "edge_dense", linear(p, pre + "edge_models.0", torch.cat((x[src], x[dst], e, u[eg]), 1)))
    m = scatter_mean(e, dst, x.shape[0])
    x = linear(p, pre + "node_dense", linear(p, pre + "node_models.0", torch.cat((x, m, u[batch]), 1)))
    means = (scatter_mean(e, eg, u.shape[0]), scatter_mean(x, batch, u.shape[0]))
    u = linear(p, pre + "global_dense", linear(p, pre + "global_models.0", torch.cat(means + (u,), 1)))
    if undirected:
        e = (e[:E] + e[E:]) / 2
    if residual:
        e, x, u = e + e0, x + x0, u + u0
    return x, e, u


# ------------------------------------------------------------------------------------------------ lists
def lists(ei, batch, n_graphs, undirected):
    """dict of int64 numpy arrays: node_ptr, edge_ptr, inc_ptr / inc_edge / inc_other (the directed edges ARRIVING at
    each node, in the order of the (doubled) edge list) and, directed, out_ptr / out_edge / out_other."""
    ei, batch = np.asarray(ei), np.asarray(batch)
    N, E = batch.size, ei.shape[1]
    arriving = [[] for _ in range(N)]
    leaving = [[] for _ in range(N)]
    for k in range(E):
        arriving[ei[1, k]].append((k, ei[0, k]))
        leaving[ei[0, k]].append((k, ei[1, k]))
    if undirected:
        for k in range(E):
            arriving[ei[0, k]].append((k, ei[1, k]))

    def flat(per_node):
        ptr = np.concatenate([[0], np.cumsum([len(entries) for entries in per_node])])
        pairs = np.asarray([t for entries in per_node for t in entries], np.int64).reshape(-1, 2)
        return ptr, pairs[:, 0], pairs[:, 1]
    out = {"node_ptr": np.concatenate([[0], np.cumsum(np.bincount(batch, minlength=n_graphs))]),
           "edge_ptr": np.concatenate([[0], np.cumsum(np.bincount(batch[ei[0]], minlength=n_graphs))])}
    out["inc_ptr"], out["inc_edge"], out["inc_other"] = flat(arriving)
    if not undirected:
        out["out_ptr"], out["out_edge"], out["out_other"] = flat(leaving)
    return out


# ------------------------------------------------------------------------------------------------ the split algebra
def edge_pass(Ps, Pd, Q, R, ei, batch, undirected):
    s, d = ei[0], ei[1]
    p = Ps[s] + Pd[d]
    if undirected:
        p = (p + (Ps[d] + Pd[s])) * 0.5
    return (Q + R[batch[s]]) + p


def node_pass(Ps, Pd, Q, R, L, batch):
    """``L``: ``lists`` as int64 tensors."""
    N = Pd.shape[0]
    cnt = (L["inc_ptr"][1:] - L["inc_ptr"][:-1])
    owner = torch.repeat_interleave(torch.arange(N), cnt)
    acc = Pd.new_zeros(Pd.shape).index_add(0, owner, Ps[L["inc_other"]] + Q[L["inc_edge"]])
    has = (cnt > 0).to(Pd.dtype).unsqueeze(1)
    return ((Pd + R[batch]) + acc / cnt.clamp(min=1).to(Pd.dtype).unsqueeze(1)) * has


def seg_mean(x, ptr):
    cnt = ptr[1:] - ptr[:-1]
    index = torch.repeat_interleave(torch.arange(cnt.numel()), cnt)
    return scatter_mean(x, index, cnt.numel())


def tensor_lists(ei, batch, n_graphs, undirected):
    return {k: torch.as_tensor(v, dtype=torch.int64) for k, v in lists(ei, batch, n_graphs, undirected).items()}


def projections(p, pre, x, e, u):
    W1, b1 = p[pre + "edge_models.0.weight"], p[pre + "edge_models.0.bias"]
    Fn, Fe = x.shape[1], e.shape[1]
    return (x @ W1[:, :Fn].t(), x @ W1[:, Fn:2 * Fn].t(), e @ W1[:, 2 * Fn:2 * Fn + Fe].t(), u @ W1[:, 2 * Fn + Fe:].t() + b1)


def block_split(p, pre, x, ei, e, u, batch, undirected, residual, L=None):
    L = tensor_lists(ei.numpy(), batch.numpy(), u.shape[0], undirected) if L is None else L
    Fn, Fe = x.shape[1], e.shape[1]
    Ps, Pd, Q, R = projections(p, pre, x, e, u)
    W2, b2 = p[pre + "edge_dense.weight"], p[pre + "edge_dense.bias"]
    Wn, bn = p[pre + "node_models.0.weight"], p[pre + "node_models.0.bias"]
    Wg, bg = p[pre + "global_models.0.weight"], p[pre + "global_models.0.bias"]
    Hs = edge_pass(Ps, Pd, Q, R, ei, batch, undirected)
    Mh = node_pass(Ps, Pd, Q, R, L, batch)
    node_has = ((L["inc_ptr"][1:] - L["inc_ptr"][:-1]) > 0).to(x.dtype).unsqueeze(1)
    graph_has = ((L["edge_ptr"][1:] - L["edge_ptr"][:-1]) > 0).to(x.dtype).unsqueeze(1)
    e_new = Hs @ W2.t() + b2
    m = (Mh @ W2.t() + b2) * node_has
    hn = (u @ Wn[:, Fn + Fe:].t() + bn)[batch] + x @ Wn[:, :Fn].t() + m @ Wn[:, Fn:Fn + Fe].t()
    x_new = linear(p, pre + "node_dense", hn)
    ebar = (seg_mean(Hs, L["edge_ptr"]) @ W2.t() + b2) * graph_has
    nbar = seg_mean(x_new, L["node_ptr"])
    hg = (u @ Wg[:, Fe + Fn:].t() + bg) + ebar @ Wg[:, :Fe].t() + nbar @ Wg[:, Fe:Fe + Fn].t()
    u_new = linear(p, pre + "global_dense", hg)
    if residual:
        e_new, x_new, u_new = e_new + e, x_new + x, u_new + u
    return x_new, e_new, u_new


# ------------------------------------------------------------------------------------------------ Set2Set
def set2set(w_ih, w_hh, b_ih, b_hh, x, index, n_sets, steps=3):
    """q_star (n_sets, 2 C): ``steps`` rounds of one LSTM layer (gates i, f, g, o) and a softmax readout per set."""
    C = x.shape[1]
    h, c = x.new_zeros((n_sets, C)), x.new_zeros((n_sets, C))
    q_star = x.new_zeros((n_sets, 2 * C))
    for _ in range(steps):
        z = q_star @ w_ih.t() + b_ih + h @ w_hh.t() + b_hh
        i, f, g, o = z[:, :C], z[:, C:2 * C], z[:, 2 * C:3 * C], z[:, 3 * C:]
        c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
        h = torch.sigmoid(o) * torch.tanh(c)
        score = (x * h[index]).sum(-1)
        top = score.new_full((n_sets,), float("-inf")).scatter_reduce(0, index, score.detach(), "amax", include_self=True)
        a = torch.exp(score - top[index])
        a = a / (x.new_zeros(n_sets).index_add(0, index, a)[index] + 1e-16)
        r = x.new_zeros((n_sets, C)).index_add(0, index, a.unsqueeze(1) * x)
        q_star = torch.cat((h, r), 1)
    return q_star


# ------------------------------------------------------------------------------------------------ the model
class MEGNetRef(torch.nn.Module):
    """MEGNet on a state dict (numpy arrays or tensors by key), in ``dtype``; ``form``: 'direct' or 'split'."""

    def __init__(self, state, dtype, n_blocks, undirected=True, residual=True, mode="regression", n_tasks=1, n_classes=2,
                 form="direct"):
        super().__init__()
        self.keys = list(state)
        self.params = torch.nn.ParameterList([torch.nn.Parameter(_t(state[k], dtype).clone()) for k in self.keys])
        self.dtype, self.n_blocks, self.undirected, self.residual = dtype, n_blocks, undirected, residual
        self.mode, self.n_tasks, self.n_classes, self.form = mode, n_tasks, n_classes, form

    def p(self):
        return dict(zip(self.keys, self.params))

    def forward(self, inputs):
        """``inputs``: (x, edge_index, edge_attr, global_features, batch) as arrays."""
        x, ei, e, u, batch = inputs
        x, e, u = _t(x, self.dtype), _t(e, self.dtype), _t(u, self.dtype)
        ei, batch = torch.as_tensor(np.asarray(ei), dtype=torch.int64), torch.as_tensor(np.asarray(batch), dtype=torch.int64)
        p, G = self.p(), u.shape[0]
        block = block_direct if self.form == "direct" else block_split
        for i in range(self.n_blocks):
            x, e, u = block(p, "megnet_blocks.%d." % i, x, ei, e, u, batch, self.undirected, self.residual)
        qs = []
        for name, rows, index in (("set2set_nodes", x, batch), ("set2set_edges", e, batch[ei[0]])):
            qs.append(set2set(*(p["%s.lstm.%s_l0" % (name, k)] for k in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")),
                              rows, index, G))
        out = linear(p, "out", linear(p, "dense.1", linear(p, "dense.0", torch.cat(qs + [u], 1))))
        if self.mode == "classification":
            return out.view(-1, self.n_classes) if self.n_tasks == 1 else out.view(-1, self.n_tasks, self.n_classes)
        return out


def loss_fn(mode, out, y, w):
    """TorchModel's _StandardLoss over L2Loss / SparseSoftmaxCrossEntropy (``out``: the logits in classification),
    with the reference's broadcasting of the weights."""
    y, w = _t(y, out.dtype), _t(w, out.dtype)
    if mode == "regression":
        losses = torch.square(out - y.reshape(out.shape))
    else:
        logits = out.permute(0, 2, 1) if out.dim() == 3 else out
        labels = y.squeeze(-1) if y.dim() == logits.dim() else y
        losses = torch.nn.functional.cross_entropy(logits, labels.long(), reduction="none")
    if w.dim() < losses.dim():
        w = w.reshape(tuple(w.shape) + (1,) * (losses.dim() - w.dim()))
    return (losses * w).mean()


def fit(model, batches, learning_rate=0.001):
    """One Adam step (torch defaults: the reference's) per batch of ``(inputs, y, w)``; the per-step losses."""
    opt = torch.optim.Adam(model.parameters(), lr=learning_rate)
    losses = []
    for inputs, y, w in batches:
        opt.zero_grad()
        loss = loss_fn(model.mode, model(inputs), y, w)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    return losses


# ------------------------------------------------------------------------------------------------ graphs
class Graph:
    """A GraphData stand-in: node_features, edge_index, edge_features, global_features (1, Fg)."""

    def __init__(self, node_features, edge_index, edge_features, global_features):
        self.node_features, self.edge_index = node_features, edge_index
        self.edge_features, self.global_features = edge_features, global_features
        self.num_nodes, self.num_edges = node_features.shape[0], edge_index.shape[1]


def make_graph(edge_index, n_nodes, rng, Fn=5, Fe=3, Fg=4):
    ei = np.asarray(edge_index, np.int64).reshape(2, -1)
    return Graph(rng.normal(0, 1, (n_nodes, Fn)), ei, rng.normal(0, 1, (ei.shape[1], Fe)), rng.normal(0, 1, (1, Fg)))


def random_graph(rng, n_nodes, n_extra, Fn=5, Fe=3, Fg=4, extras=True):
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
    return make_graph(np.asarray([src, dst])[:, order], n_nodes, rng, Fn, Fe, Fg)


FIXTURE_NODES = [10, 7, 12, 9, 11, 8, 10, 13, 6, 10, 9, 12, 11, 7, 10, 8, 14, 9, 10, 11]


def fixture_graphs():
    """The 20 graphs of tests/golden/megnet_model.npz (about 10 nodes, average degree 4), regenerated from their seed."""
    rng = np.random.RandomState(2025)
    return [random_graph(rng, n, 3 * n - 2, extras=(k % 3 == 0)) for k, n in enumerate(FIXTURE_NODES)]


def pack(graphs):
    """(x, edge_index, edge_attr, global_features, batch) of a list of graphs, float64 / int64."""
    at, idx = 0, []
    for g in graphs:
        idx.append(np.asarray(g.edge_index, np.int64) + at)
        at += g.node_features.shape[0]
    return (np.concatenate([np.asarray(g.node_features, np.float64) for g in graphs]), np.concatenate(idx, 1),
            np.concatenate([np.asarray(g.edge_features, np.float64) for g in graphs]),
            np.concatenate([np.asarray(g.global_features, np.float64) for g in graphs]),
            np.repeat(np.arange(len(graphs)), [g.node_features.shape[0] for g in graphs]))


STAR_ARMS = (1, 2, 31, 32, 33, 63, 64, 65, 129)


def edge_case_graphs(rng, Fn=5, Fe=3, Fg=4):
    """One batch: a 1-node graph without an edge first, in the middle and last; a node without an incident edge at the
    highest index of its graph; a self-loop; a triple edge; stars whose centres have 1 .. 129 incident edges; a
    300-node ring."""
    lone = lambda: make_graph(np.zeros((2, 0)), 1, rng, Fn, Fe, Fg)  # noqa: E731
    gs = [lone()]
    gs.append(make_graph([[0, 1, 1, 1, 2, 2], [1, 0, 0, 0, 2, 1]], 4, rng, Fn, Fe, Fg))  # triple edge, self-loop, node 3 bare
    for arms in STAR_ARMS:  # spokes alternate direction, so directed mode sees both lists filled unevenly
        spokes = np.arange(1, arms + 1)
        s = np.where(spokes % 2 == 0, 0, spokes)
        d = np.where(spokes % 2 == 0, spokes, 0)
        gs.append(make_graph([s, d], arms + 1, rng, Fn, Fe, Fg))
        if arms == 32:
            gs.append(lone())
    ring = np.arange(300)
    gs.append(make_graph([ring, np.roll(ring, -1)], 300, rng, Fn, Fe, Fg))
    gs.append(lone())
    return gs


# ------------------------------------------------------------------------------------------------ grid-stride wrap cases
# (shared by tests/test_mat_megnet_edge_cases_host.py and tests/test_gpu_megnet_edges.py)
GN_MAX_BLOCKS = 8192  # the documented cap of a grid-stride launch (kMaxBlocks of csrc/common.h)
GN_SEG_THREADS = 256  # threads per workgroup of the segment kernels: GN_MAX_BLOCKS x 256 (range, column) pairs per turn
WRAP_RING_SIZES = [3, 131072, 1, 2, 131099]  # 8192 * 32 + 33 nodes and as many edges: 33 rows past one turn of the grid
WRAP_SEG_RANGES, WRAP_SEG_WIDTH = 65537, 33


def ring_batch(sizes):
    """(edge_index (2, N), batch (N,)) of directed rings i -> i + 1 of the given sizes, one graph each: edge k leaves
    node k.  A ring of one node is a self-loop, a ring of two a pair of opposite edges."""
    sizes = np.asarray(sizes, np.int64)
    base = np.repeat(np.concatenate([[0], np.cumsum(sizes)[:-1]]), sizes)
    n = np.repeat(sizes, sizes)
    node = np.arange(int(sizes.sum()))
    return np.stack([node, base + (node - base + 1) % n]), np.repeat(np.arange(sizes.size), sizes)


def ring_lists(sizes, undirected):
    """``lists`` of ``ring_batch(sizes)`` in closed form: the edge arriving at node v is edge prev(v) from prev(v), and
    undirected the doubled list adds (edge v, next(v)) after it; the edge leaving v is (edge v, next(v))."""
    sizes = np.asarray(sizes, np.int64)
    ei, batch = ring_batch(sizes)
    node, nxt = ei[0], ei[1]
    base = np.repeat(np.concatenate([[0], np.cumsum(sizes)[:-1]]), sizes)
    prev = base + (node - base - 1) % np.repeat(sizes, sizes)
    ptr = np.concatenate([[0], np.cumsum(sizes)])
    out = {"node_ptr": ptr, "edge_ptr": ptr}
    if undirected:
        pair = lambda a, b: np.stack([a, b], 1).reshape(-1)  # noqa: E731
        out.update(inc_ptr=2 * np.arange(node.size + 1), inc_edge=pair(prev, node), inc_other=pair(prev, nxt))
    else:
        out.update(inc_ptr=np.arange(node.size + 1), inc_edge=prev, inc_other=prev,
                   out_ptr=np.arange(node.size + 1), out_edge=node, out_other=nxt)
    return {k: np.asarray(v, np.int64) for k, v in out.items()}


def wrap_segment_ptr():
    """65 537 ranges of one or two rows: at width 33 more (range, column) pairs than one turn of the grid takes."""
    counts = np.random.RandomState(7).randint(1, 3, WRAP_SEG_RANGES)
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)


def rel_err(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))
