"""Restatements of LCNN for the tests and for tools/gen_golden_lcnn.py, on the CPU in a chosen precision (torch tensors,
so float64 gradients come from autograd; nothing here touches the package under test).

* ``block``         one LCNNBlock from ``x`` (N, F) and the neighbour table ``nbr`` (N, P, K), in three summation orders:
                    ``"concat"`` (the reference's: the gathered (N, P, K * F) rows through one Linear), ``"split"`` (Y = x
                    [W_0; ...; W_{K-1}]^T, then X = b + sum_j Y[nbr[:, :, j], j] with j ascending: what csrc/lcnn.hip
                    does) and ``"split_rev"`` (j descending).  Training: the mean and biased variance over the P rows
                    of each site; the running statistics by ``running_closed``.
* ``block_loop``    the literal per-site loop: one ``F.batch_norm`` call per site on its (P, O) rows, which also runs the
                    running-statistics recurrence ``r <- 0.9 r + 0.1 s_v`` in site order; pins the closed form.
* ``running_loop`` / ``running_closed``  the recurrence and its closed form on per-site statistics.
* ``LCNNRef``       the whole model on a state dict; ``fit`` is that of tests/megnet_refs.py with the masks injected.
* ``torus``, ``random_sites``, ``hub_sites``: the graphs.  ``torus(a, b)`` is an a x b periodic triangular lattice in
  axial coordinates: the 19 sites within two shells as neighbour slots and the six 60-degree rotations (q, r) -> (-r, q
  + r) as permutations; small tori wrap (on 1 x 1 every neighbour is the site itself).
"""
import numpy as np
import torch
import torch.nn.functional as F

from tests.megnet_refs import _t, loss_fn, rel_err  # noqa: F401

EPS, MOMENTUM, SHIFT = 1e-5, 0.1, 0.69310


class BNState:
    """running_mean, running_var, num_batches_tracked of one BatchNorm1d, in ``dtype``."""

    def __init__(self, width, dtype, mean=None, var=None, tracked=0):
        self.mean = torch.zeros(width, dtype=dtype) if mean is None else _t(mean, dtype).clone()
        self.var = torch.ones(width, dtype=dtype) if var is None else _t(var, dtype).clone()
        self.tracked = int(tracked)


def running_loop(s, r0, momentum=MOMENTUM):
    """r after ``r <- (1 - m) r + m s[v]`` for v = 0 .. N - 1, in the dtype of ``s``."""
    r = _t(r0, s.dtype).clone()
    for v in range(s.shape[0]):
        r = (1 - momentum) * r + momentum * s[v]
    return r


def running_closed(s, r0, momentum=MOMENTUM):
    """(1 - m)^N r0 + m sum_v (1 - m)^(N - 1 - v) s[v], weights and sum in float64."""
    N, keep = s.shape[0], 1.0 - momentum
    w = momentum * keep ** torch.arange(N - 1, -1, -1, dtype=torch.float64)
    return (keep ** N * _t(r0, torch.float64) + (w.unsqueeze(1) * s.double()).sum(0)).to(s.dtype)


def site_rows(x, nbr, W, b, order):
    """X (N, P, O)."""
    N, P, K = nbr.shape
    O = W.shape[0]
    if order == "concat":
        return x[nbr.reshape(N, P * K)].reshape(N, P, -1) @ W.t() + b
    Wk = W.view(O, K, -1).permute(1, 0, 2).reshape(K * O, -1)
    Y = (x @ Wk.t()).view(N, K, O)
    X = b.expand(N, P, O)
    for j in (range(K) if order == "split" else range(K - 1, -1, -1)):
        X = X + Y[nbr[:, :, j], j]
    return X


def block(x, nbr, W, b, gamma, beta, mask, state, training, order="concat"):
    """out (N, O).  ``mask`` (N, P) already scaled, None: ones.  ``state`` (a ``BNState``) moves in training."""
    nbr = torch.as_tensor(np.asarray(nbr), dtype=torch.int64)
    N, P, K = nbr.shape
    X = site_rows(x, nbr, W, b, order)
    if training:
        if P < 2:
            raise ValueError("Expected more than 1 value per channel when training")
        mean, var = X.mean(1, keepdim=True), X.var(1, unbiased=False, keepdim=True)
        with torch.no_grad():
            state.mean = running_closed(mean.squeeze(1), state.mean)
            state.var = running_closed(var.squeeze(1) * (P / (P - 1.0)), state.var)
            state.tracked += N
    else:
        mean, var = state.mean, state.var
    Xhat = (X - mean) / torch.sqrt(var + EPS) * gamma + beta
    return Xhat.sum(1) if mask is None else (_t(mask, x.dtype).unsqueeze(2) * Xhat).sum(1)


def block_loop(x, nbr, W, b, gamma, beta, mask, state, training):
    """The reference's two Python loops, literally."""
    nbr = torch.as_tensor(np.asarray(nbr), dtype=torch.int64)
    X = site_rows(x, nbr, W, b, "concat")
    rows = []
    for v in range(X.shape[0]):
        xh = F.batch_norm(X[v], state.mean, state.var, gamma, beta, training, MOMENTUM, EPS)
        state.tracked += int(training)
        rows.append(xh.sum(0) if mask is None else (_t(mask[v], x.dtype).unsqueeze(1) * xh).sum(0))
    return torch.stack(rows)


# ------------------------------------------------------------------------------------------------ the model
def ssp(x):
    return F.softplus(x) - SHIFT


class LCNNRef(torch.nn.Module):
    """LCNN on a state dict (numpy arrays or tensors by key), in ``dtype``.  ``inputs``: (x, nbr (N, P, K), node_ptr,
    masks) with ``masks = ([one (N, P) per block], (N, S))`` or None in eval."""
    mode = "regression"

    def __init__(self, state, dtype, n_conv=2, order="concat"):
        super().__init__()
        frozen = ("running_mean", "running_var", "num_batches_tracked", "shift", "ones")
        self.keys = [k for k in state if not k.endswith(frozen)]
        self.params = torch.nn.ParameterList([torch.nn.Parameter(_t(state[k], dtype).clone()) for k in self.keys])
        self.bn = []
        for i in range(n_conv):
            pre = "LCNN_blocks.%d.batch_norm." % i
            self.bn.append(BNState(0, dtype, state[pre + "running_mean"], state[pre + "running_var"],
                                   int(np.asarray(state[pre + "num_batches_tracked"]))))
        self.dtype, self.n_conv, self.order = dtype, n_conv, order

    def p(self):
        return dict(zip(self.keys, self.params))

    def forward(self, inputs):
        x, nbr, node_ptr, masks = inputs
        p, h = self.p(), _t(x, self.dtype)
        block_masks, atom_mask = masks if self.training else ([None] * self.n_conv, None)
        for i in range(self.n_conv):
            pre = "LCNN_blocks.%d." % i
            h = block(h, nbr, p[pre + "conv_weights.weight"], p[pre + "conv_weights.bias"], p[pre + "batch_norm.weight"],
                      p[pre + "batch_norm.bias"], block_masks[i], self.bn[i], self.training, self.order)
        pre = "Atom_wise_Conv."
        h = h @ p[pre + "conv_weights.weight"].t() + p[pre + "conv_weights.bias"]
        h = ssp(F.layer_norm(h, h.shape[1:], p[pre + "batch_norm.weight"], p[pre + "batch_norm.bias"], EPS))
        if atom_mask is not None:
            h = h * _t(atom_mask, self.dtype)
        h = ssp(h @ p["Atom_wise_Lin.weight"].t() + p["Atom_wise_Lin.bias"])
        ptr = np.asarray(node_ptr)
        y = torch.stack([h[ptr[g]:ptr[g + 1]].mean(0) for g in range(len(ptr) - 1)])
        return y @ p["fc.weight"].t() + p["fc.bias"]


def fit(model, batches, learning_rate=0.01):
    """One step of plain gradient descent per batch of ``(inputs, y, w)`` (what the fixture's fit uses: Adam would turn
    the rounding of the zero gradient of a block's convolution bias into steps of the full rate); the per-step losses."""
    opt = torch.optim.SGD(model.parameters(), lr=learning_rate)
    losses = []
    model.train()
    for inputs, y, w in batches:
        opt.zero_grad()
        loss = loss_fn("regression", model(inputs), y, w)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    return losses


# ------------------------------------------------------------------------------------------------ graphs
class Graph:
    """A GraphData stand-in: node_features, edge_index."""

    def __init__(self, node_features, edge_index):
        self.node_features, self.edge_index = node_features, edge_index
        self.num_nodes, self.num_edges = node_features.shape[0], edge_index.shape[1]


def two_shells():
    """The 19 axial offsets (q, r) within hexagonal distance 2, the site itself first, by distance then by (q, r)."""
    cells = [(q, r) for q in range(-2, 3) for r in range(-2, 3) if max(abs(q), abs(r), abs(q + r)) <= 2]
    return sorted(cells, key=lambda c: (max(abs(c[0]), abs(c[1]), abs(c[0] + c[1])), c))


def torus_table(a, b, P=6, K=19):
    """nbr (a * b, P, K) of the a x b periodic triangular lattice: permutation p turns the K offsets by p * 60 degrees."""
    cells = two_shells()[:K]
    nbr = np.zeros((a * b, P, K), np.int64)
    for p in range(P):
        for j, (q, r) in enumerate(cells):
            for _ in range(p):
                q, r = -r, q + r
            for sq in range(a):
                for sr in range(b):
                    nbr[sq * b + sr, p, j] = ((sq + q) % a) * b + (sr + r) % b
    return nbr


def edges_of(nbr):
    """edge_index [u, v] of a neighbour table, as LCNNFeaturizer lays it out: v = arange(n).repeat(P * K)."""
    n = nbr.shape[0]
    return np.stack([nbr.reshape(-1), np.arange(n).repeat(nbr.shape[1] * nbr.shape[2])]).astype(np.int64)


def one_hot(rng, n, F):
    return np.eye(F)[rng.randint(0, F, n)]


def torus(rng, a, b, F=3, P=6, K=19, features=None):
    nbr = torus_table(a, b, P, K)
    return Graph(one_hot(rng, a * b, F) if features is None else features(rng, a * b, F), edges_of(nbr))


def random_sites(rng, n, P, K, F, lonely=False):
    """Every entry a random site; ``lonely``: the last site is nobody's neighbour."""
    nbr = rng.randint(0, n - 1 if lonely and n > 1 else n, (n, P, K))
    return Graph(rng.normal(0, 1, (n, F)), edges_of(nbr))


def hub_sites(rng, n, P, K, F):
    """Site 0 fills slot 0 of every (v, p): a reverse list of n * P entries."""
    nbr = rng.randint(0, n, (n, P, K))
    nbr[:, :, 0] = 0
    return Graph(rng.normal(0, 1, (n, F)), edges_of(nbr))


def table_of(graph, P, K):
    """nbr (n, P, K) of a graph whose edges arrive grouped by destination or not (a stable sort by destination)."""
    u, v = np.asarray(graph.edge_index)
    return u[np.argsort(v, kind="stable")].reshape(graph.num_nodes, P, K)


def pack(graphs, P, K):
    """(x, nbr (N, P, K), node_ptr) of the concatenated graphs."""
    ptr = np.concatenate([[0], np.cumsum([g.num_nodes for g in graphs])])
    return (np.concatenate([g.node_features for g in graphs]),
            np.concatenate([table_of(g, P, K) + at for g, at in zip(graphs, ptr)]), ptr)


def fixture_graphs(F=3, K=19):
    """The 20 graphs of the model fixtures: small tori with one-hot occupancies, none of width 1 (there all permutations
    of a site coincide, the variance over them is zero and BatchNorm multiplies rounding by 1 / sqrt(eps))."""
    rng = np.random.RandomState(5)
    shapes = [(3, 3), (2, 3), (3, 4), (4, 2), (3, 2), (2, 5), (4, 3), (2, 6), (3, 3), (5, 2)] * 2
    return [torus(rng, a, b, F, 6, K) for a, b in shapes]
