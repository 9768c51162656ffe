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
* ``site_fwd_ref``, ``site_bwd_ref``, ``rev_sum_ref``, ``running_ref``  the four ops of csrc/lcnn.hip one by one, from Y
                    (no product ahead of them), in a chosen precision and slot order; ``op_case`` / ``op_references``:
                    the inputs of an op-level case and the float64 values with the float32 restatements' errors.
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


# ------------------------------------------------------------------------------------------------ the ops one by one
SLOT_ORDERS = ("asc", "desc")
OP_NAMES = ("out", "X", "dX", "dgamma", "dbeta", "db", "dY", "rm", "rv")


def _g(a, dtype):
    """``a`` in ``dtype``; a tensor that already has it passes through (so a leaf keeps its place in the graph)."""
    return a if torch.is_tensor(a) and a.dtype == dtype else _t(a, dtype)


def site_fwd_ref(Y, nbr, bias, gamma, beta, mask, mean, var, eps, dtype, slot_order="asc"):
    """lc_site_fwd: (out (N, O), X (N, P, O)) from Y (N, K * O).  X[v, p] = bias + sum_j Y[nbr[v, p, j], j] with j
    ascending (``"asc"``, what the kernel does) or descending; ``mean`` None: training, each site's own mean and biased
    variance over its P rows; ``mask`` (N, P) or None (ones); ``bias`` None: zero."""
    nbr = torch.as_tensor(np.asarray(nbr), dtype=torch.int64)
    N, P, K = nbr.shape
    gamma, beta = _g(gamma, dtype), _g(beta, dtype)
    O = gamma.numel()
    Y = _g(Y, dtype).reshape(N, K, O)
    X = (torch.zeros(O, dtype=dtype) if bias is None else _g(bias, dtype)).expand(N, P, O)
    for j in (range(K) if slot_order == "asc" else range(K - 1, -1, -1)):
        X = X + Y[nbr[:, :, j], j]
    if mean is None:
        mu, v = X.mean(1, keepdim=True), X.var(1, unbiased=False, keepdim=True)
    else:
        mu, v = _g(mean, dtype), _g(var, dtype)
    Xhat = (X - mu) / torch.sqrt(v + eps) * gamma + beta
    return (Xhat.sum(1) if mask is None else (_g(mask, dtype).unsqueeze(2) * Xhat).sum(1)), X


def site_bwd_ref(Y, nbr, bias, gamma, beta, mask, mean, var, eps, dout, dtype, slot_order="asc"):
    """lc_site_bwd by autograd on ``site_fwd_ref`` with respect to X: (dX (N, P, O), dgamma, dbeta, db) for the output
    gradient ``dout`` (N, O)."""
    gamma, beta = (_t(a, dtype).clone().requires_grad_(True) for a in (gamma, beta))
    b = (torch.zeros(gamma.numel(), dtype=dtype) if bias is None else _t(bias, dtype).clone()).requires_grad_(True)
    out, X = site_fwd_ref(Y, nbr, b, gamma, beta, mask, mean, var, eps, dtype, slot_order)
    dX, dgamma, dbeta, db = torch.autograd.grad((out * _t(dout, dtype)).sum(), [X, gamma, beta, b])
    return dX, dgamma, dbeta, db


def rev_sum_ref(dX, nbr, dtype, slot_order="asc"):
    """lc_rev_sum: dY (N, K * O), dY[u, j] = the sum of dX[v, p] over the (v, p) with nbr[v, p, j] = u, one term after the
    other in ascending order of v * P + p (``"asc"``, the kernel's list order) or descending."""
    nbr = np.asarray(nbr, np.int64)
    N, P, K = nbr.shape
    rows = _t(dX, dtype).numpy().reshape(N * P, -1)
    out = np.zeros((N, K, rows.shape[1]), rows.dtype)
    step = 1 if slot_order == "asc" else -1
    for j in range(K):
        np.add.at(out[:, j], nbr[:, :, j].reshape(-1)[::step], rows[::step])  # (unbuffered: in index order)
    return torch.as_tensor(out.reshape(N, -1))


def running_ref(X, rm0, rv0, momentum, dtype):
    """lc_running: the literal loop of the N per-site BatchNorm updates in site order, in ``dtype`` throughout: the mean
    and the unbiased variance over the P rows of site v, then r = (1 - m) r + m s for both."""
    X = _t(X, dtype)
    rm, rv = _t(rm0, dtype).clone(), _t(rv0, dtype).clone()
    P = X.shape[1]
    for v in range(X.shape[0]):
        mean = X[v].sum(0) / P
        var = ((X[v] - mean) ** 2).sum(0) / (P - 1)
        rm = (1 - momentum) * rm + momentum * mean
        rv = (1 - momentum) * rv + momentum * var
    return rm, rv


_OP_CASES = {}
# cases whose two float32 slot orders lay more than 4 times apart at the first seed (on the CPU, before any GPU run):
# the seed of their values moved on, the sites stay
OP_RESEED = {}


def op_case(O, P, K, n_sites, training):
    """The inputs of one op-level case (cached): random sites, Y drawn N(0, 1) directly, gamma in [0.5, 1.5], the mask
    of the block tests (kept rows / 0.8 in training, ones in eval)."""
    key = (O, P, K, n_sites, bool(training))
    if key not in _OP_CASES:
        seed = 7 + O + 64 * (P + 8 * (K + 32 * (n_sites % 9973)))
        graph = random_sites(np.random.RandomState(seed), n_sites, P, K, 1)
        rng = np.random.RandomState(seed + 1 + OP_RESEED.get((O, P, K, n_sites), 0))
        f = lambda a: a.astype(np.float32)  # noqa: E731
        c = dict(O=O, P=P, K=K, N=n_sites, training=bool(training), graph=graph, nbr=table_of(graph, P, K),
                 Y=f(rng.normal(0, 1, (n_sites, K * O))), b=f(rng.normal(0, 0.3, O)), gamma=f(rng.uniform(0.5, 1.5, O)),
                 beta=f(rng.normal(0, 0.3, O)), rm=f(rng.normal(0, 0.3, O)), rv=f(rng.uniform(0.5, 2, O)),
                 cot=f(rng.normal(0, 1, (n_sites, O))))
        c["mask"] = f((rng.rand(n_sites, P) >= 0.2) / 0.8) if training else np.ones((n_sites, P), np.float32)
        _OP_CASES[key] = c
    return _OP_CASES[key]


def op_chain(c, dtype, slot_order):
    """The four ops one after the other on a case, as the GPU test calls them: forward, backward of ``cot``, reverse
    sum of dX, and in training the running statistics from X.  Float64 arrays by ``OP_NAMES``."""
    stats = (None, None) if c["training"] else (c["rm"], c["rv"])
    args = (c["Y"], c["nbr"], c["b"], c["gamma"], c["beta"], c["mask"]) + stats + (EPS,)
    out, X = site_fwd_ref(*args, dtype, slot_order)
    dX, dgamma, dbeta, db = site_bwd_ref(*args, c["cot"], dtype, slot_order)
    dY = rev_sum_ref(dX, c["nbr"], dtype, slot_order)
    rm, rv = running_ref(X, c["rm"], c["rv"], MOMENTUM, dtype) if c["training"] else (_t(c["rm"], dtype), _t(c["rv"], dtype))
    vals = (out, X, dX, dgamma, dbeta, db, dY, rm, rv)
    return {n: v.detach().double().numpy() for n, v in zip(OP_NAMES, vals)}


def op_references(c):
    """(float64 values by name, e32 by name: the larger error of the float32 chains in the two slot orders, and the
    largest ratio between the two orders' errors over the tensors), cached on the case."""
    if "refs" not in c:
        want = op_chain(c, torch.float64, "asc")
        errs = {n: [] for n in OP_NAMES}
        for order in SLOT_ORDERS:
            got = op_chain(c, torch.float32, order)
            for n in OP_NAMES:
                errs[n].append(float(np.max(np.abs(got[n] - want[n]))))
        spread = max([max(e) / max(min(e), 1e-300) for e in errs.values() if max(e) > 0] or [1.0])
        c["refs"] = (want, {n: max(e) for n, e in errs.items()}, spread)
    return c["refs"]


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
