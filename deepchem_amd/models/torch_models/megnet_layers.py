"""``GraphNetwork`` (the block of MEGNet) and ``Set2Set`` with the interface and the state-dict keys of the reference's
``deepchem/models/torch_models/layers.py`` and of torch_geometric's ``Set2Set``.

Two routes through ``GraphNetwork``.  The TORCH ROUTE follows the reference's own order: the doubled edge list of an
undirected graph, the concatenated rows, three scatter-means.  The NATIVE ROUTE (CUDA tensors, nodes sorted by graph,
edges grouped by graph) splits ``edge_models[0].weight`` by columns into ``A_s | A_d | C | D``, takes the four plain
products ``P = x [A_s; A_d]^T``, ``Q = e C^T``, ``R = u D^T + b1`` and leaves everything between the products to
``csrc/megnet.hip`` on rows of the hidden width 32: no tensor with 2E rows, none of a concatenated width, no copy of
the edge list or the edge features, no atomics.  ``last_route`` says which one ran.

Where the routes and the reference differ: a node without an arriving edge, and a graph without an edge, get a ZERO
mean row here (not ``edge_dense.bias``).  torch_geometric's ``scatter`` gives the same row when such a node or graph
is in the middle, and a shorter result (so the reference raises in ``torch.cat``) when it is the last one.
"""
from typing import Optional

import numpy as np
import torch
import torch.nn as nn

from deepchem_amd import ops
from deepchem_amd.models.torch_models.functions import AttendFn, LstmCellFn

HIDDEN = ops.GN_WIDTH


def scatter_mean(src: torch.Tensor, index: torch.Tensor, n: int) -> torch.Tensor:
    """Row means of ``src`` by ``index`` into ``n`` rows; a zero row where nothing arrives."""
    out = src.new_zeros((n, src.shape[1])).index_add_(0, index, src)
    count = src.new_zeros(n).index_add_(0, index, src.new_ones(index.shape[0]))
    return out / count.clamp(min=1).unsqueeze(1)


class GraphNetwork(nn.Module):
    """One graph-network block (Battaglia et al. 2018): updated node, edge and global features."""

    def __init__(self, n_node_features: int = 32, n_edge_features: int = 32, n_global_features: int = 32,
                 is_undirected: bool = True, residual_connection: bool = True):
        super().__init__()
        self.n_node_features, self.n_edge_features, self.n_global_features = n_node_features, n_edge_features, n_global_features
        self.is_undirected, self.residual_connection = is_undirected, residual_connection
        self.edge_models, self.node_models, self.global_models = nn.ModuleList(), nn.ModuleList(), nn.ModuleList()
        self.edge_models.append(nn.Linear(n_node_features * 2 + n_edge_features + n_global_features, HIDDEN))
        self.node_models.append(nn.Linear(n_node_features + n_edge_features + n_global_features, HIDDEN))
        self.global_models.append(nn.Linear(n_node_features + n_edge_features + n_global_features, HIDDEN))
        self.edge_dense = nn.Linear(HIDDEN, n_edge_features)
        self.node_dense = nn.Linear(HIDDEN, n_node_features)
        self.global_dense = nn.Linear(HIDDEN, n_global_features)
        self.last_route = None

    def reset_parameters(self) -> None:
        for m in (self.edge_dense, self.node_dense, self.global_dense, *self.edge_models, *self.node_models,
                  *self.global_models):
            m.reset_parameters()

    def _check(self, x, e, u):
        if x.dim() != 2 or e.dim() != 2 or u.dim() != 2 or x.shape[1] != self.n_node_features or \
                e.shape[1] != self.n_edge_features or u.shape[1] != self.n_global_features:
            raise ValueError("GraphNetwork: node, edge and global features of widths %d, %d, %d expected, got %s, %s, %s" %
                             (self.n_node_features, self.n_edge_features, self.n_global_features, tuple(x.shape),
                              tuple(e.shape), tuple(u.shape)))

    # ---- the reference's order
    def forward_torch(self, x, edge_index, e, u, batch):
        src, dst = edge_index[0].long(), edge_index[1].long()
        batch = batch.long()
        n_edges = e.shape[0]
        x0, e0, u0 = x, e, u
        if self.is_undirected:
            src, dst = torch.cat((src, dst)), torch.cat((dst, src))
            e = torch.cat((e, e), dim=0)
        edge_graph = batch[src]
        e = self.edge_dense(self.edge_models[0](torch.cat((x[src], x[dst], e, u[edge_graph]), dim=1)))
        m = scatter_mean(e, dst, x.shape[0])
        x = self.node_dense(self.node_models[0](torch.cat((x, m, u[batch]), dim=1)))
        u = self.global_dense(self.global_models[0](torch.cat((scatter_mean(e, edge_graph, u.shape[0]),
                                                               scatter_mean(x, batch, u.shape[0]), u), dim=1)))
        if self.is_undirected:
            e = (e[:n_edges] + e[n_edges:]) / 2
        if self.residual_connection:
            e, x, u = e + e0, x + x0, u + u0
        return x, e, u

    # ---- the split algebra on csrc/megnet.hip
    def forward_native(self, x, e, u, g: "ops.GnGraph"):
        Fn, Fe = self.n_node_features, self.n_edge_features
        W1, b1 = self.edge_models[0].weight, self.edge_models[0].bias
        Wn, Wg = self.node_models[0].weight, self.global_models[0].weight
        W2t, b2 = self.edge_dense.weight.t(), self.edge_dense.bias
        node_mask, graph_mask = g.masks
        P = x @ torch.cat((W1[:, :Fn], W1[:, Fn:2 * Fn]), dim=0).t()  # [Ps | Pd]: a (64, Fn) weight, N rows
        Q = e @ W1[:, 2 * Fn:2 * Fn + Fe].t()
        R = torch.addmm(b1, u, W1[:, 2 * Fn + Fe:].t())
        Hs = ops.GnEdgeFn.apply(P, Q, R, g)
        Mh = ops.GnNodeFn.apply(P, Q, R, g)
        e_new = torch.addmm(b2, Hs, W2t)  # already the halved sum of both directions
        m = torch.addmm(b2, Mh, W2t) * node_mask
        un = torch.addmm(self.node_models[0].bias, u, Wn[:, Fn + Fe:].t())
        hn = ops.GnSegSpreadFn.apply(un, g.node_ptr, g.n_nodes).addmm(x, Wn[:, :Fn].t()).addmm(m, Wn[:, Fn:Fn + Fe].t())
        x_new = self.node_dense(hn)
        ebar = torch.addmm(b2, ops.GnSegMeanFn.apply(Hs, g.edge_ptr), W2t) * graph_mask
        nbar = ops.GnSegMeanFn.apply(x_new, g.node_ptr)
        hg = torch.addmm(self.global_models[0].bias, u, Wg[:, Fe + Fn:].t()).addmm(ebar, Wg[:, :Fe].t()) \
            .addmm(nbar, Wg[:, Fe:Fe + Fn].t())
        u_new = self.global_dense(hg)
        if self.residual_connection:
            e_new, x_new, u_new = e_new + e, x_new + x, u_new + u
        return x_new, e_new, u_new

    def native_covers(self, x, e, u, graph) -> bool:
        return isinstance(graph, ops.GnGraph) and graph.ref is not None and x.is_cuda and e.is_cuda and u.is_cuda and \
            x.dtype == e.dtype == u.dtype == torch.float32 and graph.undirected == bool(self.is_undirected) and \
            graph.n_nodes == x.shape[0] and graph.n_edges == e.shape[0] and graph.n_graphs == u.shape[0]

    def forward(self, node_features, edge_index, edge_features, global_features, batch: Optional[torch.Tensor] = None,
                graph: Optional["ops.GnGraph"] = None):
        """``edge_index`` (2, E) and ``batch`` as in the reference; ``graph``: the prebuilt ``ops.GnGraph`` of the same
        batch (then ``edge_index`` and ``batch`` are only read by the torch route and may be None on the native one).
        Without one, CUDA inputs get a ``GnGraph`` built here (one read-back of ``edge_index``); batches it cannot
        describe (nodes not sorted by graph, edges not grouped by graph) take the torch route."""
        x, e, u = node_features, edge_features, global_features
        self._check(x, e, u)
        if graph is None and x.is_cuda and x.dtype == torch.float32:
            b = np.zeros(x.shape[0], np.int64) if batch is None else batch.detach().cpu().numpy()
            try:
                graph = ops.GnGraph(edge_index.detach().cpu().numpy(), b, u.shape[0], bool(self.is_undirected), x.device)
            except ValueError:
                graph = None
        if self.native_covers(x, e, u, graph):
            self.last_route = "native"
            return self.forward_native(x, e, u, graph)
        self.last_route = "torch"
        if edge_index is None:
            edge_index = torch.stack((graph.src, graph.dst))
            batch = graph.node_graph
        if batch is None:
            batch = x.new_zeros(x.shape[0], dtype=torch.int64)
        return self.forward_torch(x, edge_index, e, u, batch)

    def __repr__(self) -> str:
        fields = ("n_node_features", "n_edge_features", "n_global_features", "is_undirected", "residual_connection")
        return "%s(%s)" % (type(self).__name__, ", ".join("%s=%s" % (k, getattr(self, k)) for k in fields))


class Set2Set(nn.Module):
    """Set2Set readout (Vinyals et al. 2016) as torch_geometric defines it: ``q_star`` (sets, 2 C) after
    ``processing_steps`` rounds of ``q, h = LSTM(q_star, h)``, ``a = softmax_set(<x, q>)``, ``r = sum_set a x``,
    ``q_star = [q | r]``.  The parameters live in the ``nn.LSTM`` submodule ``lstm`` (keys ``lstm.weight_ih_l0`` ...).
    A set without rows reads out ``r = 0``.  ``forward(x, index)`` with the set of every row; ``ptr`` (int32 offsets of
    the sorted sets, on the GPU) selects the kernels ``gcmi_set2set_attend`` / ``gcmi_lstm_cell``."""

    MAX_NATIVE_CHANNELS = 512

    def __init__(self, in_channels: int, processing_steps: int, num_layers: int = 1):
        super().__init__()
        self.in_channels, self.out_channels = in_channels, 2 * in_channels
        self.processing_steps, self.num_layers = processing_steps, num_layers
        self.lstm = nn.LSTM(self.out_channels, in_channels, num_layers)

    def native_covers(self, x, ptr) -> bool:
        return ptr is not None and x.is_cuda and x.dtype == torch.float32 and self.num_layers == 1 and \
            self.in_channels <= self.MAX_NATIVE_CHANNELS

    def forward(self, x, index=None, n_sets: Optional[int] = None, ptr: Optional[torch.Tensor] = None):
        C = self.in_channels
        if self.native_covers(x, ptr):
            B = ptr.numel() - 1
            # nn.LSTM orders its gates i, f, g, o; the cell kernel takes i, f, o, g
            perm = torch.cat((torch.arange(0, 2 * C), torch.arange(3 * C, 4 * C), torch.arange(2 * C, 3 * C))).to(x.device)
            w_ih, w_hh = self.lstm.weight_ih_l0.index_select(0, perm), self.lstm.weight_hh_l0.index_select(0, perm)
            bias = (self.lstm.bias_ih_l0 + self.lstm.bias_hh_l0).index_select(0, perm)
            q_star = x.new_zeros((B, 2 * C))
            h, c = x.new_zeros((B, C)), x.new_zeros((B, C))
            for _ in range(self.processing_steps):
                z = torch.addmm(bias, q_star, w_ih.t()).addmm(h, w_hh.t())
                h, c = LstmCellFn.apply(z, c)
                q_star = AttendFn.apply(x, h, ptr) if x.shape[0] else torch.cat((h, torch.zeros_like(h)), dim=1)
            return q_star
        if index is None:
            counts = (ptr[1:] - ptr[:-1]).long()
            index = torch.repeat_interleave(torch.arange(counts.numel(), device=x.device), counts)
        index = index.long()
        B = int(n_sets) if n_sets is not None else (ptr.numel() - 1 if ptr is not None else int(index.max()) + 1)
        hc = (x.new_zeros((self.num_layers, B, C)), x.new_zeros((self.num_layers, B, C)))
        q_star = x.new_zeros((B, 2 * C))
        for _ in range(self.processing_steps):
            q, hc = self.lstm(q_star.unsqueeze(0), hc)
            q = q.view(B, C)
            score = (x * q[index]).sum(dim=-1)
            top = score.new_full((B,), float("-inf")).scatter_reduce(0, index, score, "amax", include_self=True)
            w = torch.exp(score - top[index])
            w = w / score.new_zeros(B).index_add_(0, index, w)[index]
            r = x.new_zeros((B, C)).index_add_(0, index, w.unsqueeze(1) * x)
            q_star = torch.cat((q, r), dim=-1)
        return q_star

    def __repr__(self) -> str:
        return f'{self.__class__.__name__}({self.in_channels}, {self.out_channels})'
