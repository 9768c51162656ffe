"""``MEGNet`` / ``MEGNetModel``: the MatErials Graph Network (Chen et al. 2019) with the interface of the reference's
``deepchem/models/torch_models/megnet.py``: constructor arguments, ``L2Loss`` with ``["prediction"]`` or
``SparseSoftmaxCrossEntropy`` with ``["prediction", "loss"]``, ``default_generator`` (an object array of ``GraphData``,
each with ``global_features`` of shape ``(1, Fg)``) and the reference's state-dict keys (``megnet_blocks.{i}.*``,
``set2set_nodes.lstm.*``, ``set2set_edges.lstm.*``, ``dense.0``, ``dense.1``, ``out``).

``_prepare_batch`` turns the graphs of a batch into a ``MegnetBatch``: nodes, edges and global rows concatenated, the
index lists of ``ops.GnGraph`` built once on the host, everything uploaded in one packed transfer.  On the GPU the
blocks run on ``csrc/megnet.hip`` and the two readouts on the set2set kernels (the NATIVE ROUTE); on the CPU, and for
anything the native route declines, the same batch runs through torch ops in the reference's order (the TORCH ROUTE).
``model.last_route`` says which route the last batch took; ``MEGNetModel(..., route="torch")`` forces the second.
"""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from deepchem_amd import ops
from deepchem_amd.models.losses import L2Loss, SparseSoftmaxCrossEntropy
from deepchem_amd.models.torch_models.megnet_layers import GraphNetwork, Set2Set
from deepchem_amd.models.torch_models.torch_model import TorchModel


class MegnetBatch:
    """One batch: ``x`` (nodes, Fn), ``edge_attr`` (edges, Fe), ``global_features`` (graphs, Fg) and ``graph``
    (``ops.GnGraph``: ``src``, ``dst``, ``node_graph`` = the reference's ``batch``, offsets and incidence lists), all
    from ONE upload.  Indexing by the reference's names (``batch['x']`` ...) works."""

    def __init__(self, graphs, is_undirected: bool, device):
        graphs = list(graphs)
        if not graphs:
            raise ValueError("MegnetBatch: no graphs")
        xs, es, us, idx, at = [], [], [], [], 0
        for k, gr in enumerate(graphs):
            if not all(hasattr(gr, a) for a in ("node_features", "edge_index", "edge_features")):
                raise ValueError("MEGNetModel takes GraphData objects, got %r" % type(gr))
            u = getattr(gr, "global_features", None)
            if u is None:
                raise ValueError("MEGNetModel: graph %d has no global_features (GraphData(..., global_features=array "
                                 "of shape (1, n_global_features)))" % k)
            u = np.asarray(u, np.float32)
            if u.ndim != 2 or u.shape[0] != 1:
                raise ValueError("MEGNetModel: global_features of graph %d must have shape (1, n_global_features), got %s" %
                                 (k, u.shape))
            if gr.edge_features is None:
                raise ValueError("MEGNetModel: graph %d has no edge_features" % k)
            x, e = np.asarray(gr.node_features, np.float32), np.asarray(gr.edge_features, np.float32)
            xs.append(x), es.append(e), us.append(u)
            idx.append(np.asarray(gr.edge_index, np.int64) + at)
            at += x.shape[0]
        for name, rows in (("node_features", xs), ("edge_features", es), ("global_features", us)):
            if any(r.ndim != 2 or r.shape[1] != rows[0].shape[1] for r in rows):
                raise ValueError("MEGNetModel: the %s of a batch must be 2-D with one width" % name)
        batch = np.repeat(np.arange(len(graphs)), [x.shape[0] for x in xs])
        self.graph = ops.GnGraph(np.concatenate(idx, axis=1), batch, len(graphs), is_undirected, device,
                                 floats=(np.concatenate(xs), np.concatenate(es), np.concatenate(us)))
        self.x, self.edge_attr, self.global_features = self.graph.floats
        self.n_graphs = len(graphs)

    def __getitem__(self, key):
        if key == "edge_index":
            return torch.stack((self.graph.src, self.graph.dst))
        if key == "batch":
            return self.graph.node_graph
        if key in ("x", "edge_attr", "global_features"):
            return getattr(self, key)
        raise KeyError(key)


class MEGNet(nn.Module):
    """The reference's module: ``n_blocks`` GraphNetwork blocks, a Set2Set readout over the nodes and one over the
    edges, two linear layers and the output layer."""

    def __init__(self, n_node_features: int = 32, n_edge_features: int = 32, n_global_features: int = 32,
                 n_blocks: int = 1, is_undirected: bool = True, residual_connection: bool = True,
                 mode: str = 'regression', n_classes: int = 2, n_tasks: int = 1):
        super(MEGNet, self).__init__()
        if mode not in ['classification', 'regression']:
            raise ValueError("mode must be either 'classification' or 'regression'")
        self.n_node_features, self.n_edge_features, self.n_global_features = n_node_features, n_edge_features, n_global_features
        self.megnet_blocks = nn.ModuleList()
        self.n_blocks = n_blocks
        self.is_undirected = is_undirected
        for _ in range(n_blocks):
            self.megnet_blocks.append(GraphNetwork(n_node_features=n_node_features, n_edge_features=n_edge_features,
                                                   n_global_features=n_global_features, is_undirected=is_undirected,
                                                   residual_connection=residual_connection))
        self.n_tasks, self.mode, self.n_classes = n_tasks, mode, n_classes
        self.set2set_nodes = Set2Set(in_channels=n_node_features, processing_steps=3, num_layers=1)
        self.set2set_edges = Set2Set(in_channels=n_edge_features, processing_steps=3, num_layers=1)
        self.dense = nn.Sequential(nn.Linear(2 * n_node_features + 2 * n_edge_features + n_global_features, 32),
                                   nn.Linear(32, 16))
        self.out = nn.Linear(16, n_tasks if mode == 'regression' else n_tasks * n_classes)
        self.route = "auto"  # "torch": never the native route
        self.last_route = None

    def native_covers(self, b: MegnetBatch) -> bool:
        return self.route != "torch" and b.graph.ref is not None and b.graph.undirected == bool(self.is_undirected) and \
            self.set2set_nodes.native_covers(b.x, b.graph.node_ptr) and \
            self.set2set_edges.native_covers(b.edge_attr, b.graph.edge_ptr)

    def forward(self, pyg_batch):
        b = pyg_batch
        if not isinstance(b, MegnetBatch):
            raise ValueError("MEGNet takes a MegnetBatch (MegnetBatch(graphs, is_undirected, device))")
        g = b.graph
        x, e, u = b.x, b.edge_attr, b.global_features
        if self.native_covers(b):
            self.last_route = "native"
            for block in self.megnet_blocks:
                x, e, u = block(x, None, e, u, graph=g)
            nodes_q = self.set2set_nodes(x, ptr=g.node_ptr)
            edges_q = self.set2set_edges(e, ptr=g.edge_ptr)
        else:
            self.last_route = "torch"
            edge_index, batch = b["edge_index"].long(), g.node_graph.long()
            for block in self.megnet_blocks:
                x, e, u = block.forward_torch(x, edge_index, e, u, batch)
                block.last_route = "torch"
            nodes_q = self.set2set_nodes(x, batch, n_sets=b.n_graphs)
            edges_q = self.set2set_edges(e, batch[edge_index[0]], n_sets=b.n_graphs)
        out = self.out(self.dense(torch.cat([nodes_q, edges_q, u], dim=1)))
        if self.mode == 'classification':
            if self.n_tasks == 1:
                logits, softmax_dim = out.view(-1, self.n_classes), 1
            else:
                logits, softmax_dim = out.view(-1, self.n_tasks, self.n_classes), 2
            return F.softmax(logits, dim=softmax_dim), logits
        return out


class MEGNetModel(TorchModel):
    """MatErials Graph Network for molecules and crystals, on datasets of ``GraphData`` with ``global_features``."""

    def __init__(self, n_node_features: int = 32, n_edge_features: int = 32, n_global_features: int = 32,
                 n_blocks: int = 1, is_undirected: bool = True, residual_connection: bool = True,
                 mode: str = 'regression', n_classes: int = 2, n_tasks: int = 1, route: str = "auto", **kwargs):
        if route not in ("auto", "torch"):
            raise ValueError("route must be 'auto' or 'torch'")
        model = MEGNet(n_node_features=n_node_features, n_edge_features=n_edge_features,
                       n_global_features=n_global_features, n_blocks=n_blocks, is_undirected=is_undirected,
                       residual_connection=residual_connection, mode=mode, n_classes=n_classes, n_tasks=n_tasks)
        model.route = route
        if mode == 'regression':
            loss, output_types = L2Loss(), ['prediction']
        else:
            loss, output_types = SparseSoftmaxCrossEntropy(), ['prediction', 'loss']
        super(MEGNetModel, self).__init__(model, loss=loss, output_types=output_types, **kwargs)

    @property
    def last_route(self):
        return self.model.last_route

    def _prepare_batch(self, batch):
        """The graphs of ``default_generator`` (an object array nested in a list) become one ``MegnetBatch``."""
        graphs, labels, weights = batch
        if not isinstance(graphs, MegnetBatch):
            graphs = MegnetBatch(graphs[0], self.model.is_undirected, self.device)
            m = self.model
            got = (graphs.x.shape[1], graphs.edge_attr.shape[1], graphs.global_features.shape[1])
            if got != (m.n_node_features, m.n_edge_features, m.n_global_features):
                raise ValueError("MEGNetModel: node, edge and global widths %s, the model was built for %s" %
                                 (got, (m.n_node_features, m.n_edge_features, m.n_global_features)))
        return (graphs, [self._to_device(x) for x in labels or ()], [self._to_device(x) for x in weights or ()])
