"""``CGCNN`` / ``CGCNNModel``: the Crystal Graph Convolutional Neural Network (Xie & Grossman 2018) with the interface of
the reference's ``deepchem/models/torch_models/cgcnn.py``: constructor arguments and defaults, ``L2Loss`` with
``["prediction"]`` or ``SparseSoftmaxCrossEntropy`` with ``["prediction", "loss"]``, ``default_generator`` (an object
array of ``GraphData`` with edge features) and the reference's state-dict keys (``embedding.*``,
``conv_layers.{i}.linear.*``, ``conv_layers.{i}.batch_norm.*``, ``fc.*``, ``out.*``), so a reference checkpoint loads.

``_prepare_batch`` turns the graphs of a batch into a ``CgcnnBatch``: nodes and edges concatenated, the arriving and
leaving lists of a DIRECTED ``ops.GnGraph`` built once on the host, everything uploaded in one packed transfer.  On the
GPU, with ``hidden_node_dim`` a multiple of 4 in [4, 128], the layers run on ``csrc/cgcnn.hip`` and the readout on the
segment-mean kernel (the NATIVE ROUTE); on the CPU, at other widths and with ``route="torch"`` the same batch runs
through torch ops in the reference's order (the TORCH ROUTE).  ``model.last_route`` says which route the last batch took.

Where this differs from the reference on purpose (``cgcnn_layers`` and DESIGN section 8): a node without an arriving
edge gets a zero row; the class probabilities are the softmax over the CLASS axis, of shape ``(B, n_classes)`` for one
task and ``(B, n_tasks, n_classes)`` otherwise (the reference squeezes the logits and calls ``softmax`` without ``dim``,
which drops the batch axis of a one-graph batch and normalises over the batch for several tasks); a training batch with
fewer than two edges raises ``ValueError`` before anything runs.
"""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from deepchem_amd import ops
from deepchem_amd.models.losses import L2Loss, SparseSoftmaxCrossEntropy
from deepchem_amd.models.torch_models.cgcnn_layers import CGCNNLayer
from deepchem_amd.models.torch_models.functions import linear
from deepchem_amd.models.torch_models.torch_model import TorchModel


class CgcnnBatch:
    """One batch: ``x`` (nodes, Fn), ``edge_attr`` (edges, Fe) and ``graph`` (a directed ``ops.GnGraph``: ``src``, ``dst``,
    ``node_graph``, offsets, arriving and leaving lists), all from ONE upload."""

    def __init__(self, graphs, device):
        graphs = list(graphs)
        if not graphs:
            raise ValueError("CgcnnBatch: no graphs")
        xs, es, idx = [], [], []
        for k, gr in enumerate(graphs):
            if not all(hasattr(gr, a) for a in ("node_features", "edge_index", "edge_features")):
                raise ValueError("CGCNNModel takes GraphData objects, got %r" % type(gr))
            if gr.edge_features is None:
                raise ValueError("CGCNNModel: graph %d has no edge_features" % k)
            xs.append(np.asarray(gr.node_features, np.float32)), es.append(np.asarray(gr.edge_features, np.float32))
            idx.append(np.asarray(gr.edge_index, np.int64).reshape(2, -1))
            if es[-1].ndim != 2 or es[-1].shape[0] != idx[-1].shape[1]:
                raise ValueError("CGCNNModel: edge_features of graph %d needs one row per edge of edge_index" % k)
        for name, rows in (("node_features", xs), ("edge_features", es)):
            if any(r.ndim != 2 or r.shape[1] != rows[0].shape[1] for r in rows):
                raise ValueError("CGCNNModel: the %s of a batch must be 2-D with one width" % name)
        node_ptr = np.concatenate([[0], np.cumsum([x.shape[0] for x in xs])])
        batch = np.repeat(np.arange(len(graphs)), np.diff(node_ptr))
        self.graph = ops.GnGraph(np.concatenate([ei + at for ei, at in zip(idx, node_ptr)], axis=1), batch, len(graphs),
                                 False, device, floats=(np.concatenate(xs), np.concatenate(es)))
        self.x, self.edge_attr = self.graph.floats
        self.n_graphs = self.graph.n_graphs

    def __getitem__(self, key):
        if key == "edge_index":
            return torch.stack((self.graph.src, self.graph.dst))
        if key == "batch":
            return self.graph.node_graph
        if key in ("x", "edge_attr"):
            return getattr(self, key)
        raise KeyError(key)


class CGCNN(nn.Module):
    """The reference's module: an embedding, ``num_conv`` CGCNNLayers, the mean over the nodes of each graph and two
    linear layers, softplus in between."""

    def __init__(self, in_node_dim: int = 92, hidden_node_dim: int = 64, in_edge_dim: int = 41, num_conv: int = 3,
                 predictor_hidden_feats: int = 128, n_tasks: int = 1, mode: str = 'regression', n_classes: int = 2):
        super(CGCNN, self).__init__()
        if mode not in ['classification', 'regression']:
            raise ValueError("mode must be either 'classification' or 'regression'")
        self.n_tasks, self.mode, self.n_classes = n_tasks, mode, n_classes
        self.in_node_dim, self.hidden_node_dim, self.in_edge_dim = in_node_dim, hidden_node_dim, in_edge_dim
        self.embedding = nn.Linear(in_node_dim, hidden_node_dim)
        self.conv_layers = nn.ModuleList([CGCNNLayer(hidden_node_dim=hidden_node_dim, edge_dim=in_edge_dim, batch_norm=True)
                                          for _ in range(num_conv)])
        self.fc = nn.Linear(hidden_node_dim, predictor_hidden_feats)
        self.out = nn.Linear(predictor_hidden_feats, n_tasks if mode == 'regression' else n_tasks * n_classes)
        self.route = "auto"  # "torch": never the native route
        self.last_route = None

    def native_covers(self, b: CgcnnBatch) -> bool:
        return self.route != "torch" and b.graph.ref is not None and b.x.is_cuda and ops.cg_width_ok(self.hidden_node_dim)

    def forward(self, batch):
        b = batch
        if not isinstance(b, CgcnnBatch):
            raise ValueError("CGCNN takes a CgcnnBatch (CgcnnBatch(graphs, device))")
        g, e = b.graph, b.edge_attr
        if b.x.shape[1] != self.in_node_dim or e.shape[1] != self.in_edge_dim:
            raise ValueError("CGCNN: node and edge widths %s, the model was built for %s" %
                             ((b.x.shape[1], e.shape[1]), (self.in_node_dim, self.in_edge_dim)))
        if self.native_covers(b):
            self.last_route = "native"
            h = linear(b.x, self.embedding)
            for conv in self.conv_layers:
                h = conv(g, h, e)
            graph_feat = F.softplus(ops.GnSegMeanFn.apply(h, g.node_ptr))
            graph_feat = F.softplus(linear(graph_feat, self.fc))
            out = linear(graph_feat, self.out)
        else:
            self.last_route = "torch"
            src, dst, node_graph = g.src.long(), g.dst.long(), g.node_graph.long()
            h = self.embedding(b.x)
            for conv in self.conv_layers:
                conv._check(h, e, g.n_edges)
                h = conv.forward_torch(h, e, src, dst)
                conv.last_route = "torch"
            sums = h.new_zeros((b.n_graphs, h.shape[1])).index_add(0, node_graph, h)
            count = h.new_zeros(b.n_graphs).index_add(0, node_graph, h.new_ones(node_graph.shape[0]))
            graph_feat = F.softplus(sums / count.unsqueeze(1))
            graph_feat = F.softplus(self.fc(graph_feat))
            out = self.out(graph_feat)
        if self.mode == 'classification':
            if self.n_tasks == 1:
                logits, softmax_dim = out.view(-1, self.n_classes), 1
            else:
                logits, softmax_dim = out.view(-1, self.n_tasks, self.n_classes), 2
            return F.softmax(logits, dim=softmax_dim), logits
        return out


class CGCNNModel(TorchModel):
    """Crystal Graph Convolutional Neural Network on datasets of ``GraphData`` with edge features."""

    def __init__(self, in_node_dim: int = 92, hidden_node_dim: int = 64, in_edge_dim: int = 41, num_conv: int = 3,
                 predictor_hidden_feats: int = 128, n_tasks: int = 1, mode: str = 'regression', n_classes: int = 2,
                 route: str = "auto", **kwargs):
        if route not in ("auto", "torch"):
            raise ValueError("route must be 'auto' or 'torch'")
        model = CGCNN(in_node_dim, hidden_node_dim, in_edge_dim, num_conv, predictor_hidden_feats, n_tasks, mode, n_classes)
        model.route = route
        if mode == "regression":
            loss, output_types = L2Loss(), ['prediction']
        else:
            loss, output_types = SparseSoftmaxCrossEntropy(), ['prediction', 'loss']
        super(CGCNNModel, self).__init__(model, loss=loss, output_types=output_types, **kwargs)

    @property
    def last_route(self):
        return self.model.last_route

    def _prepare_batch(self, batch):
        """The graphs of ``default_generator`` (an object array nested in a list) become one ``CgcnnBatch``."""
        graphs, labels, weights = batch
        if not isinstance(graphs, CgcnnBatch):
            graphs = CgcnnBatch(graphs[0], self.device)
        return (graphs, [self._to_device(x) for x in labels or ()], [self._to_device(x) for x in weights or ()])
