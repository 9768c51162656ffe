"""``GraphData``: a molecule as plain arrays, with the contract of the reference's ``deepchem/feat/graph_data.py``
(attribute names, shapes and the ``ValueError``s of the constructor).  Only what ``DMPNNModel`` reads is here: no
conversion to other graph libraries, no batching class."""
from typing import Optional

import numpy as np


class GraphData(object):
    """``node_features`` (num_nodes, num_node_features); ``edge_index`` (2, num_edges) integers, source row first;
    ``edge_features`` (num_edges, num_edge_features) or None; ``node_pos_features`` (num_nodes, dims) or None.  Any
    further keyword (``global_features=...``) becomes an attribute of that name."""

    def __init__(self, node_features: np.ndarray, edge_index: np.ndarray, edge_features: Optional[np.ndarray] = None,
                 node_pos_features: Optional[np.ndarray] = None, **kwargs):
        if not isinstance(node_features, np.ndarray):
            raise ValueError('node_features must be np.ndarray.')
        if not isinstance(edge_index, np.ndarray):
            raise ValueError('edge_index must be np.ndarray.')
        if not issubclass(edge_index.dtype.type, np.integer):
            raise ValueError('edge_index.dtype must contains integers.')
        if edge_index.shape[0] != 2:
            raise ValueError('The shape of edge_index is [2, num_edges].')
        if edge_index.size != 0 and np.max(edge_index) >= len(node_features):
            raise ValueError('edge_index contains the invalid node number.')
        if edge_features is not None:
            if not isinstance(edge_features, np.ndarray):
                raise ValueError('edge_features must be np.ndarray or None.')
            if edge_index.shape[1] != edge_features.shape[0]:
                raise ValueError('The first dimension of edge_features must be the same as the second dimension of '
                                 'edge_index.')
        if node_pos_features is not None:
            if not isinstance(node_pos_features, np.ndarray):
                raise ValueError('node_pos_features must be np.ndarray or None.')
            if node_pos_features.shape[0] != node_features.shape[0]:
                raise ValueError('The length of node_pos_features must be the same as the length of node_features.')
        self.node_features = node_features
        self.edge_index = edge_index
        self.edge_features = edge_features
        self.node_pos_features = node_pos_features
        self.kwargs = kwargs
        self.num_nodes, self.num_node_features = node_features.shape
        self.num_edges = edge_index.shape[1]
        if edge_features is not None:
            self.num_edge_features = edge_features.shape[1]
        for key, value in kwargs.items():
            setattr(self, key, value)

    def __repr__(self) -> str:
        parts = ["node_features=%s" % list(self.node_features.shape), "edge_index=%s" % list(self.edge_index.shape),
                 "edge_features=%s" % (None if self.edge_features is None else list(self.edge_features.shape))]
        for key, value in self.kwargs.items():
            if isinstance(value, np.ndarray):
                parts.append("%s=%s" % (key, list(value.shape)))
            elif isinstance(value, (str, int, float)):
                parts.append("%s=%s" % (key, value))
        return "%s(%s)" % (type(self).__name__, ", ".join(parts))
