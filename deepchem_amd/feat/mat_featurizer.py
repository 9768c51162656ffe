"""``MATEncoding`` and ``MATFeaturizer`` for SMILES strings on the native reader
(mirror of deepchem/feat/molecule_featurizers/mat_featurizer.py).

Per molecule: the node matrix (36 columns: the dummy column, then the reference's ``atom_features``: atomic number
one-hot over [5, 6, 7, 8, 9, 15, 16, 17, 35, 53, 999], heavy-neighbour count over 0..5, total hydrogens over 0..4,
formal charge over -5..5, in-ring, aromatic; a value outside its list gives an all-zero block, as ``one_hot_encode``
does), the adjacency matrix from the bond list and the TOPOLOGICAL distance matrix (bond counts by breadth-first
search, as ``Chem.GetDistanceMatrix``; unreachable pairs 1e8; no conformer is involved).  The dummy node is added as
``_add_dummy_node`` does: row and column 0, node feature 1 in column 0, adjacency 0, distance 1e6 to everything
including itself.

PARITY UNPINNED: rdkit is not installed where this package is tested, so parity with the reference's featurizer is not
generated; the featurizer is pinned by hand-derived expectations (tests/test_mat_host.py).  Atoms keep their SMILES
order.  With rdkit installed, DeepChem's own ``MATFeaturizer`` produces objects ``MATModel`` accepts.
"""
from dataclasses import dataclass
from typing import Optional

import numpy as np

from deepchem_amd.feat.graph_features import _SmilesFeaturizer, _as_list, read_smiles

ATOMIC_NUMBERS = [5, 6, 7, 8, 9, 15, 16, 17, 35, 53, 999]
N_NODE_FEATURES = 1 + len(ATOMIC_NUMBERS) + 6 + 5 + 11 + 2
DUMMY_DISTANCE = 1e6
UNREACHABLE = 1e8


@dataclass
class MATEncoding:
    node_features: np.ndarray
    adjacency_matrix: np.ndarray
    distance_matrix: np.ndarray


def _one_hot(block: np.ndarray, values: np.ndarray, allowed) -> None:
    for k, a in enumerate(allowed):
        block[:, k] = values == a


def topological_distances(n: int, bonds: np.ndarray) -> np.ndarray:
    """Bond counts between every two of ``n`` atoms (breadth-first search from each); unreachable: 1e8."""
    nbrs = [[] for _ in range(n)]
    for a, b in bonds:
        nbrs[a].append(b)
        nbrs[b].append(a)
    dist = np.full((n, n), UNREACHABLE)
    for s in range(n):
        dist[s, s] = 0.0
        frontier, d = [s], 0
        while frontier:
            d += 1
            nxt = []
            for a in frontier:
                for b in nbrs[a]:
                    if dist[s, b] == UNREACHABLE:
                        dist[s, b] = d
                        nxt.append(b)
            frontier = nxt
    return dist


class MATFeaturizer(_SmilesFeaturizer):
    """``dc.feat.MATFeaturizer`` for SMILES strings; an unreadable molecule gives an empty array."""

    def __init__(self, n_threads: Optional[int] = None):
        self.dtype = object
        self.n_threads = n_threads

    def featurize(self, datapoints, log_every_n: int = 1000, **kwargs) -> np.ndarray:
        smiles = _as_list(datapoints)
        r = read_smiles(smiles, atoms=False, adjacency=False, bonds=True, props=True, n_threads=self.n_threads)
        out = np.empty(len(smiles), dtype=object)
        props = r["atom_props"]  # z, heavy neighbours, implicit H, explicit H, charge, radicals, hybridisation, aromatic
        for i in range(len(smiles)):
            if not r["valid"][i]:
                out[i] = np.array([])
                continue
            a0, a1 = int(r["atom_off"][i]), int(r["atom_off"][i + 1])
            b0, b1 = int(r["bond_off"][i]), int(r["bond_off"][i + 1])
            n = a1 - a0
            p = props[a0:a1]
            bonds = r["bond_atoms"][b0:b1].astype(np.int64)
            ring_bond = r["bond_features"][b0:b1, 5] != 0
            in_ring = np.zeros(n, bool)
            in_ring[bonds[ring_bond].reshape(-1)] = True
            node = np.zeros((n + 1, N_NODE_FEATURES))
            node[0, 0] = 1.0
            body = node[1:]
            _one_hot(body[:, 1:12], p[:, 0], ATOMIC_NUMBERS)
            _one_hot(body[:, 12:18], p[:, 1], range(6))
            _one_hot(body[:, 18:23], p[:, 2] + p[:, 3], range(5))
            _one_hot(body[:, 23:34], p[:, 4], range(-5, 6))
            body[:, 34] = in_ring
            body[:, 35] = p[:, 7] != 0
            adj = np.zeros((n + 1, n + 1))
            adj[bonds[:, 0] + 1, bonds[:, 1] + 1] = 1.0
            adj[bonds[:, 1] + 1, bonds[:, 0] + 1] = 1.0
            dist = np.full((n + 1, n + 1), DUMMY_DISTANCE)
            dist[1:, 1:] = topological_distances(n, bonds)
            out[i] = MATEncoding(node, adj, dist)
        return out
