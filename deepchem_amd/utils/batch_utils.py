"""Batch features of Coulomb-matrix molecules for DTNN (the reference's ``deepchem/utils/batch_utils.py:8-132``).

``batch_coulomb_matrix_features`` keeps the reference's signature -- including the swapped NAMES of its two range
defaults (``distance_max=-1, distance_min=18``; ``DTNNModel.default_generator`` passes the values positionally, so the
names never bite there) -- and its five return arrays, computed without a Python loop over the molecules.
``coulomb_matrix_pairs`` is the part of it the resident-set path of ``DTNNModel`` needs: everything but the Gaussians.
"""
from typing import List, Tuple

import numpy as np


def coulomb_matrix_atoms(X_b: np.ndarray) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(num_atoms [M], atom numbers [M, A] int64 (0 past a molecule's atoms), distances [M, A, A] float64): the atom
    count is the number of non-zero entries of column 0, the atom number round((2 C_ii)^(1/2.4)), the distance
    Z_i Z_j / C_ij with -100 on the diagonal (batch_utils.py:101-113); entries past a molecule's atoms are 0."""
    X_b = np.asarray(X_b)
    if X_b.ndim != 3 or X_b.shape[1] != X_b.shape[2]:
        raise ValueError("Coulomb matrices must have shape (n, A, A), got %s" % (X_b.shape,))
    M, A = X_b.shape[0], X_b.shape[1]
    num_atoms = X_b.astype(bool)[:, :, 0].sum(axis=1).astype(np.int64)
    inside = np.arange(A)[None, :] < num_atoms[:, None]  # [M, A]
    diag = X_b[:, np.arange(A), np.arange(A)].astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        z = np.round(np.power(2 * np.where(inside, diag, 0.0), 1 / 2.4)).astype(np.int64)
        block = inside[:, :, None] & inside[:, None, :]
        dist = np.where(block, (z[:, :, None] * z[:, None, :]) / X_b.astype(np.float64), 0.0)
    eye = np.eye(A, dtype=bool)[None] & block
    dist[eye] = -100.0
    return num_atoms, z, dist


def coulomb_matrix_pairs(num_atoms: np.ndarray):
    """For molecules of ``num_atoms`` atoms laid end to end: (atom_membership [N], pair molecule [P], i [P], j [P],
    atom offsets [M + 1]) with every molecule's n x n ordered pairs in row-major (i, j) order, i and j local."""
    num_atoms = np.asarray(num_atoms, np.int64)
    M = num_atoms.shape[0]
    atom_off = np.zeros(M + 1, np.int64)
    np.cumsum(num_atoms, out=atom_off[1:])
    sq = num_atoms * num_atoms
    pair_off = np.zeros(M + 1, np.int64)
    np.cumsum(sq, out=pair_off[1:])
    atom_mem = np.repeat(np.arange(M, dtype=np.int64), num_atoms)
    pair_mol = np.repeat(np.arange(M, dtype=np.int64), sq)
    q = np.arange(pair_off[-1], dtype=np.int64) - pair_off[pair_mol]
    n = np.maximum(num_atoms[pair_mol], 1)
    return atom_mem, pair_mol, q // n, q % n, atom_off


def batch_coulomb_matrix_features(X_b: np.ndarray, distance_max: float = -1, distance_min: float = 18,
                                  n_distance: int = 100) -> List[np.ndarray]:
    """[atom_number int32 [N], gaussian_dist float64 [P, n_distance], atom_membership, distance_membership_i,
    distance_membership_j (int64)] of a batch of Coulomb matrices, as the reference returns them."""
    num_atoms, z, dist = coulomb_matrix_atoms(X_b)
    atom_mem, pair_mol, i, j, atom_off = coulomb_matrix_pairs(num_atoms)
    step_size = (distance_max - distance_min) / n_distance
    steps = np.array([distance_min + k * step_size for k in range(n_distance)])[None, :]
    distance = dist[pair_mol, i, j][:, None]
    gaussian_dist = np.exp(-np.square(distance - steps) / (2 * step_size**2)).astype(np.float64)
    A = z.shape[1] if z.ndim == 2 else 0
    atom_number = z[np.arange(A)[None, :] < num_atoms[:, None]].astype(np.int32)
    start = atom_off[pair_mol]
    return [atom_number, gaussian_dist, atom_mem, (i + start).astype(np.int64), (j + start).astype(np.int64)]
