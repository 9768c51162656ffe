"""``MATEmbedding``, ``MultiHeadedMATAttention``, ``MATEncoderLayer``, ``SublayerConnection`` and ``MATGenerator`` with
the reference's layer contract (deepchem/models/torch_models/layers.py:434-793 and :911-1060): constructor arguments and
state-dict keys are the reference's, shared modules included, so state dicts move both ways.

Two SHARED-MODULE QUIRKS of the reference, kept: ``MultiHeadedMATAttention.linear_layers`` holds the SAME ``nn.Linear``
three times and ``MATEncoderLayer.sublayer`` the SAME ``SublayerConnection`` twice.  The state dict lists the aliases
(``linear_layers.{0,1,2}.*``, ``sublayer.{0,1}.norm.*``), ``parameters()`` yields each once.  Since the encoder calls
attention with ``query = key = value = x``, Q, K and V are ONE tensor: one projection per layer, and its gradient is
``dQ + dK + dV``.

Every layer has two forms.  The reference's padded ``(B, N, ...)`` call is restated in plain torch ops (any device).
With ``batch=`` (a pad-free ``MatBatch``: the atoms of the batch concatenated, pair data as per-molecule ``n x n``
blocks) the inputs are 2-D ``(atoms, width)``, the dense layers run on the segmented product and attention on
``csrc/mat.hip``: the bias ``lambda_distance g(D) + lambda_adjacency A / (rowsum A + eps)`` is one float per pair,
computed once per batch and shared by every layer, and no ``(B, h, N, N)`` tensor exists.  Padding never reaches a real
atom in the reference (pad key columns get exactly 0 weight, pad adjacency entries are 0, the generator masks pad
rows), so the pad-free form computes the same numbers.
"""
import math
from typing import Any

import torch
import torch.nn as nn
import torch.nn.functional as F

from deepchem_amd import ops
from deepchem_amd.models.torch_models.dmpnn_layers import PositionwiseFeedForward
from deepchem_amd.models.torch_models.functions import MolSumFn, linear


class MATEmbedding(nn.Module):
    """A linear layer and dropout over the atom feature rows."""

    def __init__(self, d_input: int = 36, d_output: int = 1024, dropout_p: float = 0.0):
        super(MATEmbedding, self).__init__()
        self.linear_unit = nn.Linear(d_input, d_output)
        self.dropout = nn.Dropout(dropout_p)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        native = x.is_cuda and x.dim() == 2
        rows = linear(x, self.linear_unit) if native else F.linear(x, self.linear_unit.weight, self.linear_unit.bias)
        return self.dropout(rows)


class SublayerConnection(nn.Module):
    """``x + dropout(LayerNorm(output))`` (``x`` None: without the residual)."""

    def __init__(self, size: int, dropout_p: float = 0.0):
        super(SublayerConnection, self).__init__()
        self.norm = nn.LayerNorm(size)
        self.dropout_p = nn.Dropout(dropout_p)

    def forward(self, x: torch.Tensor, output: torch.Tensor) -> torch.Tensor:
        branch = self.dropout_p(self.norm(output))
        return branch if x is None else x + branch


class MultiHeadedMATAttention(nn.Module):
    """Self-attention whose weights are ``lambda_attention softmax(Q K^T / sqrt(d_k)) + lambda_distance g(D) +
    lambda_adjacency A / (rowsum A + eps)``."""

    def __init__(self, dist_kernel: str = 'softmax', lambda_attention: float = 0.33, lambda_distance: float = 0.33,
                 h: int = 16, hsize: int = 1024, dropout_p: float = 0.0, output_bias: bool = True):
        super().__init__()
        if dist_kernel not in ops.MAT_DIST_KERNELS:
            raise ValueError("dist_kernel must be 'softmax' or 'exp' (got %r)" % (dist_kernel,))
        self.dist_kernel_name = dist_kernel
        self.lambda_attention = lambda_attention
        self.lambda_distance = lambda_distance
        self.lambda_adjacency = 1.0 - self.lambda_attention - self.lambda_distance
        self.d_k = hsize // h
        self.h = h
        linear_layer = nn.Linear(hsize, hsize)
        self.linear_layers = nn.ModuleList([linear_layer for _ in range(3)])  # ONE module (see the module docstring)
        self.dropout_p = nn.Dropout(dropout_p)
        self.output_linear = nn.Linear(hsize, hsize, output_bias)

    def dist_kernel(self, x: torch.Tensor) -> torch.Tensor:
        return torch.softmax(-x, dim=-1) if self.dist_kernel_name == "softmax" else torch.exp(-x)

    def pair_bias(self, adjacency: torch.Tensor, distance: torch.Tensor, real_key=None, eps: float = 1e-6) -> torch.Tensor:
        """The head-independent part of the weights on padded ``(B, N, N)`` arrays, ``lambda_distance g(D) +
        lambda_adjacency A / (rowsum A + eps)``.  ``real_key`` ``(B, 1, N)``: False at pad atoms, whose columns get
        distance inf and with it weight exactly 0 (their adjacency entries are 0 already)."""
        if real_key is not None:
            distance = torch.where(real_key, distance, distance.new_tensor(float("inf")))
        degree = adjacency.sum(dim=-1, keepdim=True)
        return self.lambda_distance * self.dist_kernel(distance) + self.lambda_adjacency * (adjacency / (degree + eps))

    def _split_heads(self, rows: torch.Tensor) -> torch.Tensor:
        """(B, N, h d_k) -> (B, h, N, d_k)"""
        return rows.reshape(rows.shape[0], rows.shape[1], self.h, self.d_k).permute(0, 2, 1, 3)

    def native_covers(self, batch) -> bool:
        """Whether csrc/mat.hip covers this layer on this batch (the head width and the largest molecule)."""
        return self.d_k % 4 == 0 and 0 < self.d_k <= ops.MAT_MAX_DK and batch.offs.n_max <= ops.MAT_MAX_ATOMS and \
            not (self.training and self.dropout_p.p > 0)

    def _single_attention(self, query, key, value, mask, adj_matrix, distance_matrix, dropout_p: float = 0.0,
                          eps: float = 1e-6, inf: float = 1e12):
        """Padded form: query / key / value ``(B, h, N, d_k)``, mask ``(B, N)`` or ``(B, 1, N)`` (0 at pad atoms) or
        None.  Returns the ``(B, h, N, d_k)`` context rows and the softmax part of the weights."""
        like = dict(device=query.device, dtype=query.dtype)
        adjacency = torch.as_tensor(adj_matrix).to(**like).reshape(query.shape[0], query.shape[2], -1)
        distance = torch.as_tensor(distance_matrix).to(**like).reshape(adjacency.shape)
        real_key = None if mask is None else (torch.as_tensor(mask, device=query.device) != 0).reshape(query.shape[0], 1, -1)
        logits = torch.einsum("bhid,bhjd->bhij", query, key) / math.sqrt(self.d_k)
        if real_key is not None:
            logits = torch.where(real_key.unsqueeze(1), logits, logits.new_tensor(-inf))
        attention = logits.softmax(dim=-1)
        shared_bias = self.pair_bias(adjacency, distance, real_key, eps).unsqueeze(1)  # the same for every head
        weights = self.dropout_p(attention * self.lambda_attention + shared_bias)
        return torch.einsum("bhij,bhjd->bhid", weights, value), attention

    def forward(self, query, key, value, mask=None, adj_matrix=None, distance_matrix=None, dropout_p: float = 0.0,
                eps: float = 1e-6, inf: float = 1e12, batch=None) -> torch.Tensor:
        if batch is not None:
            return self._forward_batch(query, key, value, batch, eps)
        q, k, v = (self._split_heads(F.linear(rows, layer.weight, layer.bias))
                   for rows, layer in zip((query, key, value), self.linear_layers))
        context, _ = self._single_attention(q, k, v, mask, adj_matrix, distance_matrix, dropout_p, eps, inf)
        merged = context.permute(0, 2, 1, 3).reshape(query.shape[0], query.shape[1], self.h * self.d_k)
        return F.linear(merged, self.output_linear.weight, self.output_linear.bias)

    def _forward_batch(self, query, key, value, batch, eps: float):
        if not self.native_covers(batch):
            raise ValueError("MultiHeadedMATAttention: d_k = %d, a molecule of %d atoms or training dropout is outside "
                             "the attention kernel; use the padded call" % (self.d_k, batch.offs.n_max))
        bias = batch.bias(self.dist_kernel_name, self.lambda_distance, self.lambda_adjacency, eps)
        one_layer = self.linear_layers[0] is self.linear_layers[1] and self.linear_layers[1] is self.linear_layers[2]
        if one_layer and query is key and key is value:
            q = k = v = linear(query, self.linear_layers[0])
        else:
            q, k, v = [linear(x, layer) for layer, x in zip(self.linear_layers, (query, key, value))]
        x = ops.MatAttentionFn.apply(q, k, v, bias, batch.offs, self.h, self.lambda_attention)
        return linear(x, self.output_linear)


class MATEncoderLayer(nn.Module):
    """Self-attention and the position-wise feed-forward layer, each behind the (one) sublayer connection."""

    def __init__(self, dist_kernel: str = 'softmax', lambda_attention: float = 0.33, lambda_distance: float = 0.33,
                 h: int = 16, sa_hsize: int = 1024, sa_dropout_p: float = 0.0, output_bias: bool = True,
                 d_input: int = 1024, d_hidden: int = 1024, d_output: int = 1024, activation: str = 'leakyrelu',
                 n_layers: int = 1, ff_dropout_p: float = 0.0, encoder_hsize: int = 1024,
                 encoder_dropout_p: float = 0.0):
        super(MATEncoderLayer, self).__init__()
        self.self_attn = MultiHeadedMATAttention(dist_kernel, lambda_attention, lambda_distance, h, sa_hsize,
                                                 sa_dropout_p, output_bias)
        self.feed_forward = PositionwiseFeedForward(d_input, d_hidden, d_output, activation, n_layers, ff_dropout_p)
        layer = SublayerConnection(size=encoder_hsize, dropout_p=encoder_dropout_p)
        self.sublayer = nn.ModuleList([layer for _ in range(2)])  # ONE module (see the module docstring)
        self.size = encoder_hsize

    def _feed_forward(self, x):
        if x.dim() == 2:
            return self.feed_forward(x)
        return self.feed_forward(x.reshape(-1, x.shape[-1])).reshape(x.shape[:-1] + (-1,))

    def forward(self, x, mask=None, adj_matrix=None, distance_matrix=None, sa_dropout_p: float = 0.0,
                batch=None) -> torch.Tensor:
        connect = self.sublayer[0]  # (sublayer[1] is the same module)
        if batch is not None:
            attended = self.self_attn(x, x, x, batch=batch)
        else:
            attended = self.self_attn(x, x, x, mask, adj_matrix, distance_matrix, sa_dropout_p)
        after_attention = connect(x, attended)
        return self.sublayer[1](after_attention, self._feed_forward(after_attention))


class MATGenerator(nn.Module):
    """The readout: ``mean`` over the atoms of a molecule, ``grover`` attention pooling or ``contextual`` (none), then
    the projection."""

    def __init__(self, hsize: int = 1024, aggregation_type: str = 'mean', d_output: int = 1, n_layers: int = 1,
                 dropout_p: float = 0.0, attn_hidden: int = 128, attn_out: int = 4):
        super(MATGenerator, self).__init__()
        if aggregation_type not in ('mean', 'grover', 'contextual'):
            raise ValueError("aggregation_type must be 'mean', 'grover' or 'contextual'")
        if aggregation_type == 'grover':
            self.att_net = nn.Sequential(nn.Linear(hsize, attn_hidden, bias=False), nn.Tanh(),
                                         nn.Linear(attn_hidden, attn_out, bias=False))
            hsize *= attn_out
        if n_layers == 1:
            self.proj: Any = nn.Linear(hsize, d_output)
        else:
            proj = []
            for _ in range(n_layers - 1):
                proj += [nn.Linear(hsize, attn_hidden), nn.LeakyReLU(negative_slope=0.1), nn.LayerNorm(attn_hidden),
                         nn.Dropout(dropout_p)]
            proj.append(nn.Linear(attn_hidden, d_output))
            self.proj = torch.nn.Sequential(*proj)
        self.aggregation_type = aggregation_type

    def _project(self, x):
        if isinstance(self.proj, nn.Linear) and x.is_cuda and x.dim() == 2:
            return linear(x, self.proj)
        return self.proj(x)

    def _pool(self, rows: torch.Tensor, real: torch.Tensor) -> torch.Tensor:
        """Padded ``(B, N, d)`` rows and ``(B, N)`` real-atom flags -> what the projection reads."""
        if self.aggregation_type == 'contextual':
            return rows
        kept = torch.where(real.unsqueeze(-1), rows, rows.new_zeros(()))
        if self.aggregation_type == 'mean':
            return kept.sum(dim=1) / real.sum(dim=1, keepdim=True).to(rows.dtype)
        # grover: attn_out softmax distributions over the real atoms of a molecule, each pooling the rows once
        scores = torch.where(real.unsqueeze(-1), self.att_net(kept), rows.new_tensor(-1e9))
        return torch.einsum("bna,bnd->bad", scores.softmax(dim=1), kept).flatten(1)

    def forward(self, x: torch.Tensor, mask=None, batch=None) -> torch.Tensor:
        """``x`` ``(B, N, d)`` with ``mask`` ``(B, N)`` (0 at pad atoms), or ``(atoms, d)`` rows with ``batch=``."""
        if batch is None:
            return self.proj(self._pool(x, torch.as_tensor(mask, device=x.device) != 0))
        if self.aggregation_type == 'mean':  # every atom of a pad-free batch counts: the segment sum over its rows
            pooled = MolSumFn.apply(x, batch.offs.d_atom_off, batch.membership)
            return self._project(pooled / batch.atoms_per_mol.unsqueeze(-1))
        return self.proj(self._pool(batch.pad_rows(x), batch.pad_mask))  # grover / contextual: in torch
