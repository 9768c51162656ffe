"""``DTNNEmbedding``, ``DTNNStep``, ``DTNNGather`` with the reference's layer contract
(deepchem/models/torch_models/layers.py:3141-3224, :3742-4003): constructor arguments, parameter names, shapes and
initialisers are the reference's, so state dicts move both ways.

``DTNNStep`` is the fused pair interaction of csrc/dtnn.hip.  The reference multiplies a P x n_distance Gaussian
matrix with ``W_df``, gathers a P x n_hidden copy of the atom rows, multiplies, projects and scatters; here the atom
rows ``ah = C . W_cf + b_cf`` are one segmented product (N rows), and ONE kernel per direction does everything at the
pair level without writing a pair-sized tensor.  The layer's own ``forward`` takes the reference's inputs
(``[atom_features, gaussian P x n_distance, mem_i, mem_j]``, the kernel's form (b)); ``DTNN`` on a resident set calls
``interact`` with one float per pair, the distance (form (a): the Gaussians are generated in registers).

The self term ``tanh((b_df * ah) . W_fc)`` and the residual keep the reference's arithmetic graph: the diagonal pair
(distance -100) stays in the pair list and the self term is subtracted -- its Gaussians vanish for the default range
only.  These N-row elementwise steps, the embedding look-up and dropout are torch ops between the native ones.
"""
from typing import Callable, Optional

import torch
import torch.nn as nn
from torch.nn import init as initializers

from deepchem_amd import ops
from deepchem_amd.models.torch_models.functions import DenseFn, MolSumFn, TanhFn


def _require_tanh(activation) -> None:
    if activation not in ("tanh", torch.tanh) and not isinstance(activation, nn.Tanh):
        raise ValueError("the DTNN layers on libgcmi.so support activation='tanh' only (got %r)" % (activation,))


class PairPlan:
    """A validated pair list on the device: int32 memberships (mem_i non-decreasing, both inside [0, n_atoms)) and the
    per-pair source -- distances (``from_distance``) or Gaussian rows."""

    def __init__(self, src: torch.Tensor, from_distance: bool, mem_i: torch.Tensor, mem_j: torch.Tensor, n_atoms: int,
                 distance_min: float = 0.0, step: float = 1.0):
        self.src, self.from_distance = src, bool(from_distance)
        self.mem_i, self.mem_j, self.n_atoms = mem_i, mem_j, int(n_atoms)
        self.distance_min, self.step = float(distance_min), float(step)

    @staticmethod
    def checked(src, from_distance, mem_i, mem_j, n_atoms, device, distance_min=0.0, step=1.0) -> "PairPlan":
        """From caller-supplied memberships (host arrays or tensors): min, max and order are checked ONCE here."""
        mi = torch.as_tensor(mem_i).reshape(-1)
        mj = torch.as_tensor(mem_j).reshape(-1)
        if mi.dtype.is_floating_point or mj.dtype.is_floating_point or mi.numel() != mj.numel():
            raise ValueError("DTNNStep: distance_membership_i / _j must be integer vectors of one length")
        if mi.numel():
            bad = (mi.min() < 0) | (mi.max() >= n_atoms) | (mj.min() < 0) | (mj.max() >= n_atoms) | \
                (mi[1:] < mi[:-1]).any()
            if bool(bad):  # (device tensors: the one read-back of the call)
                raise ValueError("DTNNStep: memberships must lie inside [0, %d) with distance_membership_i in "
                                 "non-decreasing order (pairs sorted by their first atom)" % n_atoms)
        return PairPlan(src, from_distance, mi.to(device=device, dtype=torch.int32).contiguous(),
                        mj.to(device=device, dtype=torch.int32).contiguous(), n_atoms, distance_min, step)


class DtnnPairFn(torch.autograd.Function):
    """(ah, W_df, b_df, W_fc) -> Y, the pair sum of csrc/dtnn.hip; the backward recomputes from the same inputs."""

    @staticmethod
    def forward(ctx, ah, W_df, b_df, W_fc, plan: PairPlan):
        ah, W_df, b_df, W_fc = ops.rowmajor(ah), W_df.contiguous(), b_df.contiguous(), W_fc.contiguous()
        ctx.plan = plan
        ctx.params = (W_df, b_df, W_fc)
        ctx.save_for_backward(ah, W_df, b_df, W_fc)
        return ops.dtnn_pair_fwd(plan.src, plan.from_distance, plan.mem_i, plan.mem_j, ah, W_df, b_df, W_fc,
                                 plan.distance_min, plan.step)

    @staticmethod
    def backward(ctx, dy):
        ah, W_df, b_df, W_fc = ctx.saved_tensors
        plan = ctx.plan
        # (the kernel adds into its weight-gradient buffers: with ops.direct_param_grads on, straight into p.grad)
        bufs, grads = zip(*(ops.grad_buffer(p, t) for p, t in zip(ctx.params, (W_df, b_df, W_fc))))
        dah = ops.dtnn_pair_bwd(plan.src, plan.from_distance, plan.mem_i, plan.mem_j, ah, W_df, b_df, W_fc,
                                plan.distance_min, plan.step, ops.rowmajor(dy.contiguous()), *bufs)
        return dah, grads[0], grads[1], grads[2], None


class DTNNEmbedding(nn.Module):
    """Initial atomic descriptors: row ``atom_number`` of a (periodic_table_length, n_embedding) table."""

    def __init__(self, n_embedding: int = 30, periodic_table_length: int = 30, initalizer: str = 'xavier_uniform_',
                 **kwargs):
        super(DTNNEmbedding, self).__init__(**kwargs)
        self.n_embedding = n_embedding
        self.periodic_table_length = periodic_table_length
        self.initalizer = initalizer
        init_func: Callable = getattr(initializers, self.initalizer)
        self.embedding_list: nn.Parameter = nn.Parameter(
            init_func(torch.empty([self.periodic_table_length, self.n_embedding])))

    def __repr__(self) -> str:
        return f'{self.__class__.__name__}(n_embedding={self.n_embedding}, periodic_table_length={self.periodic_table_length}, initalizer={self.initalizer})'

    def forward(self, inputs, validated: bool = False):
        """``inputs``: integer atom numbers.  A number outside the table raises ``ValueError`` (the reference indexes
        with it); ``validated``: the caller has checked already (the resident set does, once per dataset)."""
        atom_number = torch.as_tensor(inputs)
        if atom_number.dtype.is_floating_point:
            raise ValueError("DTNNEmbedding takes integer atom numbers")
        if not validated and atom_number.numel():
            if bool((atom_number.min() < 0) | (atom_number.max() >= self.periodic_table_length)):
                raise ValueError("atom number outside the embedding table of %d rows" % self.periodic_table_length)
        atom_number = atom_number.to(device=self.embedding_list.device, dtype=torch.int64)
        return torch.nn.functional.embedding(atom_number, self.embedding_list)


class DTNNStep(nn.Module):
    """Eq. (7) and (6) of the DTNN paper: C_i += sum_j tanh(W_fc . ((W_cf C_j + b_cf) * (W_df d_ij + b_df)))."""

    def __init__(self, n_embedding: int = 30, n_distance: int = 100, n_hidden: int = 60,
                 initializer: str = 'xavier_uniform_', activation='tanh', **kwargs):
        super(DTNNStep, self).__init__(**kwargs)
        _require_tanh(activation)
        if n_embedding > ops.DTNN_MAX_EMBEDDING or n_hidden > ops.DTNN_MAX_HIDDEN or n_distance > ops.DTNN_MAX_DISTANCE:
            raise ValueError("DTNNStep on libgcmi.so covers n_embedding <= %d, n_hidden <= %d, n_distance <= %d" %
                             (ops.DTNN_MAX_EMBEDDING, ops.DTNN_MAX_HIDDEN, ops.DTNN_MAX_DISTANCE))
        self.n_embedding = n_embedding
        self.n_distance = n_distance
        self.n_hidden = n_hidden
        self.initializer = initializer
        self.activation = activation
        self.activation_fn = torch.tanh
        init_func: Callable = getattr(initializers, self.initializer)
        self.W_cf = nn.Parameter(init_func(torch.empty([self.n_embedding, self.n_hidden])))
        self.W_df = nn.Parameter(init_func(torch.empty([self.n_distance, self.n_hidden])))
        self.W_fc = nn.Parameter(init_func(torch.empty([self.n_hidden, self.n_embedding])))
        self.b_cf = nn.Parameter(torch.zeros(size=[self.n_hidden]))
        self.b_df = nn.Parameter(torch.zeros(size=[self.n_hidden]))

    def __repr__(self):
        return f'{self.__class__.__name__}(n_embedding={self.n_embedding}, n_distance={self.n_distance}, n_hidden={self.n_hidden}, initializer={self.initializer}, activation={self.activation})'

    def interact(self, atom_features: torch.Tensor, plan: PairPlan) -> torch.Tensor:
        if atom_features.dim() != 2 or atom_features.shape[1] != self.n_embedding or \
                atom_features.shape[0] != plan.n_atoms:
            raise ValueError("DTNNStep: atom_features must be (%d, %d), got %s" %
                             (plan.n_atoms, self.n_embedding, tuple(atom_features.shape)))
        ah = DenseFn.apply(atom_features, self.W_cf, self.b_cf, None, None, "in_out", False, False)
        pair_sum = DtnnPairFn.apply(ah, self.W_df, self.b_df, self.W_fc, plan)
        output_ii = TanhFn.apply(DenseFn.apply(self.b_df * ah, self.W_fc, None, None, None, "in_out", False, False))
        return pair_sum - output_ii + atom_features

    def forward(self, inputs):
        """``[atom_features (N, n_embedding), gaussian distances (P, n_distance), distance_membership_i (P),
        distance_membership_j (P)]``, pairs sorted by first atom.  Anything else -- such as the broadcasting 1-D
        distance of the reference's docstring example -- raises ``ValueError``."""
        if len(inputs) != 4:
            raise ValueError("DTNNStep takes [atom_features, distance, distance_membership_i, distance_membership_j]")
        atom_features, distance, mem_i, mem_j = inputs
        if not (torch.is_tensor(atom_features) and atom_features.is_cuda and atom_features.dim() == 2):
            raise ValueError("DTNNStep: atom_features must be a 2-D tensor on the GPU (there is no CPU path)")
        distance = torch.as_tensor(distance)
        n_pairs = torch.as_tensor(mem_i).numel()
        if distance.dim() != 2 or distance.shape[1] != self.n_distance or distance.shape[0] != n_pairs:
            raise ValueError("DTNNStep: distance must be the (%d, %d) Gaussian matrix, one row per pair of the "
                             "memberships; got %s" % (n_pairs, self.n_distance, tuple(distance.shape)))
        distance = ops.rowmajor(distance.to(device=atom_features.device, dtype=torch.float32))
        plan = PairPlan.checked(distance, False, mem_i, mem_j, atom_features.shape[0], atom_features.device)
        return self.interact(atom_features, plan)


class DTNNGather(nn.Module):
    """Atom-level dense layers (tanh), then the sum of the atom outputs per molecule."""

    def __init__(self, n_embedding=30, n_outputs=100, layer_sizes=[100], output_activation=True,
                 initializer='xavier_uniform_', activation='tanh', **kwargs):
        super(DTNNGather, self).__init__(**kwargs)
        _require_tanh(activation)
        self.n_embedding = n_embedding
        self.n_outputs = n_outputs
        self.layer_sizes = layer_sizes
        self.output_activation = output_activation
        self.initializer = initializer
        self.activation = activation
        self.activation_fn = torch.tanh
        self.W_list = nn.ParameterList()
        self.b_list = nn.ParameterList()
        init_func: Callable = getattr(initializers, self.initializer)
        prev_layer_size = self.n_embedding
        for layer_size in self.layer_sizes:
            self.W_list.append(nn.Parameter(init_func(torch.empty([prev_layer_size, layer_size]))))
            self.b_list.append(nn.Parameter(torch.zeros(size=[layer_size])))
            prev_layer_size = layer_size
        self.W_list.append(nn.Parameter(init_func(torch.empty([prev_layer_size, self.n_outputs]))))
        self.b_list.append(nn.Parameter(torch.zeros(size=[self.n_outputs])))

    def __repr__(self):
        return f'{self.__class__.__name__}(n_embedding={self.n_embedding}, n_outputs={self.n_outputs}, layer_sizes={self.layer_sizes}, output_activation={self.output_activation}, initializer={self.initializer}, activation={self.activation})'

    def forward(self, inputs, n_molecules: Optional[int] = None, mol_ptr: Optional[torch.Tensor] = None):
        """``[atom_features (N, n_embedding), atom_membership (N), ascending]``.  ``n_molecules``: the number of
        output rows (default: largest membership + 1, the reference's); a molecule without atoms gives a zero row.
        ``mol_ptr``: the int32 CSR of the membership on the device, when the caller has it already."""
        output, membership = inputs[0], torch.as_tensor(inputs[1]).reshape(-1)
        if not (torch.is_tensor(output) and output.is_cuda and output.dim() == 2):
            raise ValueError("DTNNGather: atom_features must be a 2-D tensor on the GPU (there is no CPU path)")
        if membership.numel() != output.shape[0] or membership.dtype.is_floating_point:
            raise ValueError("DTNNGather: atom_membership must hold one integer per atom row")
        membership = membership.to(device=output.device, dtype=torch.int64)
        if mol_ptr is None:
            if n_molecules is None:
                n_molecules = int(membership.max()) + 1 if membership.numel() else 0
            if membership.numel() and bool((membership.min() < 0) | (membership.max() >= n_molecules) |
                                           (membership[1:] < membership[:-1]).any()):
                raise ValueError("DTNNGather: atom_membership must be ascending and inside [0, %d)" % n_molecules)
            mol_ptr = torch.zeros(n_molecules + 1, dtype=torch.int64, device=output.device)
            if membership.numel():
                torch.cumsum(torch.bincount(membership, minlength=n_molecules), 0, out=mol_ptr[1:])
            mol_ptr = mol_ptr.to(torch.int32)
        n_layers = len(self.W_list)
        for k in range(n_layers):
            output = DenseFn.apply(output, self.W_list[k], self.b_list[k], None, None, "in_out", False, False)
            if k < n_layers - 1 or self.output_activation:
                output = TanhFn.apply(output)
        return MolSumFn.apply(output, mol_ptr, membership)
