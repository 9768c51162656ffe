"""``DMPNNEncoderLayer`` and ``PositionwiseFeedForward`` with the reference's layer contract
(deepchem/models/torch_models/layers.py:1261-1649 and :795-908): constructor arguments, parameter names and shapes are
the reference's, so state dicts move both ways.

The reference runs every message-passing round as ``message[mapping].sum(1)``: a ``(bonds, max_degree, hidden)`` gather
through host-built, padded index arrays.  On a ``DmpnnBatch`` (bonds sorted by source atom, ``rev`` = position of the
reverse bond, no pad rows) the same numbers are ``q[b] = S[a] - x[rev[b]]`` with ``S[a]`` the sum of the rows arriving
at the source atom ``a`` of ``b``: ``gcmi_dmpnn_message`` (csrc/dmpnn.hip), whose transposed direction is the backward.
``W_i``, ``W_o`` and the feed-forward layers run on the segmented products, ``W_o`` in their two-operand form over
``[atom_features ; S]`` without a concatenation, the readout on ``gcmi_weave_gather``.  The bond update
``act(input + q . W_h^T)`` is one kernel up to 320 hidden columns (``gcmi_dmpnn_update_fwd``: q is built in LDS as the
product's operand and never written), once per forward in reference mode (after the streaming rounds) and once per
round in paper mode; wider models run the message kernel and the segmented product.  Its backward is decomposed, and
the aggregated rows that ``dW_h`` needs are recomputed into one scratch of the batch instead of being saved per round.

A REFERENCE QUIRK, kept (``message_mode="reference"``, the default): the reference's loop reassigns
``message = message[mapping].sum(1)`` and never ``message = h_message``, so ``W_h`` acts ONCE, on the
``(depth - 1)``-fold aggregated ``act(input)``, and only the last ``h_message`` is used (``depth = 1`` is an
``UnboundLocalError`` there, a ``ValueError`` here).  ``message_mode="paper"`` is the published recursion,
``message = h_message`` each round.

``bias=True`` takes the plain torch path over ``DmpnnBatch.to_reference_arrays()``: with a bias the reference's PAD rows
carry ``act(bias)`` instead of zeros and leak into every ``-1`` slot of ``mapping``, which no pad-free layout
reproduces.  The six-argument form of ``forward`` is the reference's op for op and runs on the CPU too.
"""
from typing import List, Union

import torch
import torch.nn as nn

from deepchem_amd import ops
from deepchem_amd.models.torch_models.functions import DenseFn, MolSumFn, linear

# the widths of the reference's DMPNNFeaturizer (GraphConvConstants.ATOM_FDIM / BOND_FDIM): constants here, no featurizer
ATOM_FDIM, BOND_FDIM = 133, 14


def make_activation(activation: str, allow_linear: bool = False):
    table = {'relu': nn.ReLU, 'leakyrelu': lambda: nn.LeakyReLU(0.1), 'prelu': nn.PReLU, 'tanh': nn.Tanh,
             'selu': nn.SELU, 'elu': nn.ELU}
    if activation in table:
        return table[activation]()
    if allow_linear and activation == 'linear':
        return lambda x: x
    raise ValueError("unknown activation %r" % (activation,))


class BondPlan(object):
    """What the message kernel reads of a batch: ``out_ptr`` (n_atoms + 1) and ``rev`` (n_bonds), int32 on the device,
    VALIDATED on the host before they were uploaded; and one scratch of bond rows per width, reused by every round."""

    def __init__(self, out_ptr: torch.Tensor, rev: torch.Tensor, bond_src: torch.Tensor):
        self.out_ptr, self.rev, self.bond_src = out_ptr, rev, bond_src
        self.n_atoms, self.n_bonds = out_ptr.numel() - 1, rev.numel()
        self._scratch = {}

    def scratch(self, d: int) -> torch.Tensor:
        if d not in self._scratch:
            self._scratch[d] = torch.empty((self.n_bonds, d), dtype=torch.float32, device=self.rev.device)
        return self._scratch[d]


_IMAGE_SCRATCH = {}


def image_scratch(device) -> torch.Tensor:
    """The weight-image scratch of the fused update, one per device (each call rebuilds the image it reads)."""
    if device not in _IMAGE_SCRATCH:
        _IMAGE_SCRATCH[device] = torch.empty(ops.dmpnn_update_scratch_floats(ops.DMPNN_UPDATE_MAX_HIDDEN),
                                             dtype=torch.float32, device=device)
    return _IMAGE_SCRATCH[device]


class MessageFn(torch.autograd.Function):
    """x -> q, ``q[b] = S[a] - x[rev[b]]``; the backward is the transposed kernel.  Nothing is saved."""

    @staticmethod
    def forward(ctx, x, plan: BondPlan):
        ctx.plan = plan
        return ops.dmpnn_message(ops.rowmajor(x), plan.out_ptr, plan.rev)[1]

    @staticmethod
    def backward(ctx, g):
        plan = ctx.plan
        return ops.dmpnn_message(ops.rowmajor(g), plan.out_ptr, plan.rev, transposed=True)[1], None


class AtomSumFn(torch.autograd.Function):
    """x -> S, the sum of the bond rows arriving at every atom (the reference's ``messages_to_atoms``)."""

    @staticmethod
    def forward(ctx, x, plan: BondPlan):
        ctx.plan = plan
        return ops.dmpnn_message(ops.rowmajor(x), plan.out_ptr, plan.rev, want_s=True, want_q=False)[0]

    @staticmethod
    def backward(ctx, g):
        plan = ctx.plan
        return ops.dmpnn_message(None, plan.out_ptr, plan.rev, transposed=True, add=ops.rowmajor(g))[1], None


class MessageUpdateFn(torch.autograd.Function):
    """(x, input, W_h) -> act(input + q . W_h^T), q the aggregated rows of x, act = none or ReLU.  Up to 320 columns the
    forward is ONE kernel that never writes q (``gcmi_dmpnn_update_fwd``); wider, or with ``fused=False``, the message
    kernel writes q into the plan's scratch and the segmented product adds it to a copy of the input.  The backward is
    decomposed either way and recomputes q into that scratch for ``dW_h``."""

    @staticmethod
    def forward(ctx, x, inp, weight, plan: BondPlan, relu: bool, fused: bool = True):
        x, weight = ops.rowmajor(x), weight.contiguous()
        n, d = x.shape
        if fused and d <= ops.DMPNN_UPDATE_MAX_HIDDEN:
            h = ops.dmpnn_update_fwd(x, ops.rowmajor(inp), weight, plan.out_ptr, plan.rev, plan.bond_src, relu,
                                     image_scratch(x.device))
        else:
            q = ops.dmpnn_message(x, plan.out_ptr, plan.rev, q_out=plan.scratch(d))[1]
            h = inp.clone(memory_format=torch.contiguous_format)
            ops.dense(q, weight, layout="out_in", out=h, accumulate=True)
            if relu:
                torch.relu_(h)
        ctx.plan, ctx.relu, ctx.param = plan, relu, weight
        ctx.save_for_backward(x, weight, h)
        return h

    @staticmethod
    def backward(ctx, dh):
        x, weight, h = ctx.saved_tensors
        plan = ctx.plan
        n, d = x.shape
        dz = ops.rowmajor(dh)
        if ctx.relu:
            dz = ops.relu_bwd_(dz.clone(), h)
        dx = dw = None
        if ctx.needs_input_grad[0]:
            dq = ops.dense(dz, weight, layout="in_out")
            dx = ops.dmpnn_message(dq, plan.out_ptr, plan.rev, transposed=True)[1]
        if ctx.needs_input_grad[2]:
            q = ops.dmpnn_message(x, plan.out_ptr, plan.rev, q_out=plan.scratch(d))[1]
            acc, dw = ops.grad_buffer(ctx.param, weight)
            ops.dense_wgrad(q, dz, acc, layout="out_in")
        return dx, dz, dw, None, None, None


class PositionwiseFeedForward(nn.Module):
    """The feed-forward block of the reference (layers.py:795-908), ``dropout_at_input_no_act`` included: ``n_layers``
    linear layers with the activation and one shared dropout between them."""

    def __init__(self, d_input: int = 1024, d_hidden: int = 1024, d_output: int = 1024, activation: str = 'leakyrelu',
                 n_layers: int = 1, dropout_p: float = 0.0, dropout_at_input_no_act: bool = False):
        super(PositionwiseFeedForward, self).__init__()
        self.dropout_at_input_no_act: bool = dropout_at_input_no_act
        self.activation = make_activation(activation, allow_linear=True)
        self.n_layers: int = n_layers
        d_output = d_output if d_output != 0 else d_input
        d_hidden = d_hidden if d_hidden != 0 else d_input
        if n_layers == 1:
            linears = [nn.Linear(d_input, d_output)]
        else:
            linears = [nn.Linear(d_input, d_hidden)] + [nn.Linear(d_hidden, d_hidden) for _ in range(n_layers - 2)] + \
                [nn.Linear(d_hidden, d_output)]
        self.linears = nn.ModuleList(linears)
        dropout_layer = nn.Dropout(dropout_p)
        self.dropout_p = nn.ModuleList([dropout_layer for _ in range(n_layers)])

    def _act_linear(self, x, i: int):
        relu = isinstance(self.activation, nn.ReLU)
        y = linear(x, self.linears[i], relu)
        return y if relu else self.activation(y)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if not self.n_layers:
            return x
        if self.n_layers == 1:
            if self.dropout_at_input_no_act:
                return linear(self.dropout_p[0](x), self.linears[0])
            return self.dropout_p[0](self._act_linear(x, 0))
        if self.dropout_at_input_no_act:
            x = self.dropout_p[0](x)
        for i in range(self.n_layers - 1):
            x = self.dropout_p[i](self._act_linear(x, i))
        return linear(x, self.linears[-1])


class DMPNNEncoderLayer(nn.Module):
    """The D-MPNN encoder: bond hidden states from ``W_i``, ``depth - 1`` message-passing rounds, atom hidden states
    from ``W_o``, the per-molecule readout and the global features (see the module docstring for the two forms of
    ``forward``, ``message_mode`` and ``bias``)."""

    def __init__(self, use_default_fdim: bool = True, atom_fdim: int = 133, bond_fdim: int = 14, d_hidden: int = 300,
                 depth: int = 3, bias: bool = False, activation: str = 'relu', dropout_p: float = 0.0,
                 aggregation: str = 'mean', aggregation_norm: Union[int, float] = 100,
                 message_mode: str = "reference"):
        super(DMPNNEncoderLayer, self).__init__()
        if depth < 2:
            raise ValueError("DMPNNEncoderLayer needs depth >= 2: with depth = %r no message-passing round runs and "
                             "there is no bond hidden state to read out" % (depth,))
        if message_mode not in ("reference", "paper"):
            raise ValueError("message_mode must be 'reference' or 'paper', got %r" % (message_mode,))
        if use_default_fdim:
            self.atom_fdim: int = ATOM_FDIM
            self.concat_fdim: int = ATOM_FDIM + BOND_FDIM
        else:
            self.atom_fdim = atom_fdim
            self.concat_fdim = atom_fdim + bond_fdim
        self.depth: int = depth
        self.aggregation: str = aggregation
        self.aggregation_norm: Union[int, float] = aggregation_norm
        self.message_mode = message_mode
        self.activation = make_activation(activation)
        self.dropout = nn.Dropout(dropout_p)
        self.W_i = nn.Linear(self.concat_fdim, d_hidden, bias=bias)
        self.W_h = nn.Linear(d_hidden, d_hidden, bias=bias)
        self.W_o = nn.Linear(self.atom_fdim + d_hidden, d_hidden)

    # ------------------------------------------------------------------ the reference's form, plain torch ops
    def _get_updated_atoms_hidden_state(self, atom_features, h_message, atom_to_incoming_bonds):
        messages_to_atoms = h_message[atom_to_incoming_bonds].sum(1)
        hidden = self.W_o(torch.cat((atom_features, messages_to_atoms), 1))
        return self.dropout(self.activation(hidden))

    def _readout(self, atoms_hidden_states, molecules_unbatch_key: List):
        mol_vecs = []
        for mol_vec in torch.split(atoms_hidden_states, molecules_unbatch_key):
            if self.aggregation == 'mean':
                mol_vec = mol_vec.sum(dim=0) / len(mol_vec)
            elif self.aggregation == 'sum':
                mol_vec = mol_vec.sum(dim=0)
            elif self.aggregation == 'norm':
                mol_vec = mol_vec.sum(dim=0) / self.aggregation_norm
            else:
                raise Exception("Invalid aggregation")
            mol_vecs.append(mol_vec)
        return torch.stack(mol_vecs, dim=0)

    def _forward_reference(self, atom_features, f_ini_atoms_bonds, atom_to_incoming_bonds, mapping, global_features,
                           molecules_unbatch_key):
        input = self.W_i(f_ini_atoms_bonds)
        message = self.activation(input)
        for _ in range(1, self.depth):
            aggregated = message[mapping].sum(1)
            h_message = self.dropout(self.activation(input + self.W_h(aggregated)))
            # (reference mode: the aggregate is carried on, h_message of every round but the last is dropped)
            message = h_message if self.message_mode == "paper" else aggregated
        hidden = self._get_updated_atoms_hidden_state(atom_features, h_message, atom_to_incoming_bonds)
        output = self._readout(hidden, molecules_unbatch_key)
        if global_features.size()[0] != 0:
            if len(global_features.shape) == 1:
                global_features = global_features.view(len(output), -1)
            output = torch.cat([output, global_features], dim=1)
        return output

    # ------------------------------------------------------------------ the native form
    def _forward_native(self, batch):
        plan = batch.plan
        relu = isinstance(self.activation, nn.ReLU)
        d_hidden = self.W_h.weight.shape[0]
        if plan.n_bonds == 0:  # no bond rows: every atom's message sum is zero
            s = torch.zeros((plan.n_atoms, d_hidden), dtype=torch.float32, device=batch.atom_features.device)
        else:
            inp = DenseFn.apply(batch.f_ini_atoms_bonds, self.W_i.weight, None, None, None, "out_in", False, False)
            message = self.activation(inp)
            if self.message_mode == "reference":
                for _ in range(self.depth - 2):
                    message = MessageFn.apply(message, plan)
                rounds = 1
            else:
                rounds = self.depth - 1
            for _ in range(rounds):
                h = MessageUpdateFn.apply(message, inp, self.W_h.weight, plan, relu)
                message = self.dropout(h if relu else self.activation(h))
            s = AtomSumFn.apply(message, plan)
        hidden = DenseFn.apply(batch.atom_features, self.W_o.weight, self.W_o.bias, s, None, "out_in", relu, False)
        hidden = self.dropout(hidden if relu else self.activation(hidden))
        output = MolSumFn.apply(hidden, batch.mol_ptr, batch.atom_membership)
        if self.aggregation == 'mean':
            output = output / batch.atoms_per_mol
        elif self.aggregation == 'norm':
            output = output / self.aggregation_norm
        elif self.aggregation != 'sum':
            raise Exception("Invalid aggregation")
        if batch.global_features.shape[1] != 0:
            output = torch.cat([output, batch.global_features], dim=1)
        return output

    def forward(self, *args):
        """``forward(batch)`` with a ``DmpnnBatch``, or the reference's ``forward(atom_features, f_ini_atoms_bonds,
        atom_to_incoming_bonds, mapping, global_features, molecules_unbatch_key)``."""
        if len(args) == 6:
            return self._forward_reference(*args)
        if len(args) != 1 or not hasattr(args[0], "to_reference_arrays"):
            raise ValueError("DMPNNEncoderLayer takes a DmpnnBatch or the reference's six arguments")
        batch = args[0]
        dev = self.W_o.weight.device
        if dev.type == "cuda" and self.W_i.bias is None:
            return self._forward_native(batch.to(dev))
        # bias=True (pad rows carry act(bias), see the module docstring), or a model on the CPU
        af, f_ini, a2b, mapping, gf = batch.to_reference_arrays()
        return self._forward_reference(torch.as_tensor(af, dtype=torch.float32, device=dev),
                                       torch.as_tensor(f_ini, dtype=torch.float32, device=dev),
                                       torch.as_tensor(a2b, device=dev), torch.as_tensor(mapping, device=dev),
                                       torch.as_tensor(gf, dtype=torch.float32, device=dev),
                                       batch.molecules_unbatch_key)
