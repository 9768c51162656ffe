"""The ``torch.autograd.Function``s that more than one model uses.  They only sequence the checked wrappers of
``deepchem_amd.ops``; a Function that one model alone needs stays in that model's file."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from deepchem_amd import ops


class DenseFn(torch.autograd.Function):
    """``act(x . W [+ x2 . W2] + b)``, act = none or ReLU, on the segmented products.  ``layout`` is that of
    ``ops.dense``: "out_in" for nn.Linear's (out, in) weights, "in_out" for the Keras (in, out) ones.  Three forms:

    * single: ``x2`` is None;
    * dual, separate weights: ``x2`` and ``W2``;
    * dual, one weight: ``x2`` without ``W2``, and ``W`` holds ``[W1 | W2]`` along its input axis -- the product over
      ``[x ; x2]`` without the concatenation.  The blocks are copied contiguous, and the gradient of ``W`` is put
      together from the two block gradients and handed to autograd: a column block of an (out, in) matrix is not
      contiguous, so the kernel cannot add into ``W.grad`` as it does for the other two forms.

    ``grad_masked``: the incoming gradient is already zero where the ReLU cut, the backward does not mask it again.
    The backward runs the weight gradients before the input gradients, the first operand before the second."""

    @staticmethod
    def forward(ctx, x, W, b, x2, W2, layout: str, relu: bool, grad_masked: bool = False):
        x = ops.rowmajor(x)
        pW, pb, pW2 = W, b, W2  # (what ops.grad_buffer looks at: the parameters themselves, not copies)
        ctx.one_weight = x2 is not None and W2 is None
        if ctx.one_weight:
            k = x.shape[1]
            W, W2 = (W[:, :k], W[:, k:]) if layout == "out_in" else (W[:k], W[k:])
            pW = pb = None
        W = W.contiguous()
        if x2 is not None:
            x2, W2 = ops.rowmajor(x2), W2.contiguous()
        out = ops.dense(x, W, None if b is None else b.contiguous(), layout=layout, x2=x2, w2=W2, relu=relu)
        ctx.layout, ctx.relu, ctx.params = layout, relu and not grad_masked, (pW, pb, pW2)
        ctx.save_for_backward(x, W, b, x2, W2, out if ctx.relu else None)
        return out

    @staticmethod
    def backward(ctx, g):
        x, W, b, x2, W2, out = ctx.saved_tensors
        pW, pb, pW2 = ctx.params
        layout, need = ctx.layout, ctx.needs_input_grad
        g = ops.rowmajor(g)
        if ctx.relu:
            g = ops.relu_bwd_(g.clone(), out)
        dx = dW = db = dx2 = dW2 = None
        need_b = b is not None and need[2]
        if need[1] or need_b:
            acc, dW = ops.grad_buffer(pW, W)
            acc_b, db = ops.grad_buffer(pb, b) if b is not None else (None, None)
            ops.dense_wgrad(x, g, acc, acc_b, layout=layout)
        if x2 is not None and (need[1] or need_b if ctx.one_weight else need[4]):
            acc, dW2 = ops.grad_buffer(pW2, W2)
            ops.dense_wgrad(x2, g, acc, layout=layout)
        if ctx.one_weight:
            if dW is not None:
                dW = torch.cat([dW, dW2], dim=1 if layout == "out_in" else 0)
            dW2 = None
        # dx = g . W^T: W read in the other layout, as the weight of a layer n_out -> k
        back = "in_out" if layout == "out_in" else "out_in"
        if need[0]:
            dx = ops.dense(g, W, layout=back)
        if x2 is not None and need[3]:
            dx2 = ops.dense(g, W2, layout=back)
        return dx, dW, db, dx2, dW2, None, None, None


def linear(x, layer: nn.Linear, relu: bool = False):
    """nn.Linear, ReLU fused if asked: the segmented product on the GPU, torch on the CPU."""
    if x.is_cuda:
        return DenseFn.apply(x, layer.weight, layer.bias, None, None, "out_in", relu, False)
    y = F.linear(x, layer.weight, layer.bias)
    return torch.relu(y) if relu else y


class TanhFn(torch.autograd.Function):
    """tanh in place on a fresh product (gcmi_tanh_)."""

    @staticmethod
    def forward(ctx, x):
        y = ops.tanh_(x)
        ctx.mark_dirty(x)
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, g):
        y, = ctx.saved_tensors
        return g * (1.0 - y * y)


class MolSumFn(torch.autograd.Function):
    """Per-molecule sum of atom rows (atoms of molecule m: rows [mol_ptr[m], mol_ptr[m + 1]))."""

    @staticmethod
    def forward(ctx, x, mol_ptr, membership):
        ctx.save_for_backward(membership)
        return ops.weave_gather(ops.rowmajor(x), mol_ptr, False)

    @staticmethod
    def backward(ctx, g):
        membership, = ctx.saved_tensors
        return g.index_select(0, membership), None, None


class GruGatesFn(torch.autograd.Function):
    """(zp, rp, h) -> (z = sigmoid(zp), r = sigmoid(rp), hr = h r), in place on zp / rp."""

    @staticmethod
    def forward(ctx, zp, rp, h):
        h = h.contiguous()
        hr = ops.gru_gates_(zp, rp, h)
        ctx.mark_dirty(zp, rp)
        ctx.save_for_backward(zp, rp, h)
        return zp, rp, hr

    @staticmethod
    def backward(ctx, dz, dr_unused, dhr):
        z, r, h = ctx.saved_tensors
        dz = torch.zeros_like(z) if dz is None else dz.contiguous()
        dhr = torch.zeros_like(z) if dhr is None else dhr.contiguous()
        return ops.gru_gates_bwd(z, r, h, dz, dhr)


class GruOutFn(torch.autograd.Function):
    """(z, hpre, x) -> (1 - z) tanh(hpre) + z x."""

    @staticmethod
    def forward(ctx, z, hpre, x):
        z, hpre, x = z.contiguous(), hpre.contiguous(), x.contiguous()
        ctx.save_for_backward(z, hpre, x)
        return ops.gru_out(z, hpre, x)

    @staticmethod
    def backward(ctx, dout):
        z, hpre, x = ctx.saved_tensors
        return ops.gru_out_bwd(z, hpre, x, dout.contiguous())


class AttendFn(torch.autograd.Function):
    """One set2set attention step: (x, h) -> q_star = [h | sum_a softmax(<x_a, h>) x_a] per molecule."""

    @staticmethod
    def forward(ctx, x, h, mol_ptr):
        x, h = ops.rowmajor(x), ops.rowmajor(h)
        ctx.save_for_backward(x, h, mol_ptr)
        return ops.set2set_attend(x, mol_ptr, h)

    @staticmethod
    def backward(ctx, dq):
        x, h, mol_ptr = ctx.saved_tensors
        dx, dh = ops.set2set_attend_bwd(x, mol_ptr, h, ops.rowmajor(dq))
        return dx, dh, None


class LstmCellFn(torch.autograd.Function):
    """(z (B, 4H) gate pre-activations in order i, f, o, g; c) -> (h', c')."""

    @staticmethod
    def forward(ctx, z, c):
        z = ops.rowmajor(z)
        c_prev = c.contiguous()
        c_new = c_prev.clone()
        h_new = ops.lstm_cell_(z, c_new)
        ctx.save_for_backward(z, c_prev)
        return h_new, c_new

    @staticmethod
    def backward(ctx, dh, dc):
        z, c_prev = ctx.saved_tensors
        dh = torch.zeros_like(c_prev) if dh is None else dh.contiguous()
        return ops.lstm_cell_bwd(z, c_prev, dh, None if dc is None else dc.contiguous())
