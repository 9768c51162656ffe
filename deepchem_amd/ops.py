"""Typed wrappers over the C ABI (include/gcmi.h) and the autograd glue.

Each wrapper checks on the HOST that shapes, dtypes, strides and devices are
what the kernel and its grid assume (a faulting kernel can take the GPU down)
and then enqueues the kernel on torch's current stream.  The
``torch.autograd.Function``s below only sequence those calls; every FLOP and
every byte of the hot path moves in libgcmi.so.
"""
import ctypes
from typing import Optional

import numpy as np
import torch

from deepchem_amd import _lib
from deepchem_amd.graph import BatchGraph, _stream

_vp = ctypes.c_void_p


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else _vp(t.data_ptr())


def _mat(t: torch.Tensor, name: str, rows: Optional[int] = None, cols: Optional[int] = None,
         dtype=torch.float32):
    if not torch.is_tensor(t) or not t.is_cuda:
        raise _lib.GcmiError("%s must be a CUDA tensor: the hot path has no CPU implementation" % name)
    if t.dtype != dtype:
        raise TypeError("%s must be %s, got %s" % (name, dtype, t.dtype))
    if t.dim() != 2 or (t.numel() > 0 and t.shape[1] > 1 and t.stride(1) != 1):  # (an empty tensor's strides mean nothing)
        raise ValueError("%s must be 2-D with unit column stride (shape %s, strides %s)" %
                         (name, tuple(t.shape), t.stride()))
    if t.numel() > 0 and t.shape[0] > 1 and t.stride(0) < t.shape[1]:
        # (_ld would hand the kernel ld = columns: other rows than the view's, and past its end)
        raise ValueError("%s: rows overlap, row stride %d < %d columns" % (name, t.stride(0), t.shape[1]))
    if rows is not None and t.shape[0] != rows:
        raise ValueError("%s has %d rows, expected %d" % (name, t.shape[0], rows))
    if cols is not None and t.shape[1] != cols:
        raise ValueError("%s has %d columns, expected %d" % (name, t.shape[1], cols))
    return t


def _ld(t: torch.Tensor) -> int:
    return max(int(t.stride(0)), int(t.shape[1])) if t.shape[0] > 1 else int(t.shape[1])


def _vec(t: Optional[torch.Tensor], name: str, n: int, dtype=torch.float32):
    if t is None:
        return None
    if not t.is_cuda or t.dtype != dtype or t.numel() != n or not t.is_contiguous():
        raise ValueError("%s must be a contiguous %s CUDA vector of %d" % (name, dtype, n))
    return t


def rowmajor(t: torch.Tensor) -> torch.Tensor:
    """A view usable by the kernels (unit column stride), copying only if needed."""
    if t.dim() == 2 and (t.shape[1] <= 1 or t.stride(1) == 1) and (t.shape[0] <= 1 or t.stride(0) >= t.shape[1]):
        return t
    return t.contiguous()


# ------------------------------------------------------------------ raw kernels
def gather_sum(g: BatchGraph, x: torch.Tensor, out: Optional[torch.Tensor] = None,
               accumulate: bool = False) -> torch.Tensor:
    _mat(x, "x", rows=g.n_atoms)
    F_ = x.shape[1]
    if out is None:
        if accumulate:
            raise ValueError("accumulate needs an output")
        out = torch.empty((g.n_atoms, F_), dtype=torch.float32, device=x.device)
    _mat(out, "out", rows=g.n_atoms, cols=F_)
    _lib.call("gcmi_gather_sum_fwd", g.ref, _ptr(x), _ld(x), F_, _ptr(out), _ld(out),
              1 if accumulate else 0, _stream())
    return out


def scatter_add(g: BatchGraph, ds: torch.Tensor, dx: torch.Tensor) -> torch.Tensor:
    _mat(ds, "ds", rows=g.n_atoms)
    _mat(dx, "dx", rows=g.n_atoms, cols=ds.shape[1])
    _lib.call("gcmi_scatter_add", g.ref, _ptr(ds), _ld(ds), ds.shape[1], _ptr(dx), _ld(dx), _stream())
    return dx


def _arg_rows(arg, n_atoms: int, n_feat: int):
    if arg.dtype != torch.uint8 or tuple(arg.shape) != (n_atoms, n_feat) or not arg.is_contiguous() or not arg.is_cuda:
        raise ValueError("bad arg tensor")
    return arg


def _out_rows(out, like: torch.Tensor, n_atoms: int, n_feat: int, name: str = "out"):
    """The caller's output rows (checked), or fresh ones of ``like``'s type."""
    if out is None:
        return torch.empty((n_atoms, n_feat), dtype=like.dtype, device=like.device)
    return _mat(out, name, rows=n_atoms, cols=n_feat, dtype=like.dtype)


def gather_max(g: BatchGraph, x: torch.Tensor, scale=None, shift=None, want_arg: bool = True, out=None, arg=None):
    _mat(x, "x", rows=g.n_atoms)
    F_ = x.shape[1]
    _vec(scale, "scale", F_)
    _vec(shift, "shift", F_)
    out = _out_rows(out, x, g.n_atoms, F_)
    if arg is not None:
        _arg_rows(arg, g.n_atoms, F_)
    elif want_arg:
        arg = torch.empty((g.n_atoms, F_), dtype=torch.uint8, device=x.device)
    _lib.call("gcmi_gather_max_fwd", g.ref, _ptr(x), _ld(x), F_, _ptr(scale), _ptr(shift), _ptr(out),
              _ld(out), _ptr(arg), _stream())
    return out, arg


def gather_max_sum(g: BatchGraph, y: torch.Tensor, scale=None, shift=None, want_arg: bool = True, pool=None, arg=None,
                   s=None):
    """``gather_max`` of ``y`` and ``gather_sum`` of its result, bit for bit, in one window pass where the batch allows.
    Returns (pooled rows, arg bytes or None, neighbour sums of the pooled rows)."""
    _mat(y, "y", rows=g.n_atoms)
    F_ = y.shape[1]
    _vec(scale, "scale", F_)
    _vec(shift, "shift", F_)
    pool = _out_rows(pool, y, g.n_atoms, F_, "pool")
    if arg is not None:
        _arg_rows(arg, g.n_atoms, F_)
    elif want_arg:
        arg = torch.empty((g.n_atoms, F_), dtype=torch.uint8, device=y.device)
    s = _out_rows(s, y, g.n_atoms, F_, "s")
    _lib.call("gcmi_gather_max_sum_fwd", g.ref, _ptr(y), _ld(y), F_, _ptr(scale), _ptr(shift), _ptr(pool),
              _ld(pool), _ptr(arg), _ptr(s), _ld(s), _stream())
    return pool, arg, s


def max_sum_launches() -> int:
    """Launches so far of the window pass behind ``gather_max_sum`` (and the model forward between two blocks)."""
    v = ctypes.c_int32(0)
    _lib.call("gcmi_get_option", _lib.GCMI_OPT_MAX_SUM_LAUNCHES, ctypes.byref(v))
    return v.value


def gather_max_bwd(g: BatchGraph, dout: torch.Tensor, arg: torch.Tensor, out=None) -> torch.Tensor:
    """``out``: the caller's dx rows -- only with reverse slots, where every row is written once (the atomic form
    adds into rows this function zeroes)."""
    _mat(dout, "dout", rows=g.n_atoms)
    F_ = dout.shape[1]
    if arg.dtype != torch.uint8 or tuple(arg.shape) != (g.n_atoms, F_) or not arg.is_contiguous():
        raise ValueError("bad arg tensor")
    if g.ensure_rev_pos():  # gather form: every row written once, no atomics
        dx = _out_rows(out, dout, g.n_atoms, F_, "out")
    else:
        if out is not None:
            raise ValueError("out needs a graph with reverse slots")
        dx = torch.zeros((g.n_atoms, F_), dtype=torch.float32, device=dout.device)
    _lib.call("gcmi_gather_max_bwd", g.ref, _ptr(dout), _ld(dout), F_, _ptr(arg), _ptr(dx), _ld(dx),
              _stream())
    return dx


# ------------------------------------------------------------------ the window passes, one operation each
# (include/gcmi.h, "the molecule-window passes"): bf16 rows are torch.bfloat16 tensors.  No other kernel stands behind
# these: a batch, width or LDS size without window pass raises GcmiError (status GCMI_ERR_UNSUPPORTED).
_BF16 = torch.bfloat16


def win_sum_h(g: BatchGraph, x: torch.Tensor, out: Optional[torch.Tensor] = None, accumulate: bool = False):
    """Neighbour sums of bf16 rows, bf16 out (``accumulate``: added to ``out``)."""
    _mat(x, "x", rows=g.n_atoms, dtype=_BF16)
    F_ = x.shape[1]
    if out is None and accumulate:
        raise ValueError("accumulate needs an output")
    out = _out_rows(out, x, g.n_atoms, F_)
    _lib.call("gcmi_win_sum_h", g.ref, _ptr(x), _ld(x), F_, _ptr(out), _ld(out), 1 if accumulate else 0, _stream())
    return out


def win_sum_fh(g: BatchGraph, x: torch.Tensor, ldo: int, s=None, xcopy=None):
    """float rows -> (bf16 neighbour sums, bf16 copy of the rows), both ``ldo`` columns wide, zero beyond x's."""
    _mat(x, "x", rows=g.n_atoms)
    F_ = x.shape[1]
    outs = []
    for t, name in ((s, "s"), (xcopy, "xcopy")):
        if t is None:
            t = torch.empty((g.n_atoms, ldo), dtype=_BF16, device=x.device)
        _mat(t, name, rows=g.n_atoms, cols=ldo, dtype=_BF16)
        if _ld(t) != ldo:  # (one number is the row pitch and the end of the zeroed columns)
            raise ValueError("%s: row stride %d, expected %d" % (name, _ld(t), ldo))
        outs.append(t)
    _lib.call("gcmi_win_sum_fh", g.ref, _ptr(x), _ld(x), F_, _ptr(outs[0]), _ptr(outs[1]), int(ldo), _stream())
    return outs[0], outs[1]


def win_max_h(g: BatchGraph, x: torch.Tensor, scale=None, shift=None, want_arg: bool = True, out=None, arg=None):
    """``gather_max`` over bf16 rows: (bf16 pooled rows, arg bytes or None)."""
    _mat(x, "x", rows=g.n_atoms, dtype=_BF16)
    F_ = x.shape[1]
    _vec(scale, "scale", F_)
    _vec(shift, "shift", F_)
    out = _out_rows(out, x, g.n_atoms, F_)
    if arg is not None:
        _arg_rows(arg, g.n_atoms, F_)
    elif want_arg:
        arg = torch.empty((g.n_atoms, F_), dtype=torch.uint8, device=x.device)
    _lib.call("gcmi_win_max_h", g.ref, _ptr(x), _ld(x), F_, _ptr(scale), _ptr(shift), _ptr(out), _ld(out), _ptr(arg),
              _stream())
    return out, arg


def _need_rev_pos(g: BatchGraph):
    if not g.ensure_rev_pos():
        raise _lib.GcmiError("the window backward passes need reverse slots (a symmetric adjacency)")


def win_max_bwd_h(g: BatchGraph, dout: torch.Tensor, arg: torch.Tensor, gamma=None, beta=None, out=None):
    """GraphPool backward over bf16 rows.  With ``gamma``/``beta`` the rows are written only where some column has
    |beta| > 64 |gamma| (pass ``out`` to see which)."""
    _mat(dout, "dout", rows=g.n_atoms, dtype=_BF16)
    F_ = dout.shape[1]
    _arg_rows(arg, g.n_atoms, F_)
    _vec(gamma, "gamma", F_)
    _vec(beta, "beta", F_)
    _need_rev_pos(g)
    out = _out_rows(out, dout, g.n_atoms, F_)
    _lib.call("gcmi_win_max_bwd_h", g.ref, _ptr(dout), _ld(dout), F_, _ptr(arg), _ptr(out), _ld(out), _ptr(gamma),
              _ptr(beta), _stream())
    return out


def win_max_bwd_if_ill(g: BatchGraph, dout: torch.Tensor, arg: torch.Tensor, gamma, beta, out=None):
    """GraphPool backward over float rows, written only where some column has |beta| > 64 |gamma|."""
    _mat(dout, "dout", rows=g.n_atoms)
    F_ = dout.shape[1]
    _arg_rows(arg, g.n_atoms, F_)
    if gamma is None or beta is None:
        raise ValueError("gamma and beta are needed")
    _vec(gamma, "gamma", F_)
    _vec(beta, "beta", F_)
    _need_rev_pos(g)
    out = _out_rows(out, dout, g.n_atoms, F_)
    _lib.call("gcmi_win_max_bwd_if_ill", g.ref, _ptr(dout), _ld(dout), F_, _ptr(arg), _ptr(out), _ld(out), _ptr(gamma),
              _ptr(beta), _stream())
    return out


def win_sumacc_max_bwd(g: BatchGraph, ds: torch.Tensor, dxs: torch.Tensor, arg: torch.Tensor, out=None):
    """The backward between two GraphConv blocks over float or bf16 rows: dy = GraphPool backward (by ``arg``) of
    dX = dxs + neighbour sums of ds.  ``dxs`` is completed in place on the rows of oversized windows only."""
    if ds.dtype not in (torch.float32, _BF16):
        raise TypeError("ds must be float32 or bfloat16, got %s" % ds.dtype)
    _mat(ds, "ds", rows=g.n_atoms, dtype=ds.dtype)
    F_ = ds.shape[1]
    _mat(dxs, "dxs", rows=g.n_atoms, cols=F_, dtype=ds.dtype)
    _arg_rows(arg, g.n_atoms, F_)
    _need_rev_pos(g)
    out = _out_rows(out, ds, g.n_atoms, F_)
    name = "gcmi_win_sumacc_max_bwd" if ds.dtype == torch.float32 else "gcmi_win_sumacc_max_bwd_h"
    _lib.call(name, g.ref, _ptr(ds), _ld(ds), F_, _ptr(dxs), _ld(dxs), _ptr(arg), _ptr(out), _ld(out), _stream())
    return out


def readout(g: BatchGraph, x: torch.Tensor, n_mols: int, scale=None, shift=None, tanh: bool = False):
    _mat(x, "x", rows=g.n_atoms)
    F_ = x.shape[1]
    _vec(scale, "scale", F_)
    _vec(shift, "shift", F_)
    g.set_mols(n_mols)
    out = torch.empty((n_mols, 2 * F_), dtype=torch.float32, device=x.device)
    arg = torch.empty((n_mols, F_), dtype=torch.int32, device=x.device)
    _lib.call("gcmi_readout_fwd", g.ref, _ptr(x), _ld(x), F_, _ptr(scale), _ptr(shift),
              1 if tanh else 0, _ptr(out), _ld(out), _ptr(arg), _stream())
    return out, arg


def readout_bwd(g: BatchGraph, dout: torch.Tensor, out: torch.Tensor, arg: torch.Tensor,
                tanh: bool) -> torch.Tensor:
    F_ = arg.shape[1]
    _mat(dout, "dout", rows=g.n_mols, cols=2 * F_)
    _mat(out, "out", rows=g.n_mols, cols=2 * F_)
    if arg.dtype != torch.int32 or arg.shape[0] != g.n_mols or not arg.is_contiguous():
        raise ValueError("bad arg tensor")
    dx = torch.empty((g.n_atoms, F_), dtype=torch.float32, device=dout.device)
    _lib.call("gcmi_readout_bwd", g.ref, _ptr(dout), _ld(dout), _ptr(out), _ld(out), F_,
              1 if tanh else 0, _ptr(arg), _ptr(dx), _ld(dx), _stream())
    return dx


def bn_stats(x, gamma, beta, running_mean, running_var, eps: float, momentum: float):
    """Training statistics + folded scale/shift; updates running stats in place."""
    _mat(x, "x")
    n, F_ = x.shape
    if n < 1:
        raise ValueError("batch norm over zero rows")
    dev = x.device
    mean = torch.empty(F_, dtype=torch.float32, device=dev)
    invstd = torch.empty(F_, dtype=torch.float32, device=dev)
    scale = torch.empty(F_, dtype=torch.float32, device=dev)
    shift = torch.empty(F_, dtype=torch.float32, device=dev)
    acc = torch.empty(_lib.bn_acc_doubles(F_), dtype=torch.float64, device=dev)
    _lib.call("gcmi_bn_stats", _ptr(x), _ld(x), n, F_, _ptr(_vec(gamma, "gamma", F_)),
              _ptr(_vec(beta, "beta", F_)), float(eps), float(momentum),
              _ptr(_vec(running_mean, "running_mean", F_)), _ptr(_vec(running_var, "running_var", F_)),
              _ptr(mean), _ptr(invstd), _ptr(scale), _ptr(shift), _ptr(acc), _stream())
    return mean, invstd, scale, shift


def bn_fold_eval(gamma, beta, running_mean, running_var, eps: float):
    F_ = running_mean.numel()
    scale = torch.empty(F_, dtype=torch.float32, device=running_mean.device)
    shift = torch.empty_like(scale)
    _lib.call("gcmi_bn_fold_eval", _ptr(_vec(gamma, "gamma", F_)), _ptr(_vec(beta, "beta", F_)),
              _ptr(_vec(running_mean, "running_mean", F_)), _ptr(_vec(running_var, "running_var", F_)),
              float(eps), F_, _ptr(scale), _ptr(shift), _stream())
    return scale, shift


def bn_apply(x, scale, shift):
    _mat(x, "x")
    n, F_ = x.shape
    y = torch.empty((n, F_), dtype=torch.float32, device=x.device)
    _lib.call("gcmi_bn_apply", _ptr(x), _ld(x), n, F_, _ptr(_vec(scale, "scale", F_)),
              _ptr(_vec(shift, "shift", F_)), _ptr(y), _ld(y), _stream())
    return y


def bn_bwd(dy, x, gamma, mean, invstd, need_dx: bool, relu_mask: bool = False):
    _mat(dy, "dy")
    _mat(x, "x", rows=dy.shape[0], cols=dy.shape[1])
    n, F_ = x.shape
    dev = x.device
    dgamma = torch.empty(F_, dtype=torch.float32, device=dev)
    dbeta = torch.empty(F_, dtype=torch.float32, device=dev)
    dx = torch.empty((n, F_), dtype=torch.float32, device=dev) if need_dx else None
    acc = torch.empty(_lib.bn_acc_doubles(F_), dtype=torch.float64, device=dev)
    _lib.call("gcmi_bn_bwd", _ptr(dy), _ld(dy), _ptr(x), _ld(x), n, F_, _ptr(_vec(gamma, "gamma", F_)),
              _ptr(_vec(mean, "mean", F_)), _ptr(_vec(invstd, "invstd", F_)), _ptr(dgamma), _ptr(dbeta),
              _ptr(dx), _ld(dx) if need_dx else 0, 1 if relu_mask else 0, _ptr(acc), _stream())
    return dgamma, dbeta, dx


def _i32arr(vals):
    return (ctypes.c_int32 * len(vals))(*[int(v) for v in vals])


def _i64arr(vals):
    return (ctypes.c_int64 * len(vals))(*[int(v) for v in vals])


def seg_gemm(seg_begin, seg_end, a1, w1, w1_off, a2, w2, w2_off, bias, bias_off, n_out: int,
             trans_w: bool, relu: bool, n_rows: int, k1: int = 0, k2: int = 0,
             out: Optional[torch.Tensor] = None, accumulate: bool = False) -> torch.Tensor:
    """out[n_rows, n_out]; rows not covered by any segment are left undefined.
    w1 / w2 / bias are flat float32 CUDA tensors holding the blocks at the
    given offsets (in floats).  ``out``: write into this (n_rows, n_out) matrix (a column block of a
    wider one is fine) instead of a fresh one.  ``accumulate``: out += result (act = 2 of gcmi_seg_gemm) instead
    of out = result; needs ``out`` and excludes ``relu``."""
    if accumulate and relu:
        raise ValueError("accumulate and relu are mutually exclusive")
    if accumulate and out is None:
        raise ValueError("accumulate needs the matrix to add to: pass out")
    n_seg = len(seg_begin)
    dev = (a1 if a1 is not None else a2).device
    for s in range(n_seg):
        if not (0 <= seg_begin[s] <= seg_end[s] <= n_rows):
            raise ValueError("segment %d = [%d,%d) outside [0,%d]" % (s, seg_begin[s], seg_end[s], n_rows))
    for a, w, off, k, nm in ((a1, w1, w1_off, k1, "a1"), (a2, w2, w2_off, k2, "a2")):
        if a is None:
            continue
        _mat(a, nm, rows=n_rows, cols=k)
        if w is None or w.dtype != torch.float32 or not w.is_cuda or not w.is_contiguous():
            raise ValueError("weights of %s must be a contiguous float32 CUDA tensor" % nm)
        for s in range(n_seg):
            if off[s] >= 0 and off[s] + k * n_out > w.numel():
                raise ValueError("weight block %d of %s runs past the buffer" % (s, nm))
    if bias is not None:
        if bias.dtype != torch.float32 or not bias.is_cuda or not bias.is_contiguous():
            raise ValueError("bias must be a contiguous float32 CUDA tensor")
        for s in range(n_seg):
            if bias_off[s] >= 0 and bias_off[s] + n_out > bias.numel():
                raise ValueError("bias block %d runs past the buffer" % s)
    if out is None:
        out = torch.empty((n_rows, n_out), dtype=torch.float32, device=dev)
    else:
        _mat(out, "out", rows=n_rows, cols=n_out)
    _lib.call("gcmi_seg_gemm", n_seg, _i32arr(seg_begin), _i32arr(seg_end),
              _ptr(a1), _ld(a1) if a1 is not None else 0, k1, _ptr(w1),
              _i64arr(w1_off) if a1 is not None else None,
              _ptr(a2), _ld(a2) if a2 is not None else 0, k2, _ptr(w2),
              _i64arr(w2_off) if a2 is not None else None,
              _ptr(bias), _i64arr(bias_off) if bias is not None else None, n_out,
              1 if trans_w else 0, 2 if accumulate else (1 if relu else 0), _ptr(out), _ld(out), _stream())
    return out


def _trans_w(layout: str) -> bool:
    if layout not in ("out_in", "in_out"):
        raise ValueError("layout must be 'out_in' (nn.Linear) or 'in_out' (Keras), got %r" % (layout,))
    return layout == "out_in"


def dense(x, w, b=None, *, layout: str, x2=None, w2=None, relu: bool = False, out=None, accumulate: bool = False):
    """act(x . W [+ x2 . W2] + b) over all rows: ``seg_gemm`` with the one segment [0, rows).  ``w`` / ``w2`` are
    matrices, ``layout`` says which way round: "out_in" is nn.Linear's (n_out, k), "in_out" the Keras (k, n_out)."""
    trans_w = _trans_w(layout)
    n, k = x.shape
    n_out = w.shape[0] if trans_w else w.shape[1]
    k2 = 0 if x2 is None else x2.shape[1]
    if (x2 is None) != (w2 is None):
        raise ValueError("x2 and w2 go together")
    for wm, kk, nm in ((w, k, "w"), (w2, k2, "w2")):
        if wm is not None and wm.shape != ((n_out, kk) if trans_w else (kk, n_out)):
            raise ValueError("%s %s is no %d -> %d matrix in the %s layout" % (nm, tuple(wm.shape), kk, n_out, layout))
    if b is not None and b.numel() != n_out:
        raise ValueError("bias has %d elements, expected %d" % (b.numel(), n_out))
    if n == 0:  # (nothing to launch, and an empty tensor has no address to hand over)
        return out if out is not None else torch.empty((0, n_out), dtype=torch.float32, device=x.device)
    return seg_gemm([0], [n], x, w.reshape(-1), [0], x2, None if x2 is None else w2.reshape(-1),
                    None if x2 is None else [0], b, [0], n_out, trans_w, relu, n, k, k2, out=out, accumulate=accumulate)


def task_head_forward(fingerprint: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor],
                      scratch: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """logits = fingerprint . weight^T + bias with nn.Linear's (n_out, k) weight, as the whole-model path runs the task
    head (gcmi_task_head_forward): with 33..256 outputs and a ``scratch`` of ``task_head_scratch_floats()`` floats, from
    fragment images of the weight prepared in it."""
    _mat(fingerprint, "fingerprint")
    n, k = fingerprint.shape
    n_out = weight.shape[0]
    if weight.shape != (n_out, k) or weight.dtype != torch.float32 or not weight.is_cuda or not weight.is_contiguous():
        raise ValueError("weight must be a contiguous float32 CUDA tensor of shape (n_out, %d)" % k)
    if out is None:
        out = torch.empty((n, n_out), dtype=torch.float32, device=fingerprint.device)
    _lib.call("gcmi_task_head_forward", _ptr(fingerprint), _ld(fingerprint), n, k, _ptr(weight),
              _ptr(bias) if bias is not None else None, n_out, _ptr(scratch) if scratch is not None else None, _ptr(out),
              _ld(out), _stream())
    return out


def task_head_scratch_floats() -> int:
    return int(_lib.load().gcmi_task_head_scratch_floats())


# ---- the persistent block kernels alone (gcmi_fwd_fused_gemm*, gcmi_fused_*_bwd): no other kernel behind a refusal,
# which raises GcmiError with status -3
def fwd_fused_scratch_floats() -> int:
    return int(_lib.load().gcmi_fwd_fused_scratch_floats())


def _flat(t, name, dtype=torch.float32):
    if t is None or t.dtype != dtype or not t.is_cuda or not t.is_contiguous():
        raise ValueError("%s must be a contiguous %s CUDA tensor" % (name, dtype))
    return t


def _blocks_inside(off, size, buf, name):
    for s, o in enumerate(off):
        if o >= 0 and o + size > buf.numel():
            raise ValueError("%s block %d runs past the buffer" % (name, s))


def _segments_inside(seg_begin, seg_end, n_rows):
    for s in range(len(seg_begin)):
        if not (0 <= seg_begin[s] <= seg_end[s] <= n_rows):
            raise ValueError("segment %d = [%d,%d) outside [0,%d]" % (s, seg_begin[s], seg_end[s], n_rows))


def _acc(t, name, n_feat):
    if t is not None and (t.dtype != torch.float64 or not t.is_cuda or not t.is_contiguous() or
                          t.numel() < _lib.bn_acc_doubles(n_feat)):
        raise ValueError("%s must be a contiguous float64 CUDA tensor of >= %d" % (name, _lib.bn_acc_doubles(n_feat)))
    return t


def fwd_fused_gemm(seg_begin, seg_end, a1, w1, w1_off, a2, w2, w2_off, bias, bias_off, n_out: int, trans_w: bool,
                   relu: bool, n_rows: int, k1: int, k2: int, out: torch.Tensor, stats=None, scratch=None):
    """gcmi_seg_gemm's contract on the persistent forward kernels alone.  float32 operand rows: gcmi_fwd_fused_gemm;
    bfloat16 operand rows: gcmi_fwd_fused_gemm_h, ``out`` bfloat16 or float32.  ``stats``: 66 * n_out doubles the
    column sums of out and out^2 are added into; ``scratch``: fwd_fused_scratch_floats() floats."""
    _segments_inside(seg_begin, seg_end, n_rows)
    half = a1.dtype == torch.bfloat16
    for a, w, off, k, nm in ((a1, w1, w1_off, k1, "a1"), (a2, w2, w2_off, k2, "a2")):
        if a is None:
            continue
        _mat(a, nm, rows=n_rows, cols=k, dtype=a1.dtype)
        _blocks_inside(off, k * n_out, _flat(w, "weights of " + nm), "weight")
    if bias is not None:
        _blocks_inside(bias_off, n_out, _flat(bias, "bias"), "bias")
    _mat(out, "out", rows=n_rows, cols=n_out, dtype=out.dtype if half else torch.float32)
    if half and out.dtype not in (torch.bfloat16, torch.float32):
        raise TypeError("out must be bfloat16 or float32")
    _acc(stats, "stats", n_out)
    if scratch is not None and (_flat(scratch, "scratch").numel() < fwd_fused_scratch_floats()):
        raise ValueError("scratch must hold fwd_fused_scratch_floats() floats")
    head = (len(seg_begin), _i32arr(seg_begin), _i32arr(seg_end),
            _ptr(a1), _ld(a1), k1, _ptr(w1), _i64arr(w1_off),
            _ptr(a2), _ld(a2) if a2 is not None else 0, k2, _ptr(w2), _i64arr(w2_off) if a2 is not None else None,
            _ptr(bias), _i64arr(bias_off) if bias is not None else None, n_out, 1 if trans_w else 0, 1 if relu else 0,
            _ptr(out), _ld(out))
    if half:
        _lib.call("gcmi_fwd_fused_gemm_h", *head, 1 if out.dtype == torch.float32 else 0, _ptr(stats), _ptr(scratch),
                  _stream())
    else:
        _lib.call("gcmi_fwd_fused_gemm", *head, _ptr(stats), _ptr(scratch), _stream())
    return out


def fused_bwd_launches() -> int:
    v = ctypes.c_int32(0)
    _lib.call("gcmi_get_option", _lib.GCMI_OPT_FUSED_BWD_LAUNCHES, ctypes.byref(v))
    return int(v.value)


def _rows_dtype(flag):
    return torch.bfloat16 if flag else torch.float32


def fused_conv_bwd(seg_begin, seg_end, w_rel_off, w_self_off, b_off, dy, gc, coef, s, x, w, dw, db, ds=None, dxs=None,
                   psums=None, act_bf16: int = 0, in_bf16: int = 0):
    """The one-pass backward of a 64-column GraphConv block (gcmi_fused_conv_bwd): dw / db are added into, ds / dxs
    written.  act_bf16 1: gc, s, x bfloat16; 2: dy, ds, dxs too; in_bf16: s and x alone."""
    n = gc.shape[0]
    k = s.shape[1]
    _segments_inside(seg_begin, seg_end, n)
    _mat(dy, "dy", rows=n, cols=64, dtype=_rows_dtype(act_bf16 == 2))
    _mat(gc, "gc", rows=n, cols=64, dtype=_rows_dtype(act_bf16))
    _mat(s, "s", rows=n, cols=k, dtype=_rows_dtype(act_bf16 or in_bf16))
    _mat(x, "x", rows=n, cols=k, dtype=_rows_dtype(act_bf16 or in_bf16))
    for t, nm in ((ds, "ds"), (dxs, "dxs")):
        if t is not None:
            _mat(t, nm, rows=n, cols=k, dtype=_rows_dtype(act_bf16 == 2))
    _vec(coef, "coef", 192)
    _flat(w, "w"), _flat(dw, "dw")
    for off in (w_rel_off, w_self_off):
        _blocks_inside(off, k * 64, w, "weight")
        _blocks_inside(off, k * 64, dw, "dw")
    if db is not None:
        _blocks_inside(b_off, 64, _flat(db, "db"), "db")
    _acc(psums, "psums", k)
    _lib.call("gcmi_fused_conv_bwd", len(seg_begin), _i32arr(seg_begin), _i32arr(seg_end), _i64arr(w_rel_off),
              _i64arr(w_self_off), _i64arr(b_off) if b_off is not None else None, _ptr(dy), _ld(dy), _ptr(gc), _ld(gc),
              _ptr(coef), _ptr(s), _ld(s), _ptr(x), _ld(x), k, _ptr(w), _ptr(dw), _ptr(db),
              _ptr(ds), _ld(ds) if ds is not None else 0, _ptr(dxs), _ld(dxs) if dxs is not None else 0, _ptr(psums),
              int(act_bf16), int(in_bf16), _stream())


def fused_dense_bwd(seg_begin, seg_end, w_off, b_off, membership, g2, arg, gc, coef, p, w, dw, db, dp, psums=None,
                    act_bf16: int = 0):
    """The one-pass backward of the 128-column dense block behind the readout (gcmi_fused_dense_bwd): dy is recomputed
    from g2 = [dsum | dmax] per molecule and arg; dw (128 x k) / db are added into, dp written."""
    n = gc.shape[0]
    k = p.shape[1]
    n_mols = g2.shape[0]
    _segments_inside(seg_begin, seg_end, n)
    _mat(g2, "g2", cols=256)
    if arg.dtype != torch.int32 or not arg.is_cuda or not arg.is_contiguous() or tuple(arg.shape) != (n_mols, 128):
        raise ValueError("arg must be a contiguous int32 CUDA tensor of shape (%d, 128)" % n_mols)
    _vec(membership, "membership", n, dtype=torch.int32)
    if n and not (0 <= int(membership.min()) and int(membership.max()) < n_mols):
        raise ValueError("membership outside [0, %d)" % n_mols)
    _mat(gc, "gc", rows=n, cols=128, dtype=_rows_dtype(act_bf16))
    _mat(p, "p", rows=n, cols=k, dtype=_rows_dtype(act_bf16))
    _mat(dp, "dp", rows=n, cols=k, dtype=_rows_dtype(act_bf16 == 2))
    _vec(coef, "coef", 384)
    _flat(w, "w"), _flat(dw, "dw")
    _blocks_inside(w_off, k * 128, w, "weight")
    _blocks_inside(w_off, k * 128, dw, "dw")
    if db is not None:
        _blocks_inside(b_off, 128, _flat(db, "db"), "db")
    _acc(psums, "psums", k)
    _lib.call("gcmi_fused_dense_bwd", len(seg_begin), _i32arr(seg_begin), _i32arr(seg_end), _i64arr(w_off),
              _i64arr(b_off) if b_off is not None else None, _ptr(membership), _ptr(g2), _ld(g2), _ptr(arg), n_mols,
              _ptr(gc), _ld(gc), _ptr(coef), _ptr(p), _ld(p), k, _ptr(w), _ptr(dw), _ptr(db), _ptr(dp), _ld(dp),
              _ptr(psums), int(act_bf16), _stream())


def head_backward(kind: int, logits, labels, weights, n_rows: int, n_tasks: int, n_classes: int, fp, w, dw, db, g2,
                  loss_acc, sums=None, runs=None, arg=None, rawsum=None, mean=None, invstd=None, dl_scratch=None,
                  img_scratch=None) -> int:
    """The per-molecule head backward kernels alone (gcmi_head_backward): loss (the sum of w l, ADDED into the 16
    doubles of ``loss_acc``), d logits, dw (outputs x 256) / db added into, g2 written for every row of ``fp``, and
    with ``sums`` (66 * 128 doubles) the dense BatchNorm's backward sums added from ``runs`` (n_mols, n_deg, 2),
    ``arg`` (n_mols, 128), ``rawsum`` (n_mols, 256), ``mean`` and ``invstd`` (128).  logits / labels hold at least
    n_rows x outputs floats, weights n_rows x n_tasks.  Returns the route: 0 head_bwd_kernel, 1 the wide pair
    (which needs ``dl_scratch``, n_mols x outputs floats, and ``img_scratch``, task_head_scratch_floats() floats)."""
    n_out = n_tasks * (n_classes if kind == 0 else 1)
    _mat(fp, "fp", cols=256)
    n_mols = fp.shape[0]
    _mat(g2, "g2", rows=n_mols, cols=256)
    if not 1 <= n_rows <= n_mols:
        raise ValueError("n_rows %d outside [1, %d]" % (n_rows, n_mols))
    for t, nm, need in ((logits, "logits", n_rows * n_out), (labels, "labels", n_rows * n_out)):
        if _flat(t, nm).numel() < need:
            raise ValueError("%s holds fewer than n_rows x outputs = %d floats" % (nm, need))
    if weights is not None and _flat(weights, "weights").numel() < n_rows * n_tasks:
        raise ValueError("weights holds fewer than n_rows x n_tasks = %d floats" % (n_rows * n_tasks))
    if _flat(w, "w").numel() < n_out * 256 or _flat(dw, "dw").numel() < n_out * 256:
        raise ValueError("w and dw must hold outputs x 256 = %d floats" % (n_out * 256))
    if db is not None and _flat(db, "db").numel() < n_out:
        raise ValueError("db must hold %d floats" % n_out)
    if _flat(loss_acc, "loss_acc", torch.float64).numel() < 16:
        raise ValueError("loss_acc must hold 16 doubles")
    n_deg = 1  # (sums without runs: the entry's refusal, not an argument error)
    if sums is not None:
        _acc(sums, "sums", 128)
        if runs is not None:
            if runs.dtype != torch.int32 or not runs.is_cuda or not runs.is_contiguous() or runs.dim() != 3 or \
                    runs.shape[0] != n_mols or runs.shape[2] != 2:
                raise ValueError("runs must be a contiguous int32 CUDA tensor of shape (%d, n_deg, 2)" % n_mols)
            n_deg = runs.shape[1]
        if arg is not None and (arg.dtype != torch.int32 or not arg.is_cuda or not arg.is_contiguous() or
                                tuple(arg.shape) != (n_mols, 128)):
            raise ValueError("arg must be a contiguous int32 CUDA tensor of shape (%d, 128)" % n_mols)
        if rawsum is not None and not _mat(rawsum, "rawsum", rows=n_mols, cols=256).is_contiguous():
            raise ValueError("rawsum must be contiguous")
        _vec(mean, "mean", 128), _vec(invstd, "invstd", 128)
    if dl_scratch is not None and _flat(dl_scratch, "dl_scratch").numel() < n_mols * n_out:
        raise ValueError("dl_scratch must hold n_mols x outputs = %d floats" % (n_mols * n_out))
    if img_scratch is not None and _flat(img_scratch, "img_scratch").numel() < task_head_scratch_floats():
        raise ValueError("img_scratch must hold task_head_scratch_floats() floats")
    route = ctypes.c_int32(-1)
    _lib.call("gcmi_head_backward", int(kind), _ptr(logits), _ptr(labels), _ptr(weights), n_rows, n_tasks, n_classes,
              _ptr(fp), _ld(fp), n_mols, _ptr(w), _ptr(dw), _ptr(db), _ptr(g2), _ld(g2), _ptr(loss_acc), _ptr(sums),
              _ptr(runs), n_deg, _ptr(arg), _ptr(rawsum), _ptr(mean), _ptr(invstd), _ptr(dl_scratch), _ptr(img_scratch),
              ctypes.byref(route), _stream())
    return int(route.value)


def seg_gemm_wgrad(seg_begin, seg_end, a, g, dw, dw_off, dbias, dbias_off, trans_w: bool):
    """dw (+)= a^T g per segment; dw / dbias are flat, pre-zeroed, accumulated in place."""
    n_seg = len(seg_begin)
    _mat(a, "a")
    _mat(g, "g", rows=a.shape[0])
    k, n = a.shape[1], g.shape[1]
    for s in range(n_seg):
        if not (0 <= seg_begin[s] <= seg_end[s] <= a.shape[0]):
            raise ValueError("bad segment %d" % s)
        if dw_off[s] >= 0 and dw_off[s] + k * n > dw.numel():
            raise ValueError("dw block %d runs past the buffer" % s)
        if dbias is not None and dbias_off[s] >= 0 and dbias_off[s] + n > dbias.numel():
            raise ValueError("dbias block %d runs past the buffer" % s)
    if dw.dtype != torch.float32 or not dw.is_cuda or not dw.is_contiguous():
        raise ValueError("dw must be a contiguous float32 CUDA tensor")
    _lib.call("gcmi_seg_gemm_wgrad", n_seg, _i32arr(seg_begin), _i32arr(seg_end), _ptr(a), _ld(a), k,
              _ptr(g), _ld(g), n, _ptr(dw), _i64arr(dw_off), _ptr(dbias),
              _i64arr(dbias_off) if dbias is not None else None, 1 if trans_w else 0, _stream())


def dense_wgrad(a, g, dw, db=None, *, layout: str):
    """dw += a^T g (``layout`` "in_out") or g^T a ("out_in"), db += column sums of g, over all rows: ``seg_gemm_wgrad``
    with the one segment [0, rows).  Nothing is launched for zero rows."""
    trans_w = _trans_w(layout)
    if a.shape[0] > 0:
        seg_gemm_wgrad([0], [a.shape[0]], a, g, dw, [0], db, [0], trans_w)


def relu_bwd_(g: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    _mat(g, "g")
    _mat(y, "y", rows=g.shape[0], cols=g.shape[1])
    if g.shape[0] > 0:
        _lib.call("gcmi_relu_bwd", _ptr(g), _ld(g), _ptr(y), _ld(y), g.shape[0], g.shape[1], _stream())
    return g


def loss_fwd_bwd(kind: int, logits, labels, weights, want_probs: bool = False):
    """(loss scalar tensor, dlogits, probs|None).  kind 0: softmax CE over the last
    dim of (rows, tasks, classes); kind 1: L2 over (rows, tasks)."""
    if not logits.is_cuda:
        raise _lib.GcmiError("loss needs CUDA tensors")
    logits = logits.contiguous()
    labels = labels.contiguous().to(torch.float32)
    if kind == 0:
        if logits.dim() == 2:
            logits = logits.unsqueeze(1)
            labels = labels.unsqueeze(1)
        n_rows, n_tasks, n_classes = logits.shape
    else:
        if logits.dim() == 1:
            logits = logits.unsqueeze(1)
        n_rows, n_tasks = logits.shape[0], logits[0].numel()
        n_classes = 1
    if labels.numel() != logits.numel():
        raise ValueError("labels %s do not match outputs %s" % (tuple(labels.shape), tuple(logits.shape)))
    if weights is not None:
        weights = weights.contiguous().to(torch.float32)
        if weights.numel() != n_rows * n_tasks:
            raise ValueError("weights %s do not match (%d, %d)" % (tuple(weights.shape), n_rows, n_tasks))
    dev = logits.device
    loss = torch.empty((), dtype=torch.float32, device=dev)
    dlogits = torch.empty_like(logits)
    probs = torch.empty_like(logits) if (want_probs and kind == 0) else None
    acc = torch.empty(1, dtype=torch.float64, device=dev)
    _lib.call("gcmi_loss_fwd_bwd", kind, _ptr(logits), _ptr(labels), _ptr(weights), n_rows, n_tasks,
              n_classes, _ptr(loss), _ptr(dlogits), _ptr(probs), _ptr(acc), _stream())
    return loss, dlogits, probs


def softmax_lastdim(logits: torch.Tensor) -> torch.Tensor:
    x = logits.contiguous()
    out = torch.empty_like(x)
    c = x.shape[-1]
    _lib.call("gcmi_softmax", _ptr(x), x.numel() // max(c, 1), c, _ptr(out), _stream())
    return out


def adam_step_(p, grad, m, v, lr, beta1, beta2, eps, step: int):
    n = p.numel()
    for t, nm in ((p, "param"), (grad, "grad"), (m, "exp_avg"), (v, "exp_avg_sq")):
        if not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != n:
            raise ValueError("adam: %s must be a contiguous float32 CUDA tensor of %d" % (nm, n))
    _lib.call("gcmi_adam_step", _ptr(p), _ptr(grad), _ptr(m), _ptr(v), n, float(lr), float(beta1),
              float(beta2), float(eps), int(step), _stream())


OPT_RULES = {"sgd": _lib.RULE_SGD, "adagrad": _lib.RULE_ADAGRAD, "rmsprop": _lib.RULE_RMSPROP,
             "adam_l2": _lib.RULE_ADAM_L2, "adamw": _lib.RULE_ADAMW, "lamb": _lib.RULE_LAMB}


def opt_desc(rule, beta1=0.0, beta2=0.0, eps=0.0, weight_decay=0.0, alpha=0.0, momentum=0.0) -> "_lib.GcmiOptDesc":
    """struct gcmi_opt_desc; ``rule``: a key of ``OPT_RULES`` or the number itself."""
    d = _lib.GcmiOptDesc()
    d.rule = OPT_RULES[rule] if isinstance(rule, str) else int(rule)
    d.beta1, d.beta2, d.eps = float(beta1), float(beta2), float(eps)
    d.weight_decay, d.alpha, d.momentum = float(weight_decay), float(alpha), float(momentum)
    return d


def _flat_f32(t, name, n):
    if t is None:
        return
    if not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != n:
        raise ValueError("%s must be a contiguous float32 CUDA tensor of %d" % (name, n))


def opt_step_(desc, p, grad, state1, state2, lr, step: int):
    """One elementwise optimizer step (gcmi_opt_step) on flat float32 tensors, in place.  ``state1`` / ``state2``:
    what the rule keeps (include/gcmi.h); None where it keeps nothing."""
    n = p.numel()
    for t, nm in ((p, "param"), (grad, "grad"), (state1, "state1"), (state2, "state2")):
        _flat_f32(t, "opt: " + nm, n)
    _lib.call("gcmi_opt_step", ctypes.byref(desc), _ptr(p), _ptr(grad), _ptr(state1), _ptr(state2), n, float(lr),
              int(step), _stream())


def lamb_scratch_floats(n: int, n_segments: int) -> int:
    need = int(_lib.load().gcmi_lamb_scratch_floats(int(n), int(n_segments)))
    if need < 0:
        raise ValueError("lamb: bad sizes (%d floats, %d segments)" % (n, n_segments))
    return need


def lamb_step_(desc, p, grad, m, v, scratch, segments, norms, lr):
    """One Lamb step (gcmi_lamb_step) over flat float32 arenas, in place.  ``segments``: int64 CUDA tensor
    (n_segments, 2) of (offset, numel); ``norms``: float32 CUDA tensor (n_segments, 3) or None; ``scratch``:
    ``lamb_scratch_floats`` floats."""
    n = p.numel()
    for t, nm in ((p, "param"), (grad, "grad"), (m, "exp_avg"), (v, "exp_avg_sq")):
        _flat_f32(t, "lamb: " + nm, n)
    if (not segments.is_cuda or segments.dtype != torch.int64 or not segments.is_contiguous() or segments.dim() != 2
            or segments.shape[1] != 2):
        raise ValueError("lamb: segments must be a contiguous int64 CUDA tensor (n_segments, 2)")
    n_seg = int(segments.shape[0])
    _flat_f32(scratch, "lamb: scratch", scratch.numel())
    if scratch.numel() < lamb_scratch_floats(n, n_seg):
        raise ValueError("lamb: the scratch holds %d floats, %d needed" % (scratch.numel(), lamb_scratch_floats(n, n_seg)))
    if norms is not None:
        _flat_f32(norms, "lamb: norms", 3 * n_seg)
    _lib.call("gcmi_lamb_step", ctypes.byref(desc), _ptr(p), _ptr(grad), _ptr(m), _ptr(v), _ptr(scratch), _ptr(segments),
              n_seg, n, _ptr(norms), float(lr), _stream())


# ------------------------------------------------------------------ Weave
def fold_affine(w: torch.Tensor, b: Optional[torch.Tensor], scale: Optional[torch.Tensor],
                shift: Optional[torch.Tensor], trans_w: bool = False):
    """(W * diag(scale), b*scale + shift): an eval-mode BatchNorm folded into the preceding product."""
    w = _mat(w, "w")
    k, n = (w.shape[1], w.shape[0]) if trans_w else (w.shape[0], w.shape[1])
    w_out = torch.empty_like(w)
    b_out = torch.empty(n, dtype=torch.float32, device=w.device)
    _lib.call("gcmi_fold_affine", _ptr(w), _ptr(_vec(b, "b", n)), _ptr(_vec(scale, "scale", n)),
              _ptr(_vec(shift, "shift", n)), k, n, 1 if trans_w else 0, _ptr(w_out), _ptr(b_out), _stream())
    return w_out, b_out


def _i32vec(t: torch.Tensor, name: str, n: Optional[int] = None) -> torch.Tensor:
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.int32 and t.is_contiguous()):
        raise _lib.GcmiError("%s must be a contiguous int32 CUDA tensor" % name)
    if n is not None and t.numel() != n:
        raise _lib.GcmiError("%s has %d entries, expected %d" % (name, t.numel(), n))
    return t


def weave_pair_to_atom(pair_feat: torch.Tensor, pair_src: torch.Tensor, n_atoms: int, w: torch.Tensor, b: torch.Tensor):
    """sum over the pairs of every source atom (pair_src ascending) of relu(pair_feat . w + b)."""
    pf = _mat(pair_feat, "pair_feat")
    w = _mat(w, "w", rows=pf.shape[1])
    H = w.shape[1]
    out = torch.empty((n_atoms, H), dtype=torch.float32, device=pf.device)
    _lib.call("gcmi_weave_pair_to_atom", _ptr(pf), _ld(pf), pf.shape[1], _ptr(_i32vec(pair_src, "pair_src", pf.shape[0])),
              pf.shape[0], n_atoms, _ptr(w), _ptr(_vec(b, "b", H)), H, _ptr(out), _ld(out), _stream())
    return out


def weave_pair_features(u: torch.Tensor, v: torch.Tensor, b_ap, pair_feat: torch.Tensor, w_pp, b_pp,
                        atom_to_pair: torch.Tensor, out: Optional[torch.Tensor] = None):
    """[relu(U[i]+V[j]+b) + relu(U[j]+V[i]+b) | relu(pair_feat . w_pp + b_pp)] per ordered pair.
    ``w_pp=None``: only the atom-pair block.  ``out``: write into this (P, H + H2) matrix (may be a column
    block of a wider one)."""
    u, v = _mat(u, "u"), _mat(v, "v", rows=u.shape[0], cols=u.shape[1])
    if _ld(u) != _ld(v):
        raise _lib.GcmiError("u and v must share their leading dimension")
    pf = _mat(pair_feat, "pair_feat")
    if w_pp is not None:
        w_pp = _mat(w_pp, "w_pp", rows=pf.shape[1])
    P, H, H2 = pf.shape[0], u.shape[1], 0 if w_pp is None else w_pp.shape[1]
    if out is None:
        z = torch.empty((P, H + H2), dtype=torch.float32, device=pf.device)
    else:
        z = _mat(out, "out", rows=P, cols=H + H2)
    _lib.call("gcmi_weave_pair_features", _ptr(u), _ptr(v), _ld(u), H, _ptr(_vec(b_ap, "b_ap", H)), _ptr(pf), _ld(pf),
              pf.shape[1], _ptr(w_pp), _ptr(_vec(b_pp, "b_pp", H2)) if H2 else None, H2,
              _ptr(_i32vec(atom_to_pair, "atom_to_pair", 2 * P)), P, _ptr(z), _ld(z), _stream())
    return z


def weave_gather(x: torch.Tensor, mol_ptr: torch.Tensor, gaussian_expand: bool):
    x = _mat(x, "x")
    n_mols = mol_ptr.numel() - 1
    out = torch.empty((n_mols, x.shape[1] * (11 if gaussian_expand else 1)), dtype=torch.float32, device=x.device)
    _lib.call("gcmi_weave_gather", _ptr(x), _ld(x), x.shape[1], _ptr(_i32vec(mol_ptr, "mol_ptr")), n_mols,
              1 if gaussian_expand else 0, _ptr(out), _ld(out), _stream())
    return out


def tanh_(x: torch.Tensor) -> torch.Tensor:
    x = _mat(x, "x")
    _lib.call("gcmi_tanh_", _ptr(x), _ld(x), x.shape[0], x.shape[1], _stream())
    return x


# ------------------------------------------------------------------ DTNN
DTNN_MAX_EMBEDDING, DTNN_MAX_HIDDEN, DTNN_MAX_DISTANCE, DTNN_MAX_ATOMS = 64, 64, 128, 64


def _dtnn_common(src, from_distance, mem_i, mem_j, ah, w_df, b_df, w_fc):
    """The argument list both directions of the pair interaction share, checked against each other."""
    ah = _mat(ah, "ah")
    w_df, w_fc = _mat(w_df, "W_df"), _mat(w_fc, "W_fc")
    K, H = w_df.shape
    E = w_fc.shape[1]
    if w_fc.shape[0] != H or ah.shape[1] != H:
        raise ValueError("dtnn_pair: W_df (%d, %d), W_fc %s and atom rows of %d columns do not chain" %
                         (K, H, tuple(w_fc.shape), ah.shape[1]))
    if E > DTNN_MAX_EMBEDDING or H > DTNN_MAX_HIDDEN or K > DTNN_MAX_DISTANCE:
        raise ValueError("dtnn_pair covers n_embedding <= %d, n_hidden <= %d, n_distance <= %d (got %d, %d, %d)" %
                         (DTNN_MAX_EMBEDDING, DTNN_MAX_HIDDEN, DTNN_MAX_DISTANCE, E, H, K))
    if not (w_df.is_contiguous() and w_fc.is_contiguous()):
        raise ValueError("dtnn_pair: weights must be contiguous")
    P = mem_i.numel()
    _i32vec(mem_i, "mem_i"), _i32vec(mem_j, "mem_j", P)
    if from_distance:
        _vec(src, "distance", P)
        ld_src = 1
    else:
        _mat(src, "gaussian", rows=P, cols=K)
        ld_src = _ld(src)
    return (_ptr(src), ld_src, 1 if from_distance else 0, _ptr(mem_i), _ptr(mem_j), P, ah.shape[0], _ptr(ah), _ld(ah), H,
            _ptr(w_df), _ptr(_vec(b_df, "b_df", H)), K, _ptr(w_fc), E), (P, ah.shape[0], K, H, E)


def dtnn_pair_fwd(src, from_distance: bool, mem_i, mem_j, ah, w_df, b_df, w_fc, distance_min: float = 0.0,
                  step: float = 1.0) -> torch.Tensor:
    """Y[i] = sum_{p: mem_i[p] = i} tanh(((g_p . W_df + b_df) * ah[mem_j[p]]) . W_fc); ``src`` = the distances
    (``from_distance``) or the Gaussian matrix.  The memberships must have been validated (inside [0, N), mem_i sorted)."""
    args, (P, N, K, H, E) = _dtnn_common(src, from_distance, mem_i, mem_j, ah, w_df, b_df, w_fc)
    y = torch.empty((N, E), dtype=torch.float32, device=ah.device)
    _lib.call("gcmi_dtnn_pair_fwd", *args, float(distance_min), float(step), _ptr(y), _ld(y), _stream())
    return y


def dtnn_pair_bwd(src, from_distance: bool, mem_i, mem_j, ah, w_df, b_df, w_fc, distance_min: float, step: float,
                  dy, dw_df, db_df, dw_fc) -> torch.Tensor:
    """d_ah (returned); dW_df, db_df, dW_fc are ADDED into the given buffers."""
    args, (P, N, K, H, E) = _dtnn_common(src, from_distance, mem_i, mem_j, ah, w_df, b_df, w_fc)
    dy = _mat(dy, "dy", rows=N, cols=E)
    dah = torch.empty((N, H), dtype=torch.float32, device=ah.device)
    _lib.call("gcmi_dtnn_pair_bwd", *args, float(distance_min), float(step), _ptr(dy), _ld(dy), _ptr(dah), _ld(dah),
              _ptr(_vec(dw_df.reshape(-1), "dW_df", K * H)), _ptr(_vec(db_df, "db_df", H)),
              _ptr(_vec(dw_fc.reshape(-1), "dW_fc", H * E)), _stream())
    return dah


def dtnn_collate(z_all, dist_all, n_atoms_all, mol_idx, n_atoms: int, n_pairs: int):
    """One batch from a resident Coulomb-matrix set: (atom_off, pair_off, z, d, mem_i, mem_j) on the device."""
    M, A = z_all.shape
    dev = z_all.device
    _i32vec(z_all.reshape(-1), "z_all"), _i32vec(n_atoms_all, "n_atoms_all", M), _i32vec(mol_idx, "mol_idx")
    _vec(dist_all.reshape(-1), "dist_all", M * A * A)
    B = mol_idx.numel()
    atom_off = torch.empty(B + 1, dtype=torch.int32, device=dev)
    pair_off = torch.empty(B + 1, dtype=torch.int32, device=dev)
    z = torch.zeros(n_atoms, dtype=torch.int32, device=dev)
    d = torch.zeros(n_pairs, dtype=torch.float32, device=dev)
    mem_i = torch.zeros(n_pairs, dtype=torch.int32, device=dev)
    mem_j = torch.zeros(n_pairs, dtype=torch.int32, device=dev)
    _lib.call("gcmi_dtnn_collate", _ptr(z_all), _ptr(dist_all), _ptr(n_atoms_all), M, A, _ptr(mol_idx), B, n_atoms, n_pairs,
              _ptr(atom_off), _ptr(pair_off), _ptr(z), _ptr(d), _ptr(mem_i), _ptr(mem_j), _stream())
    return atom_off, pair_off, z, d, mem_i, mem_j


# ------------------------------------------------------------------ Molecule Attention Transformer
MAT_MAX_ATOMS, MAT_MAX_DK = 128, 64
MAT_DIST_KERNELS = {"softmax": 0, "exp": 1}


class MatOffsets:
    """The molecules of a pad-free batch: atom offsets and pair offsets (exclusive sums of n and n^2), on the host
    (validated HERE, and again by every C entry before a launch) and on the device (what the kernels read)."""

    def __init__(self, n_atoms_per_mol, device, uploaded: Optional[torch.Tensor] = None):
        n = np.ascontiguousarray(n_atoms_per_mol, np.int64).reshape(-1)
        if n.size == 0 or n.min() <= 0:
            raise ValueError("MatOffsets: at least one molecule, every molecule with at least one atom")
        if int((n * n).sum()) >= 2**31:
            raise ValueError("MatOffsets: the pair blocks of a batch must stay below 2^31 entries")
        self.n = n
        self.atom_off = np.concatenate([[0], np.cumsum(n)]).astype(np.int32)
        self.pair_off = np.concatenate([[0], np.cumsum(n * n)]).astype(np.int32)
        self.n_mols, self.n_atoms, self.n_pairs = int(n.size), int(self.atom_off[-1]), int(self.pair_off[-1])
        self.n_max = int(n.max())
        self.device = torch.device(device)
        # uploaded: [atom_off | pair_off] as int32 on the device already (part of the caller's own packed upload)
        both = uploaded if uploaded is not None else torch.as_tensor(self.host_words(n), device=self.device)
        if both.dtype != torch.int32 or both.numel() != 2 * self.n_mols + 2 or both.device.type != self.device.type or \
                not both.is_contiguous():
            raise ValueError("MatOffsets: the uploaded offsets must be 2 (n_mols + 1) contiguous int32 words on the device")
        self.d_atom_off, self.d_pair_off = both[:self.n_mols + 1], both[self.n_mols + 1:]

    @staticmethod
    def host_words(n_atoms_per_mol) -> np.ndarray:
        """[atom_off | pair_off] as int32: what the device copy holds."""
        n = np.asarray(n_atoms_per_mol, np.int64).reshape(-1)
        return np.concatenate([[0], np.cumsum(n), [0], np.cumsum(n * n)]).astype(np.int32)

    def _args(self):
        return (_vp(self.atom_off.ctypes.data), _vp(self.pair_off.ctypes.data), _ptr(self.d_atom_off),
                _ptr(self.d_pair_off), self.n_mols)


def _mat_offsets(offs, what: str) -> MatOffsets:
    if not isinstance(offs, MatOffsets) or offs.device.type != "cuda":
        raise _lib.GcmiError("%s: offsets must be a MatOffsets on the GPU" % what)
    return offs


def mat_bias(adj: torch.Tensor, dist: torch.Tensor, offs: MatOffsets, dist_kernel: str, lambda_distance: float,
             lambda_adjacency: float, eps: float = 1e-6) -> torch.Tensor:
    """One float per atom pair of the batch: lambda_distance * g(D) + lambda_adjacency * A / (rowsum(A) + eps)."""
    offs = _mat_offsets(offs, "mat_bias")
    if dist_kernel not in MAT_DIST_KERNELS:
        raise ValueError("mat_bias: dist_kernel must be 'softmax' or 'exp'")
    _vec(adj, "adjacency blocks", offs.n_pairs), _vec(dist, "distance blocks", offs.n_pairs)
    bias = torch.empty(offs.n_pairs, dtype=torch.float32, device=adj.device)
    _lib.call("gcmi_mat_bias", _ptr(adj), _ptr(dist), *offs._args(), MAT_DIST_KERNELS[dist_kernel], float(lambda_distance),
              float(lambda_adjacency), float(eps), _ptr(bias), _stream())
    return bias


def _mat_rows(t, name, offs, width, ld=None):
    t = _mat(t, name, rows=offs.n_atoms, cols=width)
    if _ld(t) % 4 or t.data_ptr() % 16:
        raise ValueError("%s: rows must be 16-byte aligned with a leading dimension of whole 16-byte pieces" % name)
    if ld is not None and _ld(t) != ld:
        raise ValueError("%s: leading dimension %d, expected %d" % (name, _ld(t), ld))
    return t


def _mat_attention_common(q, k, v, bias, offs, n_heads: int, d_k: int):
    offs = _mat_offsets(offs, "mat_attention")
    if n_heads <= 0 or d_k <= 0 or d_k % 4 or d_k > MAT_MAX_DK:
        raise ValueError("mat_attention covers d_k a multiple of 4 up to %d (got %d heads of %d)" % (MAT_MAX_DK, n_heads, d_k))
    if offs.n_max > MAT_MAX_ATOMS:
        raise ValueError("mat_attention covers molecules of up to %d atoms (got %d)" % (MAT_MAX_ATOMS, offs.n_max))
    width = n_heads * d_k
    q = _mat_rows(q, "q", offs, width)
    k, v = _mat_rows(k, "k", offs, width, _ld(q)), _mat_rows(v, "v", offs, width, _ld(q))
    _vec(bias, "bias", offs.n_pairs)
    return (_ptr(q), _ptr(k), _ptr(v), _ld(q), _ptr(bias)) + offs._args() + (n_heads, d_k), width


def mat_attention_fwd(q, k, v, bias, offs: MatOffsets, n_heads: int, d_k: int, lambda_attention: float,
                      out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """O = (lambda_attention * softmax(Q K^T / sqrt(d_k)) + bias) V per (molecule, head); q, k, v: (atoms, n_heads * d_k)
    views (they may be one tensor).  ``out``: write into these rows (columns of a wider matrix are left alone)."""
    args, width = _mat_attention_common(q, k, v, bias, offs, n_heads, d_k)
    o = torch.empty((offs.n_atoms, width), dtype=torch.float32, device=q.device) if out is None else \
        _mat_rows(out, "out", offs, width)
    _lib.call("gcmi_mat_attention_fwd", *args, float(lambda_attention), _ptr(o), _ld(o), _stream())
    return o


def mat_attention_bwd(q, k, v, bias, offs: MatOffsets, n_heads: int, d_k: int, lambda_attention: float, dO,
                      shared: bool = False, out=None):
    """(dQ, dK, dV), or with ``shared`` (q, k, v one tensor) their sum.  ``out``: the buffer(s) to write into."""
    args, width = _mat_attention_common(q, k, v, bias, offs, n_heads, d_k)
    dO = _mat_rows(dO, "dO", offs, width)
    if shared and not (q.data_ptr() == k.data_ptr() == v.data_ptr()):
        raise ValueError("mat_attention_bwd: shared needs q, k and v to be one tensor")
    n_out = 1 if shared else 3
    if out is None:
        bufs = [torch.empty((offs.n_atoms, width), dtype=torch.float32, device=q.device) for _ in range(n_out)]
    else:
        bufs = [out] if torch.is_tensor(out) else list(out)
        if len(bufs) != n_out:
            raise ValueError("mat_attention_bwd: %d output buffer(s) expected" % n_out)
        bufs = [_mat_rows(b, "gradient buffer", offs, width, _ld(bufs[0])) for b in bufs]
        if len({b.data_ptr() for b in bufs}) != n_out:
            raise ValueError("mat_attention_bwd: the gradient buffers must be distinct")
    ptrs = [_ptr(b) for b in bufs] + [None] * (3 - n_out)
    _lib.call("gcmi_mat_attention_bwd", *args, float(lambda_attention), _ptr(dO), _ld(dO), *ptrs, _ld(bufs[0]),
              1 if shared else 0, _stream())
    return bufs[0] if shared else tuple(bufs)


class MatAttentionFn(torch.autograd.Function):
    """(q, k, v) -> O of csrc/mat.hip.  Nothing is saved beyond the inputs; the backward recomputes the attention matrix.
    Called with ONE tensor three times, the backward forms dQ + dK + dV in one buffer."""

    @staticmethod
    def forward(ctx, q, k, v, bias, offs: MatOffsets, n_heads: int, lambda_attention: float):
        shared = q is k and k is v
        q = rowmajor(q)
        k, v = (q, q) if shared else (rowmajor(k), rowmajor(v))
        d_k = q.shape[1] // n_heads
        if d_k * n_heads != q.shape[1]:
            raise ValueError("MatAttentionFn: %d columns are not %d heads" % (q.shape[1], n_heads))
        ctx.meta = (offs, n_heads, d_k, float(lambda_attention), shared)
        if shared:
            ctx.save_for_backward(q, bias)
        else:
            ctx.save_for_backward(q, bias, k, v)
        return mat_attention_fwd(q, k, v, bias, offs, n_heads, d_k, lambda_attention)

    @staticmethod
    def backward(ctx, dO):
        offs, n_heads, d_k, lam, shared = ctx.meta
        dO = rowmajor(dO)
        if dO.data_ptr() % 16 or _ld(dO) % 4:
            dO = dO.contiguous()
        if shared:
            q, bias = ctx.saved_tensors
            return mat_attention_bwd(q, q, q, bias, offs, n_heads, d_k, lam, dO, True), None, None, None, None, None, None
        q, bias, k, v = ctx.saved_tensors
        dq, dk, dv = mat_attention_bwd(q, k, v, bias, offs, n_heads, d_k, lam, dO, False)
        return dq, dk, dv, None, None, None, None


# ------------------------------------------------------------------ collation from a resident graph set
def _batch_layout(entry: str, sizes, blocks, shapes):
    """``(words, {block: (offset, shape)})`` of a packed batch buffer as the C routine ``entry`` places its ``blocks``
    (``-1``: a block the mode lacks, left out)."""
    off = (ctypes.c_int64 * len(blocks))()
    words = int(getattr(_lib.load(), entry)(*[int(v) for v in sizes], off))
    if words < 0:
        raise _lib.GcmiError("%s: %s" % (entry, _lib.load().gcmi_last_error().decode()))
    return words, {b: (int(off[i]), shapes[i]) for i, b in enumerate(blocks) if off[i] >= 0}


def _check_set(arrays, offsets, on_device: bool, what: str):
    """Every array of a resident set -- the ``offsets`` arrays int64, ``*features`` float32, the rest int32 -- is a
    contiguous CUDA tensor (``_lib.GcmiError``) or, for the host routine, a C-contiguous numpy array (``ValueError``)."""
    lib = torch if on_device else np
    for k, a in arrays.items():
        want = lib.int64 if k in offsets else lib.float32 if k.endswith("features") else lib.int32
        if on_device:
            if not (torch.is_tensor(a) and a.is_cuda and a.is_contiguous() and a.dtype == want):
                raise _lib.GcmiError("%s: %s must be a contiguous %s CUDA tensor" % (what, k, want))
        elif not (isinstance(a, np.ndarray) and a.flags.c_contiguous and a.dtype == want):
            raise ValueError("%s: %s must be a C-contiguous %s array" % (what, k, np.dtype(want)))


def _check_host_plan(plan, n: int, noun: str, what: str):
    if not (isinstance(plan, np.ndarray) and plan.dtype == np.int32 and plan.flags.c_contiguous and plan.size == 3 * n + 2):
        raise ValueError("%s: plan must hold 3 * %s + 2 int32 words" % (what, noun))


def _check_host_out(out, what: str):
    if not (out.dtype == np.int32 and out.flags.c_contiguous and out.ndim == 1):
        raise ValueError("%s: out must be a contiguous int32 vector" % what)


# ------------------------------------------------------------------ graph-network block (MEGNet)
GN_WIDTH, GN_ROWS_PER_WG = 32, 32


GN_INT_BLOCKS = ("src", "dst", "node_graph", "node_ptr", "edge_ptr", "inc_ptr", "inc_edge", "inc_other", "out_ptr",
                 "out_edge", "out_other")
GN_FLOAT_BLOCKS = ("x", "edge_attr", "global_features")
GN_BATCH_BLOCKS = GN_INT_BLOCKS + GN_FLOAT_BLOCKS
# collate_set_kernel over the MEGNet args: one workgroup of GN_COLLATE_THREADS threads per graph; a pass of the workgroup covers that many words
GN_COLLATE_THREADS = 256


def gn_batch_layout(n_graphs: int, n_nodes: int, n_edges: int, undirected: bool, n_node_features: int = 0,
                    n_edge_features: int = 0, n_global_features: int = 0):
    """The packed MEGNet batch buffer (``gcmi_gn_collate_words``): ``(words, {block: (offset, shape)})`` for the blocks
    of ``GN_BATCH_BLOCKS`` the mode has (undirected: no ``out_*``), 4-byte words, every block at a 16-byte boundary.  The
    one routine that places the blocks: for ``GnGraph``'s upload, for ``gcmi_gn_collate`` and for ``GnGraph.from_device``."""
    sizes = (n_graphs, n_nodes, n_edges, n_node_features, n_edge_features, n_global_features)
    if min(sizes) < 0 or max(n_graphs, n_nodes, 2 * n_edges) > 2 ** 31 - 2 or max(sizes[3:]) > 2 ** 31 - 1:
        raise ValueError("gn_batch_layout: sizes must be within [0, 2^31): %r" % (sizes,))
    G, N, E, k = int(n_graphs), int(n_nodes), int(n_edges), 2 if undirected else 1
    shapes = ((E,), (E,), (N,), (G + 1,), (G + 1,), (N + 1,), (k * E,), (k * E,), (N + 1,), (E,), (E,),
              (N, int(n_node_features)), (E, int(n_edge_features)), (G, int(n_global_features)))
    return _batch_layout("gcmi_gn_collate_words", (G, N, E, 1 if undirected else 0) + sizes[3:], GN_BATCH_BLOCKS, shapes)


class GnGraph:
    """The graphs of one batch for csrc/megnet.hip: ``src``, ``dst``, ``node_graph``, ``node_ptr``, ``edge_ptr``, the
    incidence list of every node (``inc_ptr``, ``inc_edge``, ``inc_other``: the edges ARRIVING there; undirected: every
    edge at both its ends, in the order of the reference's doubled edge list) and, directed, the list of the edges
    LEAVING every node.  Built on the host in numpy, validated there by ``gcmi_gn_graph_check``, uploaded in ONE
    packed transfer together with ``floats`` (arrays that travel along, e.g. the features: ``self.floats``) in the
    layout of ``gn_batch_layout``.  ``from_device`` wraps a buffer the device collated in that layout instead.

    ``batch``: the graph of every node, non-decreasing; every graph of ``range(n_graphs)`` holds a node; the edges are
    grouped by graph in the same order (what concatenating graphs gives).  Anything else: ``ValueError``."""

    _INT_FIELDS = GN_INT_BLOCKS

    def __init__(self, edge_index, batch, n_graphs: int, undirected: bool, device, floats=()):
        ei = np.asarray(edge_index)
        if ei.ndim != 2 or ei.shape[0] != 2:
            raise ValueError("GnGraph: edge_index must be (2, n_edges), got %s" % (ei.shape,))
        src, dst = ei[0].astype(np.int64), ei[1].astype(np.int64)
        batch = np.asarray(batch, np.int64).reshape(-1)
        N, E, G = int(batch.size), int(src.size), int(n_graphs)
        if N == 0 or G <= 0:
            raise ValueError("GnGraph: at least one node and one graph")
        if E and (min(src.min(), dst.min()) < 0 or max(src.max(), dst.max()) >= N):
            raise ValueError("GnGraph: edge_index names a node outside [0, %d)" % N)
        counts = np.bincount(batch, minlength=G) if batch.min() >= 0 else None
        if counts is None or counts.size != G or counts.min() == 0 or np.any(np.diff(batch) < 0):
            raise ValueError("GnGraph: batch must be non-decreasing and give every graph of range(%d) a node" % G)
        eg = batch[src]
        if np.any(batch[dst] != eg) or np.any(np.diff(eg) < 0):
            raise ValueError("GnGraph: every edge inside one graph, the edges grouped by graph in the graphs' order")
        if 2 * E >= 2**31 or N >= 2**31:
            raise ValueError("GnGraph: too many edges for 32-bit lists")
        self.n_nodes, self.n_edges, self.n_graphs, self.undirected = N, E, G, bool(undirected)
        self.device = torch.device(device)

        def csr(ids, n):
            return np.concatenate([[0], np.cumsum(np.bincount(ids, minlength=n))])
        h = {"src": src, "dst": dst, "node_graph": batch, "node_ptr": csr(batch, G), "edge_ptr": csr(eg, G)}
        edges = np.arange(E)
        if self.undirected:
            owner, other, edge = np.concatenate([dst, src]), np.concatenate([src, dst]), np.concatenate([edges, edges])
        else:
            owner, other, edge = dst, src, edges
        order = np.argsort(owner, kind="stable")
        h.update(inc_ptr=csr(owner, N), inc_edge=edge[order], inc_other=other[order])
        if not self.undirected:
            order = np.argsort(src, kind="stable")
            h.update(out_ptr=csr(src, N), out_edge=edges[order], out_other=dst[order])
        self.n_inc = int(h["inc_edge"].size)
        self._host = {k: np.ascontiguousarray(v, np.int32) for k, v in h.items()}
        self._host_ref_ = self._desc({k: v.ctypes.data for k, v in self._host.items()})
        _lib.call("gcmi_gn_graph_check", ctypes.byref(self._host_ref_))
        # one upload: the int32 lists as raw words, each block padded to 16 bytes, then the float arrays.  The three
        # feature arrays of a MEGNet batch are blocks of gn_batch_layout; other arrays follow the lists the same way
        fl = [np.ascontiguousarray(a, np.float32) for a in floats]
        features = len(fl) == 3 and all(a.ndim == 2 for a in fl) and [a.shape[0] for a in fl] == [N, E, G]
        total, layout = gn_batch_layout(G, N, E, self.undirected, *([a.shape[1] for a in fl] if features else (0, 0, 0)))
        where = [layout[k][0] for k in GN_FLOAT_BLOCKS] if features else []
        for a in ([] if features else fl):
            where.append(total)
            total += a.size + (-a.size % 4)
        words = np.zeros(total, np.int32)
        for k, v in self._host.items():
            words[layout[k][0]:layout[k][0] + v.size] = v
        for o, a in zip(where, fl):
            words[o:o + a.size] = a.reshape(-1).view(np.int32)
        self._adopt(torch.as_tensor(words.view(np.float32), device=self.device), layout, list(zip(where, (a.shape for a in fl))))

    def _adopt(self, packed: torch.Tensor, layout, floats):
        """The lists, ``floats`` ((offset, shape) each) and ``ref`` as views of the packed float32 buffer on its device."""
        words = packed.view(torch.int32)
        for k in self._INT_FIELDS:
            if k in layout:
                setattr(self, k, words[layout[k][0]:layout[k][0] + layout[k][1][0]])
        self.floats = [packed[o:o + int(np.prod(shape))].view(shape) for o, shape in floats]
        self._packed = packed
        self.ref = self._desc({k: getattr(self, k).data_ptr() for k in self._INT_FIELDS if k in layout}) \
            if self.device.type == "cuda" else None
        self._masks = None

    @classmethod
    def from_device(cls, words: torch.Tensor, n_graphs: int, n_nodes: int, n_edges: int, undirected: bool, widths) -> "GnGraph":
        """Around a buffer ``gcmi_gn_collate`` wrote (``gn_batch_layout`` with the three feature ``widths``): the
        attributes of the constructor as views of it, ``floats`` = x, edge_attr, global_features; nothing on the host
        until ``host`` is asked for.  Not validated per batch: see ``ResidentMegnetSet``."""
        self = cls.__new__(cls)
        self.n_nodes, self.n_edges, self.n_graphs, self.undirected = int(n_nodes), int(n_edges), int(n_graphs), bool(undirected)
        self.n_inc = (2 if self.undirected else 1) * self.n_edges
        self.device = words.device
        total, layout = gn_batch_layout(self.n_graphs, self.n_nodes, self.n_edges, self.undirected, *widths)
        if words.dtype != torch.int32 or words.dim() != 1 or words.numel() != total or words.data_ptr() % 16:
            raise ValueError("GnGraph.from_device: the buffer must hold the %d int32 words of the layout, 16-byte aligned" % total)
        self._host, self._host_ref_ = None, None
        self._layout = layout
        self._adopt(words.view(torch.float32), layout, [layout[k] for k in GN_FLOAT_BLOCKS])
        return self

    @property
    def host(self):
        """The int32 lists on the host.  A graph collated by the device (``from_device``) downloads its buffer and
        splits it on first use."""
        if self._host is None:
            words = self._packed.view(torch.int32).cpu().numpy()
            self._host = {k: words[self._layout[k][0]:self._layout[k][0] + self._layout[k][1][0]].copy()
                          for k in self._INT_FIELDS if k in self._layout}
        return self._host

    @property
    def _host_ref(self):
        if self._host_ref_ is None:
            self._host_ref_ = self._desc({k: v.ctypes.data for k, v in self.host.items()})
        return self._host_ref_

    def _desc(self, ptrs) -> "_lib.GcmiGnGraph":
        d = _lib.GcmiGnGraph(n_nodes=self.n_nodes, n_edges=self.n_edges, n_graphs=self.n_graphs,
                             undirected=1 if self.undirected else 0, n_inc=self.n_inc)
        for k in self._INT_FIELDS:
            setattr(d, k, ptrs.get(k) or None)
        return d

    @property
    def masks(self):
        """(nodes with an incident edge (N, 1), graphs with an edge (G, 1)) as 0 / 1 floats on the device."""
        if self._masks is None:
            self._masks = ((self.inc_ptr[1:] > self.inc_ptr[:-1]).to(torch.float32).unsqueeze(1),
                           (self.edge_ptr[1:] > self.edge_ptr[:-1]).to(torch.float32).unsqueeze(1))
        return self._masks


GN_SET_ARRAYS = ("node_ptr", "edge_ptr", "node_features", "edge_features", "global_features", "src", "dst", "inc_start",
                 "inc_edge", "inc_other", "out_start", "out_edge", "out_other")
_GN_SET_DIRECTED_ONLY = ("out_start", "out_edge", "out_other")


def _gn_set_desc(arrays, undirected: bool, n_graphs: int, n_nodes: int, n_edges: int, ptr_of, what: str):
    """``(gcmi_gn_set, widths)`` of the set ``arrays`` (``GN_SET_ARRAYS``; undirected: without the ``out_*`` lists) after
    the size checks the C entry cannot make: it sees pointers only."""
    names = [k for k in GN_SET_ARRAYS if not (undirected and k in _GN_SET_DIRECTED_ONLY)]
    if set(arrays) != set(names):
        raise ValueError("%s: the set of a%s batch holds %s" % (what, "n undirected" if undirected else " directed", ", ".join(names)))
    M = arrays["node_ptr"].shape[0] - 1
    if M < 0 or arrays["edge_ptr"].shape[0] != M + 1 or arrays["global_features"].shape[0] != M or \
            any(arrays[k].ndim != 2 for k in ("node_features", "edge_features", "global_features")):
        raise ValueError("%s: node_ptr, edge_ptr and global_features (2-D) must cover the same graphs" % what)
    N, E, k = arrays["node_features"].shape[0], arrays["edge_features"].shape[0], 2 if undirected else 1
    entries = {"src": E, "dst": E, "inc_start": N, "inc_edge": k * E, "inc_other": k * E, "out_start": N, "out_edge": E,
               "out_other": E}
    for name in names:
        if name in entries and tuple(arrays[name].shape) != (entries[name],):
            raise ValueError("%s: %s needs %d entries" % (what, name, entries[name]))
    if min(n_graphs, n_nodes, n_edges) < 0 or max(n_graphs, n_nodes, k * n_edges) > 2 ** 31 - 2:
        raise ValueError("%s: a batch holds at most 2^31 - 2 graphs, nodes and incidence entries" % what)
    widths = tuple(int(arrays[k].shape[1]) for k in ("node_features", "edge_features", "global_features"))
    d = _lib.GcmiGnSet(n_graphs=M, undirected=1 if undirected else 0, fn=widths[0], fe=widths[1], fg=widths[2])
    for name in names:
        setattr(d, name, ptr_of(arrays[name]) or None)
    return d, widths


def gn_collate(arrays, undirected: bool, plan: torch.Tensor, n_graphs: int, n_nodes: int, n_edges: int,
               out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``gcmi_gn_collate``: the packed batch buffer (int32 words, ``gn_batch_layout``) of the graphs named by ``plan`` =
    ``[graph_idx ; node_off ; edge_off]`` (int32, on the device), gathered from the resident set ``arrays``
    (``GN_SET_ARRAYS``: contiguous CUDA tensors, the two offset arrays int64, indices int32, features float32 2-D).
    The graph indices must have been validated by the caller: the kernel skips a bad one, it does not report it.
    ``out``: an int32 CUDA vector of exactly the layout's words to write into."""
    _check_set(arrays, ("node_ptr", "edge_ptr"), True, "gn_collate")
    d, widths = _gn_set_desc(arrays, undirected, n_graphs, n_nodes, n_edges, lambda t: t.data_ptr(), "gn_collate")
    _i32vec(plan, "plan", 3 * n_graphs + 2)
    words, _ = gn_batch_layout(n_graphs, n_nodes, n_edges, undirected, *widths)
    if out is None:
        out = torch.empty(words, dtype=torch.int32, device=plan.device)
    _i32vec(out, "out", words)
    _lib.call("gcmi_gn_collate", ctypes.byref(d), _ptr(plan), n_graphs, n_nodes, n_edges, _ptr(out), words, _stream())
    return out


def gn_collate_host(arrays, undirected: bool, plan: np.ndarray, n_graphs: int, n_nodes: int, n_edges: int,
                    out: Optional[np.ndarray] = None) -> np.ndarray:
    """``gcmi_gn_collate_host``: the same routine over numpy arrays, for tests without a GPU.  ``out``: a 16-byte
    aligned int32 vector of exactly the layout's words to write into."""
    _check_set(arrays, ("node_ptr", "edge_ptr"), False, "gn_collate_host")
    d, widths = _gn_set_desc(arrays, undirected, n_graphs, n_nodes, n_edges, lambda a: a.ctypes.data, "gn_collate_host")
    _check_host_plan(plan, n_graphs, "n_graphs", "gn_collate_host")
    words, _ = gn_batch_layout(n_graphs, n_nodes, n_edges, undirected, *widths)
    if out is None:
        out = torch.empty(words, dtype=torch.int32).numpy()  # (torch allocates 64-byte aligned)
    _check_host_out(out, "gn_collate_host")
    _lib.call("gcmi_gn_collate_host", ctypes.byref(d), _vp(plan.ctypes.data), n_graphs, n_nodes, n_edges,
              _vp(out.ctypes.data), out.size)
    return out


def _gn_graph(g, what: str) -> GnGraph:
    if not isinstance(g, GnGraph) or g.ref is None:
        raise _lib.GcmiError("%s: the graph must be a GnGraph on the GPU" % what)
    return g


def _gn_rows(t, name: str, rows: int, ld: Optional[int] = None):
    t = _mat(t, name, rows=rows, cols=GN_WIDTH)
    if rows and (_ld(t) % 4 or t.data_ptr() % 16):
        raise ValueError("%s: rows must be 16-byte aligned with a leading dimension of whole 16-byte pieces" % name)
    if ld is not None and rows > 1 and _ld(t) != ld:
        raise ValueError("%s: leading dimension %d, expected %d" % (name, _ld(t), ld))
    return t


def _gn_ld(t) -> int:
    return max(_ld(t), GN_WIDTH)  # (an empty or one-row tensor reports its width)


def _gn_inputs(g: GnGraph, ps, pd, q, r, what):
    g = _gn_graph(g, what)
    ps = _gn_rows(ps, "Ps", g.n_nodes)
    pd = _gn_rows(pd, "Pd", g.n_nodes, _ld(ps))
    q, r = _gn_rows(q, "Q", g.n_edges), _gn_rows(r, "R", g.n_graphs)
    return (ctypes.byref(g.ref), _ptr(ps), _ptr(pd), _gn_ld(ps), _ptr(q) if g.n_edges else None, _gn_ld(q), _ptr(r), _gn_ld(r))


def gn_edge_fwd(g: GnGraph, ps, pd, q, r) -> torch.Tensor:
    """Hs (n_edges, 32): Q[e] + R[g] + Ps[s] + Pd[d], undirected the mean of both directions (csrc/megnet.hip)."""
    args = _gn_inputs(g, ps, pd, q, r, "gn_edge_fwd")
    hs = torch.empty((g.n_edges, GN_WIDTH), dtype=torch.float32, device=ps.device)
    _lib.call("gcmi_gn_edge_fwd", *args, _ptr(hs) if g.n_edges else None, GN_WIDTH, _stream())
    return hs


def gn_node_fwd(g: GnGraph, ps, pd, q, r) -> torch.Tensor:
    """Mh (n_nodes, 32): Pd[v] + R[g] + the mean over v's incidence list of Ps[other] + Q[edge]; 0 for an empty list."""
    args = _gn_inputs(g, ps, pd, q, r, "gn_node_fwd")
    mh = torch.empty((g.n_nodes, GN_WIDTH), dtype=torch.float32, device=ps.device)
    _lib.call("gcmi_gn_node_fwd", *args, _ptr(mh), GN_WIDTH, _stream())
    return mh


def _gn_grad_buffers(g: GnGraph, dev):
    dp = torch.empty((g.n_nodes, 2 * GN_WIDTH), dtype=torch.float32, device=dev)  # [dPs | dPd]
    return dp, torch.empty((g.n_graphs, GN_WIDTH), dtype=torch.float32, device=dev)


def gn_edge_bwd(g: GnGraph, dhs):
    """(dP = [dPs | dPd] (n_nodes, 64), dR) of the edge pass; dQ is ``dhs`` itself."""
    g = _gn_graph(g, "gn_edge_bwd")
    dhs = _gn_rows(dhs, "dHs", g.n_edges)
    dp, dr = _gn_grad_buffers(g, dhs.device)
    _lib.call("gcmi_gn_edge_bwd", ctypes.byref(g.ref), _ptr(dhs) if g.n_edges else None, _gn_ld(dhs), _ptr(dp[:, :GN_WIDTH]),
              _ptr(dp[:, GN_WIDTH:]), 2 * GN_WIDTH, _ptr(dr), GN_WIDTH, _stream())
    return dp, dr


def gn_node_bwd(g: GnGraph, dmh):
    """(dP = [dPs | dPd], dQ, dR) of the node pass."""
    g = _gn_graph(g, "gn_node_bwd")
    dmh = _gn_rows(dmh, "dMh", g.n_nodes)
    dp, dr = _gn_grad_buffers(g, dmh.device)
    dq = torch.empty((g.n_edges, GN_WIDTH), dtype=torch.float32, device=dmh.device)
    _lib.call("gcmi_gn_node_bwd", ctypes.byref(g.ref), _ptr(dmh), _gn_ld(dmh), _ptr(dq) if g.n_edges else None, GN_WIDTH,
              _ptr(dp[:, :GN_WIDTH]), _ptr(dp[:, GN_WIDTH:]), 2 * GN_WIDTH, _ptr(dr), GN_WIDTH, _stream())
    return dp, dq, dr


def _gn_seg_args(ptr, x, n_rows, what):
    ptr = _i32vec(ptr, "ptr")
    if ptr.numel() < 2:
        raise ValueError("%s: ptr needs at least one range" % what)
    x = _mat(x, "rows", rows=n_rows)
    if x.shape[1] == 0:
        raise ValueError("%s: rows without columns" % what)
    return ptr, x


def gn_seg_reduce(x: torch.Tensor, ptr: torch.Tensor, mean: bool) -> torch.Tensor:
    """out[s] = the sum (or mean) of rows [ptr[s], ptr[s + 1]) of x (any width); a zero row for an empty range."""
    ptr, x = _gn_seg_args(ptr, x, None, "gn_seg_reduce")
    out = torch.empty((ptr.numel() - 1, x.shape[1]), dtype=torch.float32, device=x.device)
    _lib.call("gcmi_gn_seg_reduce", _ptr(ptr), ptr.numel() - 1, x.shape[0], x.shape[1], 1 if mean else 0,
              _ptr(x) if x.shape[0] else _ptr(out), max(_ld(x), x.shape[1]), _ptr(out), x.shape[1], _stream())
    return out


def gn_seg_spread(x: torch.Tensor, ptr: torch.Tensor, n_rows: int, mean: bool) -> torch.Tensor:
    """The transpose of ``gn_seg_reduce``: out[r] = x[s] (mean: / count(s)) for the rows of range s; ptr covers
    [0, n_rows]."""
    ptr, x = _gn_seg_args(ptr, x, ptr.numel() - 1, "gn_seg_spread")
    out = torch.empty((n_rows, x.shape[1]), dtype=torch.float32, device=x.device)
    if n_rows:
        _lib.call("gcmi_gn_seg_spread", _ptr(ptr), ptr.numel() - 1, n_rows, x.shape[1], 1 if mean else 0, _ptr(x),
                  max(_ld(x), x.shape[1]), _ptr(out), x.shape[1], _stream())
    return out


def _gn_halves(p: torch.Tensor):
    if p.dim() != 2 or p.shape[1] != 2 * GN_WIDTH:
        raise ValueError("the node projections must be one (n_nodes, %d) matrix [Ps | Pd]" % (2 * GN_WIDTH))
    p = rowmajor(p)
    if p.data_ptr() % 16 or _ld(p) % 4:
        p = p.contiguous()
    return p[:, :GN_WIDTH], p[:, GN_WIDTH:]


def _gn_aligned(t: torch.Tensor) -> torch.Tensor:
    t = rowmajor(t)
    return t.contiguous() if t.numel() and (t.data_ptr() % 16 or _ld(t) % 4) else t


class GnEdgeFn(torch.autograd.Function):
    """(P = [Ps | Pd] (n_nodes, 64), Q, R, graph) -> Hs.  Nothing is saved: the pass is linear."""

    @staticmethod
    def forward(ctx, p, q, r, g: GnGraph):
        ctx.g = g
        ps, pd = _gn_halves(p)
        return gn_edge_fwd(g, ps, pd, _gn_aligned(q), _gn_aligned(r))

    @staticmethod
    def backward(ctx, dhs):
        dhs = _gn_aligned(dhs)
        dp, dr = gn_edge_bwd(ctx.g, dhs)
        return dp, dhs, dr, None


class GnNodeFn(torch.autograd.Function):
    """(P = [Ps | Pd], Q, R, graph) -> Mh."""

    @staticmethod
    def forward(ctx, p, q, r, g: GnGraph):
        ctx.g = g
        ps, pd = _gn_halves(p)
        return gn_node_fwd(g, ps, pd, _gn_aligned(q), _gn_aligned(r))

    @staticmethod
    def backward(ctx, dmh):
        dp, dq, dr = gn_node_bwd(ctx.g, _gn_aligned(dmh))
        return dp, dq, dr, None


class GnSegMeanFn(torch.autograd.Function):
    """(rows, ptr) -> the mean of every contiguous range of rows."""

    @staticmethod
    def forward(ctx, x, ptr):
        ctx.save_for_backward(ptr)
        ctx.n_rows = x.shape[0]
        return gn_seg_reduce(rowmajor(x), ptr, True)

    @staticmethod
    def backward(ctx, dout):
        (ptr,) = ctx.saved_tensors
        return gn_seg_spread(rowmajor(dout), ptr, ctx.n_rows, True), None


class GnSegSpreadFn(torch.autograd.Function):
    """(x (n_ranges, w), ptr, n_rows) -> x[s] in every row of range s: ``x[batch]`` for sorted ``batch``, with a
    backward that sums each range in order (index_select's adds with atomics)."""

    @staticmethod
    def forward(ctx, x, ptr, n_rows: int):
        ctx.save_for_backward(ptr)
        return gn_seg_spread(rowmajor(x), ptr, n_rows, False)

    @staticmethod
    def backward(ctx, dout):
        (ptr,) = ctx.saved_tensors
        return gn_seg_reduce(rowmajor(dout), ptr, False), None, None


# ------------------------------------------------------------------ crystal-graph convolution (CGCNN)
CG_MIN_WIDTH, CG_MAX_WIDTH = 4, 128


def cg_width_ok(hidden: int) -> bool:
    """Whether csrc/cgcnn.hip covers the hidden width."""
    return CG_MIN_WIDTH <= hidden <= CG_MAX_WIDTH and hidden % 4 == 0


def _cg_graph(g, what: str) -> GnGraph:
    g = _gn_graph(g, what)
    if g.undirected:
        raise _lib.GcmiError("%s: the graph must be a DIRECTED GnGraph (arriving and leaving lists)" % what)
    return g


def _cg_rows(t, name: str, rows: int, cols: int, ld: Optional[int] = None):
    t = _mat(t, name, rows=rows, cols=cols)
    if rows and (_ld(t) % 4 or t.data_ptr() % 16):
        raise ValueError("%s: rows must be 16-byte aligned with a leading dimension of whole 16-byte pieces" % name)
    if ld is not None and rows > 1 and _ld(t) != ld:
        raise ValueError("%s: leading dimension %d, expected %d" % (name, _ld(t), ld))
    return t


def _cg_ld(t, cols: int) -> int:
    return max(_ld(t), cols)  # (an empty or one-row tensor reports its width)


def _cg_inputs(g, p, q, what: str):
    """The leading arguments of every entry: graph, Ps, Pd, ldp, Q, ldq, H.  ``p`` = [Ps | Pd] (n_nodes, 4H)."""
    g = _cg_graph(g, what)
    if p.dim() != 2 or p.shape[1] % 4 or not cg_width_ok(p.shape[1] // 4):
        raise ValueError("%s: the node projections must be one (n_nodes, 4H) matrix [Ps | Pd], H a multiple of 4 in "
                         "[%d, %d]; got %s" % (what, CG_MIN_WIDTH, CG_MAX_WIDTH, tuple(p.shape)))
    H = p.shape[1] // 4
    p = _cg_rows(p, "P", g.n_nodes, 4 * H)
    q = _cg_rows(q, "Q", g.n_edges, 2 * H)
    return H, (ctypes.byref(g.ref), _ptr(p[:, :2 * H]), _ptr(p[:, 2 * H:]), _cg_ld(p, 4 * H), _ptr(q) if g.n_edges else None,
               _cg_ld(q, 2 * H), H)


def _cg_norm(H: int, mean, invstd, gamma, beta):
    return tuple(_ptr(_vec(t, name, 2 * H)) for t, name in ((mean, "mean"), (invstd, "invstd"), (gamma, "gamma"), (beta, "beta")))


def _cg_workspace(g: GnGraph, H: int, dev) -> torch.Tensor:
    n = int(_lib.load().gcmi_cg_workspace_floats(g.n_nodes, g.n_edges, H))
    return torch.empty(n, dtype=torch.float32, device=dev)


def cg_stats(g: GnGraph, p, q, eps: float = 1e-5, momentum: float = 0.1, running_mean=None, running_var=None,
             num_batches_tracked=None):
    """(mean, invstd) of the columns of z[k] = Ps[src k] + Pd[dst k] + Q[k] over the edges (biased variance), z never
    written; the running statistics (unbiased variance) and ``num_batches_tracked`` are updated in place when given."""
    H, args = _cg_inputs(g, p, q, "cg_stats")
    if g.n_edges < 2:
        raise ValueError("cg_stats: the statistics need at least 2 edges, got %d" % g.n_edges)
    _vec(running_mean, "running_mean", 2 * H)
    _vec(running_var, "running_var", 2 * H)
    if num_batches_tracked is not None and (num_batches_tracked.dtype != torch.int64 or num_batches_tracked.numel() != 1 or
                                            not num_batches_tracked.is_cuda):
        raise ValueError("num_batches_tracked must be one int64 on the GPU")
    stats = torch.empty((2, 2 * H), dtype=torch.float32, device=p.device)
    ws = _cg_workspace(g, H, p.device)
    _lib.call("gcmi_cg_stats", *args, float(eps), float(momentum), _ptr(stats[0]), _ptr(stats[1]), _ptr(running_mean),
              _ptr(running_var), _ptr(num_batches_tracked), _ptr(ws), ws.numel(), _stream())
    return stats[0], stats[1]


def cg_conv_fwd(g: GnGraph, p, q, h, mean=None, invstd=None, gamma=None, beta=None) -> torch.Tensor:
    """h' (n_nodes, H) = softplus(h + the gated messages summed over each arriving list); a zero row for an empty list."""
    H, args = _cg_inputs(g, p, q, "cg_conv_fwd")
    h = _cg_rows(h, "h", g.n_nodes, H)
    out = torch.empty((g.n_nodes, H), dtype=torch.float32, device=p.device)
    _lib.call("gcmi_cg_conv_fwd", *args, *_cg_norm(H, mean, invstd, gamma, beta), _ptr(h), _cg_ld(h, H), _ptr(out), H, _stream())
    return out


def cg_bwd_stats(g: GnGraph, p, q, hnew, dhnew, mean=None, invstd=None, gamma=None, beta=None) -> torch.Tensor:
    """[sum of dzh | sum of dzh * xhat] over the edges, (4H,): dbeta and dgamma."""
    H, args = _cg_inputs(g, p, q, "cg_bwd_stats")
    hnew, dhnew = _cg_rows(hnew, "h'", g.n_nodes, H), _cg_rows(dhnew, "dh'", g.n_nodes, H)
    sums = torch.empty(4 * H, dtype=torch.float32, device=p.device)
    ws = _cg_workspace(g, H, p.device)
    _lib.call("gcmi_cg_bwd_stats", *args, *_cg_norm(H, mean, invstd, gamma, beta), _ptr(hnew), _cg_ld(hnew, H), _ptr(dhnew),
              _cg_ld(dhnew, H), _ptr(sums), _ptr(ws), ws.numel(), _stream())
    return sums


def cg_bwd_edges(g: GnGraph, p, q, hnew, dhnew, sums=None, mean=None, invstd=None, gamma=None, beta=None):
    """(dP = [dPs | dPd] (n_nodes, 4H) with the dPd half written, dQ (n_edges, 2H), dpre (n_nodes, H)).  ``sums`` (from
    ``cg_bwd_stats``): the BatchNorm backward of training mode; without, the statistics are constants."""
    H, args = _cg_inputs(g, p, q, "cg_bwd_edges")
    hnew, dhnew = _cg_rows(hnew, "h'", g.n_nodes, H), _cg_rows(dhnew, "dh'", g.n_nodes, H)
    _vec(sums, "sums", 4 * H)
    dev = p.device
    dp = torch.empty((g.n_nodes, 4 * H), dtype=torch.float32, device=dev)
    dq = torch.empty((g.n_edges, 2 * H), dtype=torch.float32, device=dev)
    dpre = torch.empty((g.n_nodes, H), dtype=torch.float32, device=dev)
    _lib.call("gcmi_cg_bwd_edges", *args, *_cg_norm(H, mean, invstd, gamma, beta), _ptr(hnew), _cg_ld(hnew, H), _ptr(dhnew),
              _cg_ld(dhnew, H), _ptr(sums), _ptr(dq) if g.n_edges else None, 2 * H, _ptr(dp[:, 2 * H:]), 4 * H, _ptr(dpre), H,
              _stream())
    return dp, dq, dpre


def cg_bwd_src(g: GnGraph, dq, dp) -> torch.Tensor:
    """Writes dPs[v] = the sum of dQ over the leaving list of v into the first half of ``dp`` (n_nodes, 4H)."""
    g = _cg_graph(g, "cg_bwd_src")
    if dp.dim() != 2 or dp.shape[1] % 4 or not cg_width_ok(dp.shape[1] // 4):
        raise ValueError("cg_bwd_src: dP must be (n_nodes, 4H)")
    H = dp.shape[1] // 4
    dp, dq = _cg_rows(dp, "dP", g.n_nodes, 4 * H), _cg_rows(dq, "dQ", g.n_edges, 2 * H)
    _lib.call("gcmi_cg_bwd_src", ctypes.byref(g.ref), _ptr(dq) if g.n_edges else None, _cg_ld(dq, 2 * H), H, _ptr(dp[:, :2 * H]),
              _cg_ld(dp, 4 * H), _stream())
    return dp


class CgConvFn(torch.autograd.Function):
    """(P = [Ps | Pd] (n_nodes, 4H), Q (n_edges, 2H), h, mean, invstd, gamma, beta, graph, train) -> h'.  ``train``: mean
    and invstd are this batch's statistics of z (``cg_stats``) and the backward differentiates through them; otherwise
    they are constants (eval mode, or None without a BatchNorm).  Saved: P, Q and h' -- no tensor with E rows but Q."""

    @staticmethod
    def forward(ctx, p, q, h, mean, invstd, gamma, beta, g: GnGraph, train: bool):
        p, q, h = _gn_aligned(p), _gn_aligned(q), _gn_aligned(h)
        gamma = None if gamma is None else gamma.contiguous()
        beta = None if beta is None else beta.contiguous()
        out = cg_conv_fwd(g, p, q, h, mean, invstd, gamma, beta)
        ctx.g, ctx.train = g, bool(train) and mean is not None
        ctx.save_for_backward(p, q, out, mean, invstd, gamma, beta)
        return out

    @staticmethod
    def backward(ctx, dout):
        p, q, out, mean, invstd, gamma, beta = ctx.saved_tensors
        g, dout = ctx.g, _gn_aligned(dout)
        norm = dict(mean=mean, invstd=invstd, gamma=gamma, beta=beta)
        sums = dgamma = dbeta = None
        H = out.shape[1]
        if gamma is not None and g.n_edges:
            sums = cg_bwd_stats(g, p, q, out, dout, **norm)
            dbeta, dgamma = sums[:2 * H], sums[2 * H:]
        elif gamma is not None:
            dbeta, dgamma = torch.zeros_like(beta), torch.zeros_like(gamma)
        dp, dq, dpre = cg_bwd_edges(g, p, q, out, dout, sums if ctx.train else None, **norm)
        cg_bwd_src(g, dq, dp)
        return dp, dq, dpre, None, None, dgamma, dbeta, None, None


# ------------------------------------------------------------------ lattice convolution (LCNN)
LC_MAX_WIDTH, LC_MIN_PERM, LC_MAX_PERM, LC_MAX_SLOTS = 64, 2, 8, 32


def lc_shape_ok(n_sites: int, P: int, K: int, O: int) -> bool:
    """Whether csrc/lcnn.hip covers the shape."""
    return 1 <= O <= LC_MAX_WIDTH and LC_MIN_PERM <= P <= LC_MAX_PERM and 1 <= K <= LC_MAX_SLOTS and \
        0 < n_sites and n_sites * P * K * LC_MAX_WIDTH < 2 ** 31 - 1


def lc_graph_tables(edge_index, n_sites: int, P: int, K: int, graph: int = 0):
    """The tables of ONE graph in local indices: ``(nbr (n, P * K) int32, rev_count (n * K,) int32, rev_row (n * P * K,)
    int32)``.  ``nbr[v, p * K + j]`` is the source of the ``(p * K + j)``-th edge arriving at ``v`` (a stable sort by
    destination: a no-op where the edges already arrive grouped); the list of ``(u, j)`` holds the rows ``v * P + p``
    with ``nbr[v, p, j] = u`` in ascending order.  ``ValueError`` naming graph and node where an in-degree is not
    ``P * K``."""
    ei = np.asarray(edge_index)
    if ei.ndim != 2 or ei.shape[0] != 2:
        raise ValueError("lc_graph_tables: edge_index of graph %d must be (2, n_edges), got %s" % (graph, ei.shape))
    src, dst = ei[0].astype(np.int64), ei[1].astype(np.int64)
    n, D = int(n_sites), P * K
    if src.size and (min(src.min(), dst.min()) < 0 or max(src.max(), dst.max()) >= n):
        raise ValueError("lc_graph_tables: edge_index of graph %d names a node outside [0, %d)" % (graph, n))
    degree = np.bincount(dst, minlength=n)
    bad = np.nonzero(degree != D)[0]
    if bad.size:
        raise ValueError("LCNN: graph %d, node %d has in-degree %d, every site needs n_permutation * n_neighbor_sites = "
                         "%d * %d = %d arriving edges" % (graph, bad[0], degree[bad[0]], P, K, D))
    if dst.size and np.any(np.diff(dst) < 0):
        src = src[np.argsort(dst, kind="stable")]
    nbr = src.reshape(n, D)
    key = (nbr.reshape(n, P, K) * K + np.arange(K)).reshape(-1)  # (u, j) of entry (v, p, j)
    order = np.argsort(key, kind="stable")
    rev_row = (order // K).astype(np.int32)  # entry (v, p, j) -> row v * P + p
    return nbr.astype(np.int32), np.bincount(key, minlength=n * K).astype(np.int32), rev_row


class LcBatch:
    """The sites of one batch for csrc/lcnn.hip: the dense neighbour table ``nbr`` (N, P * K), the reverse lists keyed
    by (node, slot) (``rev_ptr`` (N * K + 1,), ``rev_row``) and ``node_ptr`` (graphs + 1,), put together from per-graph
    tables in local indices (``lc_graph_tables``) by concatenation plus offsets, validated on the host and uploaded in
    ONE packed transfer together with ``floats`` (``self.floats``)."""

    def __init__(self, tables, P: int, K: int, device, floats=()):
        tables = list(tables)
        if not tables:
            raise ValueError("LcBatch: no graphs")
        self.P, self.K = int(P), int(K)
        sizes = np.asarray([t[0].shape[0] for t in tables], np.int64)
        if sizes.min() <= 0 or any(t[0].shape[1] != P * K or t[1].size != t[0].shape[0] * K or t[2].size != t[0].size
                                   for t in tables):
            raise ValueError("LcBatch: every graph needs a site and tables of (n, %d), (n * %d,), (n * %d,)" % (P * K, K, P * K))
        if any(a.dtype != np.int32 for t in tables for a in t):
            raise ValueError("LcBatch: the tables must be int32 (ops.lc_graph_tables)")
        node_ptr = np.concatenate([[0], np.cumsum(sizes)])
        N = int(node_ptr[-1])
        if N * P * K * LC_MAX_WIDTH >= 2 ** 31 - 1:
            raise ValueError("LcBatch: %d sites are too many for 32-bit lists" % N)
        # the packed buffer first, the tables concatenated straight into it in int32 and offset in place: no second copy
        fl = [np.ascontiguousarray(a, np.float32) for a in floats]
        shapes = {"nbr": (N, P * K), "rev_ptr": (N * K + 1,), "rev_row": (N * P * K,), "node_ptr": (len(tables) + 1,)}
        where, total = {}, 0
        for k, shape in list(shapes.items()) + [(i, a.shape) for i, a in enumerate(fl)]:
            where[k] = total
            total += int(np.prod(shape)) + (-int(np.prod(shape)) % 4)
        words = np.zeros(total, np.int32)
        host = {k: words[where[k]:where[k] + int(np.prod(shape))].reshape(shape) for k, shape in shapes.items()}
        nbr, rev_ptr, rev_row = host["nbr"].reshape(-1), host["rev_ptr"], host["rev_row"]
        at = np.repeat(node_ptr[:-1].astype(np.int32), sizes * (P * K))
        np.concatenate([t[0].reshape(-1) for t in tables], out=nbr)
        nbr += at
        np.concatenate([t[2] for t in tables], out=rev_row)
        at *= P
        rev_row += at
        np.cumsum(np.concatenate([t[1] for t in tables]), out=rev_ptr[1:])
        host["node_ptr"][:] = node_ptr
        # validated before it leaves: the kernels compare every index again, a table that fails here is a bug upstream
        if nbr.min() < 0 or nbr.max() >= N or rev_row.min() < 0 or rev_row.max() >= N * P or rev_ptr[-1] != N * P * K or \
                np.any(rev_ptr[1:] < rev_ptr[:-1]):
            raise ValueError("LcBatch: a neighbour or reverse-list entry is out of range")
        self.n_sites, self.n_graphs = N, len(tables)
        self.device = torch.device(device)
        for i, a in enumerate(fl):
            words[where[i]:where[i] + a.size] = a.reshape(-1).view(np.int32)
        packed = torch.as_tensor(words.view(np.float32), device=self.device)
        ints = packed.view(torch.int32)
        for k, a in host.items():  # (the packed host buffer is not kept: the tables live on the device)
            setattr(self, k, ints[where[k]:where[k] + a.size].view(a.shape))
        self.floats = [packed[where[i]:where[i] + a.size].view(a.shape) for i, a in enumerate(fl)]
        self._packed = packed

    def ref(self, O: int) -> "_lib.GcmiLcBatch":
        return _lib.GcmiLcBatch(n_sites=self.n_sites, P=self.P, K=self.K, O=int(O), nbr=self.nbr.data_ptr(),
                                rev_ptr=self.rev_ptr.data_ptr(), rev_row=self.rev_row.data_ptr())


def _lc_batch(b, O: int, what: str):
    if not isinstance(b, LcBatch) or b.device.type != "cuda":
        raise _lib.GcmiError("%s: the batch must be an ops.LcBatch on the GPU" % what)
    if not lc_shape_ok(b.n_sites, b.P, b.K, O):
        raise ValueError("%s: n_sites %d, P %d, K %d, O %d are outside what csrc/lcnn.hip covers" % (what, b.n_sites, b.P, b.K, O))
    return b.ref(O)


def _lc_x(t, name: str, b: LcBatch, O: int):
    if not torch.is_tensor(t) or not t.is_cuda or t.dtype != torch.float32 or tuple(t.shape) != (b.n_sites, b.P, O) or \
            not t.is_contiguous():
        raise ValueError("%s must be a contiguous float32 CUDA tensor of (%d, %d, %d)" % (name, b.n_sites, b.P, O))
    return t


def _lc_mask(mask, b: LcBatch):
    if mask is not None and (not mask.is_cuda or mask.dtype != torch.float32 or tuple(mask.shape) != (b.n_sites, b.P) or
                             not mask.is_contiguous()):
        raise ValueError("mask must be a contiguous float32 CUDA tensor of (%d, %d)" % (b.n_sites, b.P))
    return mask


def lc_site_fwd(b: LcBatch, y, bias, gamma, beta, mean=None, var=None, eps: float = 1e-5, mask=None, want_x: bool = True):
    """(out (N, O), X (N, P, O) or None).  ``mean`` / ``var`` None: each site's own statistics over its P rows."""
    O = int(gamma.numel())
    ref = _lc_batch(b, O, "lc_site_fwd")
    y = _mat(y, "Y", rows=b.n_sites, cols=b.K * O)
    vecs = [_vec(t, name, O) for t, name in ((bias, "bias"), (gamma, "gamma"), (beta, "beta"), (mean, "mean"), (var, "var"))]
    out = torch.empty((b.n_sites, O), dtype=torch.float32, device=y.device)
    x = torch.empty((b.n_sites, b.P, O), dtype=torch.float32, device=y.device) if want_x else None
    _lib.call("gcmi_lc_site_fwd", ctypes.byref(ref), _ptr(y), _ld(y), *(_ptr(t) for t in vecs), float(eps),
              _ptr(_lc_mask(mask, b)), _ptr(out), O, _ptr(x), _stream())
    return out, x


def lc_site_bwd(b: LcBatch, x, dout, gamma, mean=None, var=None, eps: float = 1e-5, mask=None):
    """(dX (N, P, O), sums (3 O,) = [dgamma | dbeta | dbias])."""
    O = int(gamma.numel())
    ref = _lc_batch(b, O, "lc_site_bwd")
    x, dout = _lc_x(x, "X", b, O), _mat(dout, "dOut", rows=b.n_sites, cols=O)
    vecs = [_vec(t, name, O) for t, name in ((gamma, "gamma"), (mean, "mean"), (var, "var"))]
    dx, sums = torch.empty_like(x), torch.empty(3 * O, dtype=torch.float32, device=x.device)
    ws = torch.empty(int(_lib.load().gcmi_lc_workspace_floats(b.n_sites, O)), dtype=torch.float32, device=x.device)
    _lib.call("gcmi_lc_site_bwd", ctypes.byref(ref), _ptr(x), _ptr(dout), _ld(dout), _ptr(_lc_mask(mask, b)),
              *(_ptr(t) for t in vecs), float(eps), _ptr(dx), _ptr(sums), _ptr(ws), ws.numel(), _stream())
    return dx, sums


def lc_rev_sum(b: LcBatch, dx) -> torch.Tensor:
    """dY (N, K * O): dY[u, j, :] = the sum of dX over the reverse list of (u, j), in list order."""
    O = int(dx.shape[-1])
    ref = _lc_batch(b, O, "lc_rev_sum")
    dx = _lc_x(dx, "dX", b, O)
    dy = torch.empty((b.n_sites, b.K * O), dtype=torch.float32, device=dx.device)
    _lib.call("gcmi_lc_rev_sum", ctypes.byref(ref), _ptr(dx), _ptr(dy), b.K * O, _stream())
    return dy


def lc_running(b: LcBatch, x, running_mean, running_var, num_batches_tracked=None, momentum: float = 0.1):
    """The running statistics after one BatchNorm update per site, in site order, in closed form; in place."""
    O = int(x.shape[-1])
    ref = _lc_batch(b, O, "lc_running")
    x = _lc_x(x, "X", b, O)
    if running_mean is None or running_var is None:
        raise ValueError("lc_running: running_mean and running_var are needed")
    _vec(running_mean, "running_mean", O), _vec(running_var, "running_var", O)
    if num_batches_tracked is not None and (num_batches_tracked.dtype != torch.int64 or num_batches_tracked.numel() != 1 or
                                            not num_batches_tracked.is_cuda):
        raise ValueError("num_batches_tracked must be one int64 on the GPU")
    _lib.call("gcmi_lc_running", ctypes.byref(ref), _ptr(x), float(momentum), _ptr(running_mean), _ptr(running_var),
              _ptr(num_batches_tracked), _stream())


class LcSiteFn(torch.autograd.Function):
    """(Y (N, K * O), bias, gamma, beta, mean, var, mask, batch, eps, want_x) -> (out (N, O), X (N, P, O) or None).
    ``mean`` and ``var`` None: training, each site normalised by its own statistics over P and the backward
    differentiates through them; otherwise they are constants (eval).  X is written where ``want_x`` asks for it
    (training: ``lc_running`` reads it) or an input takes a gradient (the backward reads it); it is not differentiable."""

    @staticmethod
    def forward(ctx, y, bias, gamma, beta, mean, var, mask, b: LcBatch, eps: float, want_x: bool):
        y = rowmajor(y)
        bias, gamma, beta = bias.contiguous(), gamma.contiguous(), beta.contiguous()
        out, x = lc_site_fwd(b, y, bias, gamma, beta, mean, var, eps, mask, bool(want_x) or any(ctx.needs_input_grad[:4]))
        ctx.b, ctx.eps = b, eps
        ctx.save_for_backward(x, gamma, mean, var, mask)
        if x is not None:
            ctx.mark_non_differentiable(x)
        return out, x

    @staticmethod
    def backward(ctx, dout, _dx_unused):
        x, gamma, mean, var, mask = ctx.saved_tensors
        O = gamma.numel()
        dx, sums = lc_site_bwd(ctx.b, x, rowmajor(dout), gamma, mean, var, ctx.eps, mask)
        return lc_rev_sum(ctx.b, dx), sums[2 * O:], sums[:O], sums[O:2 * O], None, None, None, None, None, None


# ------------------------------------------------------------------ atomic convolution (ACNN)
AC_MAX_NEIGHBORS, AC_MAX_TYPES, AC_MAX_CHANNELS = 64, 32, 2048


def ac_types(atom_types) -> tuple:
    """The type table as the kernels take it: a tuple of float32 values, () for ``None`` or an empty list."""
    if atom_types is None:
        return ()
    return tuple(float(np.float32(t)) for t in atom_types)


def ac_width_ok(n_filters: int, types=()) -> bool:
    """Whether csrc/atomconv.hip covers the row: at most AC_MAX_TYPES types without duplicates (a neighbour stands in
    one channel block) and 1 .. AC_MAX_CHANNELS channels (a row is held in LDS)."""
    types = ac_types(types)
    return (len(types) <= AC_MAX_TYPES and len(set(types)) == len(types) and not any(t != t for t in types) and
            1 <= n_filters and max(len(types), 1) * n_filters <= AC_MAX_CHANNELS)


def ac_shape_ok(x, nbrs, z) -> bool:
    """Whether the kernels take these inputs: float32 (B, N, 3) on the GPU with 1 .. AC_MAX_NEIGHBORS neighbours."""
    return (torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 3 and x.shape[2] == 3 and
            nbrs.dim() == 3 and 1 <= nbrs.shape[2] <= AC_MAX_NEIGHBORS and x.shape[0] > 0 and x.shape[1] > 0 and
            x.shape[0] * x.shape[1] * AC_MAX_NEIGHBORS < 2 ** 31 and z.dtype == torch.float32)


class AcInput:
    """One layer input on the device as ``gcmi_ac_input`` describes it: ``x`` (B, N, 3) float32, ``nbrs`` (B, N, M) int32,
    ``z`` (B, N, M) float32, the filters ``rc``, ``rs``, ``re`` (L values each), the type table and the box.  An index of
    ``nbrs`` outside [0, N) is compared with N on the device before it is used and contributes nothing."""

    def __init__(self, x, nbrs, z, rc, rs, re, types=(), box=None):
        if not (torch.is_tensor(x) and x.is_cuda):
            raise _lib.GcmiError("x must be a CUDA tensor: the hot path has no CPU implementation")
        if x.dtype != torch.float32 or x.dim() != 3:
            raise ValueError("x must be float32 (B, N, 3), got %s %s" % (x.dtype, tuple(x.shape)))
        B, N, d = x.shape
        dev = x.device
        if not (torch.is_tensor(nbrs) and nbrs.device == dev and nbrs.dtype == torch.int32 and nbrs.dim() == 3 and
                tuple(nbrs.shape[:2]) == (B, N)):
            raise ValueError("nbrs must be int32 (B, N, M) on the device of x")
        M = nbrs.shape[2]
        if not (torch.is_tensor(z) and z.device == dev and z.dtype == torch.float32 and tuple(z.shape) == (B, N, M)):
            raise ValueError("z must be float32 (B, N, M) on the device of x")
        rc, rs, re = (t.detach().reshape(-1) for t in (rc, rs, re))
        L = rc.numel()
        for t, name in ((rc, "rc"), (rs, "rs"), (re, "re")):
            if t.device != dev or t.dtype != torch.float32 or t.numel() != L:
                raise ValueError("%s must hold %d float32 values on the device of x" % (name, L))
        self.types = ac_types(types)
        if len(self.types) > AC_MAX_TYPES:
            raise ValueError("%d atom types, at most %d" % (len(self.types), AC_MAX_TYPES))
        if box is not None:
            box = [float(v) for v in (box.tolist() if torch.is_tensor(box) else box)]
            if len(box) != d:
                raise ValueError("Length of `box_size` must be equal to `d`")
        # (the tensors are kept: the description holds their addresses)
        self.x, self.nbrs, self.z = x.contiguous(), nbrs.contiguous(), z.contiguous()
        self.rc, self.rs, self.re = rc.contiguous(), rs.contiguous(), re.contiguous()
        self.B, self.N, self.M, self.d, self.L = B, N, M, d, L
        self.C = max(len(self.types), 1) * L
        self.ref = _lib.GcmiAcInput()
        for k in ("x", "nbrs", "z", "rc", "rs", "re"):
            setattr(self.ref, k, getattr(self, k).data_ptr())
        self.ref.B, self.ref.N, self.ref.M, self.ref.d, self.ref.L = B, N, M, d, L
        self.ref.n_types = len(self.types)
        for i, t in enumerate(self.types):
            self.ref.types[i] = t
        self.ref.has_box = int(box is not None)
        for i, v in enumerate(box or ()):
            if i < 3:
                self.ref.box[i] = v

    def workspace(self) -> torch.Tensor:
        n = int(_lib.load().gcmi_ac_workspace_floats(self.B, self.N, self.L))
        if n < 0:
            raise ValueError("atomic convolution: B %d, N %d, L %d are outside the kernels' range" % (self.B, self.N, self.L))
        return torch.empty(n, dtype=torch.float32, device=self.x.device)


def _ac_stats_arg(a: AcInput, stats):
    if not (torch.is_tensor(stats) and stats.is_cuda and stats.dtype == torch.float32 and tuple(stats.shape) == (a.N, 2) and
            stats.is_contiguous()):
        raise ValueError("stats must be a contiguous float32 CUDA tensor of shape (%d, 2)" % a.N)
    return _ptr(stats)


def ac_stats(a: AcInput, eps: float = 1e-5) -> torch.Tensor:
    """stats (N, 2) = (mean, invstd) of the atom slots: over the B * C values of a slot, unbiased variance, the rows
    never written."""
    stats = torch.empty((a.N, 2), dtype=torch.float32, device=a.x.device)
    ws = a.workspace()
    _lib.call("gcmi_ac_stats", ctypes.byref(a.ref), float(eps), _ptr(stats), _ptr(ws), ws.numel(), _stream())
    return stats


def ac_fwd(a: AcInput, stats) -> torch.Tensor:
    """y (B, N, C) = (row - mean[n]) * invstd[n]."""
    out = torch.empty((a.B, a.N, a.C), dtype=torch.float32, device=a.x.device)
    _lib.call("gcmi_ac_fwd", ctypes.byref(a.ref), _ac_stats_arg(a, stats), _ptr(out), _stream())
    return out


def ac_bwd(a: AcInput, stats, dy) -> torch.Tensor:
    """(3, L): the gradients of rc, rs and re for the output gradient ``dy`` (B, N, C), the statistics being constants."""
    if not (dy.is_cuda and dy.dtype == torch.float32 and tuple(dy.shape) == (a.B, a.N, a.C)):
        raise ValueError("dy must be float32 %s on the GPU" % ((a.B, a.N, a.C),))
    dy = dy.contiguous()
    grad = torch.empty((3, a.L), dtype=torch.float32, device=a.x.device)
    ws = a.workspace()
    _lib.call("gcmi_ac_bwd", ctypes.byref(a.ref), _ac_stats_arg(a, stats), _ptr(dy), _ptr(grad), _ptr(ws), ws.numel(), _stream())
    return grad


class AtomConvFn(torch.autograd.Function):
    """(rc, rs, re, AcInput built from their values) -> y (B, N, C).  The statistics are taken in the forward and are
    constants of the backward, as in the reference; ``x`` takes no gradient.  Saved: the statistics (2 N values) -- the
    pairs are recomputed."""

    @staticmethod
    def forward(ctx, rc, rs, re, a: AcInput, eps: float):
        stats = ac_stats(a, eps)
        ctx.a, ctx.shapes = a, (rc.shape, rs.shape, re.shape)
        ctx.save_for_backward(stats)
        return ac_fwd(a, stats)

    @staticmethod
    def backward(ctx, dy):
        (stats,) = ctx.saved_tensors
        g = ac_bwd(ctx.a, stats, dy)
        return g[0].reshape(ctx.shapes[0]), g[1].reshape(ctx.shapes[1]), g[2].reshape(ctx.shapes[2]), None, None


# ------------------------------------------------------------------ message passing
# ------------------------------------------------------------------ D-MPNN
DMPNN_MAX_DEGREE = 32


def dmpnn_message(x: Optional[torch.Tensor], out_ptr: torch.Tensor, rev: torch.Tensor, transposed: bool = False,
                  add: Optional[torch.Tensor] = None, want_s: bool = False, want_q: bool = True,
                  q_out: Optional[torch.Tensor] = None):
    """``gcmi_dmpnn_message`` over a VALIDATED bond plan (``out_ptr`` of n_atoms + 1 entries, ``rev`` of n_bonds:
    ``DmpnnBatch`` checks both before any launch).  Forward: ``q[b] = S[a] - x[rev[b]]``, ``S[a]`` = the sum of the rows
    arriving at atom ``a``; transposed: ``q[rev[b]] = T[a] - x[b] + add[a]``, ``T[a]`` = the sum over a's outgoing run
    (``x`` or ``add`` may be None = zeros).  Returns ``(S or T | None, q | None)``; ``q_out``: write q there."""
    n_atoms, n_bonds = out_ptr.numel() - 1, rev.numel()
    _i32vec(out_ptr, "out_ptr"), _i32vec(rev, "rev")
    if n_atoms < 0:
        raise ValueError("dmpnn_message: out_ptr needs n_atoms + 1 entries")
    if add is not None and not transposed:
        raise ValueError("dmpnn_message: add (the gradient of the atom sums) belongs to the transposed direction")
    src = x if x is not None else add
    if src is None:
        raise ValueError("dmpnn_message: no input rows")
    if x is not None:
        _mat(x, "x", rows=n_bonds)
    d = src.shape[1]
    if add is not None:
        _mat(add, "add", rows=n_atoms, cols=d)
    s = torch.empty((n_atoms, d), dtype=torch.float32, device=src.device) if want_s else None
    q = None
    if want_q:
        q = q_out if q_out is not None else torch.empty((n_bonds, d), dtype=torch.float32, device=src.device)
        _mat(q, "q", rows=n_bonds, cols=d)
    if n_bonds == 0 or n_atoms == 0:  # nothing to launch: the sums of a batch without bonds are zero rows
        return (s.zero_() if s is not None else None), q
    _lib.call("gcmi_dmpnn_message", 1 if transposed else 0, _ptr(x), _ld(x) if x is not None else 0, d, _ptr(out_ptr),
              _ptr(rev), n_atoms, n_bonds, _ptr(add), _ld(add) if add is not None else 0, _ptr(s),
              _ld(s) if s is not None else 0, _ptr(q), _ld(q) if q is not None else 0, _stream())
    return s, q


DMPNN_UPDATE_MAX_HIDDEN = 320


def dmpnn_update_scratch_floats(d: int) -> int:
    """Floats of the weight-image scratch of ``gcmi_dmpnn_update_fwd`` at width d."""
    return ((d + 15) // 16) * ((d + 31) // 32) * 768


def dmpnn_update_fwd(x: torch.Tensor, inp: torch.Tensor, weight: torch.Tensor, out_ptr: torch.Tensor, rev: torch.Tensor,
                     bond_src: torch.Tensor, relu: bool, scratch: torch.Tensor,
                     out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``h[b] = act(inp[b] + (S[a] - x[rev[b]]) . weight^T)`` over a VALIDATED bond plan, the aggregated rows never
    written (``gcmi_dmpnn_update_fwd``; d <= 320, nn.Linear weight).  ``scratch``: a contiguous float32 CUDA vector of
    at least ``dmpnn_update_scratch_floats(d)``, overwritten with the split image of ``weight``."""
    n_atoms, n_bonds = out_ptr.numel() - 1, rev.numel()
    _i32vec(out_ptr, "out_ptr"), _i32vec(rev, "rev"), _i32vec(bond_src, "bond_src", n_bonds)
    _mat(x, "x", rows=n_bonds)
    d = x.shape[1]
    if d > DMPNN_UPDATE_MAX_HIDDEN:
        raise ValueError("dmpnn_update_fwd covers d_hidden <= %d (got %d)" % (DMPNN_UPDATE_MAX_HIDDEN, d))
    _mat(inp, "input", rows=n_bonds, cols=d), _mat(weight, "weight", rows=d, cols=d)
    if not (scratch.is_cuda and scratch.dtype == torch.float32 and scratch.is_contiguous()):
        raise ValueError("dmpnn_update_fwd: scratch must be a contiguous float32 CUDA tensor")
    h = torch.empty((n_bonds, d), dtype=torch.float32, device=x.device) if out is None else _mat(out, "out", n_bonds, d)
    if n_bonds == 0:
        return h
    _lib.call("gcmi_dmpnn_update_fwd", _ptr(x), _ld(x), _ptr(inp), _ld(inp), _ptr(weight), _ld(weight), d, 1 if relu else 0,
              _ptr(out_ptr), _ptr(rev), _ptr(bond_src), n_atoms, n_bonds, _ptr(scratch), scratch.numel(), _ptr(h), _ld(h),
              _stream())
    return h


DMPNN_BATCH_BLOCKS = ("mol_ptr", "out_ptr", "bond_src", "rev", "atom_membership", "atoms_per_mol", "atom_features",
                      "f_ini_atoms_bonds", "global_features")
# collate_set_kernel over the D-MPNN args: one workgroup of DMPNN_COLLATE_THREADS threads per molecule; a pass of the workgroup covers that
# many per-atom / per-bond words and flat atom-row words, and DMPNN_COLLATE_ROWS_PER_PASS f_ini rows (one per wave)
DMPNN_COLLATE_MOLS_PER_WORKGROUP = 1
DMPNN_COLLATE_THREADS = 256
DMPNN_COLLATE_ROWS_PER_PASS = DMPNN_COLLATE_THREADS // 64


def dmpnn_batch_layout(n_mols: int, n_atoms: int, n_bonds: int, atom_fdim: int, bond_fdim: int, global_fdim: int):
    """The packed D-MPNN batch buffer (``gcmi_dmpnn_collate_words``): ``(words, {block: (offset, shape)})`` for the
    nine blocks of ``DMPNN_BATCH_BLOCKS``, 4-byte words, every block at a 16-byte boundary."""
    sizes = (n_mols, n_atoms, n_bonds, atom_fdim, bond_fdim, global_fdim)
    if min(sizes) < 0 or max(sizes) > 2 ** 31 - 1:
        raise ValueError("dmpnn_batch_layout: sizes must be within [0, 2^31): %r" % (sizes,))
    shapes = ((n_mols + 1,), (n_atoms + 1,), (n_bonds,), (n_bonds,), (n_atoms,), (n_mols, 1), (n_atoms, atom_fdim),
              (n_bonds, atom_fdim + bond_fdim), (n_mols, global_fdim))
    return _batch_layout("gcmi_dmpnn_collate_words", sizes, DMPNN_BATCH_BLOCKS, shapes)


DMPNN_SET_ARRAYS = ("atom_ptr", "bond_ptr", "atom_features", "bond_features", "sorted_src", "sorted_rev", "out_start",
                    "global_features")


def _dmpnn_collate_sizes(arrays, n_mols: int, n_atoms: int, n_bonds: int):
    M = arrays["atom_ptr"].shape[0] - 1
    fa, fb, fg = (int(arrays[k].shape[1]) for k in ("atom_features", "bond_features", "global_features"))
    if M < 0 or arrays["bond_ptr"].shape[0] != M + 1 or arrays["global_features"].shape[0] != M:
        raise ValueError("dmpnn_collate: atom_ptr, bond_ptr and global_features must cover the same molecules")
    A, B = arrays["atom_features"].shape[0], arrays["bond_features"].shape[0]
    if arrays["out_start"].shape[0] != A or arrays["sorted_src"].shape[0] != B or arrays["sorted_rev"].shape[0] != B:
        raise ValueError("dmpnn_collate: out_start needs one entry per atom, sorted_src and sorted_rev one per bond")
    if min(n_mols, n_atoms, n_bonds) < 0 or max(n_mols, n_atoms, n_bonds) > 2 ** 31 - 2:
        raise ValueError("dmpnn_collate: a batch holds at most 2^31 - 2 molecules, atoms and bonds")
    return M, fa, fb, fg


def dmpnn_collate(arrays, plan: torch.Tensor, n_mols: int, n_atoms: int, n_bonds: int) -> torch.Tensor:
    """``gcmi_dmpnn_collate``: the packed batch buffer (int32 words, ``dmpnn_batch_layout``) of the molecules named by
    ``plan`` = ``[mol_idx ; atom_off ; bond_off]`` (int32, on the device), gathered from the resident set ``arrays``
    (``DMPNN_SET_ARRAYS``: contiguous CUDA tensors, the two offset arrays int64, indices int32, features float32 2-D).
    The molecule indices must have been validated by the caller: the kernel skips a bad one, it does not report it."""
    M, fa, fb, fg = _dmpnn_collate_sizes(arrays, n_mols, n_atoms, n_bonds)
    _check_set({k: arrays[k] for k in DMPNN_SET_ARRAYS}, ("atom_ptr", "bond_ptr"), True, "dmpnn_collate")
    _i32vec(plan, "plan", 3 * n_mols + 2)
    words, _ = dmpnn_batch_layout(n_mols, n_atoms, n_bonds, fa, fb, fg)
    out = torch.empty(words, dtype=torch.int32, device=plan.device)
    _lib.call("gcmi_dmpnn_collate", *[_ptr(arrays[k]) for k in DMPNN_SET_ARRAYS], M, fa, fb, fg, _ptr(plan), n_mols, n_atoms,
              n_bonds, _ptr(out), words, _stream())
    return out


def dmpnn_collate_host(arrays, plan: np.ndarray, n_mols: int, n_atoms: int, n_bonds: int,
                       out: Optional[np.ndarray] = None) -> np.ndarray:
    """``gcmi_dmpnn_collate_host``: the same routine over numpy arrays, for tests without a GPU.  ``out``: an int32
    vector to write into (at least the layout's words)."""
    M, fa, fb, fg = _dmpnn_collate_sizes(arrays, n_mols, n_atoms, n_bonds)
    _check_set({k: arrays[k] for k in DMPNN_SET_ARRAYS}, ("atom_ptr", "bond_ptr"), False, "dmpnn_collate_host")
    _check_host_plan(plan, n_mols, "n_mols", "dmpnn_collate_host")
    words, _ = dmpnn_batch_layout(n_mols, n_atoms, n_bonds, fa, fb, fg)
    if out is None:
        out = np.empty(words, np.int32)
    _check_host_out(out, "dmpnn_collate_host")
    _lib.call("gcmi_dmpnn_collate_host", *[_vp(arrays[k].ctypes.data) for k in DMPNN_SET_ARRAYS], M, fa, fb, fg,
              _vp(plan.ctypes.data), n_mols, n_atoms, n_bonds, _vp(out.ctypes.data), out.size)
    return out


def edge_network_sum(g: torch.Tensor, n_hidden: int, pair_feat: torch.Tensor, dst_ptr: torch.Tensor,
                     src: torch.Tensor) -> torch.Tensor:
    g = _mat(g, "g")
    pf = _mat(pair_feat, "pair_feat")
    K = pf.shape[1]
    if g.shape[1] != (K + 1) * n_hidden:
        raise ValueError("g must have (n_pair_feat + 1) * n_hidden columns")
    n_dst = dst_ptr.numel() - 1
    out = torch.empty((n_dst, n_hidden), dtype=torch.float32, device=g.device)
    _lib.call("gcmi_edge_network_sum", _ptr(g), _ld(g), n_hidden, K, _ptr(pf), _ld(pf),
              _ptr(_i32vec(dst_ptr, "dst_ptr")), _ptr(_i32vec(src, "src", pf.shape[0])), n_dst, _ptr(out), _ld(out),
              _stream())
    return out


def expand_atom_codes(codes: torch.Tensor, ld_out: int = 76) -> torch.Tensor:
    """(N, >= 8) uint8 code rows (row stride a multiple of 8 bytes) -> (N, ld_out) float32 feature rows."""
    if not torch.is_tensor(codes) or not codes.is_cuda or codes.dtype != torch.uint8 or codes.dim() != 2:
        raise _lib.GcmiError("codes must be a 2-D uint8 CUDA tensor")
    if codes.shape[1] < 8 or (codes.shape[1] > 1 and codes.stride(1) != 1):
        raise ValueError("code rows are 8 contiguous bytes")
    n = codes.shape[0]
    out = torch.empty((n, ld_out), dtype=torch.float32, device=codes.device)
    _lib.call("gcmi_expand_atom_codes", _ptr(codes), int(codes.stride(0)) if n > 1 else int(codes.shape[1]), n,
              _ptr(out), ld_out, _stream())
    return out


def edge_network_moments(h: torch.Tensor, pair_feat: torch.Tensor, dst_ptr: torch.Tensor, src: torch.Tensor,
                         mol_ptr: Optional[torch.Tensor] = None, max_mol_atoms: int = 0):
    """T[i] = [sum_p pf[p,0] h[src_p] | ... | sum_p pf[p,K-1] h[src_p] | sum_p h[src_p]] per destination atom.
    ``mol_ptr`` (int32 CSR of the atoms per molecule): the molecule-staged kernel (same T)."""
    h = _mat(h, "h")
    pf = _mat(pair_feat, "pair_feat")
    d, K = h.shape[1], pf.shape[1]
    n_dst = dst_ptr.numel() - 1
    t = torch.empty((n_dst, (K + 1) * d), dtype=torch.float32, device=h.device)
    if pf.shape[0] == 0:  # no pair at all: an empty tensor has no buffer, which the C entry points refuse
        # the limits below mirror the "bad shape" GCMI_CHECK_ARG of gcmi_edge_network_moments and
        # gcmi_edge_network_moments_mol in csrc/mpnn.hip, which this return goes past: change them together
        if not (0 < d <= 128 and 0 < K <= 16):
            raise _lib.GcmiError("edge_network_moments: bad shape (n_hidden <= 128, n_pair_feat <= 16)")
        _i32vec(dst_ptr, "dst_ptr")
        _i32vec(src, "src", 0)
        if mol_ptr is not None:
            _i32vec(mol_ptr, "mol_ptr")
        return t.zero_()
    if mol_ptr is not None:
        mp = _i32vec(mol_ptr, "mol_ptr")
        _lib.call("gcmi_edge_network_moments_mol", _ptr(h), _ld(h), d, K, _ptr(pf), _ld(pf),
                  _ptr(_i32vec(dst_ptr, "dst_ptr")), _ptr(_i32vec(src, "src", pf.shape[0])), n_dst, _ptr(mp),
                  mp.numel() - 1, int(max_mol_atoms), _ptr(t), _ld(t), _stream())
        return t
    _lib.call("gcmi_edge_network_moments", _ptr(h), _ld(h), d, K, _ptr(pf), _ld(pf), _ptr(_i32vec(dst_ptr, "dst_ptr")),
              _ptr(_i32vec(src, "src", pf.shape[0])), n_dst, _ptr(t), _ld(t), _stream())
    return t


def _gate_tensors(what: str, *named):
    shape = named[0][0].shape
    for t, nm in named:
        if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.shape == shape):
            raise ValueError("%s: %s must be a contiguous float32 CUDA tensor of the gate shape" % (what, nm))


def gru_gates_(z: torch.Tensor, r: torch.Tensor, h: torch.Tensor) -> torch.Tensor:
    _gate_tensors("gru_gates_", (z, "z"), (r, "r"), (h, "h"))
    hr = torch.empty_like(h)
    _lib.call("gcmi_gru_gates", _ptr(z), _ptr(r), _ptr(h), _ptr(hr), z.numel(), _stream())
    return hr


def gru_out(z: torch.Tensor, hpre: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
    _gate_tensors("gru_out", (z, "z"), (hpre, "hpre"), (x, "x"))
    out = torch.empty_like(x)
    _lib.call("gcmi_gru_out", _ptr(z), _ptr(hpre), _ptr(x), _ptr(out), z.numel(), _stream())
    return out


SET2SET_MAX_FEATURES = 512  # (gcmi_set2set_attend and its backward refuse wider rows)


def set2set_attend(x: torch.Tensor, mol_ptr: torch.Tensor, h: torch.Tensor) -> torch.Tensor:
    x = _mat(x, "x")
    n_mols = mol_ptr.numel() - 1
    h = _mat(h, "h", rows=n_mols, cols=x.shape[1])
    q = torch.empty((n_mols, 2 * x.shape[1]), dtype=torch.float32, device=x.device)
    _lib.call("gcmi_set2set_attend", _ptr(x), _ld(x), x.shape[1], _ptr(_i32vec(mol_ptr, "mol_ptr")), n_mols, _ptr(h),
              _ld(h), _ptr(q), _ld(q), _stream())
    return q


def lstm_cell_(z: torch.Tensor, c: torch.Tensor) -> torch.Tensor:
    z = _mat(z, "z")
    H = z.shape[1] // 4
    c = _mat(c, "c", rows=z.shape[0], cols=H)
    h = torch.empty_like(c)
    _lib.call("gcmi_lstm_cell", _ptr(z), _ld(z), H, z.shape[0], _ptr(c), _ld(c), _ptr(h), _ld(h), _stream())
    return h


def gru_gates_bwd(z: torch.Tensor, r: torch.Tensor, h: torch.Tensor, dz: torch.Tensor, dhr: torch.Tensor):
    """Backward of ``gru_gates_`` from its outputs z, r and its input h: (dzp, drp, dh)."""
    _gate_tensors("gru_gates_bwd", (z, "z"), (r, "r"), (h, "h"), (dz, "dz"), (dhr, "dhr"))
    dzp, drp, dh = torch.empty_like(z), torch.empty_like(z), torch.empty_like(z)
    _lib.call("gcmi_gru_gates_bwd", _ptr(z), _ptr(r), _ptr(h), _ptr(dz), _ptr(dhr), _ptr(dzp), _ptr(drp), _ptr(dh),
              z.numel(), _stream())
    return dzp, drp, dh


def gru_out_bwd(z: torch.Tensor, hpre: torch.Tensor, x: torch.Tensor, dout: torch.Tensor):
    """Backward of ``gru_out``: (dz, dhpre, dx)."""
    _gate_tensors("gru_out_bwd", (z, "z"), (hpre, "hpre"), (x, "x"), (dout, "dout"))
    dz, dhpre, dx = torch.empty_like(z), torch.empty_like(z), torch.empty_like(z)
    _lib.call("gcmi_gru_out_bwd", _ptr(z), _ptr(hpre), _ptr(x), _ptr(dout), _ptr(dz), _ptr(dhpre), _ptr(dx),
              z.numel(), _stream())
    return dz, dhpre, dx


def set2set_attend_bwd(x: torch.Tensor, mol_ptr: torch.Tensor, h: torch.Tensor, dq: torch.Tensor, *,
                       dx: Optional[torch.Tensor] = None, accumulate: bool = False):
    """Backward of ``set2set_attend`` (the softmax is recomputed): (dx, dh).  ``dx``: write into this matrix;
    ``accumulate``: dx += instead of dx =, needs ``dx``."""
    if accumulate and dx is None:
        raise ValueError("accumulate needs the matrix to add to: pass dx")
    x = _mat(x, "x")
    n_feat = x.shape[1]
    if not 0 < n_feat <= SET2SET_MAX_FEATURES:
        raise _lib.GcmiError("set2set_attend_bwd: %d features, the kernel covers 1..%d" % (n_feat, SET2SET_MAX_FEATURES))
    n_mols = mol_ptr.numel() - 1
    h = _mat(h, "h", rows=n_mols, cols=n_feat)
    dq = _mat(dq, "dq", rows=n_mols, cols=2 * n_feat)
    dx = torch.empty_like(x) if dx is None else _mat(dx, "dx", rows=x.shape[0], cols=n_feat)
    dh = torch.empty_like(h)
    _lib.call("gcmi_set2set_attend_bwd", _ptr(x), _ld(x), n_feat, _ptr(_i32vec(mol_ptr, "mol_ptr")), n_mols, _ptr(h),
              _ld(h), _ptr(dq), _ld(dq), _ptr(dx), _ld(dx), 1 if accumulate else 0, _ptr(dh), _ld(dh), _stream())
    return dx, dh


def lstm_cell_bwd(z: torch.Tensor, c_prev: torch.Tensor, dh: torch.Tensor, dc: Optional[torch.Tensor] = None):
    """Backward of ``lstm_cell_`` from the gate pre-activations z and the cell state it started from: (dz, dc_prev).
    ``dc``: the gradient of the new cell state, None for zero.  The C entry takes a leading dimension for z alone."""
    z = _mat(z, "z")
    H = z.shape[1] // 4
    if H == 0 or z.shape[1] != 4 * H:
        raise ValueError("z must hold four gates per hidden column, got %d columns" % z.shape[1])
    _mat(c_prev, "c_prev", rows=z.shape[0], cols=H)
    _gate_tensors("lstm_cell_bwd", (c_prev, "c_prev"), (dh, "dh"), *([] if dc is None else [(dc, "dc")]))
    dz = torch.empty(z.shape, dtype=torch.float32, device=z.device)  # (contiguous whatever z's row stride)
    dc_prev = torch.empty_like(c_prev)
    _lib.call("gcmi_lstm_cell_bwd", _ptr(z), _ld(z), H, z.shape[0], _ptr(c_prev), _ptr(dh), _ptr(dc), _ptr(dz),
              _ptr(dc_prev), _stream())
    return dz, dc_prev


def timing_enable(kernel_id: int, on: bool = True):
    _lib.call("gcmi_timing_enable", kernel_id, 1 if on else 0)


def timing_read(kernel_id: int, reset: bool = True):
    n = ctypes.c_int64(0)
    ms = ctypes.c_double(0.0)
    _lib.call("gcmi_timing_read", kernel_id, ctypes.byref(n), ctypes.byref(ms), 1 if reset else 0)
    return int(n.value), float(ms.value)


# ------------------------------------------------------------------ autograd glue
def _graphconv_offsets(max_deg: int, k: int, n_out: int):
    """Offsets (floats) of the per-degree blocks inside the packed parameter
    order of the reference: rel_1, self_1, ..., rel_max, self_max, self_0
    (models/torch_models/layers.py:6189-6224).  Segment d = degree d."""
    blk = k * n_out
    w_rel = [-1] + [(2 * (d - 1)) * blk for d in range(1, max_deg + 1)]
    w_self = [2 * max_deg * blk] + [(2 * (d - 1) + 1) * blk for d in range(1, max_deg + 1)]
    b_off = [d * n_out for d in range(max_deg + 1)]
    return w_rel, w_self, b_off


class GraphConvFn(torch.autograd.Function):
    """out = act(S . W_rel[deg] + X . W_self[deg] + bsum[deg]),  S = gather-sum(X).
    wpack: (2*max_deg+1, K, n_out) in reference order; bsum: (max_deg+1, n_out)."""

    @staticmethod
    def forward(ctx, x, wpack, bsum, graph: BatchGraph, relu: bool, grad_masked: bool = False):
        """grad_masked: the consumer's backward already multiplies by (out > 0) (a folded
        BatchNorm does), so the ReLU derivative is not applied again."""
        x = rowmajor(x)
        wpack = wpack.contiguous()
        bsum = bsum.contiguous()
        k, n_out = wpack.shape[1], wpack.shape[2]
        if wpack.shape[0] != 2 * graph.max_deg + 1 or tuple(bsum.shape) != (graph.max_deg + 1, n_out):
            raise ValueError("GraphConv parameters do not match max_deg=%d" % graph.max_deg)
        _mat(x, "atom_features", rows=graph.n_atoms)
        if x.shape[1] < k or x.shape[1] >= k + 4:
            raise ValueError("atom_features has %d columns, the layer expects %d" % (x.shape[1], k))
        # x may carry zero padding columns (DeviceBatch pads 75 -> 76 so that the gather moves
        # 16 bytes per lane); the GEMMs read the first k columns only
        w_rel, w_self, b_off = _graphconv_offsets(graph.max_deg, k, n_out)
        s = gather_sum(graph, x)
        out = seg_gemm(list(graph.seg_begin), list(graph.seg_end), s[:, :k], wpack, w_rel, x[:, :k],
                       wpack, w_self, bsum, b_off, n_out, False, relu, graph.n_atoms, k, k)
        ctx.graph = graph
        ctx.relu = relu and not grad_masked
        ctx.save_for_backward(x, s, wpack, out)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, s, wpack, out = ctx.saved_tensors
        graph = ctx.graph
        k, n_out = wpack.shape[1], wpack.shape[2]
        w_rel, w_self, b_off = _graphconv_offsets(graph.max_deg, k, n_out)
        sb, se = list(graph.seg_begin), list(graph.seg_end)
        g = rowmajor(dout)
        if ctx.relu:
            g = relu_bwd_(g.clone(), out)
        dw = dbs = dx = None
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            dw = torch.zeros_like(wpack)
            dbs = torch.zeros((graph.max_deg + 1, n_out), dtype=torch.float32, device=g.device)
            seg_gemm_wgrad(sb, se, s[:, :k], g, dw, w_rel, None, None, False)
            seg_gemm_wgrad(sb, se, x[:, :k], g, dw, w_self, dbs, b_off, False)
        if ctx.needs_input_grad[0]:
            # dS = g . W_rel^T, dX = g . W_self^T  (same blocks read transposed)
            ds = seg_gemm(sb, se, g, wpack, w_rel, None, None, None, None, None, k, True, False,
                          graph.n_atoms, n_out, 0)
            dx = seg_gemm(sb, se, g, wpack, w_self, None, None, None, None, None, k, True, False,
                          graph.n_atoms, n_out, 0)
            if graph.symmetric:
                gather_sum(graph, ds, dx, accumulate=True)  # no atomics: bonds are listed from both ends
            else:
                scatter_add(graph, ds, dx)
            if x.shape[1] > k:
                dx = torch.nn.functional.pad(dx, (0, x.shape[1] - k))
        return dx, dw, dbs, None, None, None


class PoolFn(torch.autograd.Function):
    """GraphPool, optionally with the preceding BatchNorm1d folded into it."""

    @staticmethod
    def forward(ctx, x, gamma, beta, running_mean, running_var, graph: BatchGraph, bn: bool,
                training: bool, eps: float, momentum: float, relu_in: bool = False):
        """relu_in: x is the output of a fused ReLU whose producer was told
        ``grad_masked``; the returned gradient is then w.r.t. the ReLU input."""
        x = rowmajor(x)
        _mat(x, "atom_features", rows=graph.n_atoms)
        mean = invstd = scale = shift = None
        if bn:
            if training:
                mean, invstd, scale, shift = bn_stats(x, gamma, beta, running_mean, running_var, eps,
                                                      momentum)
            else:
                scale, shift = bn_fold_eval(gamma, beta, running_mean, running_var, eps)
        out, arg = gather_max(graph, x, scale, shift)
        if relu_in and not (bn and training):
            raise ValueError("relu_in needs a training-mode BatchNorm to fold the mask into")
        ctx.graph, ctx.bn, ctx.training, ctx.relu_in = graph, bn, training, relu_in
        ctx.save_for_backward(x, gamma, mean, invstd, scale, arg)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, gamma, mean, invstd, scale, arg = ctx.saved_tensors
        dy = gather_max_bwd(ctx.graph, rowmajor(dout), arg)
        if not ctx.bn:
            return (dy,) + (None,) * 10
        if not ctx.training:
            raise NotImplementedError("gradients through an eval-mode BatchNorm are not implemented")
        dgamma, dbeta, dx = bn_bwd(dy, x, gamma, mean, invstd, ctx.needs_input_grad[0], ctx.relu_in)
        return (dx, dgamma, dbeta) + (None,) * 8


class ReadoutFn(torch.autograd.Function):
    """GraphGather ([sum | max] per molecule, optional tanh), optionally with the
    preceding BatchNorm1d folded into it."""

    @staticmethod
    def forward(ctx, x, gamma, beta, running_mean, running_var, graph: BatchGraph, n_mols: int,
                bn: bool, training: bool, eps: float, momentum: float, tanh: bool,
                relu_in: bool = False):
        x = rowmajor(x)
        _mat(x, "atom_features", rows=graph.n_atoms)
        mean = invstd = scale = shift = None
        if bn:
            if training:
                mean, invstd, scale, shift = bn_stats(x, gamma, beta, running_mean, running_var, eps,
                                                      momentum)
            else:
                scale, shift = bn_fold_eval(gamma, beta, running_mean, running_var, eps)
        out, arg = readout(graph, x, n_mols, scale, shift, tanh)
        if relu_in and not (bn and training):
            raise ValueError("relu_in needs a training-mode BatchNorm to fold the mask into")
        ctx.graph, ctx.bn, ctx.training, ctx.tanh, ctx.relu_in = graph, bn, training, tanh, relu_in
        ctx.save_for_backward(x, gamma, mean, invstd, out, arg)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, gamma, mean, invstd, out, arg = ctx.saved_tensors
        dy = readout_bwd(ctx.graph, rowmajor(dout), out, arg, ctx.tanh)
        if not ctx.bn:
            return (dy,) + (None,) * 12
        if not ctx.training:
            raise NotImplementedError("gradients through an eval-mode BatchNorm are not implemented")
        dgamma, dbeta, dx = bn_bwd(dy, x, gamma, mean, invstd, ctx.needs_input_grad[0], ctx.relu_in)
        return (dx, dgamma, dbeta) + (None,) * 10


# ---- parameter gradients straight into ``p.grad``
# The weight-gradient kernels ADD into their output.  When a training step has put a zeroed view of one flat arena
# behind every ``p.grad`` (deepchem_amd.dist.FlatGradArena.attach) and switches this on around ``backward()``, the
# autograd functions below and in models/torch_models hand the kernels ``p.grad`` itself and return no gradient for
# the parameter: a weight that is used T times (the message rounds of MPNN share theirs) then costs neither T
# temporaries with their zero fills nor T - 1 additions by the autograd engine.
_DIRECT_GRAD = [False]


class direct_param_grads:
    def __init__(self, on: bool = True):
        self.on = bool(on)

    def __enter__(self):
        self.prev = _DIRECT_GRAD[0]
        _DIRECT_GRAD[0] = self.on
        return self

    def __exit__(self, *exc):
        _DIRECT_GRAD[0] = self.prev
        return False


def grad_target(p):
    """``p.grad`` if gradients of ``p`` may be accumulated in place right now, else None."""
    if not _DIRECT_GRAD[0] or p is None or not isinstance(p, torch.nn.Parameter):
        return None
    g = p.grad
    if g is None or g.dtype != torch.float32 or not g.is_contiguous() or g.shape != p.shape:
        return None
    return g


def grad_buffer(p, like: torch.Tensor):
    """Where a kernel that adds into its output accumulates the gradient of ``p``, and what the autograd Function
    returns for it: ``(p.grad, None)`` if ``grad_target`` allows, else ``(zeros, those same zeros)`` shaped like ``like``."""
    target = grad_target(p)
    if target is not None:
        return target, None
    buf = torch.zeros_like(like)
    return buf, buf


class StandardLossFn(torch.autograd.Function):
    """mean(w * loss(outputs, labels)) with the gradient produced in the same pass."""

    @staticmethod
    def forward(ctx, outputs, labels, weights, kind: int):
        loss, dlogits, _ = loss_fwd_bwd(kind, outputs, labels, weights)
        ctx.save_for_backward(dlogits)
        ctx.shape = outputs.shape
        return loss

    @staticmethod
    def backward(ctx, gl):
        (dlogits,) = ctx.saved_tensors
        return (dlogits * gl).reshape(ctx.shape), None, None, None


class SoftmaxFn(torch.autograd.Function):

    @staticmethod
    def forward(ctx, logits):
        p = softmax_lastdim(logits)
        ctx.save_for_backward(p)
        return p

    @staticmethod
    def backward(ctx, gp):
        (p,) = ctx.saved_tensors
        return p * (gp - (gp * p).sum(-1, keepdim=True))
