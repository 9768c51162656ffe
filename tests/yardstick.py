"""What the float32 yardsticks of the GPU tests share.  No test is collected here.

A bar of the form ``FACTOR * e32`` is only a bar if ``e32`` is a fixed number and if it measures what a correct kernel
is allowed to do.  Two things follow ("Float32 yardsticks: reproducible and order-aware"):

* ``f32_threads(n)``: torch's float32 reductions and scatter-adds on the CPU follow the number of threads, and some are
  not even repeatable at more than one.  A restatement that serves as a yardstick runs under a stated count.
* ``any_order_e32``: torch's float32 sums are blocked, far more accurate than a chain of float atomics that land in
  arrival order.  For a tensor that a kernel adds atomically the yardstick also holds what float32 accumulation of the
  SAME addends makes in seeded random orders: the order-dependent part of the error, from the reference alone.
"""
import contextlib

import numpy as np
import torch


@contextlib.contextmanager
def f32_threads(n):
    """torch's intra-op thread count set to ``n`` inside the block and put back after it."""
    prev = torch.get_num_threads()
    torch.set_num_threads(n)
    try:
        yield
    finally:
        torch.set_num_threads(prev)


def restatement_threads(dtype, n):
    """``f32_threads(n)`` where ``dtype`` is float32 (the run that serves as a yardstick), nothing otherwise: for the
    ``for dtype in (float64, float32)`` loops of the restatements."""
    return f32_threads(n) if dtype == torch.float32 else contextlib.nullcontext()


def any_order_e32(addends, index, n_rows, scale, orders=8, seed=0):
    """The largest ``max |acc - sum64| / scale`` over ``orders`` permutations drawn from ``RandomState(seed)``, where
    ``acc`` (n_rows, C) float32 receives the float32-rounded ``addends`` (A, C), addend ``a`` into row ``index[a]``,
    strictly one after another (``np.add.at`` on a float32 target), and ``sum64`` is the float64 sum of the unrounded
    addends.  A fixed number that never sees the code under test."""
    addends = np.asarray(addends, np.float64)
    if addends.ndim != 2:
        raise ValueError("any_order_e32: addends must be (A, C)")
    index = np.asarray(index, np.int64).reshape(-1)
    A, C = addends.shape
    if index.shape[0] != A or (A and (index.min() < 0 or index.max() >= n_rows)):
        raise ValueError("any_order_e32: one row inside [0, %d) per addend" % n_rows)
    if not scale > 0:
        raise ValueError("any_order_e32: scale must be positive")
    sum64 = np.zeros((n_rows, C), np.float64)
    np.add.at(sum64, index, addends)
    a32 = addends.astype(np.float32)
    rng = np.random.RandomState(seed)
    worst = 0.0
    for _ in range(orders):
        perm = rng.permutation(A)
        acc = np.zeros((n_rows, C), np.float32)
        np.add.at(acc, index[perm], a32[perm])
        if acc.size:
            worst = max(worst, float(np.max(np.abs(acc.astype(np.float64) - sum64))) / scale)
    return worst
