"""Shared pieces of the kernel edge suites (TEST INFRASTRUCTURE: tests/test_gpu_mpnn_edges.py and
tests/test_gpu_weave_edges.py): moving float32 test data to the GPU as column blocks of wider matrices, and the two
kinds of tolerance those suites use against a float64 restatement.

* ``assert_sum_bound``: sums and products, per element ``|got - ref| <= (n_terms + 2) eps32 sum|terms|`` -- the
  standard forward bound, whatever the order of the additions; ``sum|terms|`` is the restatement run on absolute
  values, ``n_terms`` the longest chain of additions behind the element.
* ``family_error`` / ``allowed``: kernels through expf / tanhf.  The same formula is run on the CPU in torch
  float32 and float64 on the test's own inputs; ``E`` is the largest float32 error over all cases of a family, per
  output and relative to ``max(|ref|, 1)``; the kernel gets ``max(4 E, 8 eps32) max(|ref|, 1)`` per element.
"""
import numpy as np
import torch

DEV = "cuda:0"
EPS32 = float(np.finfo(np.float32).eps)
SENTINEL = 7.5


def to_dev(a, grad=False):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t.requires_grad_(True) if grad else t


def wide(a, left, right, grad=False):
    """(column slice holding ``a``, the wider sentinel-filled float32 matrix it is a view of)."""
    n, c = a.shape
    full = np.full((n, left + c + right), SENTINEL, np.float32)
    full[:, left:left + c] = a
    w = to_dev(full, grad)
    return w[:, left:left + c], w


def to_np(t):
    return t.detach().double().cpu().numpy() if torch.is_tensor(t) else np.asarray(t, np.float64)


def assert_outside_untouched(wide_matrix, lo, width, what, value=SENTINEL):
    """Every column of ``wide_matrix`` outside [lo, lo + width) still holds ``value`` (the fill of ``wide``)."""
    outside = wide_matrix.detach().clone()
    outside[:, lo:lo + width] = value
    assert bool((outside == value).all()), what + ": columns outside the block were written"


def assert_sum_bound(got, ref, ref_abs, n_terms, what):
    got = to_np(got)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.isfinite(got).all(), what
    err = np.abs(got - ref)
    bound = np.broadcast_to((np.asarray(n_terms, np.float64) + 2) * EPS32 * ref_abs, err.shape)
    bad = err > bound
    assert not bad.any(), "%s: %d elements over the bound, worst err %.3e at bound %.3e" % (
        what, int(bad.sum()), float(err[bad].max()), float(bound[bad].min()))


def assert_close(got, ref, allowed_rel, what):
    """|got - ref| <= allowed_rel * max(|ref|, 1) per element."""
    got = to_np(got)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.isfinite(got).all(), what
    rel = np.abs(got - ref) / np.maximum(np.abs(ref), 1.0)
    worst = float(rel.max()) if rel.size else 0.0
    print("%s: worst %.3e allowed %.3e" % (what, worst, allowed_rel))
    assert worst <= allowed_rel, "%s: error %.3e relative to max(|ref|, 1), allowed %.3e" % (what, worst, allowed_rel)


def family_error(cases):
    """Per output: the largest error of ``case.cpu(torch.float32)`` against ``case.cpu(torch.float64)`` over the
    cases, relative to max(|ref|, 1).  Every case returns the same list of outputs."""
    worst = None
    for c in cases:
        errs = [float((np.abs(b - a) / np.maximum(np.abs(a), 1.0)).max()) if a.size else 0.0
                for a, b in zip(c.cpu(torch.float64), c.cpu(torch.float32))]
        worst = errs if worst is None else [max(x, y) for x, y in zip(worst, errs)]
    return worst


def allowed(cases):
    return [max(4.0 * e, 8.0 * EPS32) for e in family_error(cases)]
