"""The crystal-graph convolution kernels (csrc/cgcnn.hip) at the sizes their launch arithmetic depends on.

Bar: ``check_kernels`` of tests/test_gpu_cgcnn.py, unchanged (``bar`` of tests/test_gpu_mat.py per tensor: the error
against the float64 restatement at most 4 times the float32 restatement's, floor one float32 ulp of the tensor's largest
entry); the ratios are printed.  Where two launches differ only in leading dimension, column offset or tiling the
assertion is ``torch.equal``: no atomics, fixed summation orders.  A row of H floats takes H / 4 lanes and a workgroup
256 // (H / 4) rows; cg_stats and cg_bwd_stats leave one partial row per workgroup of a grid cut to 1024, and the
finishing kernels give lane l the partials l, l + 64, ...; the other kernels stride under the 8192 workgroups of
``grid_for``.

Cases and what each pins:
* widths, 'above' (129 nodes, 193 edges), both modes: H = 8 and 12 (2 and 3 lanes per row, 128 and 85 rows per
  workgroup, 0 and 1 idle threads), 44 and 100 (22 and 25 lanes, 11 and 10 rows, 14 and 6 idle threads), 124 (31 lanes,
  8 rows, 8 idle threads; cg_list_sum at width 248 with 62 lanes, 4 rows and 8 idle threads).
* 'cap' (8200 nodes, 8300 edges) at H = 128, both modes: 1038 edge groups and 1025 node groups of 8 rows, past the 1024
  partial rows: cg_stats and cg_bwd_stats take a second turn.  In training also with the cancellation offset
  (``OFFSET_SIGMAS`` of tests/test_gpu_cgcnn.py as it stands): the pivot a workgroup re-uses for its later turns stands
  under a mean 300 standard deviations from zero.
* 'pair' (two nodes, the edges 0 -> 1 and 1 -> 0) at H = 64 in training: statistics of 2 rows.
* views, 'edge' batch at H = 60 and 128, both modes, the five entries called directly: Q as the columns [4, 4 + 2H) of a
  NaN matrix of 2H + 8 (ldq), h, h' and the cotangent as the columns [4, 4 + H), [8, 8 + H) and [12, 12 + H) of NaN
  matrices of H + 8, H + 12 and H + 16 (ldh, ldhn, lddh): every result has the dense call's bits.
* tiling: 'tile' (2731 nodes, 4099 edges) at H = 128 in eval mode, itself under the bar, 25 times in one batch: 68 275
  nodes = 8535 node groups of 8 rows and 17 069 of cg_list_sum (4 rows), past 8192 workgroups; 102 475 edges.  Every
  copy's rows of out, dh, dP and dQ equal the base's.

Measured on an MI355X (worst ratio): the widths 1.88 (H = 44, eval, dQ), 'cap' 1.37 (eval, h'), 'cap' under the offset
1.04, 'pair' 1.07, 'tile' 1.12.  Worst of the family: 1.88.
"""
import numpy as np
import pytest
import torch

from deepchem_amd import ops
from tests import cgcnn_refs as R
from tests.test_gpu_cgcnn import DEV, OFFSET_SIGMAS, check_kernels, kernel_case

pytestmark = pytest.mark.gpu
NAN = float("nan")
EDGE_WIDTHS = [8, 12, 44, 100, 124]
MODES = pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
TILE_COPIES = 25


def label(name, hidden, training):
    return "%s H%d %s" % (name, hidden, "train" if training else "eval")


@MODES
@pytest.mark.parametrize("hidden", EDGE_WIDTHS)
def test_kernels_at_the_widths_between_the_tested_ones(hidden, training):
    check_kernels(kernel_case("above", hidden, training), label("above", hidden, training))


@MODES
def test_kernels_past_the_cap_of_partial_rows(training):
    c = kernel_case("cap", 128, training)
    assert -(-c["ei"].shape[1] // 8) == 1038 and -(-c["batch"].size // 8) == 1025
    check_kernels(c, label("cap", 128, training))


def test_statistics_past_the_cap_under_cancellation():
    check_kernels(kernel_case("cap", 128, True, OFFSET_SIGMAS), "cap, offset %g sigma" % OFFSET_SIGMAS)


def test_the_smallest_batch():
    c = kernel_case("pair", 64, True)
    assert c["ei"].tolist() == [[0, 1], [1, 0]] and c["batch"].size == 2
    check_kernels(c, label("pair", 64, True))


# ------------------------------------------------------------------------------------------------ views
def padded(x, ld, col0):
    """x as the columns [col0, col0 + width) of a NaN matrix with ``ld`` columns."""
    t = torch.full((x.shape[0], ld), NAN, dtype=torch.float32, device=DEV)
    t[:, col0:col0 + x.shape[1]] = x
    return t[:, col0:col0 + x.shape[1]]


def run_direct(c, g, views):
    """The five entries one after the other through ``ops``; ``views``: Q, h, h' and the cotangent go in as column
    views of wider NaN matrices.  Device tensors by name."""
    H = c["H"]
    P, Q, h, cot, gamma, beta = (torch.tensor(c[n], device=DEV) for n in ("P", "Q", "h", "cot", "gamma", "beta"))
    if views:
        Q, h, cot = padded(Q, 2 * H + 8, 4), padded(h, H + 8, 4), padded(cot, H + 16, 12)
    rm, rv = torch.tensor(c["rm0"], device=DEV), torch.tensor(c["rv0"], device=DEV)
    res = {}
    if c["training"]:
        mean, invstd = ops.cg_stats(g, P, Q, R.EPS, R.MOMENTUM, rm, rv)
        res.update(mean=mean, invstd=invstd, rm=rm, rv=rv)
    else:
        mean, invstd = rm, torch.rsqrt(rv + R.EPS)
    norm = dict(mean=mean, invstd=invstd, gamma=gamma, beta=beta)
    out = ops.cg_conv_fwd(g, P, Q, h, **norm)
    hnew = padded(out, H + 12, 8) if views else out
    sums = ops.cg_bwd_stats(g, P, Q, hnew, cot, **norm)
    dP, dQ, dh = ops.cg_bwd_edges(g, P, Q, hnew, cot, sums if c["training"] else None, **norm)
    ops.cg_bwd_src(g, dQ, dP)
    torch.cuda.synchronize()
    res.update(out=out, sums=sums, dP=dP, dQ=dQ, dh=dh)
    return res


@MODES
@pytest.mark.parametrize("hidden", [60, 128])
def test_leading_dimensions_of_q_h_hnew_and_the_cotangent(hidden, training):
    c = kernel_case("edge", hidden, training)
    g = ops.GnGraph(c["ei"], c["batch"], c["G"], False, DEV)
    dense, views = run_direct(c, g, False), run_direct(c, g, True)
    assert sorted(dense) == sorted(views)
    for k in dense:
        assert not bool(torch.isnan(dense[k]).any()), k
        assert torch.equal(dense[k], views[k]), "%s: %s differs" % (label("edge", hidden, training), k)


# ------------------------------------------------------------------------------------------------ tiling
def tiled_graph(c, copies, device):
    """``copies`` times the one graph of a case in one batch."""
    N, E = c["batch"].size, c["ei"].shape[1]
    ei = np.concatenate([c["ei"] + k * N for k in range(copies)], axis=1)
    assert ei.shape == (2, copies * E)
    return ops.GnGraph(ei, np.repeat(np.arange(copies), N), copies, False, device)


def run_fn(c, g, copies):
    """``CgConvFn`` forward and backward on a case tiled ``copies`` times; device tensors by name."""
    P, Q, h = (torch.tensor(c[n], device=DEV).repeat(copies, 1).requires_grad_(True) for n in ("P", "Q", "h"))
    gamma, beta = (torch.tensor(c[n], device=DEV) for n in ("gamma", "beta"))
    mean, invstd = torch.tensor(c["rm0"], device=DEV), torch.rsqrt(torch.tensor(c["rv0"], device=DEV) + R.EPS)
    out = ops.CgConvFn.apply(P, Q, h, mean, invstd, gamma, beta, g, False)
    out.backward(torch.tensor(c["cot"], device=DEV).repeat(copies, 1))
    torch.cuda.synchronize()
    return dict(out=out.detach(), dh=h.grad, dP=P.grad, dQ=Q.grad)


def test_tiling_past_the_grid_cap():
    """25 copies of a graph in one batch, eval mode: every copy's rows have the single copy's bits."""
    c = kernel_case("tile", 128, False)
    check_kernels(c, label("tile", 128, False))  # the base is itself under the float64 bar
    g1 = ops.GnGraph(c["ei"], c["batch"], c["G"], False, DEV)
    one = run_fn(c, g1, 1)
    g = tiled_graph(c, TILE_COPIES, DEV)
    assert (g.n_nodes, g.n_edges) == (68275, 102475) and -(-g.n_nodes // 8) == 8535 and -(-g.n_nodes // 4) == 17069
    many = run_fn(c, g, TILE_COPIES)
    for k in one:
        rows = many[k].reshape(TILE_COPIES, *one[k].shape)
        for i in range(TILE_COPIES):
            assert torch.equal(rows[i], one[k]), "%s of copy %d" % (k, i)
