"""The graph-network kernels (csrc/megnet.hip) at the edges their launches depend on: every leading dimension with its
own value and column-block views on the input and on the output side, the segment kernels called directly in all four
modes on views with spare columns, and the second turn of the grid-stride loops (more than 8192 workgroups of rows,
more than 2 097 152 (range, column) pairs).

Bar: ``bar`` of tests/test_gpu_mat.py, unchanged; the ratios are printed.  A call that differs from another only in
leading dimensions or column offsets must give the same bits, and every spare column must keep its NaN.
"""
import ctypes

import numpy as np
import pytest
import torch

from deepchem_amd import _lib, ops
from tests import megnet_refs as R
from tests.test_gpu_mat import bar
from tests.test_gpu_megnet import batch_graphs, kernel_case, run_native
from tests.yardstick import restatement_threads

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H = ops.GN_WIDTH
NAN = float("nan")
MODES = [True, False]


def label(undirected):
    return "undirected" if undirected else "directed"


def nan_buffer(rows, ld):
    return torch.full((rows, ld), NAN, dtype=torch.float32, device=DEV)


def padded(x, ld, col0=0):
    """x as the columns [col0, col0 + width) of a NaN matrix with ``ld`` columns: (the view, the matrix)."""
    x = torch.as_tensor(x, device=DEV)
    t = nan_buffer(x.shape[0], ld)
    t[:, col0:col0 + x.shape[1]] = x
    return t[:, col0:col0 + x.shape[1]], t


def only_written(t, blocks, name):
    """The columns of ``blocks`` hold numbers, every other column still NaN."""
    keep = torch.ones(t.shape[1], dtype=torch.bool, device=t.device)
    for lo, hi in blocks:
        keep[lo:hi] = False
        assert not bool(torch.isnan(t[:, lo:hi]).any()), "%s: NaN inside columns [%d, %d)" % (name, lo, hi)
    assert bool(torch.isnan(t[:, keep]).all()), "%s: a spare column was written" % name


def halves(res):
    """dP = [dPs | dPd] as two tensors: ten result tensors of the two passes."""
    out = {}
    for k, v in res.items():
        if k.endswith("_dP"):
            out[k + "s"], out[k + "d"] = v[:, :H], v[:, H:]
        else:
            out[k] = v
    return out


def check_bar(c, got, what):
    worst = max(bar(got[k], c["f64"][k], c["f32"][k], "%s %s" % (what, k)) for k in c["f64"])
    print("worst ratio %s: %.2f" % (what, worst))


def same_bits(a, b, what):
    assert sorted(a) == sorted(b)
    for k in a:
        assert a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), "%s: %s differs" % (what, k)


# ------------------------------------------------------------------------------------------------ leading dimensions
@pytest.mark.parametrize("undirected", MODES)
def test_input_leading_dimensions_through_ops(undirected):
    """Ps / Pd as the column blocks [0, 32) and [36, 68) of one (N, 72) matrix, Q with ld 36, R 40, dHs 44, dMh 48."""
    c = kernel_case("edge", undirected)
    want, g = run_native(c)
    P72 = nan_buffer(c["P"].shape[0], 72)
    P72[:, :H] = torch.as_tensor(c["P"][:, :H], device=DEV)
    P72[:, 36:36 + H] = torch.as_tensor(c["P"][:, H:], device=DEV)
    ps, pd = P72[:, :H], P72[:, 36:36 + H]
    (Q, Qm), (Rr, Rm), (dHs, dHm), (dMh, dMm) = (padded(c[n], ld) for n, ld in (("Q", 36), ("R", 40), ("dHs", 44), ("dMh", 48)))
    assert [ops._ld(t) for t in (ps, pd, Q, Rr, dHs, dMh)] == [72, 72, 36, 40, 44, 48]
    res = {"edge_out": ops.gn_edge_fwd(g, ps, pd, Q, Rr), "node_out": ops.gn_node_fwd(g, ps, pd, Q, Rr)}
    res["edge_dP"], res["edge_dR"] = ops.gn_edge_bwd(g, dHs)
    res["edge_dQ"] = dHs
    res["node_dP"], res["node_dQ"], res["node_dR"] = ops.gn_node_bwd(g, dMh)
    torch.cuda.synchronize()
    only_written(P72, [(0, H), (36, 36 + H)], "P")
    for t, name in ((Qm, "Q"), (Rm, "R"), (dHm, "dHs"), (dMm, "dMh")):
        only_written(t, [(0, H)], name)
    got = {k: v.cpu().numpy() for k, v in res.items()}
    check_bar(c, got, "input lds %s" % label(undirected))
    assert len(halves(got)) == 10
    same_bits(halves(got), halves(want), "input leading dimensions against contiguous rows")


def call_with_output_lds(g, c):
    """The four C entries the way ``ops`` calls them, with ldh 36, ldm 40, ldq 44, ldr 48 and dPs / dPd as the column
    blocks [4, 36) and [40, 72) of one (N, 76) matrix; every buffer NaN before the call."""
    P, Q, Rr, dHs, dMh = (torch.tensor(c[n], device=DEV) for n in ("P", "Q", "R", "dHs", "dMh"))
    N, E, G = g.n_nodes, g.n_edges, g.n_graphs
    ref, p, st = ctypes.byref(g.ref), ops._ptr, ops._stream()
    ps, pd = P[:, :H], P[:, H:]
    hs, mh = nan_buffer(E, 36), nan_buffer(N, 40)
    _lib.call("gcmi_gn_edge_fwd", ref, p(ps), p(pd), 2 * H, p(Q), H, p(Rr), H, p(hs), 36, st)
    _lib.call("gcmi_gn_node_fwd", ref, p(ps), p(pd), 2 * H, p(Q), H, p(Rr), H, p(mh), 40, st)
    e_dp, e_dr = nan_buffer(N, 76), nan_buffer(G, 48)
    _lib.call("gcmi_gn_edge_bwd", ref, p(dHs), H, p(e_dp[:, 4:4 + H]), p(e_dp[:, 40:40 + H]), 76, p(e_dr), 48, st)
    n_dp, n_dr, n_dq = nan_buffer(N, 76), nan_buffer(G, 48), nan_buffer(E, 44)
    _lib.call("gcmi_gn_node_bwd", ref, p(dMh), H, p(n_dq), 44, p(n_dp[:, 4:4 + H]), p(n_dp[:, 40:40 + H]), 76, p(n_dr), 48, st)
    torch.cuda.synchronize()
    for t, name in ((hs, "Hs"), (mh, "Mh"), (e_dr, "edge dR"), (n_dr, "node dR"), (n_dq, "node dQ")):
        only_written(t, [(0, H)], name)
    for t, name in ((e_dp, "edge dPs | dPd"), (n_dp, "node dPs | dPd")):
        only_written(t, [(4, 4 + H), (40, 40 + H)], name)
    res = {"edge_out": hs[:, :H], "node_out": mh[:, :H], "edge_dR": e_dr[:, :H], "node_dR": n_dr[:, :H], "node_dQ": n_dq[:, :H],
           "edge_dPs": e_dp[:, 4:4 + H], "edge_dPd": e_dp[:, 40:40 + H], "node_dPs": n_dp[:, 4:4 + H],
           "node_dPd": n_dp[:, 40:40 + H]}
    return {k: v.cpu().numpy() for k, v in res.items()}


@pytest.mark.parametrize("undirected", MODES)
def test_output_leading_dimensions_through_the_c_entries(undirected):
    c = kernel_case("edge", undirected)
    want, g = run_native(c)
    want = halves(want)
    del want["edge_dQ"]  # (dHs itself: no output)
    same_bits(call_with_output_lds(g, c), want, "output leading dimensions against ops")


# ------------------------------------------------------------------------------------------------ segment kernels
def segment_sums(x, ptr, mean, dtype):
    """Rows of x summed (or averaged) per range, one row after the other, in ``dtype``."""
    counts = np.diff(ptr)
    out = np.zeros((counts.size, x.shape[1]), dtype)
    np.add.at(out, np.repeat(np.arange(counts.size), counts), x.astype(dtype))
    if mean:
        out = out / np.maximum(counts, 1).astype(dtype)[:, None]
    return out


def check_segments(ptr, width, mean, seed, what):
    """``ops.gn_seg_reduce`` and ``ops.gn_seg_spread`` on the ranges of ``ptr`` (int64, from 0 to the row count), their
    operands views with three spare NaN columns."""
    counts = np.diff(ptr)
    n_seg, n_rows = counts.size, int(ptr[-1])
    rng = np.random.RandomState(seed)
    d_ptr = torch.as_tensor(ptr, dtype=torch.int32, device=DEV)
    x = rng.normal(0, 1, (n_rows, width)).astype(np.float32)
    xv, xm = padded(x, width + 3)
    got = ops.gn_seg_reduce(xv, d_ptr, mean).cpu().numpy()
    only_written(xm, [(0, width)], "x")
    ratio = bar(got, segment_sums(x, ptr, mean, np.float64), segment_sums(x, ptr, mean, np.float32), what + " reduce")
    assert got.shape == (n_seg, width) and not got[counts == 0].any()  # an empty range: a zero row
    u = rng.normal(0, 1, (n_seg, width)).astype(np.float32)
    uv, um = padded(u, width + 3)
    rows = ops.gn_seg_spread(uv, d_ptr, n_rows, mean).cpu().numpy()
    only_written(um, [(0, width)], "u")
    owner = np.repeat(np.arange(n_seg), counts)
    want = u[owner] / counts[owner].astype(np.float32)[:, None] if mean else u[owner]
    assert want.dtype == np.float32 and rows.shape == want.shape and np.array_equal(rows, want), what + " spread"
    return ratio


@pytest.mark.parametrize("width", [1, 33])
@pytest.mark.parametrize("mean", [False, True])
def test_segment_kernels_directly(mean, width):
    _, ei, _, _, batch = R.pack(batch_graphs("edge"))
    ptr = R.lists(ei, batch, int(batch.max()) + 1, True)["edge_ptr"]
    counts = np.diff(ptr)
    assert counts[0] == 0 and counts[-1] == 0 and (counts[1:-1] == 0).any() and ptr[-1] == ei.shape[1]
    print("ratio", check_segments(ptr, width, mean, 10 * width + mean, "edge_ptr %s w%d" % ("mean" if mean else "sum", width)))


# ------------------------------------------------------------------------------------------------ second turn of the grid
def ring_case(undirected):
    """``kernel_case`` on the rings of ``R.WRAP_RING_SIZES``, its lists in closed form (``R.ring_lists``: the walk of
    ``R.lists`` over every node in Python is too slow at this size)."""
    ei, batch = R.ring_batch(R.WRAP_RING_SIZES)
    G, N, E = len(R.WRAP_RING_SIZES), batch.size, ei.shape[1]
    rng = np.random.default_rng(9)  # (draws float32 directly: a third of the time at this size)
    c = {"ei": ei, "batch": batch, "G": G, "undirected": undirected, "lists": R.ring_lists(R.WRAP_RING_SIZES, undirected)}
    for n, shape in (("P", (N, 2 * H)), ("Q", (E, H)), ("R", (G, H)), ("dHs", (E, H)), ("dMh", (N, H))):
        c[n] = rng.standard_normal(shape, dtype=np.float32)
    L = {k: torch.as_tensor(v) for k, v in c["lists"].items()}
    tei, tb = torch.as_tensor(ei), torch.as_tensor(batch)
    for dtype, tag in ((torch.float64, "f64"), (torch.float32, "f32")):
        with restatement_threads(dtype, 1):
            res = {}
            for which, cot in (("edge", "dHs"), ("node", "dMh")):
                P, Q, Rr = (torch.tensor(c[n], dtype=dtype, requires_grad=True) for n in ("P", "Q", "R"))
                if which == "edge":
                    out = R.edge_pass(P[:, :H], P[:, H:], Q, Rr, tei, tb, undirected)
                else:
                    out = R.node_pass(P[:, :H], P[:, H:], Q, Rr, L, tb)
                (out * torch.tensor(c[cot], dtype=dtype)).sum().backward()
                res.update({which + "_out": out.detach().numpy(), which + "_dP": P.grad.numpy(), which + "_dQ": Q.grad.numpy(),
                            which + "_dR": Rr.grad.numpy()})
            c[tag] = res
    return c


@pytest.mark.parametrize("undirected", MODES)
def test_edge_and_node_passes_past_one_turn_of_the_grid(undirected):
    """8192 * 32 + 33 nodes and edges: the last 33 rows of every launch belong to a workgroup's second turn."""
    c = ring_case(undirected)
    assert c["batch"].size == c["ei"].shape[1] == R.GN_MAX_BLOCKS * ops.GN_ROWS_PER_WG + 33
    got, g = run_native(c)
    assert all(np.array_equal(g.host[k], v) for k, v in c["lists"].items())
    check_bar(c, got, "wrap %s" % label(undirected))


def test_segment_kernels_past_one_turn_of_the_grid():
    ptr = R.wrap_segment_ptr()
    assert (ptr.size - 1) * R.WRAP_SEG_WIDTH > R.GN_MAX_BLOCKS * R.GN_SEG_THREADS
    print("ratio", check_segments(ptr, R.WRAP_SEG_WIDTH, True, 3, "65 537 ranges mean w33"))
