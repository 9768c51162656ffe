"""The case builders of tests/test_gpu_mat_edges.py and tests/test_gpu_megnet_edges.py do what they claim, and the
accuracy bar of the MAT kernels (``bar`` of tests/test_gpu_mat.py) is attainable at the tiny shapes: a float32 emulation
of the kernels' own order of operations, in numpy, is held to it.  No GPU.
"""
import numpy as np
import pytest

from deepchem_amd import ops
from tests import mat_refs as M
from tests import megnet_refs as G
from tests.test_gpu_mat import bar


# ------------------------------------------------------------------------------------------------ MAT builders
def test_n_max_batches_have_the_stated_largest_molecule():
    assert sorted(M.N_MAX_BATCHES) == [1, 2, 3, 63, 64, 65, 127]
    for n_max, n_list in M.N_MAX_BATCHES.items():
        assert max(n_list) == n_max and min(n_list) >= 1
        if n_max <= 3:
            assert len(n_list) >= 48
        waves = (n_max + 63) // 64
        assert waves == (1 if n_max <= 64 else 2)
    assert M.N_MAX_BATCHES[64] == [63, 1, 64] and M.N_MAX_BATCHES[65] == [65, 2]
    assert M.MAT_CAP == ops.MAT_MAX_ATOMS


def test_instantiation_of_every_head_width():
    assert [M.nv_of(d) for d in (4, 8, 12, 16, 20, 32, 36, 60, 64)] == [1, 2, 4, 4, 8, 8, 16, 16, 16]


@pytest.mark.parametrize("nv", M.MAT_NV)
def test_lds_boundary_pairs_straddle_64_kib(nv):
    for bwd in (False, True):
        below, above = M.lds_boundary(nv, bwd)
        assert (below, above) == M.LDS_TABLE[nv][bwd]
        assert M.lds_bytes(nv, below, bwd) <= 65536 < M.lds_bytes(nv, above, bwd)
        print(nv, bwd, below, M.lds_bytes(nv, below, bwd), above, M.lds_bytes(nv, above, bwd))
    # the figure in the header comment of csrc/mat.hip: the cap at d_k = 64, backward
    assert M.lds_bytes(16, 128, True) == 136192


def test_bias_batch_is_not_a_multiple_of_the_rows_of_a_workgroup():
    n_list, adj, dist = M.bias_edge_case()
    assert n_list == M.BIAS_EDGE_SIZES and sum(n_list) == 333 and sum(n_list) % 4 != 0
    assert adj.size == dist.size == sum(n * n for n in n_list)
    assert n_list[0] == n_list[-1] == 1 and {63, 64, 65, 127} <= set(n_list)


def test_reordered_case_moves_whole_molecules():
    c = M.attention_edge_case([1, 2, 3], 1, 4)
    r, rows = M.reorder_case(c, [2, 1, 0])
    assert r["n_list"] == [3, 2, 1] and list(rows) == [3, 4, 5, 1, 2, 0]
    assert np.array_equal(r["q"], c["q"][rows]) and np.array_equal(r["bias"][:9], c["bias"][5:]) and r["bias"][-1] == c["bias"][0]


# ------------------------------------------------------------------------------------------------ the bar at tiny shapes
@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("d_k", [16, 64])
@pytest.mark.parametrize("n_max", [1, 2, 3, 64, 65])
def test_float32_in_the_kernel_order_meets_the_bar(n_max, d_k, shared):
    c = M.attention_edge_case(M.N_MAX_BATCHES[n_max], 3, d_k, shared=shared)
    got = M.attention_emulation(c)
    assert sorted(got) == sorted(c["f64"])
    worst = max(bar(got[name], c["f64"][name], c["f32"][name], "n_max %d d_k %d %s" % (n_max, d_k, name)) for name in got)
    print("worst ratio", worst)
    if n_max == 1 and not shared:  # the softmax of one score is 1, so dS = 0
        assert not got["dQ"].any() and not got["dK"].any() and got["dV"].any()


def test_compensated_row_sums_where_plain_running_sums_missed_the_bar():
    """tests/test_gpu_mat_edges.py::test_both_sides_of_64_kib_of_lds[4] missed the bar on the GPU with plain running sums
    for the softmax denominator and delta (n_max 110, one shared tensor, dQ: ratio 4.12; this emulation with plain sums:
    4.31, and 7.10 with five such molecules).  One row with a near one-hot softmax carries all of it: dS_ii cancels, and
    the rounding of l and delta over 110 atoms returns multiplied by |dP_ii|.  With both sums compensated, as the kernels
    have them now, the emulation stays near ratio 1."""
    c = M.attention_edge_case([5, 110, 1], 3, 16, shared=True)
    plain = M.attention_emulation(c, compensated=False)["dQ"]
    e32 = np.abs(c["f32"]["dQ"] - c["f64"]["dQ"]).max()
    print("plain running sums: ratio %.2f" % (np.abs(plain - c["f64"]["dQ"]).max() / e32))
    got = M.attention_emulation(c)
    print("compensated: worst ratio %.2f" % max(bar(got[name], c["f64"][name], c["f32"][name], "compensated " + name)
                                                 for name in got))


def test_k_equal_v_case_keeps_two_leaves():
    c = M.attention_edge_case([3, 1, 2], 3, 16, kv_same=True)
    assert c["k"] is c["v"] and c["k"] is not c["q"]
    assert sorted(c["f64"]) == ["O", "dK", "dQ", "dV"] and not np.array_equal(c["f64"]["dK"], c["f64"]["dV"])


# ------------------------------------------------------------------------------------------------ MEGNet builders
@pytest.mark.parametrize("undirected", [True, False])
def test_ring_lists_are_the_lists_of_the_ring_batch(undirected):
    sizes = [3, 5, 1, 2, 33]
    ei, batch = G.ring_batch(sizes)
    assert ei.shape == (2, 44) and batch.size == 44 and np.array_equal(ei[0], np.arange(44))
    want = G.lists(ei, batch, len(sizes), undirected)
    got = G.ring_lists(sizes, undirected)
    assert sorted(got) == sorted(want)
    for k in want:
        assert np.array_equal(got[k], want[k]), k


def test_wrap_cases_exceed_one_turn_of_the_grid():
    n = sum(G.WRAP_RING_SIZES)
    assert n == G.GN_MAX_BLOCKS * ops.GN_ROWS_PER_WG + 33
    assert -(-n // ops.GN_ROWS_PER_WG) > G.GN_MAX_BLOCKS  # nodes and edges alike: a ring has as many edges
    assert len(G.WRAP_RING_SIZES) > 1 and min(G.WRAP_RING_SIZES) == 1
    ptr = G.wrap_segment_ptr()
    counts = np.diff(ptr)
    assert counts.size == G.WRAP_SEG_RANGES and set(counts) == {1, 2} and ptr[0] == 0
    assert G.WRAP_SEG_RANGES * G.WRAP_SEG_WIDTH > G.GN_MAX_BLOCKS * G.GN_SEG_THREADS == 2097152


def test_edge_batch_has_empty_ranges_at_both_ends_and_in_the_middle():
    _, ei, _, _, batch = G.pack(G.edge_case_graphs(np.random.RandomState(17)))
    counts = np.diff(G.lists(ei, batch, int(batch.max()) + 1, True)["edge_ptr"])
    assert counts[0] == 0 and counts[-1] == 0 and (counts[1:-1] == 0).any() and counts.max() == 300
