"""The restatements tests/test_gpu_direct_ops.py compares the direct gather kernels (csrc/gather.hip) with, checked
without a device: the two scatter forms against float64 autograd of the oracle's sum_neigh / graph_pool (on a symmetric
batch and on one with a bond listed from one end only) and against the gather forms, HostGraph.rev against a brute-force
pairing on multi-bonds and self-loops, the launch geometry on hand-made counts, the builder against the project's host
collation, every named batch against the property it exists for, and the exactness the atomic comparisons lean on."""
import itertools

import numpy as np
import pytest
import torch

from deepchem_amd.feat.mol_graphs import collate_packed
from oracle import graphconv_oracle as O
from tests import edge_refs as R

F = 12


def _tables(name):
    adjs, max_deg = R.direct_batch_adjs(name)
    return R.collate_adjs(adjs, max_deg)


def _oracle_tail(counts, col, membership):
    """The oracle's layer inputs behind the features: deg_slice, membership, the tables of the degrees 1..max."""
    starts = np.concatenate([[0], np.cumsum(counts)[:-1]])
    deg_slice = torch.from_numpy(np.stack([starts, np.asarray(counts)], 1).astype(np.int64))
    nt = R.NeighbourTables(counts, col)
    return [deg_slice, torch.from_numpy(membership)] + [torch.from_numpy(nt.nb[d]).long() for d in range(1, len(counts))]


def _sum_t(x, tail):
    n0 = int(tail[0][0, 1])
    return torch.cat([torch.zeros((n0, x.shape[1]), dtype=x.dtype)] + O.sum_neigh(x, tail[2:]), 0)


@pytest.mark.parametrize("name", ["mixed", "multi", "one_sided"])
def test_scatter_forms_equal_float64_autograd_of_the_oracle(name):
    counts, col, mem = _tables(name)
    nt, tail = R.NeighbourTables(counts, col), _oracle_tail(counts, col, mem)
    rng = np.random.RandomState(1)
    x, ds = rng.standard_normal((nt.n_atoms, F)), rng.standard_normal((nt.n_atoms, F))  # no ties: one route
    xt = torch.from_numpy(x).requires_grad_(True)
    (_sum_t(xt, tail) * torch.from_numpy(ds)).sum().backward()
    assert np.abs(R.scatter_ref(nt, ds) - xt.grad.numpy()).max() < 1e-13
    val, arg = R.pool_max(nt, x)
    xt = torch.from_numpy(x).requires_grad_(True)
    pooled = O.graph_pool([xt] + tail)
    assert np.array_equal(val, pooled.detach().numpy())
    (pooled * torch.from_numpy(ds)).sum().backward()
    assert np.abs(R.pool_bwd_scatter(nt, ds, arg) - xt.grad.numpy()).max() < 1e-13
    # onto a start value
    assert np.abs(R.scatter_ref(nt, ds, dx0=x) - (R.scatter_ref(nt, ds) + x)).max() < 1e-13


@pytest.mark.parametrize("name", [n for n in R.DIRECT_BATCHES if n != "one_sided"])
def test_scatter_forms_equal_the_gather_forms_on_symmetric_batches(name):
    counts, col, _ = _tables(name)
    hg = R.HostGraph(counts, col)
    rng = np.random.RandomState(2)
    x = R.plant_winners(hg, R.exact_rows(rng, hg.n_atoms, F))
    g = R.exact_rows(rng, hg.n_atoms, F)
    _, arg = R.pool_max(hg, x)
    assert np.array_equal(R.scatter_ref(hg, g), R.neigh_sum(hg, g))
    assert np.array_equal(R.pool_bwd_scatter(hg, g, arg), R.pool_bwd(hg, g, arg))
    assert R.scatter_ref(hg, g).dtype == np.float32
    # the sibling class gives what HostGraph gives
    nt = R.NeighbourTables(counts, col)
    assert np.array_equal(R.neigh_sum(nt, g), R.neigh_sum(hg, g)) and np.array_equal(R.pool_max(nt, x)[1], arg)


def test_one_sided_adjacency_is_refused_by_hostgraph_and_taken_by_the_sibling():
    counts, col, _ = _tables("one_sided")
    with pytest.raises(AssertionError):
        R.HostGraph(counts, col)
    nt = R.NeighbourTables(counts, col)
    g = np.ones((nt.n_atoms, 1), np.float32)
    # the transpose counts the times a row is LISTED, the gather the entries it lists: one row each differs
    listed, lists = R.scatter_ref(nt, g)[:, 0], R.neigh_sum(nt, g)[:, 0]
    assert (listed != lists).sum() == 2 and listed.sum() == lists.sum() == len(col)


def _brute_force_rev(nt):
    deg_of = np.repeat(np.arange(len(nt.deg_counts)), nt.deg_counts)
    lists = [nt.nb[deg_of[k]][k - nt.row0[deg_of[k]]].tolist() for k in range(nt.n_atoms)]
    out = []
    for k, lk in enumerate(lists):
        for j, i in enumerate(lk):
            n = lk[:j].count(i)  # this is the (n + 1)-th entry of k that names i ...
            where = [p for p, v in enumerate(lists[i]) if v == k]
            out.append(where[n])  # ... paired with the (n + 1)-th entry of i that names k
    return np.array(out, np.int64)


@pytest.mark.parametrize("name", ["multi", "mixed", "high_only"])
def test_reverse_positions_equal_a_brute_force_pairing(name):
    counts, col, _ = _tables(name)
    hg = R.HostGraph(counts, col)
    rev = np.concatenate([r.reshape(-1) for r in hg.rev])
    want = _brute_force_rev(R.NeighbourTables(counts, col))
    assert np.array_equal(rev, want)
    if name == "multi":
        # the pairing is not "the first entry that names me": a first-match table differs on the multi-bonds
        nt = R.NeighbourTables(counts, col)
        deg_of = np.repeat(np.arange(len(counts)), counts)
        first = []
        for d, rows, nb, _ in nt.degree_blocks():
            for r, k in enumerate(rows):
                for i in nb[r]:
                    first.append(nt.nb[deg_of[i]][i - nt.row0[deg_of[i]]].tolist().index(k))
        assert (np.array(first) != want).sum() >= 2 * 2 + 2 * 45  # the second bonds, and the loops beyond the first
        # a null atom's j-th loop is paired with itself
        for d in range(1, 11):
            loops = (hg.nb[d] == hg.rows(d)[:, None]).all(1)
            assert loops.sum() == 2 and np.array_equal(hg.rev[d][loops], np.tile(np.arange(d), (2, 1)))


def test_direct_tiles_on_hand_made_counts():
    S = R.DIRECT_SLOTS
    assert S == 1024
    # empty blocks in front, in the middle and at the end; lpr 16: 64 rows fill a workgroup
    counts = [0, 64, 0, 0, 65, 1, 0, 200, 0, 0, 0]
    t = R.direct_tiles(counts, 16, False)
    assert t[0] == (0, 0, 0) and t[1] == (0, 1, S) and t[2] == t[3] == (1, 0, 0)
    assert t[4] == (1, 2, 16) and t[5] == (3, 1, 16) and t[6] == (4, 0, 0) and t[7] == (4, 4, 200 * 16 - 3 * S)
    assert t[8] == t[9] == t[10] == (8, 0, 0)
    # skip_deg0 with and without degree-0 rows
    assert R.direct_tiles(counts, 16, True) == t
    counts[0] = 130
    t0, ts = R.direct_tiles(counts, 16, False), R.direct_tiles(counts, 16, True)
    assert t0[0] == (0, 3, 2 * 16) and t0[1] == (3, 1, S) and ts[0] == (0, 0, 0) and ts[1:] == t[1:]
    # one row wider than a workgroup, and a single lane slot
    assert R.direct_tiles([0, 1], 1025, False)[1] == (0, 2, 1) and R.direct_tiles([1], 1, False) == [(0, 1, 1)]
    assert R.direct_tiles([5], 16, True) == [(0, 0, 0)]
    # the workgroup -> degree lookup of block_degree: count the starts at or below b among the degrees >= 1
    for cs, skip in itertools.product(([0, 64, 0, 0, 65], [7, 0, 0, 3], [0, 0, 129]), (False, True)):
        tt = R.direct_tiles(cs, 16, skip)
        total = sum(n for _, n, _ in tt)
        starts = [tt[d][0] if d < len(cs) else total for d in range(12)]
        for d, (first, n, _) in enumerate(tt):
            for b in range(first, first + n):
                assert sum(b >= starts[k] for k in range(1, 11)) == d


def test_direct_vec():
    assert R.direct_vec(4096, 64, 64) == 4 and R.direct_vec(4096, 72, 64) == 4
    assert R.direct_vec(4100, 72, 64) == 1  # the pointer 4 bytes off
    assert R.direct_vec(4096, 66, 64) == 1  # ld
    assert R.direct_vec(4096, 76, 75) == 1 and R.direct_vec(4096, 4, 2) == 1  # width


@pytest.mark.parametrize("name", R.DIRECT_BATCHES)
def test_named_batches_are_what_they_are_named_for_and_collate_like_the_project(name):
    adjs, max_deg = R.direct_batch_adjs(name)
    counts, col, mem = R.collate_adjs(adjs, max_deg)
    assert R.direct_batch_check(name, counts, col)
    multi = collate_packed(R.packed_from_adjs(adjs), max_deg=max_deg)
    assert counts == [int(c) for c in np.asarray(multi.deg_slice)[:, 1]] and len(counts) == max_deg + 1
    tables = [np.asarray(t).reshape(-1) for t in multi.get_deg_adjacency_lists()[1:]]
    assert np.array_equal(col, np.concatenate(tables + [np.zeros(0, np.int32)]))
    assert np.array_equal(mem, multi.membership) and col.dtype == np.int32 and mem.dtype == np.int32


def test_a_wrong_batch_fails_its_check():
    counts, col, _ = _tables("tile_exact")
    with pytest.raises(AssertionError):
        R.direct_batch_check("tile_plus", counts, col)
    counts, col, _ = _tables("mixed")
    with pytest.raises(AssertionError):
        R.direct_batch_check("one_sided", counts, col)
    with pytest.raises(AssertionError):
        R.direct_batch_check("high_only", *_tables("gappy")[:2])


@pytest.mark.parametrize("name", ["mixed", "multi", "one_sided"])
def test_quarter_valued_terms_add_exactly_in_any_order(name):
    """Up to 11 terms k / 4, |k| <= 3 (a start value and ten neighbours, or the self part and ten routes): every partial
    sum in any order is a multiple of 1/4 below 2^24 / 4 -- a float32 number.  The atomic kernels are compared bit for
    bit on such rows."""
    counts, col, _ = _tables(name)
    nt = R.NeighbourTables(counts, col)
    rng = np.random.RandomState(3)
    g, old = R.exact_rows(rng, nt.n_atoms, F), R.exact_rows(rng, nt.n_atoms, F)
    _, arg = R.pool_max(nt, R.plant_winners(nt, R.exact_rows(rng, nt.n_atoms, F)))
    S = R.scatter_ref(nt, np.abs(g).astype(np.float64), dx0=np.abs(old).astype(np.float64))
    assert R.is_multiple(g, 0.25) and R.is_multiple(old, 0.25) and R.any_order_exact(S, 0.25) and S.max() <= 11 * 0.75
    assert R.any_order_exact(R.pool_bwd_scatter(nt, np.abs(g).astype(np.float64), arg), 0.25)
    # hence float32 == float64, and a shuffled order of the same terms gives the same bits
    s32 = R.scatter_ref(nt, g, dx0=old)
    assert np.array_equal(s32.astype(np.float64), R.scatter_ref(nt, g.astype(np.float64), dx0=old.astype(np.float64)))
    p32 = R.pool_bwd_scatter(nt, g, arg)
    assert np.array_equal(p32.astype(np.float64), R.pool_bwd_scatter(nt, g.astype(np.float64), arg))
    dx = old.copy()
    entries = [(int(i), int(k)) for d, rows, nb, _ in nt.degree_blocks() for k, row in zip(rows, nb) for i in row]
    for e in rng.permutation(len(entries)):
        i, k = entries[e]
        dx[i] = dx[i] + g[k]
    assert dx.dtype == np.float32 and np.array_equal(dx, s32)
