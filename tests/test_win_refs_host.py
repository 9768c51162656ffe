"""The restatements of the molecule-window operations in tests/edge_refs.py (neigh_sum, pool_max, pool_bwd, the
two-stage backward, bf16 rounding), checked without a device: against the oracle's sum_neigh / graph_pool, against
autograd in float64, and the exactness conditions tests/test_gpu_win_ops.py leans on for its bit-for-bit comparisons
of the folded BatchNorm."""
import numpy as np
import pytest
import torch

from deepchem_amd.feat.mol_graphs import collate_packed
from deepchem_amd.utils.synthetic import concat_packed, single_atom_and_edge_cases, synthetic_molecules
from oracle import graphconv_oracle as O
from tests import edge_refs as R

F = 12


@pytest.fixture(scope="module")
def batch():
    """(HostGraph, the oracle's layer inputs without the features): degrees 0..4, 6 and 10, a multi-atom mix."""
    packed = concat_packed([synthetic_molecules(40, seed=3, max_atoms=40), single_atom_and_edge_cases(75, 1)])
    multi = collate_packed(packed)
    tables = multi.get_deg_adjacency_lists()[1:]
    counts = [int(c) for c in np.asarray(multi.deg_slice)[:, 1]]
    col = np.concatenate([np.asarray(t).reshape(-1) for t in tables])
    hg = R.HostGraph(counts, col)
    assert counts[0] > 0 and counts[10] > 0 and hg.n_atoms == packed.n_atoms
    tail = [torch.from_numpy(np.asarray(multi.deg_slice)), torch.from_numpy(multi.membership)] + \
        [torch.from_numpy(np.asarray(t)).long() for t in tables]
    return hg, tail


def _pool_t(x, tail):
    return O.graph_pool([x] + tail)


def _sum_t(x, tail):
    n0 = int(tail[0][0, 1])
    return torch.cat([torch.zeros((n0, x.shape[1]), dtype=x.dtype)] + O.sum_neigh(x, tail[2:]), 0)


def test_reverse_positions_name_the_atom_itself(batch):
    hg, _ = batch
    deg_of = np.repeat(np.arange(len(hg.deg_counts)), hg.deg_counts)
    for d, rows, nb, rev in hg.degree_blocks():
        for r, k in enumerate(rows):
            for j in range(d):
                i = int(nb[r, j])
                di = int(deg_of[i])
                assert hg.nb[di][i - hg.row0[di], rev[r, j]] == k


def test_neigh_sum_equals_the_oracle(batch):
    hg, tail = batch
    rng = np.random.RandomState(0)
    x = rng.standard_normal((hg.n_atoms, F))
    old = rng.standard_normal((hg.n_atoms, F))
    ref = _sum_t(torch.from_numpy(x), tail).numpy()
    assert np.abs(R.neigh_sum(hg, x) - ref).max() < 1e-13
    assert np.abs(R.neigh_sum(hg, x, old=old) - (ref + old)).max() < 1e-13
    xi = rng.randint(-3, 4, size=(hg.n_atoms, F)).astype(np.float32)  # exact in any order
    got = R.neigh_sum(hg, xi)
    assert got.dtype == np.float32 and np.array_equal(got, _sum_t(torch.from_numpy(xi).double(), tail).numpy())
    assert not got[:hg.deg_counts[0]].any()  # lone atoms: zero


def test_pool_max_equals_the_oracle_and_names_its_winner(batch):
    hg, tail = batch
    rng = np.random.RandomState(1)
    for x in (rng.standard_normal((hg.n_atoms, F)), R.exact_rows(rng, hg.n_atoms, F)):
        val, arg = R.pool_max(hg, x)
        assert np.array_equal(val, _pool_t(torch.from_numpy(x), tail).numpy())
        for d, rows, nb, _ in hg.degree_blocks():
            cand = np.concatenate([x[rows][:, None], x[nb]], 1) if d else x[rows][:, None]
            assert np.array_equal(arg[rows], cand.argmax(1))  # numpy: the FIRST maximum
    _, arg = R.pool_max(hg, R.plant_winners(hg, x))
    star = hg.row0[10]
    assert arg[star].tolist() == [c % 11 for c in range(F)]  # every candidate position wins somewhere


def test_pool_bwd_and_two_stage_equal_autograd(batch):
    hg, tail = batch
    rng = np.random.RandomState(2)
    x = rng.standard_normal((hg.n_atoms, F))  # no ties: the gradient has one route
    ds, dxs = rng.standard_normal(x.shape), rng.standard_normal(x.shape)
    _, arg = R.pool_max(hg, x)
    xt = torch.from_numpy(x).requires_grad_(True)
    pooled = _pool_t(xt, tail)
    (pooled * torch.from_numpy(dxs)).sum().backward()
    assert np.abs(R.pool_bwd(hg, dxs, arg) - xt.grad.numpy()).max() < 1e-13
    xt = torch.from_numpy(x).requires_grad_(True)
    pooled = _pool_t(xt, tail)
    ((_sum_t(pooled, tail) * torch.from_numpy(ds)).sum() + (pooled * torch.from_numpy(dxs)).sum()).backward()
    dx, dy = R.two_stage_bwd(hg, ds, dxs, arg)
    assert np.abs(dx - (R.neigh_sum(hg, ds) + dxs)).max() < 1e-13
    assert np.abs(dy - xt.grad.numpy()).max() < 1e-12


def test_bf16_round_is_torchs_rounding():
    rng = np.random.RandomState(3)
    x = np.concatenate([rng.standard_normal(4096).astype(np.float32) * 37.0,
                        # ties: exactly half way between two bf16 numbers, even and odd below
                        np.array([1.00390625, 1.01171875, -1.00390625, 257.0, 259.0, 0.0, -0.0], np.float32)])
    want = torch.from_numpy(x).to(torch.bfloat16).float().numpy()
    assert np.array_equal(R.bf16_round(x).view(np.uint32), want.view(np.uint32))
    assert np.array_equal(R.bf16_round(want), want)  # idempotent


def test_exact_inputs_evaluate_alike_in_float32_float64_and_bf16(batch):
    """What lets the GPU tests demand bit equality through the folded BatchNorm (fmaf in the kernel, a rounded
    product and a rounded sum here) and through bf16 stores."""
    hg, _ = batch
    rng = np.random.RandomState(4)
    x = R.exact_rows(rng, hg.n_atoms, 64)
    sc, sh = R.exact_bn(rng, 64)
    assert (sc > 0).any() and (sc < 0).any() and (sh > 0).any() and (sh < 0).any()
    assert set(np.unique(np.abs(sc))) <= {0.5, 1.0, 1.5, 2.0} and np.abs(sh * 4).max() <= 8
    y32 = x * sc + sh
    assert y32.dtype == np.float32
    y64 = x.astype(np.float64) * sc.astype(np.float64) + sh.astype(np.float64)
    assert np.array_equal(y32.astype(np.float64), y64)
    assert np.array_equal(R.bf16_round(y32), y32) and np.array_equal(R.bf16_round(x), x)
    assert np.array_equal(y64 * 8, np.rint(y64 * 8)) and np.abs(y64).max() <= 3.5
    # pooled values are candidates, hence exact; the arg bytes agree whatever the precision of the comparison
    v32, a32 = R.pool_max(hg, y32)
    v64, a64 = R.pool_max(hg, y64)
    assert np.array_equal(v32.astype(np.float64), v64) and np.array_equal(a32, a64)
    # sums of at most 11 rows of quarters (ten neighbours and the self part): below 2^8 quarter-units, exact in bf16
    s = R.neigh_sum(hg, x, old=x)
    assert np.abs(s * 4).max() < 256 and np.array_equal(R.bf16_round(s), s)
    assert np.array_equal(s.astype(np.float64), R.neigh_sum(hg, x.astype(np.float64), old=x.astype(np.float64)))
    # ... and so is the two-stage backward over them, with and without the bf16 roundings
    dx, dy = R.two_stage_bwd(hg, x, x, a32)
    dxh, dyh = R.two_stage_bwd(hg, x, x, a32, bf16=True)
    assert np.array_equal(dx, dxh)
    # (dy sums up to 11 values of up to 33 quarters: beyond 8 bits, so dy itself is rounded -- once)
    assert np.array_equal(dyh, R.bf16_round(dy))


def test_ulp_and_window_rows():
    assert R.ulp(1.0) == 2.0 ** -23 and R.ulp(1.5, bf16=True) == 2.0 ** -7 and R.ulp(-4.0) == 2.0 ** -21
    meta = [10, 19, 0, 0, 0, 0, 0, 0, 0, 0, 0] + [2, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5] + [0, 6]
    # two rows of degree 0 from row 10, three of degree 1: slots 2..4 -> rows 21..23
    assert R.window_rows(meta).tolist() == [10, 11, 21, 22, 23]
