"""The slot tables of the molecule-window kernels (csrc/gather_lds.hip: WinSlots, fill_slot_table), for what only
they can get wrong.  While a window is staged, thread = slot looks the slot's degree up once and writes
``degree | first neighbour entry << 4`` into one of two 128-entry tables in the head of the workgroup's LDS; the compute
phase reads it per piece.  Batches whose largest ordinary window has more than 128 atoms, and oversized windows, keep
the per-piece search.

  * the capacity edge: a largest window of exactly 128 atoms (tables) and of 129 (search), same molecules otherwise;
  * the largest value an entry holds: windows of 128 atoms of degree 10 (first entry 1 270, degree 10);
  * all eleven degrees inside every window, the first and last slot of every degree block looked at by itself, and a
    batch that stops at degree 2, where the entries of absent degrees are never formed;
  * both tables used again and again: more than three windows per workgroup, for the two ops with third tiles beside
    the tables;
  * the LDS plan: what runs windowed, fused or two-stage and what is refused or falls back is what the restatement of
    tests/edge_refs.py says -- the tables take no LDS of their own.

Everything is compared BIT FOR BIT with the restatements of tests/edge_refs.py, each operation twice in a row (the
two sweep directions), outputs inside sentinel guards -- the helpers of tests/test_gpu_win_ops.py.
"""
import functools

import numpy as np
import pytest
import torch

from deepchem_amd.utils.synthetic import concat_packed
from tests import edge_refs as R
from tests import test_gpu_win_ops as W
from tests.test_gpu_win_ops import BF16, Guarded, dev, same

pytestmark = pytest.mark.gpu

TAB_SLOTS = 128  # kTabSlots of csrc/gather_lds.hip


# ------------------------------------------------------------------------------------------------ molecules
def _complete(n):
    return [[j for j in range(n) if j != i] for i in range(n)]


def _circulant(n, reach):
    """n atoms on a ring, each bonded to the ``reach`` nearest on either side: 2 * reach neighbours each."""
    return [sorted({(i + k) % n for k in range(-reach, reach + 1) if k}) for i in range(n)]


def _caterpillar():
    """47 atoms with every degree from 1 to 10: a spine of atoms of degree 2 .. 10 in a row, leaves making up the
    rest."""
    spine = list(range(9))  # atom k has degree k + 2
    adj = [[] for _ in spine]
    for a, b in zip(spine, spine[1:]):
        adj[a].append(b)
        adj[b].append(a)
    for k in spine:
        while len(adj[k]) < k + 2:
            adj.append([k])
            adj[k].append(len(adj) - 1)
    return adj


_K11 = _complete(11)
_DEG10_18 = _circulant(18, 5)
# the first window: 4 * 11 + 40 + 4 * 5 + 4 + tail atoms, degrees 0, 1, 2, 4 and 10
_HEAD = [_K11] * 4 + [W._chain(40)] + [W._STAR] * 4 + [W._LONE] * 4


def _filled(tail):
    """A first window of 108 + tail atoms, then ordinary molecules of up to 40 atoms with degrees 0 .. 10."""
    return lambda: concat_packed([W._from_adjs(_HEAD + [W._chain(tail)]), W._ONE_EACH()])


# name -> (molecules, window cap or None for the default of 96)
BATCHES = {
    "at_capacity": (_filled(20), TAB_SLOTS),
    "above_capacity": (_filled(21), TAB_SLOTS + 1),
    # four windows of 10 * 11 + 18 = 128 atoms of degree 10 each, and a fifth of 22
    "degree10_full": (lambda: W._from_adjs(([_K11] * 10 + [_DEG10_18]) * 4 + [_K11] * 2), TAB_SLOTS),
    # a lone atom and a caterpillar, 48 atoms: two of each per window of 96
    "all_degrees": (lambda: W._from_adjs([W._LONE, _caterpillar()] * 7), None),
    "to_degree2": (lambda: W._from_adjs(([W._LONE] * 2 + [W._chain(n) for n in (2, 3, 30, 7, 50)]) * 3), None),
}


class Batch(W.Batch):
    """The batch object of tests/test_gpu_win_ops.py (inputs, references, planted arg bytes) over the batches above."""

    def __init__(self, name):
        from deepchem_amd.data.collate import collate_to_device
        make, cap = BATCHES[name]
        self.name = name
        self.dev = collate_to_device(make(), None, W.DEV, **({} if cap is None else {"win_cap": cap}))
        self.g = g = self.dev.graph
        self.c = c = g.c
        self.n = g.n_atoms
        assert c.n_win > 1 and c.n_win_big == 0 and g.ensure_rev_pos()
        self.hg = R.HostGraph(g.deg_counts, g.col_idx.cpu().numpy())
        self.meta = meta = g.win_meta.cpu().numpy().reshape(c.n_win, 24)
        self.big_rows = np.zeros(0, np.int64)
        self.norm_rows = np.arange(self.n)
        present = [d for d, k in enumerate(g.deg_counts) if k]
        atoms, entries = meta[:, 21], meta[:, 23]
        # ---- what the batch is here for
        if name == "at_capacity":
            assert c.win_alloc == TAB_SLOTS == atoms[0] and present[0] == 0 and present[-1] == 10
        elif name == "above_capacity":
            assert c.win_alloc == TAB_SLOTS + 1 == atoms[0] and present[0] == 0 and present[-1] == 10
        elif name == "degree10_full":
            assert c.win_alloc == TAB_SLOTS and present == [10] and (atoms[:4] == TAB_SLOTS).all()
            assert entries.max() == 10 * TAB_SLOTS  # the last slot's first entry: 1 270
        elif name == "all_degrees":
            sizes = np.diff(np.concatenate([np.zeros((c.n_win, 1), np.int64), meta[:, 11:22]], 1), axis=1)
            assert present == list(range(11)) and (sizes > 0).all()  # every degree in every window
        elif name == "to_degree2":
            assert present == [0, 1, 2]

    def block_edge_rows(self):
        """The global rows of the first and the last slot of every degree block of every window."""
        rows = []
        for m in self.meta:
            base, start = m[:11], np.concatenate([[0], m[11:22]])
            for d in range(11):
                if start[d + 1] > start[d]:
                    rows += [base[d] + start[d], base[d] + start[d + 1] - 1]
        return np.unique(np.array(rows, np.int64))


@functools.lru_cache(maxsize=None)
def batch(name):
    return Batch(name)


def fits(b, width, aux=0, third_tiles=0, bf16=False):
    return R.win_fits(b.c, width * (2 if bf16 else 4), aux, third_tiles)


# ------------------------------------------------------------------------------------------------ one op, twice
def run_sum(b, width, accumulate=False):
    from deepchem_amd import ops
    x, old = b.rows("normal", width), b.rows("old", width)
    ref = R.neigh_sum(b.hg, x, old=old if accumulate else None)
    xd = dev(x)
    for _ in range(2):
        out = Guarded(b.n, width)
        if accumulate:
            out.rows.copy_(dev(old))
        ops.gather_sum(b.g, xd, out.rows, accumulate=accumulate)
        assert same(out, ref)
    return out, ref


def run_sum_fh(b, width, ldo):
    from deepchem_amd import ops
    x = b.rows("normal", width)
    pad = np.zeros((b.n, ldo - width), np.float32)
    ref_s = np.concatenate([R.bf16_round(R.neigh_sum(b.hg, x)), pad], 1)
    ref_x = np.concatenate([R.bf16_round(x), pad], 1)
    xd = dev(x)
    for _ in range(2):
        s, xc = Guarded(b.n, ldo, BF16, pad=0), Guarded(b.n, ldo, BF16, pad=0)
        ops.win_sum_fh(b.g, xd, ldo, s.rows, xc.rows)
        assert same(s, ref_s) and same(xc, ref_x)


def run_pool(b, width, bn):
    """MaxOp<bn> with arg bytes, on the exact rows (planted winners and ties, exact BatchNorm vectors)."""
    from deepchem_amd import ops
    x = dev(b.rows("exact", width))
    sc, sh = (dev(b.vec("sc_e", width)), dev(b.vec("sh_e", width))) if bn else (None, None)
    ref = b.pool_ref(width, bn)
    for _ in range(2):
        out, arg = Guarded(b.n, width), Guarded(b.n, width, torch.uint8)
        ops.gather_max(b.g, x, sc, sh, out=out.rows, arg=arg.rows)
        assert same(out, ref[0]) and same(arg, ref[1])
    return arg, ref[1]


def run_pool_bwd(b, width):
    from deepchem_amd import ops
    arg, g = b.planted_arg(width), b.rows("ds", width)
    ref = R.pool_bwd(b.hg, g, arg)
    argd, gd = dev(arg), dev(g)
    for _ in range(2):
        out = Guarded(b.n, width)
        ops.gather_max_bwd(b.g, gd, argd, out=out.rows)
        assert same(out, ref)
    return out, ref


def run_sum_h(b, width):
    from deepchem_amd import ops
    x = b.rows("normal", width, bf16=True)
    ref = R.bf16_round(R.neigh_sum(b.hg, x))
    xd = dev(x, bf16=True)
    for _ in range(2):
        out = Guarded(b.n, width, BF16)
        ops.win_sum_h(b.g, xd, out.rows, accumulate=False)
        assert same(out, ref)


def run_pool_bwd_h(b, width):
    from deepchem_amd import ops
    arg, g = b.planted_arg(width), b.rows("ds", width, bf16=True)
    ref = R.bf16_round(R.pool_bwd(b.hg, g, arg))
    argd, gd = dev(arg), dev(g, bf16=True)
    for _ in range(2):
        out = Guarded(b.n, width, BF16)
        ops.win_max_bwd_h(b.g, gd, argd, None, None, out=out.rows)
        assert same(out, ref)


def run_pool_then_sum(b, width, bn):
    """MaxSumOp where the restatement finds room for its scratch tile, the two window kernels elsewhere."""
    W._pool_then_sum(b, width, bn, fused=width in (64, 128) and fits(b, width, 0, third_tiles=1))


def run_two_stage(b, width, bf16=False):
    """SumAccMaxBwdOp where the restatement finds room for its two third tiles, refused elsewhere."""
    took = W._two_stage(b, width, bf16)
    assert took == ("ran" if fits(b, width, 8 if bf16 else 4, third_tiles=2, bf16=bf16) else "refused")
    return took


# ------------------------------------------------------------------------------------------------ the capacity edge
EDGE_OPS = {
    "SumOp-lpr16": lambda b: run_sum(b, 64),
    "SumOp_acc-lpr16": lambda b: run_sum(b, 64, accumulate=True),
    "SumOpFH-lpr16": lambda b: run_sum_fh(b, 64, 72),
    "MaxOp-lpr16": lambda b: run_pool(b, 64, False),
    "MaxOp_bn-lpr16": lambda b: run_pool(b, 64, True),
    "MaxSumOp-lpr16": lambda b: run_pool_then_sum(b, 64, False),
    "MaxSumOp_bn-lpr16": lambda b: run_pool_then_sum(b, 64, True),
    "MaxBwdOp-lpr16": lambda b: run_pool_bwd(b, 64),
    "SumAccMaxBwdOp-lpr16": lambda b: run_two_stage(b, 64),
    "SumOpFH-lpr19": lambda b: run_sum_fh(b, 76, 80),
    "MaxOp_bn-lpr32": lambda b: run_pool(b, 128, True),
    "SumOpH-lpr8": lambda b: run_sum_h(b, 64),
    "MaxBwdOpH-lpr8": lambda b: run_pool_bwd_h(b, 64),
}


@pytest.mark.parametrize("name", ["at_capacity", "above_capacity"])
@pytest.mark.parametrize("op", list(EDGE_OPS))
def test_capacity_edge(op, name):
    b = batch(name)
    # every launch here runs over the windows: the widest single-stage plan with arg bytes at 64 columns, the rows
    # of 76 and 128 columns without
    assert fits(b, 64, 4) and fits(b, 64, 8, bf16=True) and fits(b, 76) and fits(b, 128)
    EDGE_OPS[op](b)


# ------------------------------------------------------------------------------------------------ largest entry
@pytest.mark.parametrize("op", ["SumOp", "MaxOp_bn", "MaxBwdOp", "SumAccMaxBwdOp"])
def test_largest_entry(op):
    b = batch("degree10_full")
    assert fits(b, 64, 4, third_tiles=2)
    if op == "SumOp":
        run_sum(b, 64)
    elif op == "MaxOp_bn":
        arg, _ = run_pool(b, 64, True)
        assert sorted(torch.unique(arg.rows).tolist()) == list(range(11))  # every neighbour position wins somewhere
    elif op == "MaxBwdOp":
        run_pool_bwd(b, 64)
    else:
        assert run_two_stage(b, 64) == "ran"


# ------------------------------------------------------------------------------------------------ block boundaries
@pytest.mark.parametrize("name", ["all_degrees", "to_degree2"])
@pytest.mark.parametrize("op", ["SumOp", "MaxOp", "MaxBwdOp", "SumAccMaxBwdOp"])
def test_degree_blocks(op, name):
    b = batch(name)
    assert fits(b, 64, 4, third_tiles=2)
    edge = torch.from_numpy(b.block_edge_rows()).to(W.DEV)
    assert len(edge) > len([k for k in b.g.deg_counts if k])

    def at_block_edges(out, ref):  # (part of the whole comparison above; by itself for the message)
        assert torch.equal(W.bits(out.rows[edge]), W.bits(dev(ref)[edge])), "first or last slot of a degree block"

    if op == "SumOp":
        at_block_edges(*run_sum(b, 64))
    elif op == "MaxOp":
        at_block_edges(*run_pool(b, 64, False))
    elif op == "MaxBwdOp":
        at_block_edges(*run_pool_bwd(b, 64))
    else:
        assert run_two_stage(b, 64) == "ran"


# ------------------------------------------------------------------------------------------------ tables reused
@pytest.mark.parametrize("op", ["MaxSumOp", "SumAccMaxBwdOp"])
def test_tables_reused(op):
    """More than 3 * 256 * 8 windows (the ``many`` batch of tests/test_gpu_win_ops.py, cap 16): some workgroup walks
    more than three, so both tables are written a second time beside the third tiles."""
    b = W.batch("many")
    assert b.c.n_win > W.MANY_WINDOWS and b.c.win_alloc <= 16
    if op == "MaxSumOp":
        assert fits(b, 64, 0, third_tiles=1)
        W._pool_then_sum(b, 64, True, fused=True)
    else:
        assert run_two_stage(b, 64) == "ran"


# ------------------------------------------------------------------------------------------------ the LDS plan
# 128 float columns: a window atom costs 2 * 512 + 512 bytes with a scratch tile (105 atoms fit) and
# 2 * (512 + 128) + 2 * 512 with two third tiles (70 atoms); 64 columns: 768 and 1 152 (209 and 140 atoms)
@pytest.mark.parametrize("name", ["at_capacity", "above_capacity", "degree10_full", "all_degrees"])
def test_plan_is_the_restatement(name):
    b = batch(name)
    wide = b.c.win_alloc >= TAB_SLOTS
    assert R.win_plan_bytes(b.c, 256, 4, 2)[1] == b.c.win_alloc  # (no oversized windows: the buffers do not grow)
    # what fits by the restatement, the head of 2 368 bytes included: with the tables as without
    assert fits(b, 64, 0, third_tiles=1) and fits(b, 64, 4, third_tiles=2)
    assert fits(b, 128, 0, third_tiles=1) == (not wide)
    assert fits(b, 128, 4, third_tiles=2) == (b.c.win_alloc <= 70)
    run_pool_then_sum(b, 64, True)  # fused
    run_pool_then_sum(b, 128, True)  # fused, or the two window kernels
    assert run_two_stage(b, 64) == "ran"
    assert run_two_stage(b, 128) == ("ran" if b.c.win_alloc <= 70 else "refused")
