"""The molecule-window kernels (csrc/gather_lds.hip), one operation at a time, against the plain restatements of
tests/edge_refs.py (checked on the CPU by tests/test_win_refs_host.py): every operation at every row width its
launch switch has, over batches that make the window walker do what a handful of windows never asks of it -- three
and more windows per workgroup, oversized windows (one, more than 64, nothing else), empty degree blocks, windows
without atoms and without neighbour entries.

The kernels add in float32 in neighbour-table order and so do the restatements: results are compared BIT FOR BIT.
The folded BatchNorm is an fmaf in the kernel; it is compared bit for bit on inputs where every product and sum is
exact, and within one ulp of the output type against float64 on standard-normal inputs (the kernel rounds the exact
value once, a float64 evaluation rounded to the output type twice).

Every operation runs twice in a row: consecutive windowed launches walk the ordinary windows in opposite directions
(next_sweep_direction), so the two runs are one of each.  Outputs are pre-filled with a sentinel and carry guard
columns and a guard row that must stay as they were.  Case ids: operation - pieces per row - batch - both directions.
"""
import functools

import numpy as np
import pytest
import torch

from deepchem_amd.utils.synthetic import PackedMols, concat_packed, single_atom_and_edge_cases, synthetic_molecules
from tests import edge_refs as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
BF16 = torch.bfloat16

# launch_lpr gives the ordinary windows min(n_norm, 256 * per_cu) workgroups, per_cu <= 8: above 3 * 256 * 8 windows
# some workgroup walks more than three, so both buffers, all three ring slots and the third tiles are used again
MANY_WINDOWS = 3 * 256 * 8
W32 = (64, 76, 128)  # float rows: 16, 19, 32 pieces
W16 = (64, 80, 128)  # bf16 rows: 8, 10, 16 pieces
WMAX = 128
SENTINEL = -777.0
ARG_SENTINEL = 0xEE


# ------------------------------------------------------------------------------------------------ batches
def _from_adjs(adjs):
    sizes = np.array([len(a) for a in adjs], np.int64)
    atom_ptr = np.zeros(len(adjs) + 1, np.int64)
    np.cumsum(sizes, out=atom_ptr[1:])
    deg = np.array([len(nb) for a in adjs for nb in a], np.int64)
    adj_ptr = np.zeros(deg.shape[0] + 1, np.int64)
    np.cumsum(deg, out=adj_ptr[1:])
    adj_idx = np.array([j for a in adjs for nb in a for j in nb], np.int32)
    return PackedMols(np.zeros((int(atom_ptr[-1]), 4), np.float32), atom_ptr, adj_ptr, adj_idx)


def _topology(p):  # (the atom features play no part here)
    return PackedMols(np.zeros((p.n_atoms, 4), np.float32), p.atom_ptr, p.adj_ptr, p.adj_idx)


def _syn(*a, **k):
    return _topology(synthetic_molecules(*a, **k))


def _chain(n):
    return [[j for j in (i - 1, i + 1) if 0 <= j < n] for i in range(n)]


_STAR = [[1, 2, 3, 4], [0], [0], [0], [0]]
_LONE = [[]]
_EDGE = lambda: _topology(single_atom_and_edge_cases(75, 1))  # noqa: E731  (degrees 0, 1, 2, 6 and 10)
_ONE_EACH = lambda: concat_packed([_syn(40, seed=3, max_atoms=40), _EDGE()])  # noqa: E731
# 80 + 80 ordinary molecules around one of 100..132 atoms (60 in all leave at most 61 oversized windows at a cap of
# 16, and the strided loop over oversized windows needs more than 64)
_BIG_MIXED = lambda: concat_packed([_syn(80, seed=5, max_atoms=40),  # noqa: E731
                                    _syn(1, seed=6, mean_atoms=118, max_atoms=132, min_atoms=100),
                                    _syn(80, seed=7, max_atoms=40), _EDGE()])

# name -> (molecules, window cap or None for the default)
BATCHES = {
    "one_each": (_ONE_EACH, None),
    "many": (lambda: concat_packed([_syn(10000, seed=4, mean_atoms=10, max_atoms=16), _EDGE()]), 16),
    "big_mixed": (_BIG_MIXED, None),
    "big_mixed_cap16": (_BIG_MIXED, 16),
    "only_big": (lambda: _syn(5, seed=8, mean_atoms=30, max_atoms=40, min_atoms=20, single_atom_frac=0.0), 16),
    "low_degree": (lambda: _from_adjs([_chain(n) for n in (2, 3, 5, 8, 13, 21, 2, 40, 7)]), None),
    "gappy": (lambda: _from_adjs(([_LONE] * 3 + [_STAR] * 4) * 5), None),
    "lone": (lambda: _from_adjs([_LONE] * 300), 1),
    "empty_first": (lambda: concat_packed([_from_adjs([[], _chain(120)]), _syn(20, seed=9, max_atoms=40), _EDGE()]),
                    None),
    # the LDS limits: the same molecules as one_each under other caps
    "cap48": (_ONE_EACH, 48),
    "cap96": (_ONE_EACH, 96),
    "cap128": (_ONE_EACH, 128),
}
MAIN = ["one_each", "many", "big_mixed", "big_mixed_cap16", "only_big", "low_degree", "gappy", "lone", "empty_first"]


class Batch:
    def __init__(self, name):
        from deepchem_amd.data.collate import collate_to_device
        make, cap = BATCHES[name]
        packed = make()
        self.name = name
        self.dev = collate_to_device(packed, None, DEV, **({} if cap is None else {"win_cap": cap}))
        self.g = g = self.dev.graph
        self.c = c = g.c
        self.n = g.n_atoms
        assert c.n_win > 0 and g.ensure_rev_pos()
        self.hg = R.HostGraph(g.deg_counts, g.col_idx.cpu().numpy())
        self.meta = g.win_meta.cpu().numpy().reshape(c.n_win, 24)
        n_norm = c.n_win - c.n_win_big
        self.big_rows = np.concatenate([R.window_rows(m) for m in self.meta[n_norm:]] + [np.zeros(0, np.int64)])
        self.norm_rows = np.setdiff1d(np.arange(self.n), self.big_rows)
        counts = g.deg_counts
        present = [d for d, k in enumerate(counts) if k]
        # ---- what the batch is here for
        if name == "one_each":
            assert counts[0] > 0 and counts[10] > 0 and c.n_win_big == 0
        elif name == "many":
            assert c.n_win > MANY_WINDOWS and c.n_win_big == 0 and counts[10] > 0
            assert (self.meta[:, 23] == 0).any()  # windows without neighbour entries
        elif name == "big_mixed":
            assert c.n_win_big == 1 and n_norm > 1
        elif name == "big_mixed_cap16":
            # more oversized windows than the 64 workgroups they get, and two ordinary buffers that must grow to hold one
            assert c.n_win_big > 64 and c.win_alloc_big > 2 * c.win_alloc and n_norm > 1
            assert R.win_plan_bytes(c, 256, 0)[1] > c.win_alloc
        elif name == "only_big":
            assert c.n_win == c.n_win_big and c.win_alloc == 0
        elif name == "low_degree":
            assert present == [1, 2]
        elif name == "gappy":
            assert present == [0, 1, 4]
        elif name == "lone":
            assert g.n_edges == 0 and c.n_win == self.n == 300 and c.win_alloc == 1
        elif name == "empty_first":
            assert (self.meta[:n_norm, 21] == 0).any() and c.n_win_big == 1  # an ordinary window without atoms
        # every single-stage launch of this module runs over the windows (the fp32 entry points would otherwise take
        # the direct kernels without a word); the widest rows with arg bytes are the largest plan.  cap128 is there
        # for a plan that does NOT fit.
        if name != "cap128":
            assert R.win_fits(c, 4 * WMAX, 4) and R.win_fits(c, 2 * WMAX, 8)
        assert len(np.unique(np.concatenate([self.big_rows, self.norm_rows]))) == self.n

    @functools.lru_cache(maxsize=None)
    def inputs(self):
        """Host inputs of WMAX columns (a narrower case takes the first columns): ``normal`` rows, ``exact`` rows with
        planted winners (ties everywhere, every arg byte up to the highest degree), three gradient-like matrices."""
        rng = np.random.RandomState(len(self.name) * 1000 + self.n % 997)
        d = {k: rng.standard_normal((self.n, WMAX)).astype(np.float32) for k in ("normal", "ds", "dxs", "old")}
        d["exact"] = R.plant_winners(self.hg, R.exact_rows(rng, self.n, WMAX))
        d["sc_e"], d["sh_e"] = R.exact_bn(rng, WMAX)
        d["sc_n"] = rng.standard_normal(WMAX).astype(np.float32)
        d["sh_n"] = rng.standard_normal(WMAX).astype(np.float32)
        return d

    def rows(self, key, width, bf16=False):
        a = np.ascontiguousarray(self.inputs()[key][:, :width])
        return R.bf16_round(a) if bf16 else a

    def vec(self, key, width):
        return np.ascontiguousarray(self.inputs()[key][:width])

    @functools.lru_cache(maxsize=None)
    def pool_ref(self, width, bn):
        """(values, arg bytes) of the GraphPool of the exact rows, ``bn``: through the exact BatchNorm vectors --
        computed once for the float, the bf16 and the fused forms."""
        y = self.rows("exact", width)
        if bn:
            y = y * self.vec("sc_e", width) + self.vec("sh_e", width)
        assert y.dtype == np.float32
        return R.pool_max(self.hg, y)

    def planted_arg(self, width):
        """The arg bytes of the GraphPool of the exact rows: the restatement's, which the forward tests prove the
        kernels give too.  Every value 0 .. highest degree occurs."""
        arg = self.pool_ref(width, False)[1]
        assert sorted(np.unique(arg).tolist()) == list(range(self.hg.max_present + 1))
        return arg


@functools.lru_cache(maxsize=None)
def batch(name):
    return Batch(name)


# ------------------------------------------------------------------------------------------------ helpers
def dev(a, bf16=False):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t.to(BF16) if bf16 else t  # (exact: bf16 cases hand over bf16_round'ed values)


class Guarded:
    """(n, width) output rows inside a sentinel-filled (n + 1, width + pad) buffer."""

    def __init__(self, n, width, dtype=torch.float32, pad=None):
        pad = (0 if dtype == torch.uint8 else 8 if dtype == BF16 else 4) if pad is None else pad
        fill = ARG_SENTINEL if dtype == torch.uint8 else SENTINEL
        self.buf = torch.full((n + 1, width + pad), fill, dtype=dtype, device=DEV)
        self.fill = self.buf[n, 0].clone()
        self.n, self.width = n, width
        self.rows = self.buf[:n, :width] if pad else self.buf[:n]

    def guards_intact(self):
        return bool((self.buf[self.n:] == self.fill).all()) and bool((self.buf[:self.n, self.width:] == self.fill).all())

    def untouched(self):
        return bool((self.buf == self.fill).all())


def bits(t):
    t = t.contiguous()
    return t.view({torch.float32: torch.int32, BF16: torch.int16, torch.uint8: torch.uint8}[t.dtype])


def same(out, ref):
    """``out`` (device; Guarded or tensor) equals the host array ``ref`` bit for bit, guards intact."""
    if isinstance(out, Guarded):
        assert out.guards_intact(), "a guard row or guard column was written"
        out = out.rows
    want = dev(ref, bf16=out.dtype == BF16)
    assert want.dtype == out.dtype and want.shape == out.shape
    return torch.equal(bits(out), bits(want))


def lpr(width, bf16=False):
    return width // (8 if bf16 else 4)


def ident(op, width, name, bf16=False):
    return "%s-lpr%d-%s-fwd+rev" % (op, lpr(width, bf16), name)


def cases(op, widths, bf16=False, names=MAIN):
    return [pytest.param(name, w, id=ident(op, w, name, bf16)) for name in names for w in widths]


def other_direction(b):
    """One more windowed launch: the sweep direction of the next one flips.  For rounds that take an even number of
    turns themselves (gather_max_sum takes two for its one pass: launch_lpr)."""
    from deepchem_amd import ops
    small = batch("one_each")
    ops.gather_sum(small.g, dev(small.rows("normal", 64)))


def refused(fn):
    """fn() fails with GCMI_ERR_UNSUPPORTED (-3) and an error text."""
    from deepchem_amd import _lib
    with pytest.raises(_lib.GcmiError) as e:
        fn()
    assert "status -3" in str(e.value) and len(str(e.value)) > 40
    return True


def bn_float64(b, x, width):
    return x.astype(np.float64) * b.vec("sc_n", width).astype(np.float64) + b.vec("sh_n", width).astype(np.float64)


def assert_pool_within_one_ulp(b, y64, out, arg, bf16):
    """Values within one ulp of the output type of max_j y64_j; the candidate the arg byte names within the same ulp
    of that maximum (the kernel compares float32 roundings of y, so it may name a candidate half an ulp below)."""
    assert out.guards_intact() and arg.guards_intact()
    ref, _ = R.pool_max(b.hg, y64)
    got = out.rows.float().cpu().numpy().astype(np.float64)
    tol = R.ulp(np.maximum(np.abs(ref), np.abs(got)), bf16=bf16)
    err = np.abs(got - ref) / tol
    print("pool value error in ulps of the output type: max %.3f" % err.max())
    assert err.max() <= 1.0
    named = R.candidate_value(b.hg, y64, arg.rows.cpu().numpy())
    gap = (ref - named) / tol
    print("named candidate below the maximum, ulps: max %.3f" % gap.max())
    assert gap.min() >= 0.0 and gap.max() <= 1.0


# ------------------------------------------------------------------------------------------------ neighbour sums
@pytest.mark.parametrize("accumulate", [False, True], ids=["set", "accumulate"])
@pytest.mark.parametrize("name,width", cases("SumOp", W32))
def test_sum_f32(name, width, accumulate):
    from deepchem_amd import ops
    b = batch(name)
    x, old = b.rows("normal", width), b.rows("old", width)
    ref = R.neigh_sum(b.hg, x, old=old if accumulate else None)
    xd = dev(x)
    for _ in range(2):
        out = Guarded(b.n, width)
        if accumulate:
            out.rows.copy_(dev(old))
        ops.gather_sum(b.g, xd, out.rows, accumulate=accumulate)
        assert same(out, ref)


@pytest.mark.parametrize("accumulate", [False, True], ids=["SumOpH", "SumAccOpH"])
@pytest.mark.parametrize("name,width", cases("sum_h", W16, bf16=True))
def test_sum_bf16(name, width, accumulate):
    from deepchem_amd import ops
    b = batch(name)
    x, old = b.rows("normal", width, bf16=True), b.rows("old", width, bf16=True)
    ref = R.bf16_round(R.neigh_sum(b.hg, x, old=old if accumulate else None))
    xd = dev(x, bf16=True)
    for _ in range(2):
        out = Guarded(b.n, width, BF16)
        if accumulate:
            out.rows.copy_(dev(old, bf16=True))
        ops.win_sum_h(b.g, xd, out.rows, accumulate=accumulate)
        assert same(out, ref)


FH = [(76, 80), (64, 72), (128, 128)]  # the model's shape; two groups of four zeroed columns; none


@pytest.mark.parametrize("name,width,ldo", [pytest.param(n, w, o, id="SumOpFH-lpr%d-to%d-%s-fwd+rev" % (w // 4, o, n))
                                            for n in MAIN for w, o in FH])
def test_sum_f32_to_bf16(name, width, ldo):
    from deepchem_amd import ops
    b = batch(name)
    x = b.rows("normal", width)
    pad = np.zeros((b.n, ldo - width), np.float32)
    ref_s = np.concatenate([R.bf16_round(R.neigh_sum(b.hg, x)), pad], 1)
    ref_x = np.concatenate([R.bf16_round(x), pad], 1)
    xin = Guarded(b.n, width)  # (input rows with a pitch of their own)
    xin.rows.copy_(dev(x))
    for _ in range(2):
        s, xc = Guarded(b.n, ldo, BF16, pad=0), Guarded(b.n, ldo, BF16, pad=0)  # (ldo is pitch and end of the zeros)
        ops.win_sum_fh(b.g, xin.rows, ldo, s.rows, xc.rows)
        assert same(s, ref_s) and same(xc, ref_x)


@pytest.mark.parametrize("ldo", [76, 78, 84], ids=["ldo76-not8", "ldo78-pad-not4", "ldo84-not8"])
def test_sum_f32_to_bf16_refuses_bad_ldo(ldo):
    from deepchem_amd import ops
    b = batch("one_each")
    x = dev(b.rows("normal", 76))
    s, xc = Guarded(b.n, ldo, BF16, pad=0), Guarded(b.n, ldo, BF16, pad=0)
    assert refused(lambda: ops.win_sum_fh(b.g, x, ldo, s.rows, xc.rows))
    torch.cuda.synchronize()
    assert s.untouched() and xc.untouched()


# ------------------------------------------------------------------------------------------------ GraphPool forward
def _pool_case(b, width, variant, bf16):
    """(input rows, scale, shift, reference (values, arg) or None for the one-ulp comparison)"""
    if variant == "plain":
        return b.rows("exact", width), None, None, b.pool_ref(width, False)
    if variant == "bn_exact":
        return b.rows("exact", width), b.vec("sc_e", width), b.vec("sh_e", width), b.pool_ref(width, True)
    x = b.rows("normal", width, bf16=bf16)
    return x, b.vec("sc_n", width), b.vec("sh_n", width), None


POOL_VARIANTS = ["plain", "bn_exact", "bn_normal"]


@pytest.mark.parametrize("variant", POOL_VARIANTS)
@pytest.mark.parametrize("name,width", cases("MaxOp", W32))
def test_pool_f32(name, width, variant):
    from deepchem_amd import ops
    b = batch(name)
    x, sc, sh, ref = _pool_case(b, width, variant, False)
    xd, scd, shd = dev(x), None if sc is None else dev(sc), None if sh is None else dev(sh)
    for _ in range(2):
        out, arg = Guarded(b.n, width), Guarded(b.n, width, torch.uint8)
        ops.gather_max(b.g, xd, scd, shd, out=out.rows, arg=arg.rows)
        if ref is not None:
            assert same(out, ref[0]) and same(arg, ref[1])
        else:
            assert_pool_within_one_ulp(b, bn_float64(b, x, width), out, arg, False)
    if variant == "plain":
        assert same(arg, b.planted_arg(width))
        if b.hg.max_present == 10:
            assert sorted(torch.unique(arg.rows).tolist()) == list(range(11))
        out2 = Guarded(b.n, width)  # evaluation: no arg bytes
        ops.gather_max(b.g, xd, want_arg=False, out=out2.rows)
        assert same(out2, ref[0])


@pytest.mark.parametrize("variant", POOL_VARIANTS)
@pytest.mark.parametrize("name,width", cases("MaxOpH", W16, bf16=True))
def test_pool_bf16(name, width, variant):
    from deepchem_amd import ops
    b = batch(name)
    x, sc, sh, ref = _pool_case(b, width, variant, True)
    xd, scd, shd = dev(x, bf16=True), None if sc is None else dev(sc), None if sh is None else dev(sh)
    for _ in range(2):
        out, arg = Guarded(b.n, width, BF16), Guarded(b.n, width, torch.uint8)
        ops.win_max_h(b.g, xd, scd, shd, out=out.rows, arg=arg.rows)
        if ref is not None:
            assert same(out, ref[0]) and same(arg, ref[1])  # (exact inputs: the winner IS a bf16 number)
        else:
            assert_pool_within_one_ulp(b, bn_float64(b, x, width), out, arg, True)
    if variant == "plain":
        out2 = Guarded(b.n, width, BF16)
        ops.win_max_h(b.g, xd, want_arg=False, out=out2.rows)
        assert same(out2, ref[0])
    if variant != "bn_normal" and width in W32:
        # the float kernel on the same (bf16-representable) rows: identical arg bytes, identical values
        o32, a32 = ops.gather_max(b.g, dev(x), scd, shd)
        assert torch.equal(a32, arg.rows) and torch.equal(o32, out.rows.float())


def _pool_then_sum(b, width, bn, fused):
    """gather_max_sum against the restatements; ``fused``: whether the one-pass kernel must have run."""
    from deepchem_amd import ops
    if bn:
        x, sc, sh = b.rows("exact", width), b.vec("sc_e", width), b.vec("sh_e", width)
        pool_ref, arg_ref = b.pool_ref(width, True)
    else:
        x, sc, sh = b.rows("normal", width), None, None
        pool_ref, arg_ref = R.pool_max(b.hg, x)
    s_ref = R.neigh_sum(b.hg, pool_ref)
    xd, scd, shd = dev(x), None if sc is None else dev(sc), None if sh is None else dev(sh)
    for _ in range(2):
        pool, arg, s = Guarded(b.n, width), Guarded(b.n, width, torch.uint8), Guarded(b.n, width)
        before = ops.max_sum_launches()
        ops.gather_max_sum(b.g, xd, scd, shd, pool=pool.rows, arg=arg.rows, s=s.rows)
        assert ops.max_sum_launches() - before == (1 if fused else 0)
        assert same(pool, pool_ref) and same(arg, arg_ref) and same(s, s_ref)
        other_direction(b)  # (the pass takes two turns of the sweep direction, or two launches one each)


@pytest.mark.parametrize("bn", [False, True], ids=["plain", "bn_exact"])
@pytest.mark.parametrize("name,width", cases("MaxSumOp", W32))
def test_pool_then_sum_f32(name, width, bn):
    """76 columns have no fused form, a batch of oversized windows only has nothing for it to do: the two window
    kernels run there."""
    b = batch(name)
    assert R.win_fits(b.c, 4 * width, 0, third_tiles=1)
    _pool_then_sum(b, width, bn, fused=width != 76 and name != "only_big")


# ------------------------------------------------------------------------------------------------ GraphPool backward
@pytest.mark.parametrize("name,width", cases("MaxBwdOp", W32))
def test_pool_bwd_f32(name, width):
    from deepchem_amd import ops
    b = batch(name)
    arg, g = b.planted_arg(width), b.rows("ds", width)
    ref = R.pool_bwd(b.hg, g, arg)
    argd, gd = dev(arg), dev(g)
    for _ in range(2):
        out = Guarded(b.n, width)
        ops.gather_max_bwd(b.g, gd, argd, out=out.rows)
        assert same(out, ref)


def _gamma_beta(width, ill):
    """Every column inside |beta| <= 64 |gamma| (the edge itself in column 1); ``ill``: one column outside."""
    gamma = np.linspace(0.5, 2.0, width).astype(np.float32)
    beta = (gamma * np.where(np.arange(width) % 2, 64.0, -63.0)).astype(np.float32)
    if ill:
        beta[width - 3] = np.float32(64.5) * gamma[width - 3]
    return dev(gamma), dev(beta)


@pytest.mark.parametrize("name,width", cases("MaxBwdOp_if_ill", W32))
def test_pool_bwd_f32_conditional(name, width):
    from deepchem_amd import ops
    b = batch(name)
    arg, g = b.planted_arg(width), b.rows("dxs", width)
    ref = R.pool_bwd(b.hg, g, arg)
    argd, gd = dev(arg), dev(g)
    for _ in range(2):
        out = Guarded(b.n, width)
        ops.win_max_bwd_if_ill(b.g, gd, argd, *_gamma_beta(width, True), out=out.rows)
        assert same(out, ref)
        out = Guarded(b.n, width)
        ops.win_max_bwd_if_ill(b.g, gd, argd, *_gamma_beta(width, False), out=out.rows)
        torch.cuda.synchronize()
        assert out.untouched()
        other_direction(b)  # (two launches so far in this round: a third, so that the next round sweeps the other way)


@pytest.mark.parametrize("cond", ["always", "ill", "well"], ids=["no_gamma", "ill_conditioned", "well_conditioned"])
@pytest.mark.parametrize("name,width", cases("MaxBwdOpH", W16, bf16=True))
def test_pool_bwd_bf16(name, width, cond):
    """The arg bytes reach the kernel through the split image of Piece<bf16_t>::arg: 64 low dwords, 64 high dwords."""
    from deepchem_amd import ops
    b = batch(name)
    arg, g = b.planted_arg(width), b.rows("ds", width, bf16=True)
    ref = R.bf16_round(R.pool_bwd(b.hg, g, arg))
    argd, gd = dev(arg), dev(g, bf16=True)
    gb = (None, None) if cond == "always" else _gamma_beta(width, cond == "ill")
    for _ in range(2):
        out = Guarded(b.n, width, BF16)
        ops.win_max_bwd_h(b.g, gd, argd, *gb, out=out.rows)
        torch.cuda.synchronize()
        assert out.untouched() if cond == "well" else same(out, ref)


# ------------------------------------------------------------------------------------------------ two-stage backward
def _two_stage(b, width, bf16):
    from deepchem_amd import ops
    dt = BF16 if bf16 else torch.float32
    arg = b.planted_arg(width)
    ds, dxs = b.rows("ds", width, bf16=bf16), b.rows("dxs", width, bf16=bf16)
    argd, dsd = dev(arg), dev(ds, bf16=bf16)
    row_bytes = width * (2 if bf16 else 4)
    if not R.win_fits(b.c, row_bytes, 8 if bf16 else 4, third_tiles=2):
        # no room for the third tiles: refused, nothing written
        dy, keep = Guarded(b.n, width, dt), Guarded(b.n, width, dt)
        keep.rows.copy_(dev(dxs, bf16=bf16))
        before = keep.buf.clone()
        assert refused(lambda: ops.win_sumacc_max_bwd(b.g, dsd, keep.rows, argd, out=dy.rows))
        torch.cuda.synchronize()
        assert dy.untouched() and torch.equal(bits(keep.buf), bits(before))
        return "refused"
    dx_ref, dy_ref = R.two_stage_bwd(b.hg, ds, dxs, arg, bf16=bf16)
    for _ in range(2):
        dy, acc = Guarded(b.n, width, dt), Guarded(b.n, width, dt)
        acc.rows.copy_(dev(dxs, bf16=bf16))
        ops.win_sumacc_max_bwd(b.g, dsd, acc.rows, argd, out=dy.rows)
        assert same(dy, dy_ref)
        # the contract for dXs: as it was on the rows of ordinary windows, the complete dX on those of oversized ones
        assert acc.guards_intact()
        after = acc.rows.float().cpu().numpy()
        want = dxs.copy()
        want[b.big_rows] = dx_ref[b.big_rows]
        assert np.array_equal(after.view(np.uint32), want.view(np.uint32))
        # ... and the two separate entries, one after the other, give the same bits
        sep = Guarded(b.n, width, dt)
        sep.rows.copy_(dev(dxs, bf16=bf16))
        dy2 = Guarded(b.n, width, dt)
        if bf16:
            ops.win_sum_h(b.g, dsd, sep.rows, accumulate=True)
            ops.win_max_bwd_h(b.g, sep.rows, argd, out=dy2.rows)
        else:
            ops.gather_sum(b.g, dsd, sep.rows, accumulate=True)
            ops.gather_max_bwd(b.g, sep.rows, argd, out=dy2.rows)
        assert same(sep, dx_ref) and same(dy2, dy_ref) and torch.equal(bits(dy2.rows), bits(dy.rows))
    return "ran"


# at 128 float columns a window atom costs 2 * (512 + 128) + 2 * 512 bytes of the 160 KiB: batches collated at the
# default cap of 96 atoms must be refused there, the others run
REFUSED_F32_128 = {"one_each", "big_mixed", "low_degree", "gappy", "empty_first"}


@pytest.mark.parametrize("name,width", cases("SumAccMaxBwdOp", W32))
def test_two_stage_bwd_f32(name, width):
    took = _two_stage(batch(name), width, False)
    assert took == ("refused" if width == 128 and name in REFUSED_F32_128 else "ran")


@pytest.mark.parametrize("name,width", cases("SumAccMaxBwdOpH", W16, bf16=True))
def test_two_stage_bwd_bf16(name, width):
    assert _two_stage(batch(name), width, True) == "ran"


# ------------------------------------------------------------------------------------------------ the LDS limits
@pytest.mark.parametrize("name,fits", [("cap48", True), ("cap96", False)],
                         ids=["SumAccMaxBwdOp-lpr32-cap48-fits", "SumAccMaxBwdOp-lpr32-cap96-refused"])
def test_two_stage_bwd_at_the_lds_limit(name, fits):
    """128 float columns: 2 * (512 + 128) + 2 * 512 = 2 304 bytes per window atom, 160 KiB - 2 368 bytes of head =
    70 atoms.  The molecules of ``one_each``: windows of up to 48 atoms fit, windows of up to 96 do not."""
    b = batch(name)
    assert (b.c.win_alloc <= 48) if fits else (b.c.win_alloc > 70)
    assert _two_stage(b, 128, False) == ("ran" if fits else "refused")


def test_pool_then_sum_without_room_for_the_scratch_tile():
    """128 float columns: 2 * 512 + 512 bytes per window atom for the fused pass -- 105 atoms.  Under a cap of 128 the
    two buffers still fit (157 atoms) and the scratch tile does not: the fused kernel is not launched and the two
    window kernels give the same results."""
    b = batch("cap128")
    assert b.c.win_alloc > 105 and R.win_fits(b.c, 512, 0) and not R.win_fits(b.c, 512, 0, third_tiles=1)
    _pool_then_sum(b, 128, True, fused=False)
    _pool_then_sum(b, 128, False, fused=False)
