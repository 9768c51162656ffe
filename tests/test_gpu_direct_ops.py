"""The direct gather kernels (csrc/gather.hip), one operation at a time, against the plain restatements of
tests/edge_refs.py (checked on the CPU by tests/test_win_refs_host.py and tests/test_direct_refs_host.py).  They run
behind gcmi_gather_sum_fwd, gcmi_scatter_add, gcmi_gather_max_fwd, gcmi_gather_max_bwd and gcmi_build_rev_pos wherever
no window pass does: every graph here is built from host arrays and has no window plan.

The kernels add in float32 in neighbour-table order and so do the restatements: the gather forms are compared BIT FOR
BIT.  The folded BatchNorm (an fmaf) is compared bit for bit on inputs where every product and sum is exact and within
one float32 ulp of a float64 evaluation on standard-normal inputs.  The atomic forms add in no fixed order: bit for bit
on quarter-valued rows, where any order is exact, and within 10 * 2^-24 * sum |terms| per element of the float64
restatement on standard-normal rows (at most 10 float32 additions of at most 11 terms, each off by at most half an ulp
of a partial sum no larger than sum |terms|).

Batches sit on the edges of the launch geometry (one workgroup = 1024 lane slots, a row takes n_feat / V of them, the
degree of a workgroup is looked up from the first workgroup of every degree block); each asserts what it is there for
(edge_refs.direct_batch_check).  Outputs are pre-filled with a sentinel and carry guard columns and a guard row; every
operation runs twice on the same buffers.  Case ids: operation - batch - width - route - V.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import edge_refs as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
WMAX = 256
SENTINEL = -777.0
ARG_SENTINEL = 0xEE
U24 = 2.0 ** -24

# (width, route): "aligned" takes V = 4 where the width allows; the others force V = 1 at 64 columns, one cause each
ALL_LAYOUTS = [(w, "aligned") for w in (4, 64, 68, 76, 256, 1, 2, 7, 75)] + \
    [(64, r) for r in ("x_off4", "ld66", "out_off4", "arg_off1")]
FEW_LAYOUTS = [(64, "aligned"), (75, "aligned")]
EVERY_WIDTH = ("mixed", "tile_exact", "tile_plus", "tile_minus")
SYMMETRIC = [n for n in R.DIRECT_BATCHES if n != "one_sided"]
FROM_LAYER_INPUTS = ("mixed", "multi", "shallow2", "shallow0", "one_sided")  # the others: BatchGraph(...) itself


def expected_v(width, route):
    return 4 if (route == "aligned" and width % 4 == 0) else 1


def cases(op, names=R.DIRECT_BATCHES, skip_routes=("arg_off1",)):
    out = []
    for name in names:
        for w, route in (ALL_LAYOUTS if name in EVERY_WIDTH else FEW_LAYOUTS):
            if route not in skip_routes:
                out.append(pytest.param(name, w, route, id="%s-%s-f%d-%s-V%d" % (op, name, w, route, expected_v(w, route))))
    return out


# ------------------------------------------------------------------------------------------------ batches
class Batch:
    def __init__(self, name):
        adjs, max_deg = R.direct_batch_adjs(name)
        self.counts, self.col, self.mem = R.collate_adjs(adjs, max_deg)
        assert R.direct_batch_check(name, self.counts, self.col)
        self.name = name
        self.one_sided = name == "one_sided"
        self.hg = (R.NeighbourTables if self.one_sided else R.HostGraph)(self.counts, self.col)
        self.n = self.hg.n_atoms
        self.n_edges = int(self.col.shape[0])
        self.deg0 = self.hg.rows(0)
        self.col_d = torch.from_numpy(self.col).to(DEV)
        self.mem_d = torch.from_numpy(self.mem).to(DEV)
        self.g = self.graph()          # reverse slots are built on first use where the adjacency has them
        self.g_atomic = self.graph(symmetric=False)

    def graph(self, symmetric=None):
        from deepchem_amd.graph import BatchGraph
        if self.name in FROM_LAYER_INPUTS:
            starts = np.concatenate([[0], np.cumsum(self.counts)[:-1]])
            deg_slice = np.stack([starts, np.asarray(self.counts)], 1).astype(np.int64)
            nt = R.NeighbourTables(self.counts, self.col)
            tables = [torch.from_numpy(nt.nb[d].astype(np.int32)) for d in range(1, len(self.counts))]
            g = BatchGraph.from_layer_inputs(deg_slice, torch.from_numpy(self.mem), tables, DEV)
        else:
            g = BatchGraph(self.counts, self.col_d, self.mem_d)
        g.symmetric = symmetric
        assert g.c.n_win == 0 and g.rev_pos is None and g.n_atoms == self.n and g.n_edges == self.n_edges
        assert np.array_equal(g.col_idx.cpu().numpy(), self.col)
        return g

    @functools.lru_cache(maxsize=None)
    def inputs(self):
        """Host inputs of WMAX columns (a narrower case takes the first columns)."""
        rng = np.random.RandomState(len(self.name) * 1000 + self.n % 997)
        d = {k: rng.standard_normal((self.n, WMAX)).astype(np.float32) for k in ("normal", "ds", "old")}
        d["exact"] = R.plant_winners(self.hg, R.exact_rows(rng, self.n, WMAX))
        d["ds_e"], d["old_e"] = R.exact_rows(rng, self.n, WMAX), R.exact_rows(rng, self.n, WMAX)
        for k in ("old", "old_e"):  # a degree-0 row the accumulate form adds nothing to keeps even the sign of a zero
            d[k][self.deg0, 0] = -0.0
        # signed zeros and infinities around the ties, outside the planted rows; the low columns get their share
        d["special"] = x = d["exact"].copy()
        dmax = self.hg.max_present
        planted = np.concatenate([[self.hg.row0[dmax]], self.hg.nb[dmax][0]]) if dmax else np.zeros(0, np.int64)
        free = np.setdiff1d(np.arange(self.n), planted)
        values = (0.0, -0.0, np.inf, -np.inf)
        for v in values:
            k = max(4, self.n // 6)
            cols = np.where(rng.random_sample(k) < 0.5, rng.randint(0, 8, k), rng.randint(0, WMAX, k))
            x[rng.choice(free, k), cols] = v
        x[free[np.linspace(0, len(free) - 1, 4).astype(np.int64)], 0] = values  # (the one-column case sees all four)
        assert not np.isnan(x).any() and np.isinf(x[:, 0]).any() and (np.signbit(x[:, 0]) & (x[:, 0] == 0)).any()
        d["sc_e"], d["sh_e"] = R.exact_bn(rng, WMAX)
        d["sc_n"] = rng.standard_normal(WMAX).astype(np.float32)
        d["sh_n"] = rng.standard_normal(WMAX).astype(np.float32)
        return d

    def rows(self, key, width):
        return np.ascontiguousarray(self.inputs()[key][:, :width])

    def vec(self, key, width):
        return np.ascontiguousarray(self.inputs()[key][:width])

    @functools.lru_cache(maxsize=None)
    def pool_ref(self, width, variant):
        if variant == "plain":
            return R.pool_max(self.hg, self.rows("special", width))
        y = self.rows("exact", width) * self.vec("sc_e", width) + self.vec("sh_e", width)
        assert y.dtype == np.float32
        return R.pool_max(self.hg, y)

    def planted_arg(self, width):
        """Arg bytes from the restatement (never from the kernel under test); with more columns than the highest degree
        every byte 0 .. D occurs."""
        arg = self.pool_ref(width, "plain")[1]
        if width > self.hg.max_present:
            assert sorted(np.unique(arg).tolist()) == list(range(self.hg.max_present + 1))
        return arg


@functools.lru_cache(maxsize=None)
def batch(name):
    return Batch(name)


# ------------------------------------------------------------------------------------------------ buffers
def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(t):
    t = t.contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def ld(t):
    return int(t.stride(0)) if t.shape[0] > 1 else int(t.shape[1])


class Box:
    """(n, width) float rows inside a filled (n + 1, off + width + pad) buffer: ``off`` columns in front (off = 1: the
    rows start 4 bytes past a 16-byte boundary), ``pad`` behind, one guard row."""

    def __init__(self, n, width, off=0, pad=4, fill=SENTINEL):
        self.buf = torch.full((n + 1, off + width + pad), fill, dtype=torch.float32, device=DEV)
        self.start = self.buf.clone()
        self.rows = self.buf[:n, off:off + width]
        self.inside = torch.zeros(self.buf.shape, dtype=torch.bool, device=DEV)
        self.inside[:n, off:off + width] = True
        assert self.buf.data_ptr() % 16 == 0 and self.rows.data_ptr() % 16 == 4 * off

    def set(self, a):
        self.rows.copy_(a if torch.is_tensor(a) else dev(a))
        return self

    def guards_intact(self):
        return torch.equal(bits(self.buf)[~self.inside], bits(self.start)[~self.inside])

    def untouched(self):
        return torch.equal(bits(self.buf), bits(self.start))


def in_box(n, width, route, a):
    """An input: NaN around the rows, so a read outside them shows in the result."""
    off, pad = {"x_off4": (1, 7), "ld66": (0, 2)}.get(route, (0, 4))
    return Box(n, width, off, pad, fill=float("nan")).set(a)


def out_box(n, width, route):
    off, pad = (1, 7) if route == "out_off4" else (0, 4)
    return Box(n, width, off, pad)


class ArgBox:
    """(n, width) contiguous arg bytes inside a larger byte buffer, 4 (aligned) or 5 bytes from its start."""

    def __init__(self, n, width, route="aligned", tail=64):
        off = 5 if route == "arg_off1" else 4
        self.buf = torch.full((off + n * width + tail,), ARG_SENTINEL, dtype=torch.uint8, device=DEV)
        self.rows = self.buf[off:off + n * width].view(n, width)
        self.off, self.size = off, n * width
        assert self.rows.is_contiguous() and self.rows.data_ptr() % 4 == off - 4

    def set(self, a):
        self.rows.copy_(dev(a))
        return self

    def guards_intact(self):
        return bool((self.buf[:self.off] == ARG_SENTINEL).all()) and bool((self.buf[self.off + self.size:] == ARG_SENTINEL).all())

    def untouched(self):
        return bool((self.buf == ARG_SENTINEL).all())


def same(out, ref):
    """``out`` (Box, ArgBox or tensor) equals the host array ``ref`` bit for bit, guards intact."""
    if isinstance(out, (Box, ArgBox)):
        assert out.guards_intact(), "a guard row, guard column or guard byte was written"
        out = out.rows
    want = dev(ref)
    assert want.dtype == out.dtype and want.shape == out.shape
    return torch.equal(bits(out), bits(want))


def vec_of(*mats, arg=None):
    """The V the entry point must choose for these operands (vec_width restated; arg rows need 4-byte alignment)."""
    v = min(R.direct_vec(t.data_ptr(), ld(t), t.shape[1]) for t in mats)
    return 1 if (arg is not None and arg.data_ptr() % 4) else v


def _vp(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def raw(name, g, *args):
    from deepchem_amd import _lib
    from deepchem_amd.graph import _stream
    _lib.call(name, g.ref, *args, _stream())


def raw_pool_bwd(g, dout, arg, dx):
    raw("gcmi_gather_max_bwd", g, _vp(dout), ld(dout), dout.shape[1], _vp(arg), _vp(dx), ld(dx))


def within_atomic_bound(got, ref64, mag64):
    """|got - ref| <= 10 * 2^-24 * sum |terms| per element (module docstring); prints the largest ratio."""
    err = np.abs(got.astype(np.float64) - ref64)
    bound = 10 * U24 * mag64
    assert np.all(err[mag64 == 0] == 0)
    ratio = float((err[mag64 > 0] / bound[mag64 > 0]).max()) if (mag64 > 0).any() else 0.0
    print("atomic sum error / bound: max %.4f" % ratio)
    return ratio <= 1.0


# ------------------------------------------------------------------------------------------------ neighbour sums
@pytest.mark.parametrize("accumulate", [False, True], ids=["set", "accumulate"])
@pytest.mark.parametrize("name,width,route", cases("gather_sum"))
def test_gather_sum(name, width, route, accumulate):
    from deepchem_amd import ops
    b = batch(name)
    lpr = width // expected_v(width, route)
    tiles = R.direct_tiles(b.counts, lpr, accumulate)  # (the accumulate form skips the degree-0 block)
    assert lpr in R.DIRECT_LPR and (sum(n for _, n, _ in tiles) == 0) == (accumulate and b.n_edges == 0)
    for kx, kold in (("normal", "old"), ("exact", "old_e")):
        x, old = b.rows(kx, width), b.rows(kold, width)
        ref = R.neigh_sum(b.hg, x, old=old if accumulate else None)
        if accumulate:
            ref[b.deg0] = old[b.deg0]  # not "+ 0": the rows keep their bits (a -0.0 among them)
        else:
            assert not ref[b.deg0].any()
        xin, out = in_box(b.n, width, route, x), out_box(b.n, width, route)
        assert vec_of(xin.rows, out.rows) == expected_v(width, route)
        runs = []
        for _ in range(2):
            if accumulate:
                out.set(old)
            ops.gather_sum(b.g, xin.rows, out.rows, accumulate=accumulate)
            assert same(out, ref)
            runs.append(out.buf.clone())
        assert torch.equal(bits(runs[0]), bits(runs[1]))
    if accumulate and b.n_edges == 0:
        # nothing is launched: even a sentinel-filled output stays as it was
        out = out_box(b.n, width, route)
        ops.gather_sum(b.g, xin.rows, out.rows, accumulate=True)
        torch.cuda.synchronize()
        assert out.untouched()


# ------------------------------------------------------------------------------------------------ GraphPool forward
def assert_pool_within_one_ulp(b, y64, out, arg):
    """Values within one float32 ulp of max_j y64_j; the candidate the arg byte names within the same ulp of that maximum
    (the kernel compares float32 roundings of y, so it may name a candidate half an ulp below).  No case excluded."""
    assert out.guards_intact() and arg.guards_intact()
    ref, _ = R.pool_max(b.hg, y64)
    got = out.rows.cpu().numpy().astype(np.float64)
    tol = R.ulp(np.maximum(np.abs(ref), np.abs(got)))
    err = np.abs(got - ref) / tol
    print("pool value error in float32 ulps: max %.3f" % err.max())
    assert err.max() <= 1.0
    gap = (ref - R.candidate_value(b.hg, y64, arg.rows.cpu().numpy())) / tol
    print("named candidate below the maximum, ulps: max %.3f" % gap.max())
    assert gap.min() >= 0.0 and gap.max() <= 1.0


@pytest.mark.parametrize("variant", ["plain", "bn_exact", "bn_normal"])
@pytest.mark.parametrize("name,width,route", cases("gather_max", skip_routes=()))
def test_gather_max(name, width, route, variant):
    from deepchem_amd import ops
    b = batch(name)
    if variant == "plain":
        x, sc, sh, ref = b.rows("special", width), None, None, b.pool_ref(width, "plain")
    elif variant == "bn_exact":
        x, sc, sh, ref = b.rows("exact", width), b.vec("sc_e", width), b.vec("sh_e", width), b.pool_ref(width, "bn")
    else:
        x, sc, sh, ref = b.rows("normal", width), b.vec("sc_n", width), b.vec("sh_n", width), None
    xin, out, arg = in_box(b.n, width, route, x), out_box(b.n, width, route), ArgBox(b.n, width, route)
    scd, shd = (None, None) if sc is None else (dev(sc), dev(sh))
    assert vec_of(xin.rows, out.rows, arg=arg.rows) == expected_v(width, route)
    runs = []
    for _ in range(2):
        ops.gather_max(b.g, xin.rows, scd, shd, out=out.rows, arg=arg.rows)
        if ref is not None:
            assert same(out, ref[0]) and same(arg, ref[1])
        else:
            y64 = x.astype(np.float64) * sc.astype(np.float64) + sh.astype(np.float64)
            assert_pool_within_one_ulp(b, y64, out, arg)
        runs.append((out.buf.clone(), arg.buf.clone()))
    assert torch.equal(bits(runs[0][0]), bits(runs[1][0])) and torch.equal(runs[0][1], runs[1][1])
    if variant == "plain":
        assert same(arg, b.planted_arg(width))
        if b.n_edges == 0:
            assert same(out, x) and not arg.rows.any()  # no neighbour: the row itself, arg 0
        out2 = out_box(b.n, width, route)  # evaluation: no arg bytes
        ops.gather_max(b.g, xin.rows, want_arg=False, out=out2.rows)
        assert same(out2, ref[0])


# ------------------------------------------------------------------------------------------------ GraphPool backward
@pytest.mark.parametrize("name,width,route", cases("gather_max_bwd_gather", names=SYMMETRIC, skip_routes=()))
def test_gather_max_bwd_gather_form(name, width, route):
    """Reverse slots present: every dx row is written exactly once, by one lane group."""
    from deepchem_amd import ops
    b = batch(name)
    assert b.g.ensure_rev_pos() and b.g.symmetric is True and (b.g.c.d_rev_pos or b.n_edges == 0)
    arg = b.planted_arg(width)
    argd = ArgBox(b.n, width, route).set(arg)
    for key in ("ds", "ds_e"):
        g = b.rows(key, width)
        ref = R.pool_bwd(b.hg, g, arg)
        gin, out = in_box(b.n, width, route, g), out_box(b.n, width, route)
        assert vec_of(gin.rows, out.rows, arg=argd.rows) == expected_v(width, route)
        runs = []
        for _ in range(2):
            ops.gather_max_bwd(b.g, gin.rows, argd.rows, out=out.rows)
            assert same(out, ref)  # (the sentinel is gone from every row, the guards kept it)
            runs.append(out.buf.clone())
        assert torch.equal(bits(runs[0]), bits(runs[1]))
        if b.n_edges == 0:
            assert same(out, g)
    assert argd.guards_intact() and same(argd, arg)


def _atomic_graph(b):
    """one_sided: the asymmetry is found on the device; a symmetric batch: forced to the atomic form."""
    if b.one_sided:
        assert not b.g.ensure_rev_pos() and b.g.symmetric is False
        return b.g
    assert b.g_atomic.symmetric is False and not b.g_atomic.ensure_rev_pos()
    return b.g_atomic


@pytest.mark.parametrize("name,width,route", cases("gather_max_bwd_atomic", names=("mixed", "one_sided"), skip_routes=()))
def test_gather_max_bwd_atomic_form(name, width, route):
    b = batch(name)
    g = _atomic_graph(b)
    assert g.rev_pos is None and not g.c.d_rev_pos
    arg = b.planted_arg(width)
    argd = ArgBox(b.n, width, route).set(arg)
    for key in ("ds_e", "ds"):
        dout = b.rows(key, width)
        gin, out = in_box(b.n, width, route, dout), out_box(b.n, width, route)
        assert vec_of(gin.rows, out.rows, arg=argd.rows) == expected_v(width, route)
        for _ in range(2):
            out.rows.zero_()
            raw_pool_bwd(g, gin.rows, argd.rows, out.rows)
            if key == "ds_e":
                assert same(out, R.pool_bwd_scatter(b.hg, dout, arg))
            else:
                assert out.guards_intact()
                d64 = dout.astype(np.float64)
                assert within_atomic_bound(out.rows.cpu().numpy(), R.pool_bwd_scatter(b.hg, d64, arg),
                                           R.pool_bwd_scatter(b.hg, np.abs(d64), arg))
    if not b.one_sided:  # the same routes as the gather form, on quarter-valued rows to the bit
        assert np.array_equal(R.pool_bwd_scatter(b.hg, b.rows("ds_e", width), arg), R.pool_bwd(b.hg, b.rows("ds_e", width), arg))


def test_gather_max_bwd_through_ops_zeroes_its_own_rows_on_a_one_sided_graph():
    from deepchem_amd import ops
    b = batch("one_sided")
    g = _atomic_graph(b)
    arg, dout = b.planted_arg(64), b.rows("ds_e", 64)
    with pytest.raises(ValueError):
        ops.gather_max_bwd(g, dev(dout), dev(arg), out=torch.empty((b.n, 64), device=DEV))
    for _ in range(2):
        assert same(ops.gather_max_bwd(g, dev(dout), dev(arg)), R.pool_bwd_scatter(b.hg, dout, arg))


# ------------------------------------------------------------------------------------------------ scatter_add
@pytest.mark.parametrize("name,width,route", cases("scatter_add"))
def test_scatter_add(name, width, route):
    """V follows the source rows alone (the atomics are scalar): a misaligned dx keeps V = 4."""
    from deepchem_amd import ops
    b = batch(name)
    v = 4 if (route == "out_off4") else expected_v(width, route)
    ds_e, old_e, ds = b.rows("ds_e", width), b.rows("old_e", width), b.rows("ds", width)
    ref_e = R.scatter_ref(b.hg, ds_e, dx0=old_e)
    for _ in range(2):
        src, dx = in_box(b.n, width, route, ds_e), out_box(b.n, width, route).set(old_e)
        assert vec_of(src.rows) == v
        ops.scatter_add(b.g, src.rows, dx.rows)
        assert same(dx, ref_e)
    if not b.one_sided:  # bonds listed from both ends: the transpose is the gather, to the bit on these rows
        assert np.array_equal(ref_e, R.neigh_sum(b.hg, ds_e, old=old_e))
        assert torch.equal(bits(dx.rows), bits(ops.gather_sum(b.g, src.rows, dev(old_e), accumulate=True)))
    d64 = ds.astype(np.float64)
    for _ in range(2):
        src, dx = in_box(b.n, width, route, ds), out_box(b.n, width, route)
        dx.rows.zero_()
        ops.scatter_add(b.g, src.rows, dx.rows)
        assert dx.guards_intact()
        assert within_atomic_bound(dx.rows.cpu().numpy(), R.scatter_ref(b.hg, d64), R.scatter_ref(b.hg, np.abs(d64)))
    if b.n_edges == 0:
        dx = out_box(b.n, width, route)
        ops.scatter_add(b.g, src.rows, dx.rows)
        torch.cuda.synchronize()
        assert dx.untouched()


# ------------------------------------------------------------------------------------------------ reverse slots
def _build_rev(g, n_edges, flag_start):
    rev = torch.full((n_edges + 64,), ARG_SENTINEL, dtype=torch.uint8, device=DEV)
    flag = torch.full((3,), flag_start, dtype=torch.int32, device=DEV)
    raw("gcmi_build_rev_pos", g, _vp(rev), _vp(flag))
    assert bool((rev[n_edges:] == ARG_SENTINEL).all()) and flag[1:].tolist() == [flag_start] * 2
    return rev[:n_edges], int(flag[0].item())


@pytest.mark.parametrize("name", R.DIRECT_BATCHES, ids=["build_rev_pos-%s" % n for n in R.DIRECT_BATCHES])
def test_build_rev_pos(name):
    b = batch(name)
    g = b.graph()
    assert g.symmetric is None
    runs = [_build_rev(g, b.n_edges, 7) for _ in range(2)]
    assert torch.equal(runs[0][0], runs[1][0])
    if b.one_sided:
        assert runs[0][1] == 1 and runs[1][1] == 1
        assert not g.ensure_rev_pos() and g.symmetric is False and g.rev_pos is None and not g.c.d_rev_pos
        # every other entry is paired as in the same batch without the lone bond's row: 255 marks the one without a mate
        assert int((runs[0][0] == 255).sum()) == 1
        return
    want = np.concatenate([r.reshape(-1) for r in b.hg.rev] + [np.zeros(0, np.int64)]).astype(np.uint8)
    assert runs[0][1] == 0 and runs[1][1] == 0  # the flag is cleared, also where there is no edge to look at
    assert torch.equal(runs[0][0], dev(want))
    assert g.ensure_rev_pos() and g.symmetric is True
    assert torch.equal(g.rev_pos[:b.n_edges], dev(want))
    if name == "multi":
        assert len(np.unique(want[:])) >= 10


@pytest.fixture(scope="module")
def many_stars():
    """35 000 x (three ten-armed stars and a chain of seven), collated natively: 2.52 million edge slots, more than the
    8192 x 256 threads rev_pos_kernel's grid is capped at."""
    from deepchem_amd.data.collate import collate_to_device
    from deepchem_amd.utils.synthetic import PackedMols
    unit = R.packed_from_adjs([R.star_adj(10)] * 3 + [R.chain_adj(7)])
    reps, na, ne = 35000, unit.n_atoms, int(unit.adj_idx.shape[0])
    rep = np.arange(reps, dtype=np.int64)[:, None]
    atom_ptr = np.concatenate([[0], (unit.atom_ptr[1:][None, :] + na * rep).reshape(-1)])
    adj_ptr = np.concatenate([[0], (unit.adj_ptr[1:][None, :] + ne * rep).reshape(-1)])
    packed = PackedMols(np.zeros((na * reps, 4), np.float32), atom_ptr, adj_ptr, np.tile(unit.adj_idx, reps))
    return collate_to_device(packed, None, DEV)


def test_build_rev_pos_beyond_one_grid_of_threads(many_stars):
    from deepchem_amd.graph import BatchGraph
    g = many_stars.graph
    assert g.n_edges > 8192 * 256 and g.rev_pos is not None and g.deg_counts[10] == 105000
    g2 = BatchGraph(g.deg_counts, g.col_idx, g.membership)
    assert g2.c.n_win == 0 and g2.rev_pos is None and g2.symmetric is None
    assert g2.ensure_rev_pos() and g2.symmetric is True
    assert torch.equal(g2.rev_pos[:g.n_edges], g.rev_pos[:g.n_edges])


# ------------------------------------------------------------------------------------------------ pool, then sum
@pytest.mark.parametrize("bn", [False, True], ids=["plain", "bn_exact"])
@pytest.mark.parametrize("name,width,route", [
    pytest.param(n, w, "aligned", id="gather_max_sum-%s-f%d-aligned-V%d" % (n, w, expected_v(w, "aligned")))
    for n in ("mixed", "high_only", "one_sided") for w in (64, 75)])
def test_gather_max_sum_without_windows(name, width, route, bn):
    from deepchem_amd import ops
    b = batch(name)
    if bn:
        x, scd, shd = b.rows("exact", width), dev(b.vec("sc_e", width)), dev(b.vec("sh_e", width))
        pool_ref, arg_ref = b.pool_ref(width, "bn")
    else:
        x, scd, shd = b.rows("normal", width), None, None
        pool_ref, arg_ref = R.pool_max(b.hg, x)
    s_ref = R.neigh_sum(b.hg, pool_ref)
    xin = in_box(b.n, width, route, x)
    for _ in range(2):
        pool, arg, s = out_box(b.n, width, route), ArgBox(b.n, width), out_box(b.n, width, route)
        assert vec_of(xin.rows, pool.rows, s.rows, arg=arg.rows) == expected_v(width, route)
        before = ops.max_sum_launches()
        ops.gather_max_sum(b.g, xin.rows, scd, shd, pool=pool.rows, arg=arg.rows, s=s.rows)
        assert ops.max_sum_launches() == before
        assert same(pool, pool_ref) and same(arg, arg_ref) and same(s, s_ref)
        o2, a2 = ops.gather_max(b.g, xin.rows, scd, shd)
        s2 = ops.gather_sum(b.g, o2)
        assert torch.equal(bits(o2), bits(pool.rows)) and torch.equal(a2, arg.rows) and torch.equal(bits(s2), bits(s.rows))


# ------------------------------------------------------------------------------------------------ no edges at all
@pytest.mark.parametrize("name", ["lone", "shallow0"])
def test_pool_backward_without_edges_needs_no_reverse_table(name):
    """n_edges == 0: the gather form runs with a NULL reverse table and returns dout."""
    b = batch(name)
    g = b.graph()
    assert g.n_edges == 0 and not g.c.d_rev_pos and not g.c.d_col_idx
    for width, route in FEW_LAYOUTS:
        dout = b.rows("ds", width)
        gin, out = in_box(b.n, width, route, dout), out_box(b.n, width, route)
        arg = ArgBox(b.n, width).set(np.zeros((b.n, width), np.uint8))
        for _ in range(2):
            raw_pool_bwd(g, gin.rows, arg.rows, out.rows)
            assert same(out, dout)
    assert g.rev_pos is None


# ------------------------------------------------------------------------------------------------ refusals
def _refused(fn):
    """fn() fails with GCMI_ERR_ARG (-1) and an error text."""
    from deepchem_amd import _lib
    with pytest.raises(_lib.GcmiError) as e:
        fn()
    assert "status -1" in str(e.value) and len(str(e.value)) > 40
    return True


@pytest.mark.parametrize("what", ["ld_in", "ld_out", "n_feat_0", "n_feat_negative", "scale_only", "shift_only"])
def test_bad_arguments_are_refused_and_nothing_is_written(what):
    """What deepchem_amd.ops would stop first, handed to the C entry points themselves."""
    b = batch("mixed")
    w = 64
    x, out, s, arg = in_box(b.n, w, "aligned", b.rows("normal", w)), out_box(b.n, w, "aligned"), out_box(b.n, w, "aligned"), ArgBox(b.n, w)
    vec = dev(b.vec("sc_n", w))
    ldx, ldo, nf = ld(x.rows), ld(out.rows), w
    sc = sh = None
    if what == "ld_in":
        ldx = w - 1
    elif what == "ld_out":
        ldo = w - 1
    elif what == "n_feat_0":
        nf = 0
    elif what == "n_feat_negative":
        nf = -4
    elif what == "scale_only":
        sc = vec
    else:
        sh = vec
    X, O, S, A = _vp(x.rows), _vp(out.rows), _vp(s.rows), _vp(arg.rows)
    assert _refused(lambda: raw("gcmi_gather_max_fwd", b.g, X, ldx, nf, _vp(sc), _vp(sh), O, ldo, A))
    assert _refused(lambda: raw("gcmi_gather_max_sum_fwd", b.g, X, ldx, nf, _vp(sc), _vp(sh), O, ldo, A, S, ld(s.rows)))
    if what not in ("scale_only", "shift_only"):
        assert _refused(lambda: raw("gcmi_gather_sum_fwd", b.g, X, ldx, nf, O, ldo, 0))
        assert _refused(lambda: raw("gcmi_gather_sum_fwd", b.g, X, ldx, nf, O, ldo, 1))
        assert _refused(lambda: raw("gcmi_scatter_add", b.g, X, ldx, nf, O, ldo))
        for g in (b.g, b.g_atomic):
            assert _refused(lambda: raw("gcmi_gather_max_bwd", g, X, ldx, nf, A, O, ldo))
    torch.cuda.synchronize()
    assert out.untouched() and s.untouched() and arg.untouched()
