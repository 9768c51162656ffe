"""The MAT kernels (csrc/mat.hip) at the edges they dispatch on: every ``NV`` instantiation full and partly filled, the
largest molecule below the cap (one wave, odd and even tile pitches), both sides of the 64 KiB of dynamic LDS, the order
of the molecules, four different leading dimensions, q / k / v as column blocks of one matrix, ``k is v`` with its own
``q``, and the bias kernel's lane-stride loops and molecule search.

Bar: ``bar`` of tests/test_gpu_mat.py, unchanged (error against float64 at most 4 times that of the float32 restatement,
floor one fp32 ulp of the largest entry); the ratios are printed.  Where a call does the same arithmetic in the same
order as another call (other leading dimensions, column-block views, another position in the batch) the results are
compared bit for bit on top: a wrong ``ld`` or offset cannot hide inside a tolerance.
"""
import numpy as np
import pytest
import torch

from deepchem_amd import ops
from tests import mat_refs as R
from tests.test_gpu_mat import SIZES, bar

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
UNIFORM = {"qkv": 4, "O": 4, "dO": 4, "grad": 4}
FOUR_LDS = {"qkv": 4, "O": 8, "dO": 12, "grad": 16}  # ld, ldo, lddo, ldg all different


def nan_wide(x, spare):
    t = torch.full((x.shape[0], x.shape[1] + spare), NAN, dtype=torch.float32, device=DEV)
    t[:, :x.shape[1]] = torch.as_tensor(x, device=DEV)
    return t


def spare_is_nan(t, lo, hi, name):
    keep = torch.ones(t.shape[1], dtype=torch.bool, device=t.device)
    keep[lo:hi] = False
    assert bool(torch.isnan(t[:, keep]).all()), "%s: columns outside [%d, %d) were written" % (name, lo, hi)
    assert not bool(torch.isnan(t[:, lo:hi]).any()), "%s: NaN inside [%d, %d)" % (name, lo, hi)


def run_native(c, spare=UNIFORM, kv_alias=False):
    """Forward and backward through ``ops`` on NaN-padded operands; ``spare``: the spare columns behind q/k/v, O, dO and
    the gradient buffers.  ``kv_alias``: k and v are ONE tensor (their values are equal in such a case), q its own."""
    offs = ops.MatOffsets(c["n_list"], DEV)
    assert offs.n_max == max(c["n_list"])
    W = c["h"] * c["d_k"]
    bias = torch.tensor(c["bias"], device=DEV)
    Q = nan_wide(c["q"], spare["qkv"])
    if c["shared"]:
        K = V = Q
    else:
        K = nan_wide(c["k"], spare["qkv"])
        V = K if kv_alias else nan_wide(c["v"], spare["qkv"])
    dO = nan_wide(c["dO"], spare["dO"])
    O = torch.full((offs.n_atoms, W + spare["O"]), NAN, dtype=torch.float32, device=DEV)
    bufs = [torch.full((offs.n_atoms, W + spare["grad"]), NAN, dtype=torch.float32, device=DEV)
            for _ in range(1 if c["shared"] else 3)]
    ops.mat_attention_fwd(Q[:, :W], K[:, :W], V[:, :W], bias, offs, c["h"], c["d_k"], c["lam"], out=O[:, :W])
    ops.mat_attention_bwd(Q[:, :W], K[:, :W], V[:, :W], bias, offs, c["h"], c["d_k"], c["lam"], dO[:, :W], c["shared"],
                          out=bufs[0][:, :W] if c["shared"] else [b[:, :W] for b in bufs])
    out = dict(zip(("O", "dQ", "dK", "dV"), [O] + bufs))
    for name, t in out.items():
        spare_is_nan(t, 0, W, name)
    for name, t in (("q", Q), ("k", K), ("v", V), ("dO", dO)):  # (the inputs are inputs)
        spare_is_nan(t, 0, W, name)
    return {name: t[:, :W].cpu().numpy() for name, t in out.items()}


def run_column_blocks(c):
    """q, k, v as the column blocks [4, 4 + W), [4 + W, 4 + 2 W), [4 + 2 W, 4 + 3 W) of ONE NaN-padded (N, 3 W + 8)
    matrix, the three gradients into the same blocks of a second one."""
    offs = ops.MatOffsets(c["n_list"], DEV)
    W = c["h"] * c["d_k"]
    bias = torch.tensor(c["bias"], device=DEV)
    X = torch.full((offs.n_atoms, 3 * W + 8), NAN, dtype=torch.float32, device=DEV)
    D = torch.full_like(X, NAN)
    cols = [slice(4 + i * W, 4 + (i + 1) * W) for i in range(3)]
    for sl, name in zip(cols, "qkv"):
        X[:, sl] = torch.as_tensor(c[name], device=DEV)
    q, k, v = (X[:, sl] for sl in cols)
    assert len({t.data_ptr() for t in (q, k, v)}) == 3 and q.stride(0) == 3 * W + 8
    O = ops.mat_attention_fwd(q, k, v, bias, offs, c["h"], c["d_k"], c["lam"])
    ops.mat_attention_bwd(q, k, v, bias, offs, c["h"], c["d_k"], c["lam"], torch.tensor(c["dO"], device=DEV), False,
                          out=[D[:, sl] for sl in cols])
    spare_is_nan(X, 4, 4 + 3 * W, "q | k | v")
    spare_is_nan(D, 4, 4 + 3 * W, "dQ | dK | dV")
    out = {"O": O.cpu().numpy()}
    out.update({name: D[:, sl].cpu().numpy() for sl, name in zip(cols, ("dQ", "dK", "dV"))})
    return out


def check(c, got, label):
    assert sorted(got) == sorted(c["f64"])
    worst = max(bar(got[name], c["f64"][name], c["f32"][name], "%s %s" % (label, name)) for name in c["f64"])
    print("worst ratio %s: %.2f" % (label, worst))
    return worst


def same_bits(a, b, label):
    assert sorted(a) == sorted(b)
    for name in a:
        assert np.array_equal(a[name], b[name]), "%s: %s differs in %d entries" % (label, name, int((a[name] != b[name]).sum()))


def shared_equals_summed(c, got, label):
    """The one-tensor call against the three-tensor call on the same values: O bit for bit, and dQ + dK + dV are the
    same three rows added in the same order."""
    three = run_native(dict(c, shared=False))
    assert np.array_equal(got["O"], three["O"]), label
    assert np.array_equal(got["dQ"], (three["dQ"] + three["dK"]) + three["dV"]), label


# ------------------------------------------------------------------------------------------------ attention
@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("d_k", [12, 16, 32, 36, 60])
@pytest.mark.parametrize("h", [1, 3])
def test_every_instantiation_full_and_partly_filled(h, d_k, shared):
    """NV = 4 at 12 (partly filled) and 16 (full): the first run of those kernels; NV = 8 full; NV = 16 partly filled."""
    assert R.nv_of(d_k) == {12: 4, 16: 4, 32: 8, 36: 16, 60: 16}[d_k]
    c = R.attention_edge_case(SIZES, h, d_k, shared=shared)
    check(c, run_native(c), "NV%d h%d d_k%d%s" % (R.nv_of(d_k), h, d_k, " shared" if shared else ""))


@pytest.mark.parametrize("d_k", [16, 64])
@pytest.mark.parametrize("n_max", sorted(R.N_MAX_BATCHES))
def test_largest_molecule_below_the_cap(n_max, d_k):
    """The workgroup size, the tile pitch ``n_max | 1``, the LDS offsets and the dynamic LDS size all follow n_max."""
    n_list = R.N_MAX_BATCHES[n_max]
    for shared in (False, True):
        c = R.attention_edge_case(n_list, 3, d_k, shared=shared)
        got = run_native(c)
        check(c, got, "n_max %d d_k%d%s" % (n_max, d_k, " shared" if shared else ""))
        if shared:
            shared_equals_summed(c, got, "n_max %d" % n_max)
        elif n_max == 1:  # the softmax of one score is 1, so dS = 0
            assert not got["dQ"].any() and not got["dK"].any() and got["dV"].any()


@pytest.mark.parametrize("nv", R.MAT_NV)
def test_both_sides_of_64_kib_of_lds(nv):
    """The largest n_max that launches without raising the kernel's LDS limit and the one above it, per direction."""
    pairs = [R.lds_boundary(nv, bwd) for bwd in (False, True)]
    assert tuple(pairs) == R.LDS_TABLE[nv]
    for bwd, (below, above) in enumerate(pairs):
        assert R.lds_bytes(nv, below, bool(bwd)) <= 65536 < R.lds_bytes(nv, above, bool(bwd))
    for n_max in sorted({n for pair in pairs for n in pair}):
        for shared in (False, True):
            c = R.attention_edge_case([5, n_max, 1], 3, 4 * nv, shared=shared)
            got = run_native(c)
            check(c, got, "LDS NV%d n_max %d%s" % (nv, n_max, " shared" if shared else ""))
            if shared:
                shared_equals_summed(c, got, "LDS NV%d n_max %d" % (nv, n_max))


@pytest.mark.parametrize("shared", [False, True])
def test_largest_molecule_first_and_one_atom_last(shared):
    """A workgroup depends on its own molecule and on n_max only: every molecule's rows bit for bit as in the ascending
    batch."""
    c = R.attention_edge_case(SIZES, 3, 16, shared=shared)
    order = list(range(len(SIZES)))[::-1]
    r, rows = R.reorder_case(c, order)
    assert r["n_list"][0] == ops.MAT_MAX_ATOMS and r["n_list"][-1] == 1
    up, down = run_native(c), run_native(r)
    check(c, up, "ascending" + (" shared" if shared else ""))
    same_bits({name: t[rows] for name, t in up.items()}, down, "reversed batch")


@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("d_k", [8, 16])
def test_four_different_leading_dimensions(d_k, shared):
    """ld, ldo, lddo and ldg each with its own value: 4, 8, 12 and 16 spare NaN columns (checked by ``run_native``)."""
    c = R.attention_edge_case(SIZES, 3, d_k, shared=shared)
    got = run_native(c, FOUR_LDS)
    check(c, got, "four lds d_k%d%s" % (d_k, " shared" if shared else ""))
    same_bits(got, run_native(c, UNIFORM), "four leading dimensions against one")


@pytest.mark.parametrize("d_k", [8, 16])
def test_q_k_v_as_column_blocks_of_one_matrix(d_k):
    c = R.attention_edge_case(SIZES, 3, d_k)
    got = run_column_blocks(c)
    check(c, got, "column blocks d_k%d" % d_k)
    same_bits(got, run_native(c), "column blocks against separate tensors")


@pytest.mark.parametrize("d_k", [16, 64])
def test_k_is_v_with_its_own_q(d_k):
    """The forward stages ONE tile for K and V; the backward is not shared and stages X and Y from one pointer.  Against
    float64 autograd with k and v as two leaves of equal value, and bit for bit against the three-tensor call."""
    c = R.attention_edge_case(SIZES, 3, d_k, kv_same=True)
    got = run_native(c, kv_alias=True)
    check(c, got, "k is v d_k%d" % d_k)
    same_bits(got, run_native(c), "k is v against two equal tensors")


# ------------------------------------------------------------------------------------------------ bias
@pytest.mark.parametrize("kind", ["softmax", "exp"])
def test_bias_lane_strides_search_and_ragged_last_workgroup(kind):
    n_list, adj, dist = R.bias_edge_case()
    offs = ops.MatOffsets(n_list, DEV)
    assert offs.n_atoms % 4 != 0
    # the op allocates its output: the block it is about to get held NaN, so an entry left unwritten is likely to show
    # as NaN in ``bar``; the comparison below is per block in any case
    stale = torch.full((offs.n_pairs,), NAN, dtype=torch.float32, device=DEV)
    del stale
    got = ops.mat_bias(torch.tensor(adj, dtype=torch.float32, device=DEV), torch.tensor(dist, dtype=torch.float32, device=DEV),
                       offs, kind, 0.33, 0.34).cpu().numpy()
    want = R.bias_blocks(adj, dist, n_list, kind, 0.33, 0.34, 1e-6, torch.float64).numpy()
    got32 = R.bias_blocks(adj, dist, n_list, kind, 0.33, 0.34, 1e-6, torch.float32).numpy()
    assert got.shape == want.shape
    bar(got, want, got32, "bias " + kind)
    one = np.float32(0.33) if kind == "softmax" else np.float32(0.0)  # the dummy atom alone: softmax 1 / exp(-1e6), no bond
    worst = 0.0
    for m, n in enumerate(n_list):
        blk = slice(offs.pair_off[m], offs.pair_off[m + 1])
        if n == 1:
            assert got[blk].shape == (1,) and got[blk][0] == one, (m, got[blk])
        else:
            worst = max(worst, bar(got[blk], want[blk], got32[blk], "bias %s molecule %d (%d atoms)" % (kind, m, n)))
            B = got[blk].reshape(n, n)
            assert np.all(B[1:, 0] == 0.0) and np.all(B[1:].sum(1) > 0.3)
    print("worst ratio bias %s: %.2f" % (kind, worst))
