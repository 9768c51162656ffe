"""The fused D-MPNN bond update (dmpnn_update_kernel of csrc/dmpnn.hip) at its dispatch and tile edges: every accumulator
width NB, staging at the degree cap (94 rows), leading dimensions and alignment, and more tiles than one pass holds.

Exact cases: x, input in [-4, 4] and W in [-2, 2], all integers.  Every bf16 piece is then the value itself, every
product and partial sum an integer below 2^24, so the fused result must equal the float64 one bit for bit -- whatever
the order of the six piece products or of the staging sums.
Accuracy cases: ``rel_err <= max(4 * e32, 1e-6)`` relative to the largest entry of the float64 restatement, ``e32`` the
error of the same restatement in float32 on the CPU (dmpnn_refs.update_f32, at one thread) on the same case; the floor is the 1e-6 the
project recorded for this kernel on the MI355X (there is no transcendental function in it: the floor only covers the
six-term split standing in for a float32 product).  Every check prints ``rel_err / bar``; the last test prints the worst per NB.
"""
import numpy as np
import pytest
import torch

from deepchem_amd import ops
from deepchem_amd.models.torch_models.dmpnn import DmpnnBatch
from tests import dmpnn_refs as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FLOOR, FACTOR = 1e-6, 4.0
WIDTHS = [1, 16, 17, 32, 33, 64, 65, 96, 97, 160, 161, 256, 257, 320]
WORST = {}

MIXED = [([], 1), (R.chain(2), 2), (R.chain(3), 3), (R.ring(6), 6), (R.star(4), 5), (R.star(6), 7), ([], 2),
         (R.chain(130), 130)]
CAP_PAIR = R.cap_pair()
BATCHES = {
    "mixed": MIXED,
    # the 94-row tile at rows 32..63 and, 160 rows further on (the second pair starts on a tile edge again), at 192..223
    "cap": [CAP_PAIR, ([], 1), (R.chain(2), 2), (R.chain(17), 17), CAP_PAIR],
    # a degree-32 run that fills tile 0 exactly, and another (after 64 + 30 rows) that straddles
    "fill": [(R.star(32), 33), (R.chain(16), 16), (R.star(32), 33)],
    # atoms without bonds between, before and after runs, inside a molecule and as whole molecules
    "gaps": [([], 2), ([(1, 3), (3, 6)], 8), ([], 1), (R.star(32), 40), ([(0, 5)], 6), ([], 3)],
}
_BATCH = {}


def batch(name):
    if name not in _BATCH:
        rng = np.random.RandomState(1)
        _BATCH[name] = DmpnnBatch.from_graphs([R.graph(rng, b, n, 1, 1, 0) for b, n in BATCHES[name]]).to(DEV)
    return _BATCH[name]


def scratch(d):
    return torch.empty(ops.dmpnn_update_scratch_floats(d), device=DEV)


def fused(b, x, inp, W, relu, out=None):
    p = b.plan
    return ops.dmpnn_update_fwd(x, inp, W, p.out_ptr, p.rev, p.bond_src, relu, scratch(x.shape[1]), out=out)


def operands(B, d, seed, exact):
    rng = np.random.RandomState(seed)
    if exact:
        x, inp = (rng.randint(-4, 5, (B, d)).astype(np.float32) for _ in range(2))
        return x, inp, rng.randint(-2, 3, (d, d)).astype(np.float32)
    x, inp = (rng.normal(0, 1, (B, d)).astype(np.float32) for _ in range(2))
    return x, inp, rng.normal(0, 1 / np.sqrt(d), (d, d)).astype(np.float32)


# ------------------------------------------------------------------------------------------------ coverage of the tables
def test_case_tables_reach_every_nb_and_the_staging_depths():
    assert {R.dmpnn_update_branch(d)[0] for d in WIDTHS} == set(R.UPD_NB) == {1, 2, 3, 5, 8, 10}
    assert {R.dmpnn_update_branch(d)[1] for d in WIDTHS} == {1, 2, 3, 4, 5}
    rows = {k: R.staged_rows(batch(k).host["out_ptr"], batch(k).host["bond_src"], batch(k).n_bonds) for k in BATCHES}
    deg = {k: np.diff(batch(k).host["out_ptr"]) for k in BATCHES}
    assert rows["cap"].max() == 94 == R.UPD_STAGE - 2 and int((rows["cap"] == 94).sum()) == 2 and (deg["cap"] == 32).sum() == 4
    assert rows["fill"][0] == 32 and deg["fill"][0] == 32 and rows["fill"].max() > 32
    assert rows["mixed"].max() <= 32 + 5 + 5  # what the suite staged before this file
    h = batch("gaps").host
    assert deg["gaps"].max() == 32 and deg["gaps"][0] == 0 and deg["gaps"][-1] == 0
    inner = np.nonzero(deg["gaps"] == 0)[0]
    assert ((inner > 0) & (inner < len(deg["gaps"]) - 1)).sum() >= 8 and h["out_ptr"][-1] == batch("gaps").n_bonds


# ------------------------------------------------------------------------------------------------ widths
@pytest.mark.parametrize("relu", [False, True], ids=["none", "relu"])
@pytest.mark.parametrize("d", WIDTHS)
def test_exact_integers_at_every_width(d, relu):
    """Small integers: bit for bit the float64 result, on the mixed and the degree-cap batch."""
    for name in ("mixed", "cap"):
        b = batch(name)
        x, inp, W = operands(b.n_bonds, d, d + relu, exact=True)
        want = R.update_f64(x, inp, W, b.host["out_ptr"], b.host["rev"], relu)
        assert np.abs(want).max() < 2 ** 24 and (32 * 4 + 4) * 2 * d + 4 < 2 ** 24  # every partial sum is a float32 integer
        got = fused(b, *(torch.tensor(a, device=DEV) for a in (x, inp, W)), relu).cpu().numpy()
        bad = np.argwhere(got != want)
        assert got.shape == want.shape and bad.shape[0] == 0, (name, d, bad[:5], got[tuple(bad[0])], want[tuple(bad[0])])


@pytest.mark.parametrize("relu", [False, True], ids=["none", "relu"])
@pytest.mark.parametrize("d", WIDTHS)
def test_accuracy_at_every_width(d, relu):
    for name in sorted(BATCHES):
        if name in ("fill", "gaps") and (relu or d not in (1, 33, 97, 320)):
            continue  # the plan-shape batches at one width per staging-chunk count
        b = batch(name)
        x, inp, W = operands(b.n_bonds, d, 7 * d + relu, exact=False)
        want = R.update_f64(x, inp, W, b.host["out_ptr"], b.host["rev"], relu)
        e32 = R.rel_err(R.update_f32(x, inp, W, b.host["out_ptr"], b.host["rev"], relu), want)
        got = fused(b, *(torch.tensor(a, device=DEV) for a in (x, inp, W)), relu).cpu().numpy()
        e, bar = R.rel_err(got, want), max(FACTOR * e32, FLOOR)
        nb = R.dmpnn_update_branch(d)[0]
        WORST[nb] = max(WORST.get(nb, 0.0), e / bar)
        print("%s d %d NB %d rel_err %.3g e32 %.3g ratio %.3f" % (name, d, nb, e, e32, e / bar))
        assert got.shape == want.shape and e <= bar, (name, d, e, bar)


# ------------------------------------------------------------------------------------------------ strides
@pytest.mark.parametrize("d", [16, 33, 96, 320])
def test_strided_unaligned_operands_and_output(d):
    """x, input, weight and h as column slices of wider NaN-filled matrices (pads 5, 7, 3 and 6), each one float off a
    16-byte boundary: the values of the contiguous call exactly, the pads untouched."""
    b = batch("cap")
    B = b.n_bonds
    x, inp, W = (torch.tensor(a, device=DEV) for a in operands(B, d, d, exact=False))
    want = fused(b, x, inp, W, True)

    def wide(t, pad):
        w = torch.full((t.shape[0] + 1, d + pad), float("nan"), device=DEV)
        w[:t.shape[0], 1:1 + d] = t
        view = w[:t.shape[0], 1:1 + d]
        assert view.data_ptr() % 16 == 4 and view.stride(0) == d + pad
        return w, view

    (_, xs), (_, is_), (_, ws) = wide(x, 5), wide(inp, 7), wide(W, 3)
    out = torch.full((B + 1, d + 6), float("nan"), device=DEV)
    got = fused(b, xs, is_, ws, True, out=out[:B, 1:1 + d])
    assert torch.equal(got, want) and not bool(torch.isnan(got).any())
    o = out.cpu().numpy()
    assert np.isnan(o[:, 0]).all() and np.isnan(o[:, 1 + d:]).all() and np.isnan(o[B]).all()


# ------------------------------------------------------------------------------------------------ passes
def test_more_tiles_than_one_pass():
    """5 462 rings of 12 atoms: 131 088 bond rows, 4 097 tiles, one more than 2 048 workgroups of two waves hold."""
    d, n_rings, n = 8, 5462, 12
    mol_ptr, out_ptr, bond_src, rev = R.ring_arrays(n_rings, n)
    B = rev.shape[0]
    assert R.update_passes(B) == (4097, 2048, 2) and B > 2 * 2048 * 32
    b = DmpnnBatch.from_arrays(mol_ptr, out_ptr, bond_src, rev, np.zeros((n_rings * n, 1), np.float32),
                               np.zeros((B, 1), np.float32)).to(DEV)
    x, inp, W = operands(B, d, 3, exact=False)
    want = R.update_f64(x, inp, W, out_ptr, rev, True)
    e32 = R.rel_err(R.update_f32(x, inp, W, out_ptr, rev, True), want)
    out = torch.full((B + 1, d), float("nan"), device=DEV)
    got = fused(b, *(torch.tensor(a, device=DEV) for a in (x, inp, W)), True, out=out[:B]).cpu().numpy()
    e, bar = R.rel_err(got, want), max(FACTOR * e32, FLOOR)
    WORST[1] = max(WORST.get(1, 0.0), e / bar)
    print("passes rel_err %.3g e32 %.3g ratio %.3f; last tile %.3g" % (e, e32, e / bar, R.rel_err(got[-32:], want[-32:])))
    assert not np.isnan(got).any() and e <= bar and bool(torch.isnan(out[B]).all())
    # exact integers: the last tile (the second pass) bit for bit
    xi, ii, Wi = operands(B, d, 4, exact=True)
    goti = fused(b, *(torch.tensor(a, device=DEV) for a in (xi, ii, Wi)), False).cpu().numpy()
    assert np.array_equal(goti, R.update_f64(xi, ii, Wi, out_ptr, rev, False))


# ------------------------------------------------------------------------------------------------ the report
def test_zz_worst_ratio_per_nb():
    for nb in sorted(WORST):
        print("worst NB %2d %.3f" % (nb, WORST[nb]))
    print("largest ratio", max(WORST.values()) if WORST else None)
    assert not WORST or max(WORST.values()) <= 1.0
