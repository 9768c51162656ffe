"""The DTNN kernels (csrc/dtnn.hip) at their dispatch and tile edges: every template instantiation in both directions and
both input forms, pair lists that are not whole molecules, the grid caps, leading dimensions / alignment / accumulation
through the C ABI, and the device collation at every ``chunk`` of its offsets kernel.

Bar, per tensor (Y, d_ah, dW_df, db_df, dW_fc): ``rel_err <= max(4 * max(e32, e_order), 1e-6)``, errors relative to the
tensor's largest entry in the float64 restatement (dtnn_refs.pair_f64).  ``e32`` is the error of the SAME restatement run
in float32 on the CPU (dtnn_refs.pair_f32, at one thread: its scatter-adds are repeatable at no other count) on the same
case, computed here; the factor 4 over a float32 yardstick is the one test_model_fit_follows_the_reference uses.
``e_order`` (dtnn_refs.pair_e_order) is what float32 accumulation, one addend after another in 8 seeded random orders,
makes of the float64 addends the kernel adds with float atomics: Y per (run, tile), d_ah per pair, dW_df / db_df / dW_fc
per persistent wave.  torch's float32 sums are blocked, so ``e32`` alone says nothing about a chain of 2 000 atomics in
arrival order; ``e_order`` is that part of the yardstick, from the reference alone, and on short pair lists it lies below
``e32``.  The floor is 2.5 x the 4e-7 recorded for these kernels on the MI355X when
they were added, and stands for the ASSUMPTION that the device's ``tanhf`` / ``exp2f`` are accurate to a few ulp: where the
CPU's float32 run happens to be nearly exact the kernel is still allowed float32 rounding of its transcendental
functions.  Every check prints ``rel_err / bar``; the worst per tensor and instantiation is printed by the last test.
"""
import numpy as np
import pytest
import torch

from deepchem_amd import _lib, ops
from deepchem_amd.models.torch_models.dtnn_layers import DtnnPairFn, PairPlan
from tests import dtnn_refs as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FLOOR, FACTOR = 1e-6, 4.0
DMIN, DMAX = -1.0, 18.0
FORMS = (True, False)  # distances; Gaussian matrix

# (E, H, K): every (nth, nte) with E, H in {1, 32, 33, 64}, then the K sweep at (33, 32)
WIDTHS = [(1, 1, 1), (32, 32, 16), (33, 32, 17), (64, 32, 128), (32, 33, 15), (64, 64, 128), (33, 33, 100)]
K_SWEEP = [(33, 32, K) for K in (31, 32, 33, 64, 65, 96, 97)]
LIST_WIDTHS = [(33, 32, 17), (64, 64, 128)]
N_LIST = 12
CAP_CASES = {"cap": (4, 8, 6, 4097 * 32 - 5, 64), "wide_rounds": (64, 32, 128, 16 * 256 * 32 // 8, 64)}  # E, H, K, P, N
WORST = {}


def wid(w):
    return "E%dH%dK%d" % w


def lists():
    """name -> (runs, same_j) at N = 12."""
    rng = np.random.RandomState(7)
    out = {"P%d" % P: (R.random_runs(P, N_LIST, rng), None) for P in (1, 31, 32, 33, 64, 65)}
    out["run70"] = ([(5, 70)], None)
    out["runs32_32_1"] = ([(2, 32), (6, 32), (9, 1)], None)
    out["atoms3_7"] = ([(3, 40), (7, 25)], None)
    out["same_j"] = (R.random_runs(65, N_LIST, rng), 4)
    out["last_atom"] = ([(N_LIST - 1, 45)], None)
    return out


LISTS = lists()


def bar_of(e32, e_order):
    return max(FACTOR * max(e32, e_order), FLOOR)


def references(c, K):
    """Per input form: (float64 restatement, e32 per tensor, e_order per tensor).  Form (b) is handed the
    float32-rounded Gaussian matrix, so its references start from that matrix; form (a)'s float32 yardstick generates
    its Gaussians in float32."""
    g64 = R.gaussians(c["d"].astype(np.float64), DMIN, DMAX, K, torch.float64)
    g32 = g64.to(torch.float32)
    want_a, want_b = R.pair_f64(g64, c), R.pair_f64(g32, c)
    f32_a = R.pair_f32(R.gaussians(c["d"], DMIN, DMAX, K, torch.float32), c)
    f32_b = R.pair_f32(g32, c)
    return {True: (want_a, {k: R.rel_err(f32_a[k], want_a[k]) for k in want_a}, R.pair_e_order(g64, c, want_a)),
            False: (want_b, {k: R.rel_err(f32_b[k], want_b[k]) for k in want_b}, R.pair_e_order(g32, c, want_b))}, g32


def native(c, src, from_distance, step):
    t = {k: torch.tensor(c[k], device=DEV, requires_grad=True) for k in ("ah", "W_df", "b_df", "W_fc")}
    plan = PairPlan.checked(src, from_distance, c["mem_i"], c["mem_j"], c["N"], torch.device(DEV),
                            DMIN if from_distance else 0.0, step if from_distance else 1.0)
    y = DtnnPairFn.apply(t["ah"], t["W_df"], t["b_df"], t["W_fc"], plan)
    y.backward(torch.tensor(c["dY"], device=DEV))
    out = {"Y": y.detach().cpu().numpy()}
    out.update({"d_" + k: v.grad.cpu().numpy() for k, v in t.items()})
    return out


def judge(label, E, H, K, from_distance, got, want, e32, e_order):
    """Every tensor within the bar; prints rel_err / bar and keeps the worst per (instantiation, tensor)."""
    nth, nte, _, _ = R.dtnn_branch(E, H, K, from_distance)
    fails = []
    for k in R.PAIR_TENSORS:
        assert got[k].shape == want[k].shape, (label, k)
        e, bar = R.rel_err(got[k], want[k]), bar_of(e32[k], e_order[k])
        key = ("d" if from_distance else "g", nth, nte, k)
        WORST[key] = max(WORST.get(key, 0.0), e / bar)
        print("%s %s<%d,%d> %s rel_err %.3g e32 %.3g e_order %.3g ratio %.3f" % (label, key[0], nth, nte, k, e, e32[k],
                                                                                 e_order[k], e / bar))
        if not e <= bar:
            fails.append((k, e, bar))
    assert not fails, (label, fails)


def run_case(label, c, E, H, K):
    step = (DMAX - DMIN) / K
    refs, g32 = references(c, K)
    out = {}
    for form in FORMS:
        src = torch.tensor(c["d"], device=DEV) if form else g32.to(DEV)
        out[form] = native(c, src, form, step)
        judge(label, E, H, K, form, out[form], *refs[form])
    return out, refs


def small_lists(E, H, K, seed):
    """Three pair lists of at most 100 pairs over 9 atoms: random runs, one run across four tiles, single pairs."""
    rng = np.random.RandomState(seed)
    return [R.random_runs(97, 9, rng), [(0, 3), (4, 95), (8, 2)], [(a, 1) for a in range(0, 9, 2)]]


# ------------------------------------------------------------------------------------------------ coverage of the tables
def test_case_tables_reach_every_instantiation_and_k_step():
    """8 instantiations (from_distance x nth x nte) per direction: every case runs both forms, forward and backward, so
    the widths must reach all four (nth, nte); the sweep every KT = 1..4 and KS = 2..7; both cap cases sit above the cap
    they are meant for."""
    reached = {(f,) + R.dtnn_branch(E, H, K, f)[:2] for E, H, K in WIDTHS + K_SWEEP for f in FORMS}
    assert reached == {(f, th, te) for f in FORMS for th in (1, 2) for te in (1, 2)} and len(reached) == 8
    assert {R.dtnn_branch(*w, True)[:2] for w in LIST_WIDTHS} == {(1, 2), (2, 2)}
    assert {R.dtnn_branch(*w, True)[3] for w in K_SWEEP} == {1, 2, 3, 4}
    assert {R.dtnn_branch(*w, True)[2] for w in K_SWEEP} == {2, 3, 4, 5, 6, 7}
    E, H, K, P, _ = CAP_CASES["cap"]
    for backward in (False, True):
        grid, uncapped, tiles, rounds = R.dtnn_grid(P, backward)
        assert tiles == 4097 and uncapped > grid == (R.BWD_GRID_CAP if backward else R.FWD_GRID_CAP)
        assert rounds == (5 if backward else 3)  # one wave takes a tile more than the others
    E, H, K, P, _ = CAP_CASES["wide_rounds"]
    assert R.dtnn_branch(E, H, K, True)[:2] == (1, 2) and R.dtnn_grid(P, True)[2:] == (512, 4)
    tiles = lambda runs: [(sum(n for _, n in runs[:k]) // 32, (sum(n for _, n in runs[:k + 1]) - 1) // 32)  # noqa: E731
                          for k in range(len(runs))]
    assert max(b - a for a, b in tiles(LISTS["run70"][0])) == 2                # a run over three tiles
    assert [b for _, b in tiles(LISTS["runs32_32_1"][0])] == [0, 1, 2]          # runs that end on tile edges
    assert sorted(sum(n for _, n in v[0]) for k, v in LISTS.items() if k.startswith("P")) == [1, 31, 32, 33, 64, 65]


# ------------------------------------------------------------------------------------------------ widths
@pytest.mark.parametrize("widths", WIDTHS + K_SWEEP, ids=wid)
def test_every_width_both_forms_both_directions(widths):
    E, H, K = widths
    for n, runs in enumerate(small_lists(E, H, K, E + H + K)):
        rng = np.random.RandomState(100 * n + K)
        mem_i, mem_j = R.pair_list(runs, 9, rng)
        assert mem_i.shape[0] <= 100
        run_case("%s list%d" % (wid(widths), n), R.pair_case(mem_i, mem_j, 9, E, H, K, rng), E, H, K)


# ------------------------------------------------------------------------------------------------ pair lists
@pytest.mark.parametrize("widths", LIST_WIDTHS, ids=wid)
@pytest.mark.parametrize("name", sorted(LISTS))
def test_pair_lists_that_are_not_whole_molecules(name, widths):
    E, H, K = widths
    runs, same_j = LISTS[name]
    rng = np.random.RandomState(len(name) + K)
    mem_i, mem_j = R.pair_list(runs, N_LIST, rng, same_j=same_j)
    c = R.pair_case(mem_i, mem_j, N_LIST, E, H, K, rng)
    out, refs = run_case(name + " " + wid(widths), c, E, H, K)
    with_pairs = np.zeros(N_LIST, bool)
    with_pairs[mem_i] = True
    assert name != "atoms3_7" or np.nonzero(with_pairs)[0].tolist() == [3, 7]
    for form in FORMS:
        assert not out[form]["Y"][~with_pairs].any()  # atoms without pairs: exactly 0.0
        touched = np.zeros(N_LIST, bool)
        touched[mem_j] = True
        assert not out[form]["d_ah"][~touched].any()
        if same_j is not None:
            assert np.nonzero(touched)[0].tolist() == [same_j] and out[form]["d_ah"][same_j].any()


@pytest.mark.parametrize("widths", LIST_WIDTHS, ids=wid)
def test_no_pairs_with_atoms(widths):
    """P = 0, N > 0: Y and d_ah exactly zero (the launcher clears them), the added-into buffers untouched."""
    E, H, K = widths
    rng = np.random.RandomState(K)
    empty = np.zeros(0, np.int64)
    c = R.pair_case(empty, empty, N_LIST, E, H, K, rng)
    t = {k: torch.tensor(c[k], device=DEV) for k in ("ah", "W_df", "b_df", "W_fc", "dY")}
    mi = torch.zeros(0, dtype=torch.int32, device=DEV)
    for form in FORMS:
        src = torch.zeros(0, device=DEV) if form else torch.zeros((0, K), device=DEV)
        y = ops.dtnn_pair_fwd(src, form, mi, mi, t["ah"], t["W_df"], t["b_df"], t["W_fc"], DMIN, 0.19)
        bufs = [torch.full(s, 1.5, device=DEV) for s in ((K, H), (H,), (H, E))]
        dah = ops.dtnn_pair_bwd(src, form, mi, mi, t["ah"], t["W_df"], t["b_df"], t["W_fc"], DMIN, 0.19, t["dY"], *bufs)
        assert y.shape == (N_LIST, E) and dah.shape == (N_LIST, H)
        assert not bool(y.any()) and not bool(dah.any()) and all(bool((b == 1.5).all()) for b in bufs)


# ------------------------------------------------------------------------------------------------ grid caps
@pytest.mark.parametrize("name", sorted(CAP_CASES))
def test_grid_cap_and_many_rounds(name):
    """"cap": 4 097 tiles, above both caps (512 x 8 forward, 256 x 16 backward): one wave walks a third / fifth tile.
    "wide_rounds": the widest (1, 2) shape over four backward rounds of every wave."""
    E, H, K, P, N = CAP_CASES[name]
    rng = np.random.RandomState(P % 1000)
    mem_i, mem_j = R.pair_list(R.random_runs(P, N, rng), N, rng)
    assert mem_i.shape[0] == P
    run_case(name, R.pair_case(mem_i, mem_j, N, E, H, K, rng), E, H, K)


# ------------------------------------------------------------------------------------------------ the C ABI: ld, alignment
def off_boundary(rows, cols, pad, fill=None, values=None):
    """A (rows, cols) column slice of a wider matrix that starts one float off a 16-byte boundary (the scalar loads)."""
    wide = torch.full((rows, cols + pad), float("nan") if fill is None else fill, device=DEV)
    view = wide[:, 1:1 + cols]
    if values is not None:
        view.copy_(torch.as_tensor(values, device=DEV))
    assert view.data_ptr() % 16 == 4 or rows == 0
    return wide, view


def raw_call(c, E, H, K, form, src, ld_src, ah, ldah, dy, lddy, ldy, lddah, prefill):
    """gcmi_dtnn_pair_fwd / _bwd on caller-owned outputs: Y (N + 1, ldy) and d_ah (N + 1, lddah) prefilled with NaN (one
    guard row), the three added-into buffers prefilled with ``prefill``."""
    N, P = c["N"], c["mem_i"].shape[0]
    t = {k: torch.tensor(c[k], device=DEV) for k in ("W_df", "b_df", "W_fc")}
    mi, mj = (torch.tensor(c[k].astype(np.int32), device=DEV) for k in ("mem_i", "mem_j"))
    step = (DMAX - DMIN) / K
    args = (ops._ptr(src), ld_src, 1 if form else 0, ops._ptr(mi), ops._ptr(mj), P, N, ops._ptr(ah), ldah, H,
            ops._ptr(t["W_df"]), ops._ptr(t["b_df"]), K, ops._ptr(t["W_fc"]), E, DMIN if form else 0.0, step if form else 1.0)
    Y = torch.full((N + 1, ldy), float("nan"), device=DEV)
    dah = torch.full((N + 1, lddah), float("nan"), device=DEV)
    bufs = [torch.tensor(p, device=DEV) for p in prefill]
    _lib.call("gcmi_dtnn_pair_fwd", *args, ops._ptr(Y), ldy, ops._stream())
    _lib.call("gcmi_dtnn_pair_bwd", *args, ops._ptr(dy), lddy, ops._ptr(dah), lddah, ops._ptr(bufs[0]), ops._ptr(bufs[1]),
              ops._ptr(bufs[2]), ops._stream())
    torch.cuda.synchronize()
    return Y.cpu().numpy(), dah.cpu().numpy(), [b.cpu().numpy() for b in bufs]


@pytest.mark.parametrize("widths", LIST_WIDTHS, ids=wid)
def test_leading_dimensions_alignment_and_accumulation(widths):
    """ldy = E + 3 and lddah = H + 5 with NaN around the outputs; ah, dY and the Gaussian matrix once as slices one float
    off a 16-byte boundary (scalar loads) and once contiguous (vector loads wherever the width allows); dW_df, db_df and
    dW_fc added into non-zero buffers."""
    E, H, K = widths
    rng = np.random.RandomState(E)
    runs = R.random_runs(65, N_LIST, rng)
    assert max(n for _, n in runs) <= 32  # every Y row gets at most two atomic contributions: the sum is order-free
    mem_i, mem_j = R.pair_list(runs, N_LIST, rng)
    c = R.pair_case(mem_i, mem_j, N_LIST, E, H, K, rng)
    N, P = N_LIST, 65
    refs, g32 = references(c, K)
    prefill = [rng.choice(np.array([-1.0, -0.5, 0.25, 0.5, 1.0], np.float32), s) for s in ((K, H), (H,), (H, E))]
    ldy, lddah = E + 3, H + 5
    for form in FORMS:
        want, e32, e_order = refs[form]
        results = {}
        for layout in ("off", "aligned"):
            if layout == "off":
                _, ah = off_boundary(N, H, 7, values=c["ah"])
                _, dy = off_boundary(N, E, 6, values=c["dY"])
                _, g = off_boundary(P, K, 9, values=g32)
                ldah, lddy, ldg = H + 7, E + 6, K + 9
            else:
                ah, dy, g = torch.tensor(c["ah"], device=DEV), torch.tensor(c["dY"], device=DEV), g32.to(DEV)
                ldah, lddy, ldg = H, E, K
                assert ah.data_ptr() % 16 == 0 and dy.data_ptr() % 16 == 0 and g.data_ptr() % 16 == 0
            src, ld_src = (torch.tensor(c["d"], device=DEV), 1) if form else (g, ldg)
            Y, dah, bufs = raw_call(c, E, H, K, form, src, ld_src, ah, ldah, dy, lddy, ldy, lddah, prefill)
            assert np.isnan(Y[:N, E:]).all() and np.isnan(Y[N]).all() and not np.isnan(Y[:N, :E]).any()
            assert np.isnan(dah[:N, H:]).all() and np.isnan(dah[N]).all() and not np.isnan(dah[:N, :H]).any()
            got = {"Y": Y[:N, :E], "d_ah": dah[:N, :H]}
            got.update({k: bufs[n].astype(np.float64) - prefill[n] for n, k in enumerate(("d_W_df", "d_b_df", "d_W_fc"))})
            judge("ld %s %s" % (layout, wid(widths)), E, H, K, form, got, want, e32, e_order)
            results[layout] = got
        assert np.array_equal(results["off"]["Y"], results["aligned"]["Y"])
    if widths == (64, 64, 128):
        assert H % 4 == 0 and E % 4 == 0 and K % 4 == 0  # "aligned" took every vector path


# ------------------------------------------------------------------------------------------------ collation
def resident(A, M, seed):
    rng = np.random.RandomState(seed)
    n_all = rng.randint(1, A + 1, M)
    n_all[:2] = (1, A)
    z_all = rng.randint(1, 30, (M, A)).astype(np.int32)
    dist_all = rng.uniform(0.5, 12.0, (M, A, A)).astype(np.float32)
    return n_all, z_all, dist_all, rng


def on_device(n_all, z_all, dist_all):
    return (torch.tensor(z_all, device=DEV), torch.tensor(dist_all, device=DEV),
            torch.tensor(n_all.astype(np.int32), device=DEV))


def same_arrays(got, want):
    names = ("atom_off", "pair_off", "z", "d", "mem_i", "mem_j")
    for k, g, w in zip(names, got, want):
        g = g.cpu().numpy() if torch.is_tensor(g) else g
        assert g.dtype == w.dtype and np.array_equal(g, w), k


@pytest.mark.parametrize("A", [5, 64])
@pytest.mark.parametrize("B", [1, 255, 256, 257, 513, 1000])
def test_collate_equals_the_host_at_every_chunk(B, A):
    """chunk = ceil(B / 256) = 1, 1, 1, 2, 3, 4 entries per thread of the offsets kernel; repeats in mol_idx."""
    M = 40
    n_all, z_all, dist_all, rng = resident(A, M, 1000 * A + B)
    mol_idx = rng.randint(0, M, B)
    assert B < 4 or len(set(mol_idx.tolist())) < B
    assert ((B + 255) // 256 > 1) == (B > 256)
    want = R.collate_ref(z_all, dist_all, n_all, mol_idx)
    zd, dd, nd = on_device(n_all, z_all, dist_all)
    got = ops.dtnn_collate(zd, dd, nd, torch.tensor(mol_idx.astype(np.int32), device=DEV), int(want[0][-1]), int(want[1][-1]))
    same_arrays(got, want)


@pytest.mark.parametrize("B", [7, 513])
def test_collate_skips_invalid_entries(B):
    """mol_idx of -1 or M: no atoms, no pairs, the offsets repeat -- on the chunk = 1 and the chunk > 1 walk."""
    A, M = 9, 12
    n_all, z_all, dist_all, rng = resident(A, M, B)
    mol_idx = rng.randint(0, M, B)
    mol_idx[[0, B // 2, B - 1]] = (-1, M, -1)
    mol_idx[1] = M
    want = R.collate_ref(z_all, dist_all, n_all, mol_idx)
    assert want[0][1] == 0 and want[0][-1] == want[0][-2] and want[0][B // 2] == want[0][B // 2 + 1]
    zd, dd, nd = on_device(n_all, z_all, dist_all)
    got = ops.dtnn_collate(zd, dd, nd, torch.tensor(mol_idx.astype(np.int32), device=DEV), int(want[0][-1]), int(want[1][-1]))
    same_arrays(got, want)


@pytest.mark.parametrize("short", ["atoms", "pairs"])
def test_collate_capacity_guards(short):
    """A capacity one short of the batch: the molecule that does not fit writes nothing, the others are whole, and the
    elements after the stated capacity keep their fill (a raw call on slices of larger buffers)."""
    A, M, B = 9, 12, 300
    n_all, z_all, dist_all, rng = resident(A, M, 5)
    mol_idx = rng.randint(0, M, B)
    mol_idx[-1] = 1  # the last molecule has A atoms
    want = R.collate_ref(z_all, dist_all, n_all, mol_idx)
    n_atoms, n_pairs = int(want[0][-1]), int(want[1][-1])
    cap_a, cap_p = (n_atoms - 1, n_pairs) if short == "atoms" else (n_atoms, n_pairs - 1)
    zd, dd, nd = on_device(n_all, z_all, dist_all)
    idx = torch.tensor(mol_idx.astype(np.int32), device=DEV)
    guard = 64
    z = torch.full((n_atoms + guard,), -1, dtype=torch.int32, device=DEV)
    d = torch.full((n_pairs + guard,), float("nan"), device=DEV)
    mem_i = torch.full((n_pairs + guard,), -1, dtype=torch.int32, device=DEV)
    mem_j = torch.full((n_pairs + guard,), -1, dtype=torch.int32, device=DEV)
    z[:cap_a], d[:cap_p], mem_i[:cap_p], mem_j[:cap_p] = 0, 0, 0, 0  # the zero fill ops.dtnn_collate hands over
    atom_off = torch.full((B + 2,), -1, dtype=torch.int32, device=DEV)
    pair_off = torch.full((B + 2,), -1, dtype=torch.int32, device=DEV)
    _lib.call("gcmi_dtnn_collate", ops._ptr(zd), ops._ptr(dd), ops._ptr(nd), M, A, ops._ptr(idx), B, cap_a, cap_p,
              ops._ptr(atom_off), ops._ptr(pair_off), ops._ptr(z), ops._ptr(d), ops._ptr(mem_i), ops._ptr(mem_j), ops._stream())
    torch.cuda.synchronize()
    assert np.array_equal(atom_off.cpu().numpy()[:B + 1], want[0]) and int(atom_off[B + 1]) == -1
    assert np.array_equal(pair_off.cpu().numpy()[:B + 1], want[1]) and int(pair_off[B + 1]) == -1
    a0, q0 = int(want[0][B - 1]), int(want[1][B - 1])  # where the last molecule would have gone
    z, d, mem_i, mem_j = (t.cpu().numpy() for t in (z, d, mem_i, mem_j))
    assert np.array_equal(z[:a0], want[2][:a0]) and not z[a0:cap_a].any() and np.all(z[cap_a:] == -1)
    assert np.array_equal(d[:q0], want[3][:q0]) and not d[q0:cap_p].any() and np.isnan(d[cap_p:]).all()
    for got, full in ((mem_i, want[4]), (mem_j, want[5])):
        assert np.array_equal(got[:q0], full[:q0]) and not got[q0:cap_p].any() and np.all(got[cap_p:] == -1)


# ------------------------------------------------------------------------------------------------ the report
def test_zz_worst_ratio_per_instantiation_and_tensor():
    """Prints what the cases above measured (rel_err / bar, at most 1 by their assertions)."""
    for key in sorted(WORST):
        print("worst %s<%d,%d> %-7s %.3f" % (key + (WORST[key],)))
    print("largest ratio", max(WORST.values()) if WORST else None)
    assert not WORST or max(WORST.values()) <= 1.0
