"""tests/yardstick.py and the yardsticks built on it, without a device ("Float32 yardsticks: reproducible and
order-aware"): ``any_order_e32`` is a fixed number that bounds what further orders give; the DTNN addends of
``dtnn_refs.pair_addends`` add up to the float64 restatement; every float32 restatement that got a thread pin returns
the same bits whatever the ambient thread count; and the figures of the DTNN cap case are printed.
"""
import numpy as np
import pytest
import torch

from tests import dmpnn_refs as M
from tests import dtnn_refs as R
from tests.yardstick import any_order_e32, f32_threads, restatement_threads

DMIN, DMAX = -1.0, 18.0
CAP = (4, 8, 6, 4097 * 32 - 5, 64)  # (E, H, K, P, N) of tests/test_gpu_dtnn_edges.py::test_grid_cap_and_many_rounds[cap]
AMBIENT = (1, 16)


def under(n, fn):
    """``fn()`` with the ambient thread count ``n``, as a host with that many threads would run it."""
    prev = torch.get_num_threads()
    torch.set_num_threads(n)
    try:
        return fn()
    finally:
        torch.set_num_threads(prev)


def flat(x, out=None, pre=""):
    """Every array / tensor / number inside nested dicts, lists and tuples, by path."""
    out = {} if out is None else out
    if isinstance(x, dict):
        for k in sorted(x, key=str):
            flat(x[k], out, pre + str(k) + "/")
    elif isinstance(x, (list, tuple)):
        for n, v in enumerate(x):
            flat(v, out, pre + str(n) + "/")
    elif torch.is_tensor(x):
        out[pre] = x.detach().numpy().copy()
    elif isinstance(x, (np.ndarray, float, np.floating)):
        out[pre] = np.array(x)
    return out


def same_bits_at_every_ambient_count(fn, label):
    runs = [flat(under(n, fn)) for n in AMBIENT]
    assert runs[0] and sorted(runs[0]) == sorted(runs[1]), label
    for k in runs[0]:
        assert runs[0][k].dtype == runs[1][k].dtype and runs[0][k].tobytes() == runs[1][k].tobytes(), (label, k)


def pair_case(E, H, K, P, N, seed):
    rng = np.random.RandomState(seed)
    mem_i, mem_j = R.pair_list(R.random_runs(P, N, rng), N, rng)
    c = R.pair_case(mem_i, mem_j, N, E, H, K, rng)
    g64 = R.gaussians(c["d"].astype(np.float64), DMIN, DMAX, K, torch.float64)
    return c, g64


_CAP = {}


def cap_case():
    """The cap case as the GPU test builds it, with its float64 restatements, e32 and e_order per input form."""
    if not _CAP:
        E, H, K, P, N = CAP
        c, g64 = pair_case(E, H, K, P, N, P % 1000)
        g32 = g64.to(torch.float32)
        for form, g, g_f32 in (("distances", g64, R.gaussians(c["d"], DMIN, DMAX, K, torch.float32)), ("matrix", g32, g32)):
            want = R.pair_f64(g, c)
            f32 = R.pair_f32(g_f32, c)
            _CAP[form] = dict(c=c, g=g, g_f32=g_f32, want=want, e32={k: R.rel_err(f32[k], want[k]) for k in want},
                              e_order=R.pair_e_order(g, c, want))
    return _CAP


# ------------------------------------------------------------------------------------------------ f32_threads
def test_f32_threads_sets_and_restores_the_count():
    before = torch.get_num_threads()
    with f32_threads(3):
        assert torch.get_num_threads() == 3
        with restatement_threads(torch.float64, 1):
            assert torch.get_num_threads() == 3
        with restatement_threads(torch.float32, 1):
            assert torch.get_num_threads() == 1
        assert torch.get_num_threads() == 3
    with pytest.raises(KeyError):
        with f32_threads(2):
            raise KeyError("restored after an exception too")
    assert torch.get_num_threads() == before


# ------------------------------------------------------------------------------------------------ any_order_e32
def test_any_order_e32_is_zero_where_every_order_is_exact_and_seed_stable():
    rng = np.random.RandomState(1)
    quarters = rng.randint(-8, 9, (3000, 5)) / 4.0  # every partial sum is a multiple of 1/4 below 2^24 / 4: exact
    rows = rng.randint(0, 7, 3000)
    assert any_order_e32(quarters, rows, 7, 1.0) == 0.0
    x = rng.standard_normal((3000, 5))
    a, b = any_order_e32(x, rows, 7, 2.0, seed=5), any_order_e32(x, rows, 7, 2.0, seed=5)
    assert a == b and a > 0.0
    assert any_order_e32(x, rows, 7, 1.0, seed=5) == 2.0 * a  # relative to ``scale``
    assert any_order_e32(x, rows, 7, 2.0, orders=1, seed=5) <= a  # the first of the same 8 orders
    assert any_order_e32(np.zeros((0, 4)), np.zeros(0, np.int64), 3, 1.0) == 0.0
    with pytest.raises(ValueError):
        any_order_e32(x, rows + 1, 7, 1.0)  # a row outside [0, 7)
    with pytest.raises(ValueError):
        any_order_e32(x, rows, 7, 0.0)


def test_any_order_e32_adds_strictly_one_after_another():
    """2^24 + 1 + 1 in float32 is 2^24 when the ones arrive after the large term and 2^24 + 2 when they arrive first:
    the worst of the orders is the full 2, which a blocked or pairwise sum would not show."""
    x = np.array([[2.0 ** 24], [1.0], [1.0]])
    assert any_order_e32(x, np.zeros(3, np.int64), 1, 1.0, orders=8) == 2.0


def test_eight_orders_bound_what_further_orders_give():
    """4 096 standard-normal addends into one element: each of 32 further orders stays under 4 times what 8 orders gave,
    the factor the bars put on the yardstick."""
    x = np.random.RandomState(0).standard_normal((4096, 1))
    rows = np.zeros(4096, np.int64)
    e8 = any_order_e32(x, rows, 1, 1.0, orders=8, seed=0)
    further = [any_order_e32(x, rows, 1, 1.0, orders=1, seed=s) for s in range(100, 132)]
    print("8 orders %.3g; 32 further orders %.3g .. %.3g" % (e8, min(further), max(further)))
    assert e8 > 0.0 and max(further) < 4.0 * e8


# ------------------------------------------------------------------------------------------------ DTNN addends
# 1e-12 of the largest entry: float64 rounding of sums of up to 131 099 terms in two different orders is about
# sqrt(P) 2^-53 = 4e-14 of the sum of magnitudes; a wrong or missing addend shows at 1e-6 or more
COMPOSE_TOL = 1e-12
SMALL = [(33, 32, 17, 97, 9), (64, 64, 128, 65, 12), (1, 1, 1, 33, 3), (4, 8, 6, 5000, 7)]


def check_composition(c, g, want, label):
    got = R.composed(R.pair_addends(g, c))
    for k in R.PAIR_TENSORS:
        e = R.rel_err(got[k].reshape(want[k].shape), want[k])
        print("%s %s: addends against pair_f64 %.3g" % (label, k, e))
        assert e <= COMPOSE_TOL, (label, k, e)


@pytest.mark.parametrize("case", SMALL, ids=lambda t: "E%dH%dK%dP%dN%d" % t)
def test_dtnn_addends_compose_to_the_float64_restatement(case):
    E, H, K, P, N = case
    c, g64 = pair_case(E, H, K, P, N, P)
    for form, g in (("distances", g64), ("matrix", g64.to(torch.float32))):
        check_composition(c, g, R.pair_f64(g, c), form)
    add = R.pair_addends(g64, c)
    grid, _, tiles, _ = R.dtnn_grid(P, True)
    assert add["d_ah"][0].shape == (P, H) and add["d_b_df"][0].shape == (grid * R.DTNN_WAVES, H)
    assert add["d_W_df"][0].shape == (grid * R.DTNN_WAVES, K * H) and add["d_W_fc"][0].shape == (grid * R.DTNN_WAVES, H * E)
    assert tiles <= add["Y"][0].shape[0] <= tiles + len(np.unique(c["mem_i"]))  # one per (run, tile)


def test_dtnn_addends_of_the_cap_case_compose_and_follow_the_grids():
    cap = cap_case()
    E, H, K, P, N = CAP
    for form, r in cap.items():
        check_composition(r["c"], r["g"], r["want"], "cap " + form)
    g, c = cap["matrix"]["g"], cap["matrix"]["c"]
    add = R.pair_addends(g, c)
    assert R.dtnn_grid(P, True)[0] == R.BWD_GRID_CAP and add["d_b_df"][0].shape[0] == 1024  # one partial per wave
    # an uncapped backward grid (257 workgroups) would spread the same sums over 1 028 waves
    wider = R.pair_addends(g, c, grids=(R.dtnn_grid(P, False), (257, 257, 4097, 4)))
    assert wider["d_b_df"][0].shape[0] == 1028 and np.allclose(wider["d_b_df"][0].sum(0), add["d_b_df"][0].sum(0), rtol=1e-12)
    assert not np.array_equal(wider["d_b_df"][0][:1024], add["d_b_df"][0])
    with pytest.raises(ValueError):
        R.pair_addends(g, c, grids=(R.dtnn_grid(P - 64, False), R.dtnn_grid(P - 64, True)))


def test_cap_case_yardsticks_are_printed_and_above_the_old_bar_where_the_kernel_chains():
    """The figures DESIGN.md records.  d_ah (one atomic per pair, about 2 000 per element) and d_b_df (1 024 per-wave
    partials per element) are the two tensors whose order term exceeds their blocked float32 sum's error."""
    cap = cap_case()
    for form, r in cap.items():
        for k in R.PAIR_TENSORS:
            print("cap %-9s %-7s e32 %.3g e_order %.3g" % (form, k, r["e32"][k], r["e_order"][k]))
        assert r["e_order"]["d_ah"] > r["e32"]["d_ah"] and r["e_order"]["d_b_df"] > r["e32"]["d_b_df"]
        assert r["e_order"]["Y"] < r["e32"]["Y"]  # 64 partials per row: the arithmetic inside a partial dominates
        again = R.pair_e_order(r["g"], r["c"], r["want"])
        assert again == r["e_order"]  # seeded: a fixed number


# ------------------------------------------------------------------------------------------------ pinned restatements
def test_pair_f32_returns_the_same_bits_at_every_ambient_count():
    r = cap_case()["matrix"]
    same_bits_at_every_ambient_count(lambda: R.pair_f32(r["g_f32"], r["c"]), "pair_f32 cap")


def test_update_f32_returns_the_same_bits_at_every_ambient_count():
    _, out_ptr, _, rev = M.ring_arrays(700, 12)
    rng = np.random.RandomState(3)
    x, inp = (rng.normal(0, 1, (rev.shape[0], 33)).astype(np.float32) for _ in range(2))
    W = rng.normal(0, 1 / np.sqrt(33), (33, 33)).astype(np.float32)
    same_bits_at_every_ambient_count(lambda: M.update_f32(x, inp, W, out_ptr, rev, True), "update_f32")


def test_megnet_restatements_return_the_same_bits_at_every_ambient_count():
    import tests.test_gpu_megnet as T

    def case():
        T._CASES.pop(("edge", True), None)
        return T.kernel_case("edge", True)["f32"]
    same_bits_at_every_ambient_count(case, "megnet kernel_case edge")
    T._CASES.pop(("edge", True), None)


def test_cgcnn_restatements_return_the_same_bits_at_every_ambient_count():
    import tests.test_gpu_cgcnn as T
    from tests.test_cgcnn_host import case_batch

    def case():
        T._CASES.pop(("edge", 128, True, 0.0), None)
        return T.kernel_case("edge", 128, True)["f32"]
    same_bits_at_every_ambient_count(case, "cgcnn kernel_case edge")
    T._CASES.pop(("edge", 128, True, 0.0), None)
    c = case_batch("edge", True, True, 128, 41)
    c.update({k: np.asarray(c[k], np.float32) for k in ("h", "e", "cot", "rm0", "rv0")})
    c["params"] = {k: np.asarray(v, np.float32) for k, v in c["params"].items()}
    same_bits_at_every_ambient_count(lambda: [T.layer_f32(c)[0], T.layer_f32(c)[2]], "cgcnn layer")


def test_lcnn_restatements_return_the_same_bits_at_every_ambient_count():
    import tests.test_gpu_lcnn as T
    c = T.make_inputs("O64", True)
    same_bits_at_every_ambient_count(lambda: T.references(c)[1], "lcnn O64 e32")


def test_acnn_restatement_returns_the_same_bits_at_every_ambient_count():
    import tests.test_gpu_acnn as T
    import tests.test_gpu_acnn_edges as TE
    X, nbrs, Z, params, types, cot = TE.case_inputs(2, 16400, 1, 1, "none")
    same_bits_at_every_ambient_count(lambda: T.restated_f32(X, nbrs, Z, params, types, None, cot), "acnn N16400")


def oracle_batch_1024():
    from deepchem_amd.utils.synthetic import synthetic_labels, synthetic_molecules
    from oracle import graphconv_oracle as O
    packed = synthetic_molecules(1024, seed=11)
    y, w = synthetic_labels(packed.n_mols, 12, "classification", 11, pos_rate=0.3)
    return packed, y, w, O.init_state(O.ModelConfig(12, batch_size=packed.n_mols), 17)


def same_forward_bits_and_close_gradients(fn, label):
    """(loss, outputs, gradients) of an oracle step under both ambient counts: the forward bit for bit; the gradients,
    whose float32 scatter-adds land in arrival order at any count above one, within 1e-5 of each tensor's largest
    entry (sums of up to 2e4 rows: sqrt(2e4) 2^-24 = 8e-6 of a typical term; a route that flipped would show in the
    forward first, and unpinned the two counts differ by 1e-3 and more)."""
    a, b = (under(n, fn) for n in AMBIENT)
    fa, fb = flat([a[0], a[1]]), flat([b[0], b[1]])
    assert fa and all(fa[k].tobytes() == fb[k].tobytes() for k in fa), label
    for k in a[2]:
        x, y = np.asarray(a[2][k], np.float64), np.asarray(b[2][k], np.float64)
        assert np.max(np.abs(x - y)) <= 1e-5 * max(np.max(np.abs(x)), 1e-30), (label, k)


def test_float32_oracle_steps_do_not_follow_the_ambient_count():
    """The float32 oracle step of tests/test_gpu_scale.py and of tests/test_gpu_bf16_stream.py (pinned to 16 threads,
    not to one: see there), on 1 024 molecules, at which the unpinned step already differs between one thread and
    sixteen."""
    import tests.test_gpu_bf16_stream as TB
    import tests.test_gpu_scale as TS
    packed, y, w, state = oracle_batch_1024()

    def scale():
        r = TS._oracle_step(packed, y, w, 12, "full", state, double=False)
        return [r[0], list(r[1]), dict(r[2])]

    def stream():
        r = TB._oracle_step(packed, y, w, 12, "full", state, bf16=True)
        return [r[0], list(r[1]), dict(r[2])]
    same_forward_bits_and_close_gradients(scale, "scale oracle step")
    same_forward_bits_and_close_gradients(stream, "bf16 oracle step")
