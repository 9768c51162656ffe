"""tests/small_refs.py on the CPU, the additions for the large-batch step (tests/test_gpu_large_grads.py): the tiled
batch is what it says, every new entry of LARGE_CASES meets the qualification conditions q1 and q2 in both gradient
modes, and the conditions and the distance bite there too.  (The entries shared with the small-batch engine are
re-checked by tests/test_small_refs_host.py.)"""
import numpy as np
import pytest

from tests import small_refs as R

NEW = [(c, g) for c in R.LARGE_NEW for g in c.modes]


@pytest.mark.parametrize("seed", [2, 3, 5])
def test_tiled_batch_has_its_histogram(seed):
    p = R.tiled_molecules(seed)
    assert p.n_mols == 97 and p.n_atoms == 264
    # 128 + 1 rows, exactly 64, 64 - 1, six empty blocks in a row, a single row
    assert R.degree_histogram(p) == {0: 7, 1: 129, 2: 64, 3: 63, 4: 0, 5: 0, 6: 0, 7: 0, 8: 0, 9: 0, 10: 1}
    sizes = np.diff(p.atom_ptr)
    assert dict(zip(*np.unique(sizes, return_counts=True))) == {1: 7, 2: 55, 4: 16 + 15 + 3, 11: 1}
    assert not np.array_equal(sizes, np.diff(R.tiled_molecules(seed + 1).atom_ptr))  # shuffled by the seed
    assert set(np.unique(p.atom_features)) == {0.0, 1.0} and p.atom_features.dtype == np.float32
    assert p.atom_features.shape == (264, 75) and 0.07 < p.atom_features.mean() < 0.13
    assert R.batch_of("tiled", seed)[1] == 97


@pytest.mark.parametrize("k", R.WIDTHS)
def test_width_inputs(k):
    seed = next(c.seed for c in R.LARGE_NEW if c.kind == "width%d" % k)
    packed, y, w, cfg, state, n_real = R.width_inputs(k, seed)
    t = R.shaped_molecules(seed)
    assert packed.n_feat == k and packed.atom_features.dtype == np.float32 and n_real == packed.n_mols == 48
    assert np.array_equal(packed.adj_idx, t.adj_idx) and np.array_equal(packed.atom_ptr, t.atom_ptr)
    f = packed.atom_features
    assert -1 <= f.min() < -0.99 and 0.99 < f.max() <= 1 and len(np.unique(f)) > 0.99 * f.size  # continuous
    assert tuple(cfg.number_input_features) == (k, 64) and tuple(cfg.graph_conv_layers) == (64, 64)
    assert cfg.dense_layer_size == 128 and cfg.n_tasks == 3 and cfg.mode == "classification"
    assert state["graph_convs.0.W_list.0"].shape == (k, 64)
    assert R.case_inputs("A", "width%d" % k, seed)[0] is not None


def test_case_table():
    assert R.LARGE_CASES[:len(R.ONE_STEP)] == R.ONE_STEP
    new = [(c.model, c.kind) for c in R.LARGE_CASES[len(R.ONE_STEP):]]
    assert new == [("A", "tiled"), ("E", "tiled"), ("G", "tiled")] + [("A", "width%d" % k) for k in (33, 64, 65, 96, 97)]
    assert all(set(c.modes) == set(R.GRAD_MODES) for c in R.LARGE_CASES)


@pytest.mark.parametrize("case,grad_mode", NEW, ids=[R.case_id(c, g) for c, g in NEW])
def test_case_is_qualified(case, grad_mode):
    q1, q2 = R.qualify(case.model, case.kind, case.seed, grad_mode)
    print("%s: q1 %.2e (<= %.1e)  q2 %.2e (<= %.1e)" % (R.case_id(case, grad_mode), q1, R.Q1_MAX, q2, R.Q2_MAX))
    assert R.qualifies(q1, q2), (q1, q2)
    # the rule as a function of the inputs gives the same two numbers to the bit
    assert R.qualify_inputs(*R.case_inputs(case.model, case.kind, case.seed), grad_mode, draw_seed=case.seed) == (q1, q2)


def test_listed_seeds_are_the_first_that_qualify():
    """Seeds are found by scanning 1, 2, ... upward: no seed below a listed one qualifies in both modes."""
    for case in R.LARGE_NEW:
        for seed in range(1, case.seed):
            qs = [R.qualify(case.model, case.kind, seed, g) for g in R.GRAD_MODES]
            assert not all(R.qualifies(*q) for q in qs), (case, seed, qs)


def test_unqualified_tiled_batches_exist():
    """The conditions reject something there: among seeds 1 to 8 of the tiled batch on model A at least one misses."""
    missed = []
    for seed in range(1, 9):
        q1, q2 = R.qualify("A", "tiled", seed, "full")
        print("seed %d: q1 %.2e q2 %.2e" % (seed, q1, q2))
        if not R.qualifies(q1, q2):
            missed.append(seed)
    assert missed


@pytest.mark.parametrize("case", R.LARGE_NEW, ids=lambda c: "%s-%s-%d" % c[:3])
def test_a_constant_factor_is_beyond_the_bound(case):
    r64, _ = R.references(case.model, case.kind, case.seed, "full")
    seen = 0
    for k, g in r64.grads.items():
        if g is None or not g.any():
            continue
        assert R.tensor_distance(g * (1 + 2e-4), g) > R.BOUND, k
        want = np.asarray(g, np.float64)
        bound = R.BOUND * max(np.abs(want).max(), 1e-6) + 1e-7  # the device file's bound on this tensor
        if np.abs(want).max() > 1e-3:  # (below that the absolute term of the bound is more than half of it)
            assert np.abs(want * 2e-4).max() > bound, k
        seen += 1
    assert seen > (55 if case.model == "E" else 40)


def _empty_degree_blocks(layer):
    """W_list / b_list order is rel_1, self_1, ..., rel_10, self_10, self_0: degrees 4 to 9 are entries 6 to 17."""
    return ["graph_convs.%d.%s.%d" % (layer, wb, k) for wb in ("W_list", "b_list") for k in range(6, 18)]


@pytest.mark.parametrize("case", R.LARGE_NEW, ids=lambda c: "%s-%s-%d" % c[:3])
def test_exact_zeros_are_exact_in_float32_too(case):
    r64, r32 = R.references(case.model, case.kind, case.seed, "full")
    zeros = [k for k, g in r64.grads.items() if g is not None and not g.any()]
    for layer in range(len(R.MODELS[case.model].widths)):
        assert set(_empty_degree_blocks(layer)) <= set(zeros)
    for k in zeros:
        assert not r32.grads[k].any(), k
    r64r, _ = R.references(case.model, case.kind, case.seed, "reference")
    assert all(r64r.grads[k] is None for k in r64r.grads if k.startswith("graph_convs"))
