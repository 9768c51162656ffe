"""tests/small_refs.py on the CPU: the shaped batch is what it says, every case of the per-step gradient tests meets
the qualification conditions q1 and q2, and the conditions and the distance bite."""
import numpy as np
import pytest

from tests import small_refs as R


@pytest.mark.parametrize("seed", [2, 5, 10, 64])
def test_shaped_batch_has_its_histogram_and_padded_tail(seed):
    plain = R.shaped_molecules(seed)
    assert plain.n_mols == 48 and plain.n_atoms == 126
    assert R.degree_histogram(plain) == {0: 17, 1: 65, 2: 32, 3: 11, 4: 0, 5: 0, 6: 0, 7: 0, 8: 0, 9: 0, 10: 1}
    sizes = np.diff(plain.atom_ptr)
    assert sorted(np.unique(sizes, return_counts=True)[1].tolist()) == sorted([17, 8 + 11, 1, 11])  # 4-atom: rings + stars
    assert not np.array_equal(sizes, np.diff(R.shaped_molecules(seed + 1).atom_ptr))  # shuffled by the seed
    assert set(np.unique(plain.atom_features)) == {0.0, 1.0} and plain.atom_features.dtype == np.float32
    assert 0.07 < plain.atom_features.mean() < 0.13
    padded, n_real = R.batch_of("padded", seed)
    assert padded.n_mols == 48 and n_real == 43
    assert R.degree_histogram(padded) == R.degree_histogram(plain)
    for i in range(R.PAD):
        fa, aa = padded.molecule(i)
        fb, ab = padded.molecule(n_real + i)
        assert aa == ab and np.array_equal(fa, fb)
    packed, y, w, cfg, state, n_real = R.case_inputs("A", "padded", seed)
    assert np.array_equal(y[n_real:], y[:R.PAD])
    _, labels, weights = R.oracle_inputs(packed, y, w, cfg, n_real)
    assert float(weights[n_real:].abs().max()) == 0.0 and labels.shape[0] == 48


def test_ordinary_batch():
    p = R.ordinary_molecules(7)
    assert p.n_mols == 34 and 350 <= p.n_atoms <= 700
    hist = R.degree_histogram(p)
    assert hist[0] >= 1 and hist[6] == 7 and hist[10] == 1 and max(hist[1], hist[2]) > 64  # blocks of many tiles


@pytest.mark.parametrize("case,grad_mode", [(c, g) for c in R.CASES for g in c.modes],
                         ids=[R.case_id(c, g) for c in R.CASES for g in c.modes])
def test_case_is_qualified(case, grad_mode):
    q1, q2 = R.qualify(case.model, case.kind, case.seed, grad_mode)
    print("%s: q1 %.2e (<= %.1e)  q2 %.2e (<= %.1e)" % (R.case_id(case, grad_mode), q1, R.Q1_MAX, q2, R.Q2_MAX))
    assert q1 <= R.Q1_MAX, q1
    assert q2 <= R.Q2_MAX, q2


def test_case_table_covers_what_the_device_tests_run():
    assert [(c.model, c.kind) for c in R.ONE_STEP] == \
        [(m, "shaped") for m in "ABCDEF"] + [("A", "padded"), ("B", "padded")] + [(m, "ordinary") for m in "ABC"]
    listed = {(c.model, c.kind, c.seed) for c in R.CASES if set(c.modes) == set(R.GRAD_MODES)}
    for model, seed in R.SEQUENCE.items():
        for kind in R.SEQUENCE_KINDS:
            assert (model, kind, seed) in listed


def _empty_degree_blocks(layer):
    """W_list / b_list order is rel_1, self_1, ..., rel_10, self_10, self_0: degrees 4 to 9 are entries 6 to 17."""
    return ["graph_convs.%d.%s.%d" % (layer, wb, k) for wb in ("W_list", "b_list") for k in range(6, 18)]


@pytest.mark.parametrize("case", [c for c in R.CASES if c.kind != "ordinary"], ids=lambda c: "%s-%s-%d" % c[:3])
def test_exact_zeros_are_exact_in_float32_too(case):
    r64, r32 = R.references(case.model, case.kind, case.seed, "full")
    zeros = [k for k, g in r64.grads.items() if g is not None and not g.any()]
    for layer in range(len(R.MODELS[case.model].widths)):
        assert set(_empty_degree_blocks(layer)) <= set(zeros)
    for k in zeros:
        assert not r32.grads[k].any(), k
    r64r, _ = R.references(case.model, case.kind, case.seed, "reference")
    assert all(r64r.grads[k] is None for k in r64r.grads if k.startswith("graph_convs"))


def test_unqualified_batches_exist():
    """The conditions reject something: among seeds 1 to 12 of the shaped batch at the widest model at least one misses
    q1 or q2 (were every seed to pass, the conditions would say nothing about a batch)."""
    missed = []
    for seed in range(1, 13):
        q1, q2 = R.qualify("C", "shaped", seed, "full")
        print("seed %d: q1 %.2e q2 %.2e" % (seed, q1, q2))
        if not R.qualifies(q1, q2):
            missed.append(seed)
    assert missed


def test_tensor_distance_sees_a_constant_factor():
    r64, _ = R.references("A", "shaped", 5, "full")
    seen = 0
    for k, g in r64.grads.items():
        if g is None or not g.any():
            continue
        assert R.tensor_distance(g * (1 + 2e-4), g) > R.BOUND, k
        assert R.tensor_distance(g, g) == 0.0
        seen += 1
    assert seen > 40
    assert R.tensor_distance(np.zeros(3), np.zeros(3)) == 0.0
    assert R.tensor_distance(np.full(3, 1e-7), np.zeros(3)) == pytest.approx(0.1)  # the floor of the scale
