"""The metric kernels (deepchem_amd/csrc/metrics.hip) at the edges of their radix sort, carried scan and launch grids,
against a float64 NumPy reference written here (argsort, cumsum at the tie cuts) that shares nothing with them.

What is held, and why.
* ROC-AUC: **bit-equal**.  Weights are multiples of 1/4, so every partial sum and every product of the numerator is a
  multiple of 1/16 far below 2^53: fp64 (and int64) addition is exact in any order, and the final expression
  num / (2.0 * P * N) is the same operation on both sides.
* PRC-AUC: 2 * (n + 8) * 2^-53.  Two divisions per tie group; the terms sum to at most P before the last division, one
  rounding per accumulated term on each side plus a handful per term.
* Moments with inputs on a 1/8 grid, power-of-two scales and dyadic weights: every product is exact in fp64, the
  order of the atomics cannot matter: np.array_equal.  Accuracy: equal counts and weight sums.
* Moments of ordinary inputs: REL_TOL of tests/test_gpu_metrics.py, or its bound 64 * n * 2^-53 where that is smaller.
* The sort stays inside gcmi_metrics_workspace_bytes, and outputs are written for n_tasks entries only (sentinels).

test_reference_agrees_with_the_host_functions needs no GPU: it pins the reference here to the host functions that
tests/test_metrics_host.py pins to sklearn's recorded results."""
import numpy as np
import pytest
import torch

from deepchem_amd import _lib
from deepchem_amd import metrics as M
from deepchem_amd.models import device_metrics as DM

gpu = pytest.mark.gpu
DEV = "cuda"
REL_TOL = 1e-10  # tests/test_gpu_metrics.py
ROC, PRC = _lib.GCMI_METRIC_ROC_AUC, _lib.GCMI_METRIC_PRC_AUC
WINDOWS = ((1000, 1023), (1000, 1024), (1023, 1024), (1024, 1030), (0, 2100), (2040, 2060), (-3, -1))
ALL_SIZES = (2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 4097, 6145)
MAIN_SIZES = (65, 1025, 2049, 6145)


def prc_bound(n):
    return 2 * (n + 8) * 2.0 ** -53


# ------------------------------------------------------------------------------------------------ the reference
def ref_rank(score, positive, weight=None):
    """(ROC-AUC, PRC-AUC) of one task in float64: descending stable argsort, tie cuts where consecutive sorted scores
    differ, cumulative positive and negative weight at the cuts."""
    s = score.astype(np.float64) + 0.0
    order = np.argsort(-s, kind="stable")
    s, pos = s[order], np.asarray(positive, bool)[order]
    w = np.ones(s.shape[0]) if weight is None else weight.astype(np.float64)[order]
    cut = np.r_[s[1:] != s[:-1], True]
    cp, cn = np.cumsum(np.where(pos, w, 0.0))[cut], np.cumsum(np.where(pos, 0.0, w))[cut]
    cp_prev, cn_prev = np.r_[0.0, cp[:-1]], np.r_[0.0, cn[:-1]]
    P, N = cp[-1], cn[-1]
    roc = np.sum((cn - cn_prev) * (cp_prev + cp)) / (2.0 * P * N)
    seen, seen_prev = cp + cn, cp_prev + cn_prev
    prec = np.where(seen > 0, cp / np.where(seen > 0, seen, 1.0), 0.0)
    prec_prev = np.where(seen_prev > 0, cp_prev / np.where(seen_prev > 0, seen_prev, 1.0), 1.0)  # nothing precedes: 1
    prc = np.sum((cp - cp_prev) * (prec + prec_prev) / 2) / P
    return float(roc), float(prc)


# ------------------------------------------------------------------------------------------------ inputs
def _distinct(n, rng):
    """n different fp32 scores in [0, 1) with full 24-bit mantissas, in random order."""
    s = np.unique(rng.rand(2 * n + 16).astype(np.float32))
    assert s.shape[0] >= n
    return rng.permutation(s)[:n]


def _bits(u):
    return np.asarray(u, np.uint32).view(np.float32)


def scores_of(family, n, rng):
    if family == "full":
        return _distinct(n, rng)
    if family == "few":
        return (rng.randint(0, 5, n) / 4).astype(np.float32)
    if family == "constant":
        return np.full(n, 0.375, np.float32)
    if family == "mixed":
        with np.errstate(under="ignore"):
            s = (rng.randn(n) * 10.0 ** rng.uniform(-42, 3, n)).astype(np.float32)
        dup = rng.rand(n) < 0.25
        s[dup] = s[rng.randint(0, n, int(dup.sum()))]
        s[rng.randint(0, n, max(1, n // 16))] = -0.0
        s[rng.randint(0, n, max(1, n // 16))] = 0.0
        return s
    if family == "lowbyte":  # bit patterns that differ in bits 0..7 only: radix pass 0 does all the work
        return _bits(0x3F000000 | rng.randint(0, 256, n).astype(np.uint32))
    if family == "highbyte":  # bits 24..31 only (sign and the exponent's upper seven bits; never exponent 0xFF)
        s = _bits((rng.randint(0, 256, n).astype(np.uint32) << 24) | 0x00400000)
        assert np.isfinite(s).all()
        return s
    if family.startswith("placed"):  # distinct scores, one tie group at positions a..b of the descending order
        a, b = (int(v) for v in family.split(":")[1:])
        a, b = (a + n if a < 0 else a), (b + n if b < 0 else b)
        assert 0 <= a < b < n
        d = np.sort(_distinct(n, rng))[::-1].copy()
        d[a:b + 1] = d[a]
        return d[rng.permutation(n)]
    raise ValueError(family)


def make_case(family, n, T, seed, dyadic=True):
    """scores (n, T, 2) fp32 (every task and column its own draw), labels (n, T) fp64, weights (n, T) fp32 with
    weight on both classes of every task."""
    rng = np.random.RandomState(seed)
    s = np.stack([np.stack([scores_of(family, n, rng) for _ in range(2)], 1) for _ in range(T)], 1)
    y = (rng.rand(n, T) < 0.4).astype(np.float64)
    w = (rng.randint(0, 9, (n, T)) / 4 if dyadic else rng.rand(n, T) + 0.01).astype(np.float32)
    rows = np.stack([rng.permutation(n)[:2] for _ in range(T)], 1) if n >= 2 else None
    for t in range(T):
        y[rows[0, t], t], y[rows[1, t], t] = 1.0, 0.0
        if dyadic:
            w[rows[0, t], t], w[rows[1, t], t] = 1.0, 0.5
    return np.ascontiguousarray(s, np.float32), y, w


def _cases():
    out = [("full", n) for n in ALL_SIZES] + [("few", n) for n in ALL_SIZES] + [("mixed", n) for n in ALL_SIZES]
    out += [("constant", n) for n in (2, 64) + MAIN_SIZES]
    out += [(f, n) for f in ("lowbyte", "highbyte") for n in (64, 65, 256, 257, 1025, 2049, 6145)]
    for n in MAIN_SIZES:  # every window that fits into n, once
        seen = set()
        for a, b in WINDOWS:
            a, b = (a + n if a < 0 else a), (b + n if b < 0 else b)
            if b < n and (a, b) not in seen:
                seen.add((a, b))
                out.append(("placed:%d:%d" % (a, b), n))
    return out


CASES = _cases()
CASE_IDS = ["%s-n%d" % (f.replace(":", "_"), n) for f, n in CASES]


def _seed(family, n):
    return (sum(ord(c) * (i + 1) for i, c in enumerate(family)) * 31 + n) % (2 ** 31)


# ------------------------------------------------------------------------------------------------ CPU self-check
@pytest.mark.parametrize("family,n", [(f, n) for f, n in CASES if n in (2,) + MAIN_SIZES + (4097,)],
                         ids=[i for i, (f, n) in zip(CASE_IDS, CASES) if n in (2,) + MAIN_SIZES + (4097,)])
def test_reference_agrees_with_the_host_functions(family, n):
    s, y, w = make_case(family, n, 1, _seed(family, n))
    for column, positive in ((1, 1), (0, 0)):
        pos = y[:, 0] == positive
        for weight in (None, w[:, 0]):
            roc, prc = ref_rank(s[:, 0, column], pos, weight)
            assert roc == M.roc_auc_score(pos.astype(np.float64), s[:, 0, column], sample_weight=weight)
            assert abs(prc - M._binary_prc_auc(pos, s[:, 0, column],
                                               None if weight is None else weight.astype(np.float64))) <= 1e-15


def test_reference_on_a_case_worked_by_hand():
    # descending: 0.9(+) | 0.5(+, -, -) | 0.25(-): 2 * #{pos > neg} + #{ties} = 2 * (3 + 1) + 2 = 10 of 2 * 2 * 3
    s = np.array([0.5, 0.9, 0.25, 0.5, 0.5], np.float32)
    pos = np.array([True, True, False, False, False])
    roc, prc = ref_rank(s, pos)
    assert roc == 10 / 12.0
    # recall 0 -> 1/2 at precision 1 -> 1; 1/2 -> 1 at precision 1 -> 2/4
    assert abs(prc - (0.5 * 1.0 + 0.5 * (1.0 + 0.5) / 2)) <= 1e-16


# ------------------------------------------------------------------------------------------------ rank kernel
def _workspace(n, T):
    n_bytes = int(_lib.load().gcmi_metrics_workspace_bytes(n, T))
    assert n_bytes >= 16 * n * T
    return torch.empty(n_bytes, dtype=torch.uint8, device=DEV)


def _rank(which, scores, column, y, positive, w, row_stride=None, elem_stride=None):
    """One gcmi_metric_rank call; by default on column `column` of (n, T, 2) scores."""
    n, T = y.shape
    row_stride = 2 * T if row_stride is None else row_stride
    elem_stride = 2 if elem_stride is None else elem_stride
    out, status = DM.rank_scores(which, scores, column, row_stride, elem_stride, y, positive, w, _workspace(n, T))
    torch.cuda.synchronize()
    return out.cpu().numpy(), status.cpu().numpy()


def _check_rank(tag, s, y, w, want_status=0):
    """Every (weighted, ROC column 1 / ROC column 0 / PRC column 1) of one set of tasks against the reference:
    ROC bit-equal, PRC within prc_bound(n).  Returns the largest PRC difference."""
    n, T = y.shape
    s_d, y_d, w_d = torch.as_tensor(s, device=DEV), torch.as_tensor(y, device=DEV), torch.as_tensor(w, device=DEV)
    worst = 0.0
    for weighted in (False, True):
        for which, column, positive in ((ROC, 1, 1), (ROC, 0, 0), (PRC, 1, 1)):
            got, status = _rank(which, s_d, column, y_d, positive, w_d if weighted else None)
            assert (status == want_status).all(), (tag, T, weighted, which, column, status)
            want = np.array([ref_rank(s[:, t, column], y[:, t] == positive, w[:, t] if weighted else None)
                             for t in range(T)])[:, 0 if which == ROC else 1]
            if which == ROC:
                assert np.array_equal(got, want), (tag, T, weighted, column, got, want)
            else:
                diff = float(np.abs(got - want).max())
                worst = max(worst, diff)
                assert diff <= prc_bound(n), (tag, T, weighted, diff, prc_bound(n))
    return worst


@gpu
@pytest.mark.parametrize("family,n", CASES, ids=CASE_IDS)
def test_rank_kernel_against_the_reference(family, n):
    s, y, w = make_case(family, n, 3, _seed(family, n))
    worst = _check_rank(family, s, y, w)  # three tasks with different data in one call
    worst = max(worst, _check_rank(family, np.ascontiguousarray(s[:, 1:2]), np.ascontiguousarray(y[:, 1:2]),
                                   np.ascontiguousarray(w[:, 1:2])))  # and one task alone
    print("%s n=%d PRC-AUC max |diff| %.3g (bound %.3g)" % (family, n, worst, prc_bound(n)))
    if family == "constant":
        got, _ = _rank(ROC, torch.as_tensor(s, device=DEV), 1, torch.as_tensor(y, device=DEV), 1,
                       torch.as_tensor(w, device=DEV))
        assert (got == 0.5).all()


@gpu
@pytest.mark.parametrize("family", ["full", "mixed"])
def test_rank_kernel_on_a_plain_matrix_of_scores(family):
    n, T = 2049, 3
    s, y, w = make_case(family, n, T, 77)
    s2 = np.ascontiguousarray(s[:, :, 1])  # (n, T): row_stride T, elem_stride 1
    s_d, y_d, w_d = torch.as_tensor(s2, device=DEV), torch.as_tensor(y, device=DEV), torch.as_tensor(w, device=DEV)
    for weighted in (False, True):
        want = np.array([ref_rank(s2[:, t], y[:, t] == 1, w[:, t] if weighted else None) for t in range(T)])
        roc, st = _rank(ROC, s_d, 0, y_d, 1, w_d if weighted else None, T, 1)
        assert not st.any() and np.array_equal(roc, want[:, 0])
        prc, st = _rank(PRC, s_d, 0, y_d, 1, w_d if weighted else None, T, 1)
        assert not st.any() and np.abs(prc - want[:, 1]).max() <= prc_bound(n)


@gpu
def test_status_flags_are_ored_per_task_and_leave_the_others_right():
    n, T = 2049, 3
    s, y, w = make_case("full", n, T, 5)
    y[:, 1] = 1.0                                    # task 1: one class, and two NaN scores
    s[2048, 1, 1] = s[7, 1, 1] = np.nan
    s[0, 2, 1], s[2048, 2, 1] = np.inf, -np.inf      # task 2: infinite scores, ranked where they belong
    s_d, y_d, w_d = torch.as_tensor(s, device=DEV), torch.as_tensor(y, device=DEV), torch.as_tensor(w, device=DEV)
    for weighted in (False, True):
        roc, st = _rank(ROC, s_d, 1, y_d, 1, w_d if weighted else None)
        assert list(st) == [0, 3, 4]
        for t in (0, 2):
            assert roc[t] == ref_rank(s[:, t, 1], y[:, t] == 1, w[:, t] if weighted else None)[0]
        prc, st = _rank(PRC, s_d, 1, y_d, 1, w_d if weighted else None)
        assert list(st) == [0, 3, 4]
        for t in (0, 2):
            assert abs(prc[t] - ref_rank(s[:, t, 1], y[:, t] == 1, w[:, t] if weighted else None)[1]) <= prc_bound(n)
    # a NaN among two classes: 2 alone, however many there are
    y[:, 1] = y[:, 0]
    _, st = _rank(ROC, s_d, 1, torch.as_tensor(y, device=DEV), 1, None)
    assert list(st) == [0, 2, 4]
    # one row is one class
    one = torch.tensor([[[0.25, 0.75]]], device=DEV)
    for label in (0.0, 1.0):
        out, st = _rank(ROC, one, 1, torch.tensor([[label]], dtype=torch.float64, device=DEV), 1, None)
        assert list(st) == [1] and list(out) == [0.0]


@gpu
def test_rank_kernel_is_deterministic_with_ordinary_weights():
    n, T = 6145, 3
    s, y, w = make_case("few", n, T, 11, dyadic=False)
    s[:, 1] = make_case("full", n, 1, 12)[0][:, 0]
    s_d, y_d, w_d = torch.as_tensor(s, device=DEV), torch.as_tensor(y, device=DEV), torch.as_tensor(w, device=DEV)
    want = np.array([ref_rank(s[:, t, 1], y[:, t] == 1, w[:, t]) for t in range(T)])
    for k, which in enumerate((ROC, PRC)):
        first, st = _rank(which, s_d, 1, y_d, 1, w_d)
        again, _ = _rank(which, s_d, 1, y_d, 1, w_d)
        assert not st.any()
        assert first.tobytes() == again.tobytes()
        diff = float(np.abs(first - want[:, k]).max())
        print("ordinary weights n=%d %s max |diff| %.3g (bound %.3g)" % (n, ("ROC", "PRC")[k], diff, prc_bound(n)))
        assert diff <= prc_bound(n)


@gpu
@pytest.mark.parametrize("n,T", [(2049, 3), (1, 1)])
def test_rank_kernel_writes_inside_its_workspace_and_outputs(n, T):
    if n == 1:
        s, y, w = np.full((1, 1, 2), 0.5, np.float32), np.ones((1, 1)), np.ones((1, 1), np.float32)
    else:
        s, y, w = make_case("mixed", n, T, 3)
    s_d, y_d, w_d = torch.as_tensor(s, device=DEV), torch.as_tensor(y, device=DEV), torch.as_tensor(w, device=DEV)
    n_bytes = int(_lib.load().gcmi_metrics_workspace_bytes(n, T))
    stream = torch.cuda.current_stream().cuda_stream
    for which in (ROC, PRC):
        for weights in (None, w_d):
            ws = torch.full((n_bytes + 4096,), 0xA5, dtype=torch.uint8, device=DEV)
            out = torch.full((T + 8,), -12345.5, dtype=torch.float64, device=DEV)
            status = torch.full((T + 8,), -77, dtype=torch.int32, device=DEV)
            _lib.call("gcmi_metric_rank", which, s_d.data_ptr() + 4, 2 * T, 2, y_d.data_ptr(), 1,
                      weights.data_ptr() if weights is not None else None, n, T, out.data_ptr(), status.data_ptr(),
                      ws.data_ptr(), stream)
            torch.cuda.synchronize()
            assert bool((ws[n_bytes:] == 0xA5).all()), "the sort wrote past gcmi_metrics_workspace_bytes"
            assert out[T:].cpu().tolist() == [-12345.5] * 8 and status[T:].cpu().tolist() == [-77] * 8
            if n == 1:
                assert status[:T].cpu().tolist() == [1]
            else:
                assert not status[:T].any()
                want = [ref_rank(s[:, t, 1], y[:, t] == 1, None if weights is None else w[:, t])[which == PRC]
                        for t in range(T)]
                assert np.abs(out[:T].cpu().numpy() - want).max() <= (0.0 if which == ROC else prc_bound(n))


# ------------------------------------------------------------------------------------------------ moments kernel
# (1, 1) and (257, 1): lanes_t = 1; (16385, 1): 65 row passes for 64 row blocks; (300, 5): dead lanes inside one block;
# (300, 65): lanes_t = 64, two task blocks, 63 dead lanes, a striding row loop; (65, 130): three task blocks
SHAPES = [(1, 1), (257, 1), (16385, 1), (300, 2), (300, 5), (257, 64), (300, 65), (65, 130)]
SPARE_ROWS = 64  # a dead lane's task index is less than 64 past n_tasks


def _moment_inputs(n, T, seed, exact):
    rng = np.random.RandomState(seed)
    if exact:
        y = rng.randint(-128, 129, (n, T)) / 8.0
        p = (rng.randint(-128, 129, (n, T)) / 8.0).astype(np.float32)
        scale, shift = 2.0 ** rng.randint(-2, 3, T), rng.randint(-16, 17, T) / 8.0
    else:
        y = -300.0 + 2.0 * rng.randn(n, T)
        p = (y + 0.7 * rng.randn(n, T)).astype(np.float32)
        scale, shift = rng.uniform(0.5, 2.0, T), rng.randn(T)
    w = (rng.randint(0, 9, (n, T)) / 4).astype(np.float32)
    return y, p, w, scale, shift


def _moment_sums_ref(y, p, w, dtype=np.float64):
    """Sums [0..7] of the header's layout per task, and y0, p0; `p` already float64 and through scale / shift."""
    y0, p0 = y[0], p[0]
    y, p, w = y.astype(dtype), p.astype(dtype), w.astype(dtype)
    dy, dp, e = y - y0, p - p0, y - p
    sums = [w.sum(0), (w * dy).sum(0), (w * dp).sum(0), (w * dy * dy).sum(0), (w * dp * dp).sum(0),
            (w * dy * dp).sum(0), (w * np.abs(e)).sum(0), (w * e * e).sum(0)]
    return np.stack(sums, 1), y0, p0


def _moments_guarded(which, pred, row_stride, elem_stride, n_classes, y, w, scale, shift):
    """gcmi_metric_moments into an array with SPARE_ROWS sentinel rows behind the n_tasks it may write."""
    n, T = y.shape
    out = torch.full((T + SPARE_ROWS, _lib.GCMI_METRIC_MOMENT_DOUBLES), -12345.5, dtype=torch.float64, device=DEV)
    ptr = lambda a: a.data_ptr() if a is not None else None  # noqa: E731
    _lib.call("gcmi_metric_moments", which, pred.data_ptr(), row_stride, elem_stride, n_classes, y.data_ptr(), ptr(w),
              ptr(scale), ptr(shift), n, T, out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert bool((out[T:] == -12345.5).all()), "gcmi_metric_moments wrote past n_tasks rows"
    return out[:T]


@gpu
@pytest.mark.parametrize("n,T", SHAPES)
def test_moments_are_exact_on_dyadic_inputs(n, T):
    y, p, w, scale, shift = _moment_inputs(n, T, 100 + n + T, exact=True)
    y_d, p_d, w_d = torch.as_tensor(y, device=DEV), torch.as_tensor(p, device=DEV), torch.as_tensor(w, device=DEV)
    for weighted in (False, True):
        for affine in (False, True):
            sc = torch.as_tensor(scale, device=DEV) if affine else None
            sh = torch.as_tensor(shift, device=DEV) if affine else None
            guarded = _moments_guarded(_lib.GCMI_METRIC_MOMENTS, p_d, T, 1, 1, y_d, w_d if weighted else None, sc, sh)
            got = DM.moment_sums(_lib.GCMI_METRIC_MOMENTS, p_d, T, 1, 1, y_d, w_d if weighted else None, sc, sh)
            got = got.cpu().numpy()
            assert np.array_equal(got, guarded.cpu().numpy())
            ph = p.astype(np.float64) * scale + shift if affine else p.astype(np.float64)
            want, y0, p0 = _moment_sums_ref(y, ph, w if weighted else np.ones((n, T)))
            where = (n, T, weighted, affine)
            assert np.array_equal(got[:, :8], want), where
            assert np.array_equal(got[:, 8], y0) and np.array_equal(got[:, 9], p0), where
            assert not got[:, 10:].any(), where


@gpu
@pytest.mark.parametrize("n_classes", [1, 2, 3, 5])
@pytest.mark.parametrize("n,T", SHAPES)
def test_accuracy_counts_equal_argmax(n, T, n_classes):
    rng = np.random.RandomState(200 + n + T + n_classes)
    p = (rng.randint(0, 4, (n, T, n_classes)) / 4).astype(np.float32)  # four levels: tied maxima are common
    y = rng.randint(0, max(n_classes, 2), (n, T)).astype(np.float64)
    w = (rng.randint(0, 9, (n, T)) / 4).astype(np.float32)
    y_d, p_d, w_d = torch.as_tensor(y, device=DEV), torch.as_tensor(p, device=DEV), torch.as_tensor(w, device=DEV)
    hit = np.argmax(p, axis=2) == y
    for weighted in (False, True):
        wh = w.astype(np.float64) if weighted else np.ones((n, T))
        args = (_lib.GCMI_METRIC_ACCURACY, p_d, T * n_classes, n_classes, n_classes, y_d, w_d if weighted else None,
                None, None)
        guarded = _moments_guarded(*args).cpu().numpy()
        got = DM.moment_sums(*args).cpu().numpy()
        assert np.array_equal(got, guarded)
        assert np.array_equal(got[:, 10], (wh * hit).sum(0)), (n, T, n_classes, weighted)
        assert np.array_equal(got[:, 0], wh.sum(0)), (n, T, n_classes, weighted)
        assert np.array_equal(got[:, 8], y[0]) and not got[:, 1:8].any() and not got[:, 9].any()


@gpu
def test_scale_and_shift_round_twice_as_the_host_does():
    # two unweighted rows: sum dp is p[1] - p[0] alone, so [2] and [9] show every bit of p = (double) x * scale + shift
    n, T = 2, 130
    y, p, _, scale, shift = _moment_inputs(n, T, 17, exact=False)
    got = _moments_guarded(_lib.GCMI_METRIC_MOMENTS, torch.as_tensor(p, device=DEV), T, 1, 1,
                           torch.as_tensor(y, device=DEV), None, torch.as_tensor(scale, device=DEV),
                           torch.as_tensor(shift, device=DEV)).cpu().numpy()
    ph = p.astype(np.float64) * scale + shift
    fused = np.array([[float(np.longdouble(a) * np.longdouble(b) + np.longdouble(c)) for a, b, c in
                       zip(row.astype(np.float64), scale, shift)] for row in p])
    assert (fused != ph).any()  # the inputs tell one rounding from two
    assert np.array_equal(got[:, 9], ph[0]) and np.array_equal(got[:, 2], ph[1] - ph[0])


@gpu
@pytest.mark.parametrize("n,T", [(16385, 1), (300, 65)])
def test_moments_of_offset_labels_within_the_relative_bound(n, T):
    tol = min(REL_TOL, 64 * n * 2.0 ** -53)  # that file's tolerance, and its stated bound where that is smaller
    y, p, w, scale, shift = _moment_inputs(n, T, 300 + n + T, exact=False)
    y_d, p_d, w_d = torch.as_tensor(y, device=DEV), torch.as_tensor(p, device=DEV), torch.as_tensor(w, device=DEV)
    worst = 0.0
    for weighted in (False, True):
        for affine in (False, True):
            sc = torch.as_tensor(scale, device=DEV) if affine else None
            sh = torch.as_tensor(shift, device=DEV) if affine else None
            got = DM.moment_sums(_lib.GCMI_METRIC_MOMENTS, p_d, T, 1, 1, y_d, w_d if weighted else None, sc,
                                 sh).cpu().numpy()
            ph = p.astype(np.float64) * scale + shift if affine else p.astype(np.float64)  # two roundings
            wh = w if weighted else np.ones((n, T))
            want, y0, p0 = _moment_sums_ref(y, ph, wh, np.longdouble)
            assert np.array_equal(got[:, 8], y0) and np.array_equal(got[:, 9], p0)
            size = np.abs(want)
            dy, dp = np.abs(y - y0), np.abs(ph - p0)
            size[:, 1], size[:, 2] = (wh * dy).sum(0), (wh * dp).sum(0)  # signed sums: against the sum of magnitudes
            rel = float((np.abs(got[:, :8] - want) / size).max())
            worst = max(worst, rel)
            assert rel <= tol, (n, T, weighted, affine, rel, tol)
    print("moments n=%d T=%d max relative diff %.3g (bound %.3g)" % (n, T, worst, tol))
