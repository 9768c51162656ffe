"""The loss and softmax kernels (csrc/loss.hip: ops.loss_fwd_bwd, ops.softmax_lastdim) at the item counts, class
counts, labels, weights and logits their code branches on, against the float64 restatement of tests/edge_refs.py
(checked on the CPU against torch in float64 and the oracle's batch_loss by tests/test_edge_refs_host.py).

loss_kernel runs min(ceil(items / 256), 256) workgroups of 256 threads, one (row, task) item per thread and trip:
up to 65 536 items every thread has one item at the most (``nostride``), above that the grid-stride loop runs
(``stride``).  softmax_kernel is capped at 8192 workgroups: it strides above 2 097 152 items.

Bounds: TOL = 1e-4 relative to the largest reference magnitude for gradients and probabilities, TOL * max(1, |ref|)
for the loss (tests/test_gpu_kernels.py).  All-zero weights, one class and probabilities that are 0 or 1 in float32
are exact.  Every call is made twice on the same inputs and must return the same loss bits.
"""
import numpy as np
import pytest
import torch

from oracle.edge_checks import to_dev as _dev
from oracle.edge_checks import to_np as _np
from tests import edge_refs as R

pytestmark = pytest.mark.gpu
TOL = R.TOL
LABEL_KINDS = ("onehot", "soft0.3", "soft1", "soft2.5", "zero")


def _err(got, ref):
    got, ref = _np(got), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert np.isfinite(got).all()
    scale = float(np.abs(ref).max())
    worst = float(np.abs(got - ref).max())
    if scale == 0.0:  # an all-zero reference: only zeros will do
        return 0.0 if worst == 0.0 else float("inf")
    return worst / scale


def shape_for(items):
    """12 tasks where the count is divisible, 1 task elsewhere."""
    return (items // 12, 12) if items % 12 == 0 and items >= 12 else (items, 1)


def make_labels(rng, rows, tasks, classes, kind):
    """``mixed``: the five kinds in turn, item by item."""
    if kind == "mixed":
        parts = [make_labels(rng, rows, tasks, classes, k) for k in LABEL_KINDS]
        pick = (np.arange(rows * tasks) % len(LABEL_KINDS)).reshape(rows, tasks)
        y = np.zeros((rows, tasks, classes), np.float32)
        for i, p in enumerate(parts):
            y[pick == i] = p[pick == i]
        return y
    if kind == "onehot":
        return np.eye(classes, dtype=np.float32)[rng.randint(0, classes, size=(rows, tasks))]
    if kind == "zero":
        return np.zeros((rows, tasks, classes), np.float32)
    total = float(kind[4:])  # rows of soft labels that sum to 0.3, 1 or 2.5: sum_c y_c scales p in the gradient
    y = rng.rand(rows, tasks, classes) + 0.05
    return (y / y.sum(-1, keepdims=True) * total).astype(np.float32)


def make_weights(rng, rows, tasks, kind):
    if kind == "none":
        return None
    if kind == "zero":
        return np.zeros((rows, tasks), np.float32)
    if kind == "binary":
        return (rng.rand(rows, tasks) > 0.17).astype(np.float32)
    return (rng.rand(rows, tasks) * 3).astype(np.float32)  # "real"


def run_ce(logits, labels, weights, what):
    """One softmax cross-entropy case, called twice: loss, gradient and probabilities against float64; the loss bits
    of both calls equal; probs of the loss call against softmax_lastdim."""
    from deepchem_amd import ops
    lg, yg = _dev(logits), _dev(labels)
    wg = None if weights is None else _dev(weights)
    ref_loss, ref_d, ref_p = R.ce_loss_ref(logits, labels, weights)
    loss, dlogits, probs = ops.loss_fwd_bwd(0, lg, yg, wg, want_probs=True)
    loss2, dlogits2, _ = ops.loss_fwd_bwd(0, lg, yg, wg, want_probs=False)
    got = float(loss)
    e_loss = abs(got - ref_loss) / max(1.0, abs(ref_loss))
    e_d, e_p = _err(dlogits, ref_d), _err(probs, ref_p)
    sm = ops.softmax_lastdim(lg)
    e_sm = _err(sm, ref_p)
    # loss_kernel takes p = exp(logp) with logp = x - max - log(sum exp), softmax_kernel exp(x - max) / sum exp: two
    # roundings of the same number, not the same bits -- TOL between them, not equality
    e_between = _err(probs, _np(sm))
    print("%s: loss %.9g ref %.9g err %.3e | dlogits %.3e probs %.3e softmax %.3e probs-vs-softmax %.3e | allowed %.1e"
          % (what, got, ref_loss, e_loss, e_d, e_p, e_sm, e_between, TOL))
    assert np.isfinite(got) and e_loss <= TOL
    assert e_d <= TOL and e_p <= TOL and e_sm <= TOL and e_between <= TOL
    assert torch.equal(loss.view(torch.int32), loss2.view(torch.int32)), what + ": two calls, two losses"
    assert torch.equal(dlogits, dlogits2)
    assert tuple(dlogits.shape) == logits.shape and tuple(probs.shape) == logits.shape
    # where float64 says 0 or 1 to float32 precision, so must the kernels
    p32 = ref_p.astype(np.float32)
    sure = (p32 == 0) | (p32 == 1)
    assert np.array_equal(_np(probs)[sure], p32[sure].astype(np.float64)), what + ": saturated probabilities"
    assert np.array_equal(_np(sm)[sure], p32[sure].astype(np.float64)), what + ": saturated softmax"
    return loss, dlogits, probs


def _stride(items):
    return "stride" if items > 256 * 256 else "nostride"


@pytest.mark.parametrize("classes", [1, 2, 3, 5])
@pytest.mark.parametrize("items", [1, 255, 256, 257, 65536, 65537, 200003],
                         ids=lambda n: "items%d-wg%d-%s" % (n, min(-(-n // 256), 256), _stride(n)))
def test_ce_item_counts_and_classes(items, classes):
    """Standard normal logits, the five label kinds in turn (one-hot, soft rows summing to 0.3, 1 and 2.5, all-zero
    rows), non-binary weights."""
    rows, tasks = shape_for(items)
    rng = np.random.RandomState(items + classes)
    logits = rng.standard_normal((rows, tasks, classes)).astype(np.float32)
    labels = make_labels(rng, rows, tasks, classes, "mixed")
    weights = make_weights(rng, rows, tasks, "real")
    _, dlogits, _ = run_ce(logits, labels, weights, "ce items=%d classes=%d" % (items, classes))
    if classes == 1:  # log p = 0 and p = 1 exactly: the loss is 0, the gradient w (ysum - y) / count = 0
        assert not _np(dlogits).any()


@pytest.mark.parametrize("label_kind", LABEL_KINDS)
@pytest.mark.parametrize("weight_kind", ["binary", "none", "zero", "real"])
@pytest.mark.parametrize("items,classes", [(257, 2), (65537, 3)], ids=["items257-c2-nostride", "items65537-c3-stride"])
def test_ce_labels_and_weights(items, classes, weight_kind, label_kind):
    """Every label kind under every kind of weights (given and binary, None -- a path of its own in the kernel --,
    all zero, non-binary).  All-zero weights: the loss and the gradient are exactly 0."""
    rows, tasks = shape_for(items)
    rng = np.random.RandomState(items + len(label_kind) + 3 * len(weight_kind))
    logits = rng.standard_normal((rows, tasks, classes)).astype(np.float32)
    labels = make_labels(rng, rows, tasks, classes, label_kind)
    weights = make_weights(rng, rows, tasks, weight_kind)
    loss, dlogits, _ = run_ce(logits, labels, weights, "ce items=%d classes=%d w=%s y=%s" % (items, classes, weight_kind,
                                                                                           label_kind))
    if weight_kind == "zero":
        assert float(loss) == 0.0 and not _np(dlogits).any()
    if label_kind == "zero":
        assert float(loss) == 0.0 and not _np(dlogits).any()  # ysum = 0 and y = 0: nothing to learn from the item


@pytest.mark.parametrize("classes", [2, 3, 5])
@pytest.mark.parametrize("weight_kind", ["none", "real"])
def test_ce_extreme_and_equal_logits(classes, weight_kind):
    """Rows with entries at +-1e4 and mixed +-80 (exp overflows float32 without the max subtraction; with it the
    small entries underflow to exactly 0 and the largest gets exactly 1 or an exact share), rows of all-equal logits
    (p = 1 / classes), one-hot and soft labels: everything finite, saturated probabilities exact."""
    rng = np.random.RandomState(classes)
    rows, tasks = 300, 1
    logits = rng.standard_normal((rows, tasks, classes)).astype(np.float32)
    logits[0::6] = rng.choice([-1e4, 1e4], size=logits[0::6].shape)
    logits[1::6] = rng.choice([-80.0, 80.0], size=logits[1::6].shape)
    logits[2::6] = rng.choice([-3.0, 0.0, 17.5, 1e4], size=(logits[2::6].shape[0], tasks, 1))  # all classes equal
    logits[3::6, :, 0] = 1e4  # one huge entry among ordinary ones
    labels = make_labels(rng, rows, tasks, classes, "mixed")
    run_ce(logits, labels, make_weights(rng, rows, tasks, weight_kind), "ce extreme classes=%d w=%s" % (classes, weight_kind))


@pytest.mark.parametrize("weight_kind", ["binary", "none", "zero", "real"])
@pytest.mark.parametrize("items", [1, 257, 65537, 200003], ids=lambda n: "items%d-%s" % (n, _stride(n)))
def test_l2_item_counts_and_weights(items, weight_kind):
    from deepchem_amd import ops
    rows, tasks = shape_for(items)
    rng = np.random.RandomState(items)
    x = rng.standard_normal((rows, tasks)).astype(np.float32)
    y = rng.standard_normal((rows, tasks)).astype(np.float32)
    w = make_weights(rng, rows, tasks, weight_kind)
    ref_loss, ref_d = R.l2_loss_ref(x, y, w)
    wg = None if w is None else _dev(w)
    loss, dx, probs = ops.loss_fwd_bwd(1, _dev(x), _dev(y), wg, want_probs=True)
    loss2, _, _ = ops.loss_fwd_bwd(1, _dev(x), _dev(y), wg)
    e_loss, e_d = abs(float(loss) - ref_loss) / max(1.0, abs(ref_loss)), _err(dx, ref_d)
    print("l2 items=%d w=%s: loss %.9g ref %.9g err %.3e | gradient %.3e | allowed %.1e" % (items, weight_kind, float(loss),
                                                                                          ref_loss, e_loss, e_d, TOL))
    assert probs is None and e_loss <= TOL and e_d <= TOL
    assert torch.equal(loss.view(torch.int32), loss2.view(torch.int32))
    if weight_kind == "zero":
        assert float(loss) == 0.0 and not _np(dx).any()


@pytest.mark.parametrize("items,classes", [(8192 * 256 + 3, 2), (3, 2), (1000, 1), (1000, 3), (1000, 7), (3, 7)],
                         ids=lambda v: str(v))
def test_softmax_alone(items, classes):
    """8192 * 256 + 3 items: three items of the second trip of the grid-stride loop; rows sum to 1 within 1e-6."""
    from deepchem_amd import ops
    rng = np.random.RandomState(classes)
    x = rng.standard_normal((items, classes)).astype(np.float32)
    x[-1] = 50.0 * rng.choice([-1.0, 1.0], size=classes)  # (the last item of all, on the second trip when there is one)
    p = ops.softmax_lastdim(_dev(x))
    ref = R.softmax_ref(x)
    err = _err(p, ref)
    row_sum = float(np.abs(_np(p).sum(-1) - 1.0).max())
    print("softmax items=%d classes=%d: err %.3e allowed %.1e, |row sum - 1| %.3e allowed 1e-6" % (items, classes, err,
                                                                                                  TOL, row_sum))
    assert err <= TOL and row_sum <= 1e-6
    if classes == 1:
        assert bool((p == 1).all())
    # a 3-D view (rows, tasks, classes) is the same computation
    if items % 4 == 0:
        assert torch.equal(ops.softmax_lastdim(_dev(x).view(items // 4, 4, classes)).view(items, classes), p)
