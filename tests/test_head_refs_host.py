"""The float64 restatement of the per-molecule head backward (tests/edge_refs.py: head_bwd_ref, head_sums_ref) held to
two independent statements on the host, and the exactness conditions tests/test_gpu_head_bwd.py leans on.  No device.

  * torch autograd in float64 of loss(tanh(pre) . W^T + b) with the losses written as in models/losses.py
    (mse_loss(reduction='none'); -(labels * log_softmax(output)).sum(-1); the mean of loss * weights), gradients w.r.t.
    pre, W and b, for every loss kind and class count the GPU file uses, with label rows that are not one-hot, zero
    weights and padding molecules;
  * for the BatchNorm sums the row-level definition: on a collated batch (edge_refs.readout_batch, molecules without
    atoms included) dy of readout_dy_ref and xhat of the rows, summed over the rows, against the per-molecule formula;
  * every integer case of the GPU file is exact (exactness_failures), the float32 chain stays within a few units of
    float64, and the case lists name every case once.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

from tests import edge_refs as R
from tests import test_gpu_head_bwd as G

# (kind, classes) the GPU file uses, each at a small shape of its own
KINDS = sorted({(c["kind"], c["classes"]) for c in G.NARROW + G.WIDE + G.SWITCHED})


def _autograd(kind, x_rows, y, w, pre, W, b, n_rows):
    """loss and its gradients by torch in float64.  x_rows: only the shape is used (logits are recomputed)."""
    pre_t = torch.tensor(pre, dtype=torch.float64, requires_grad=True)
    W_t = torch.tensor(W, dtype=torch.float64, requires_grad=True)
    b_t = torch.tensor(b, dtype=torch.float64, requires_grad=True)
    out = (torch.tanh(pre_t) @ W_t.T + b_t)[:n_rows].reshape(x_rows.shape)
    labels = torch.tensor(y, dtype=torch.float64)
    if kind == 0:
        per = -(labels * Fn.log_softmax(out, dim=-1)).sum(dim=-1)
    else:
        per = Fn.mse_loss(out, labels, reduction='none')
    weights = torch.ones(per.shape, dtype=torch.float64) if w is None else torch.tensor(w, dtype=torch.float64)
    loss = (per * weights).mean()
    loss.backward()
    return float(loss.detach()), out.detach().numpy(), pre_t.grad.numpy(), W_t.grad.numpy(), b_t.grad.numpy()


@pytest.mark.parametrize("kind,classes", KINDS)
@pytest.mark.parametrize("data,weights", [("acc", False), ("acc", True), ("sat", True)])
def test_head_bwd_ref_is_autograd(kind, classes, data, weights):
    if data == "sat" and (kind == 1 or classes == 1):
        data = "acc"
    tasks, mols, rows = 5, 9, 6  # three padding molecules
    c = G.C(data, kind, tasks, classes, mols, rows=rows, weights=weights)
    rng = np.random.default_rng(classes + 10 * kind)
    _, y = G._logits_labels(c, rng)  # labels of every style; the logits come from the model below
    y = y[:rows].astype(np.float64)
    w = None
    if weights:
        w = (0.5 + rng.random((rows, tasks))) * (rng.random((rows, tasks)) < 0.7)
        assert (w == 0).any()
    pre, W, b = rng.standard_normal((mols, 256)), rng.standard_normal((c["tc"], 256)) * 0.2, rng.standard_normal(c["tc"])
    if data == "sat":  # saturated logits through the bias
        b = b + rng.choice(np.array([0.0, 30.0, -100.0]), c["tc"])
        assert np.any(y.sum(-1) == 0) and np.any(y.sum(-1) == 2) and np.any(np.isclose(y.sum(-1), 0.3))
    loss, logits, dpre, dW, db = _autograd(kind, y, y, w, pre, W, b, rows)
    fp = np.tanh(pre)
    ref = R.head_bwd_ref(kind, logits, y, w, rows, fp, W)
    count = rows * tasks
    assert abs(ref["loss"] / count - loss) <= 1e-13 * max(abs(loss), 1.0)
    for got, want in ((ref["g2"], dpre), (ref["dw"], dW), (ref["db"], db)):
        assert np.abs(got - want).max() <= 1e-13 * max(np.abs(want).max(), 1e-30), (kind, classes, data)
    assert np.all(ref["dl"][rows:] == 0) and np.all(ref["g2"][rows:] == 0) and np.all(dpre[rows:] == 0)
    # the magnitudes dominate the values
    for k in ("dl", "g2", "dw", "db"):
        assert np.all(np.abs(ref[k]) <= ref["S_" + k] * (1 + 1e-12) + 1e-300), k
    assert abs(ref["loss"]) <= ref["S_loss"] * (1 + 1e-12)


def _runs_of(counts):
    """(n_mols, n_deg, 2) row runs of a counts[m][d] table: rows sorted by degree, then by molecule."""
    counts = np.asarray(counts, np.int64)
    runs = np.zeros(counts.shape + (2,), np.int32)
    row = 0
    for d in range(counts.shape[1]):
        for m in range(counts.shape[0]):
            runs[m, d] = (row, row + counts[m, d])
            row += counts[m, d]
    return runs


@pytest.mark.parametrize("n_deg,n_fill,seed", [(2, 5, 0), (5, 20, 1), (11, 40, 2)])
def test_head_sums_ref_is_the_row_sum(n_deg, n_fill, seed):
    """sum over the rows of dy and of dy * xhat equals n g and g (rawsum - n mu) invstd for the sum half plus g and
    g (rawmax - mu) invstd where arg >= 0 for the max half -- molecules without atoms included."""
    counts = R.readout_batch(n_deg, n_fill, seed)
    _, membership = R.hand_batch(counts)
    n_mols = counts.shape[0]
    assert (counts.sum(1) == 0).sum() >= 4 and counts[0].sum() == 0 and counts[-1].sum() == 0
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((membership.shape[0], G.F)).astype(np.float32)
    mean, invstd = x.astype(np.float64).mean(0).astype(np.float32), (1.0 / np.sqrt(x.astype(np.float64).var(0) + R.BN_EPS)).astype(np.float32)
    out, arg = R.readout_ref(x, membership, n_mols)
    rawsum = out.astype(np.float32)
    assert np.all((arg < 0) == np.isinf(out[:, G.F:]))
    rawsum[:, G.F:][arg < 0] = np.nan  # not looked at
    g2 = rng.standard_normal((n_mols, 256)).astype(np.float32)
    dy, dy_mag = R.readout_dy_ref(g2, arg, membership, G.F)
    xhat = (R.f64(x) - R.f64(mean)) * R.f64(invstd)
    want = np.stack([dy.sum(0), (dy * xhat).sum(0)])
    si = dict(runs=_runs_of(counts), arg=arg.astype(np.int32), rawsum=rawsum, mean=mean, invstd=invstd)
    # the runs are the membership
    for m in range(n_mols):
        rows = np.concatenate([np.arange(a, b) for a, b in si["runs"][m]])
        assert np.array_equal(np.sort(rows), np.nonzero(membership == m)[0])
    sums, S = R.head_sums_ref(g2, si)
    scale = np.stack([dy_mag.sum(0), (dy_mag * np.abs(xhat)).sum(0)])
    # rawsum is the float32 rounding of the row sums: 2^-24 of the sum's own magnitude per molecule
    assert np.all(np.abs(sums.astype(np.float64) - want) <= 1e-6 * np.maximum(scale, S)), np.abs(sums.astype(np.float64) - want).max()
    assert np.all(S >= np.abs(sums.astype(np.float64)) * (1 - 1e-12))
    for rev in (True, False):
        assert np.all(np.abs(R.head_sums_seq64(g2, si, rev) - sums.astype(np.float64)) <= 64 * G.U53 * S)
    # exactly, with rawsum kept in float64 and dyadic statistics: the two statements agree to float64 rounding
    si64 = dict(si, rawsum=np.where(np.isfinite(out), out, 0.0), mean=R.f64(mean), invstd=R.f64(invstd))
    (a1, b1, a2, b2), _ = R._head_sums_terms(R.f64(g2), si64, np.float64)
    assert np.all(np.abs(np.stack([(a1 + b1).sum(0), (a2 + b2).sum(0)]) - want) <= 1e-11 * np.maximum(scale, 1.0))


def test_case_lists_name_every_case_once():
    ids = [G.case_id(c) for c in G.NARROW + G.WIDE]
    assert len(set(ids)) == len(ids)
    assert len({G.case_id(c) for c in G.SWITCHED}) == len(G.SWITCHED)
    assert all(c["wide"] == (c["tc"] > 32) for c in G.NARROW + G.WIDE) and all(c["wide"] and c["tc"] <= 32 for c in G.SWITCHED)
    assert {c["tc"] for c in G.SWITCHED} == {1, 2, 15, 16, 17, 32}
    # every mechanism has an integer case and an accuracy case, with and without sums
    for cases in (G.NARROW, G.WIDE):
        for data in ("int", "acc"):
            assert {bool(c["sums"]) for c in cases if c["data"] == data} == {True, False}
            assert {c["weights"] for c in cases if c["data"] == data} == {True, False}
            assert {c["db"] for c in cases if c["data"] == data} == {True, False}
            assert any(c["rows"] == 1 for c in cases if c["data"] == data)
            assert any(c["empties"] for c in cases if c["data"] == data)
            assert any(c["starts"] for c in cases if c["data"] == data)


INT_CASES = [c for c in G.NARROW + G.WIDE + G.SWITCHED if c["data"] == "int"]


@pytest.mark.parametrize("c", INT_CASES, ids=G.case_id)
def test_integer_cases_are_exact(c):
    d = G.build(c)
    assert G.exactness_failures(d) == []
    # and the inputs the kernels must not use are NaN
    assert np.isnan(d["fp"][:, 256:]).all()
    if c["rows"] < c["mols"]:
        assert np.isnan(d["logits"][c["rows"]:]).all() and np.isnan(d["labels"][c["rows"]:]).all()
    if d["si"] is not None and c["empties"]:
        assert np.isnan(d["si"]["rawsum"][list(c["empties"]), G.F:]).all() and np.isfinite(d["si"]["rawsum"][:, :G.F]).all()


@pytest.mark.parametrize("c", [c for c in G.NARROW + G.WIDE + G.SWITCHED if c["data"] != "int" and c["mols"] <= 100],
                         ids=G.case_id)
def test_float32_chain_is_close_to_float64(c):
    """head_bwd_f32 is head_bwd_ref's chain: within 64 units of 2^-24 of S (saturated items: the rounding of a logit
    difference of 30 is 16 units of a probability), the one-exponential two-class form included."""
    d = G.build(c)
    ref = d["ref"]
    got = R.head_bwd_f32(c["kind"], d["logits"], d["labels"], d["weights"], c["rows"], d["fp"][:, :256], d["w"], c["wide"])
    limit = 256.0 if c["data"] == "sat" else 16.0
    for k in ("dl", "g2", "dw", "db"):
        start = d[k + "0"] if k in ("dw", "db") else 0.0
        assert R.head_err_units(got[k] + start, ref[k], ref["S_" + k]) <= limit, k
    assert abs(got["loss"] + d["loss0"].sum() - ref["loss"]) <= limit * R.U24 * max(ref["S_loss"], R.TINY32)
