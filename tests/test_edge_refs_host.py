"""The float64 restatements of tests/edge_refs.py, checked without a device: against torch in float64, against the
oracle's GraphGather, and the exactness conditions the GPU edge tests lean on (integer features under power-of-two
scales are exact in float32; molecules of at most 64 atoms keep a float32 sum inside TOL)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import graphconv_oracle as O
from tests import edge_refs as R


def _close(a, b, tol=1e-12):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape
    assert float(np.abs(a - b).max()) <= tol * max(1.0, float(np.abs(b).max()))


@pytest.mark.parametrize("n,f", [(2, 3), (53, 76), (777, 64)])
def test_bn_ref_is_torch_batch_norm_in_float64(n, f):
    rng = np.random.RandomState(n)
    x, dy = rng.standard_normal((n, f)) * 2 + 1, rng.standard_normal((n, f))
    gamma, beta = rng.rand(f) + 0.5, rng.standard_normal(f)
    rm0, rv0 = rng.standard_normal(f), rng.rand(f) + 0.5
    ref = R.bn_ref(x, gamma, beta, dy)
    xt = torch.from_numpy(x).requires_grad_(True)
    gt, bt = torch.from_numpy(gamma).requires_grad_(True), torch.from_numpy(beta).requires_grad_(True)
    rm, rv = torch.from_numpy(rm0.copy()), torch.from_numpy(rv0.copy())
    for _ in range(2):
        y = F.batch_norm(xt, rm, rv, gt, bt, True, R.BN_MOMENTUM, R.BN_EPS)
    y.backward(torch.from_numpy(dy))
    _close(ref["y"], y.detach().numpy())
    _close(ref["dx"], xt.grad.numpy())
    _close(ref["dgamma"], gt.grad.numpy())
    _close(ref["dbeta"], bt.grad.numpy())
    _close(R.bn_running_ref(rm0, ref["mean"], 2), rm.numpy())
    _close(R.bn_running_ref(rv0, ref["unbiased"], 2), rv.numpy())
    s, h = R.bn_fold_eval_ref(gamma, beta, rm0, rv0)
    _close(x * s + h, F.batch_norm(torch.from_numpy(x), torch.from_numpy(rm0), torch.from_numpy(rv0),
                                   torch.from_numpy(gamma), torch.from_numpy(beta), False, 0.0, R.BN_EPS).numpy())


def test_bn_ref_one_row_and_constant_column():
    x = np.array([[1.5, -2.0, 0.25]])
    ref = R.bn_ref(x, np.ones(3), np.zeros(3), np.ones((1, 3)))
    assert (ref["var"] == 0).all() and (ref["unbiased"] == 0).all()
    _close(ref["invstd"], np.full(3, 1 / np.sqrt(R.BN_EPS)))
    assert (ref["dx"] == 0).all() and (ref["dgamma"] == 0).all()
    x = np.random.RandomState(0).standard_normal((9, 2))
    x[:, 1] = 2.5
    ref = R.bn_ref(x, np.ones(2), np.zeros(2), np.ones((9, 2)))
    assert ref["var"][1] == 0 and np.isfinite(ref["dx"]).all()


def test_bn_ref_f32_follows_bn_ref_on_well_conditioned_input():
    rng = np.random.RandomState(3)
    x, dy = (rng.standard_normal((777, 64)) * 2 + 1).astype(np.float32), rng.standard_normal((777, 64)).astype(np.float32)
    gamma, beta = (rng.rand(64) + 0.5).astype(np.float32), rng.standard_normal(64).astype(np.float32)
    a, b = R.bn_ref(x, gamma, beta, dy), R.bn_ref_f32(x, gamma, beta, dy)
    for k in ("mean", "invstd", "scale", "shift", "y", "dgamma", "dbeta", "dx", "unbiased"):
        _close(b[k], a[k], 1e-5)


@pytest.mark.parametrize("classes", [1, 2, 3, 5])
def test_ce_loss_ref_is_torch_in_float64(classes):
    rng = np.random.RandomState(classes)
    x = rng.standard_normal((37, 4, classes))
    hard = np.eye(classes)[rng.randint(0, classes, size=(37, 4))]
    soft = rng.rand(37, 4, classes) * 2.5
    w = rng.rand(37, 4) * 3
    for y in (hard, soft):
        xt = torch.from_numpy(x).requires_grad_(True)
        logp = F.log_softmax(xt, -1)
        ref = (torch.from_numpy(w) * -(torch.from_numpy(y) * logp).sum(-1)).mean()
        ref.backward()
        loss, dlogits, p = R.ce_loss_ref(x, y, w)
        _close(loss, float(ref.detach()))
        _close(dlogits, xt.grad.numpy())
        _close(p, F.softmax(xt.detach(), -1).numpy())
    # one-hot labels, weights None: F.cross_entropy itself
    ce = F.cross_entropy(torch.from_numpy(x).reshape(-1, classes), torch.from_numpy(hard.argmax(-1)).reshape(-1))
    _close(R.ce_loss_ref(x, hard, None)[0], float(ce))


def test_ce_loss_ref_is_the_oracle_batch_loss():
    rng = np.random.RandomState(1)
    x = torch.from_numpy(rng.standard_normal((37, 12, 2)))
    y = F.one_hot(torch.from_numpy(rng.randint(0, 2, size=(37, 12))), 2).double()
    w = torch.from_numpy((rng.rand(37, 12) > 0.2).astype(np.float64))
    _close(R.ce_loss_ref(x.numpy(), y.numpy(), w.numpy())[0], float(O.batch_loss(O.ModelConfig(12), [x], y, w)))
    xl, yl = torch.from_numpy(rng.standard_normal((37, 12))), torch.from_numpy(rng.standard_normal((37, 12)))
    _close(R.l2_loss_ref(xl.numpy(), yl.numpy(), w.numpy())[0],
           float(O.batch_loss(O.ModelConfig(12, mode="regression"), [xl], yl, w)))


def test_l2_loss_ref_gradient():
    rng = np.random.RandomState(2)
    x, y, w = rng.standard_normal((9, 5)), rng.standard_normal((9, 5)), rng.rand(9, 5)
    xt = torch.from_numpy(x).requires_grad_(True)
    (torch.from_numpy(w) * (xt - torch.from_numpy(y)) ** 2).mean().backward()
    _close(R.l2_loss_ref(x, y, w)[1], xt.grad.numpy())


def test_extreme_logits_stay_finite_in_the_reference():
    x = np.array([[1e4, -1e4], [-1e4, 1e4], [80.0, -80.0], [-80.0, 80.0], [3.0, 3.0]])
    loss, d, p = R.ce_loss_ref(x, np.eye(2)[[1, 1, 0, 1, 0]], None)
    assert np.isfinite(loss) and np.isfinite(d).all()
    assert p.astype(np.float32).tolist() == [[1, 0], [0, 1], [1, 0], [0, 1], [0.5, 0.5]]


@pytest.mark.parametrize("n_deg,n_fill", [(11, 20), (5, 17)])
def test_readout_ref_is_the_oracle_graph_gather(n_deg, n_fill):
    counts = R.readout_batch(n_deg, n_fill, seed=n_deg)
    deg_counts, membership = R.hand_batch(counts)
    n_mols, n_atoms = counts.shape[0], int(sum(deg_counts))
    assert n_atoms == membership.shape[0] and counts.sum(1).max() == 64
    # the batch has what the GPU test is about
    sizes = counts.sum(1)
    assert sizes[0] == 0 and sizes[-1] == 0 and (sizes[1:-1] == 0).any()
    assert set((1, 3, 4, 5, 8, 9, 12, 13, 25)) <= set(sizes.tolist())
    assert ((counts > 0).sum(1) == n_deg).any() and ((counts > 0).sum(1) == 1).any()
    assert any(c[0] > 0 and c[-1] > 0 and not c[1:-1].any() for c in counts)
    for d in range(n_deg):  # ascending inside every degree block
        blk = membership[sum(deg_counts[:d]):sum(deg_counts[:d + 1])]
        assert (np.diff(blk) >= 0).all()
    rng = np.random.RandomState(0)
    x = rng.standard_normal((n_atoms, 7)).astype(np.float32)  # (the oracle sums in float32, as the reference does)
    xt = torch.from_numpy(x).requires_grad_(True)
    deg_slice = torch.zeros((n_deg, 2), dtype=torch.int64)
    for tanh in (False, True):
        ref = O.graph_gather([xt, deg_slice, torch.from_numpy(membership)], n_mols,
                             activation=torch.tanh if tanh else None)
        out, arg = R.readout_ref(x, membership, n_mols, tanh=tanh)
        refn = ref.detach().numpy()
        assert np.array_equal(np.isfinite(out), np.isfinite(refn))
        assert tanh or np.array_equal(out[:, 7:], refn[:, 7:])  # a maximum is one of the inputs
        _close(np.where(np.isfinite(out), out, 0.0), np.where(np.isfinite(refn), refn, 0.0), 1e-6)
        assert ((arg == -1).all(1) == (sizes == 0)).all()
        # gradient of <out, dout> on the finite entries
        dout = rng.standard_normal(out.shape)
        fin = torch.isfinite(ref)
        g, = torch.autograd.grad((torch.where(fin, ref, torch.zeros_like(ref)) * torch.from_numpy(dout).float()).sum(), xt)
        _close(R.readout_bwd_ref(dout, np.where(np.isfinite(out), out, 0.0), arg, membership, tanh), g.numpy(), 1e-5)


def test_readout_ref_first_maximum_and_folded_affine():
    membership = np.array([1, 1, 1, 2], np.int32)
    x = np.array([[1.0, 2.0], [3.0, 2.0], [3.0, -1.0], [0.0, 0.0]])
    out, arg = R.readout_ref(x, membership, 4)
    assert arg.tolist() == [[-1, -1], [1, 0], [3, 3], [-1, -1]]
    assert out[1].tolist() == [7.0, 3.0, 3.0, 2.0] and np.isneginf(out[0, 2:]).all() and (out[0, :2] == 0).all()
    out, arg = R.readout_ref(x, membership, 4, scale=np.array([-1.0, 0.0]), shift=np.array([0.5, 2.0]), tanh=True)
    assert arg[1].tolist() == [0, 0]  # a negative scale turns the order round, a zero scale ties every row
    assert out[0].tolist() == [0.0, 0.0, -1.0, -1.0]


def test_integer_features_with_power_of_two_scales_are_exact_in_float32():
    """What the exact pass of the readout test leans on: x in [-3, 3], scale a signed power of two (or 0), shift a
    small integer -> x * scale + shift and the sum over at most 64 rows are multiples of 1/2 below 2^24, exact in
    float32 in any order and with or without a fused multiply-add."""
    rng = np.random.RandomState(0)
    x = rng.randint(-3, 4, size=(64, 512)).astype(np.float32)
    scale = (rng.choice([-1.0, 1.0], size=512) * 2.0 ** rng.randint(-1, 3, size=512)).astype(np.float32)
    scale[::7] = 0
    shift = rng.randint(-2, 3, size=512).astype(np.float32)
    a32 = x * scale + shift
    a64 = x.astype(np.float64) * scale + shift
    assert np.array_equal(a32.astype(np.float64), a64)
    s32 = np.zeros(512, np.float32)
    for r in range(64):
        s32 += a32[r]
    assert np.array_equal(s32.astype(np.float64), a64.sum(0))
    assert np.abs(a64).sum(0).max() < 2 ** 24


def test_float32_sums_over_64_rows_stay_inside_tol():
    """Standard forward bound of a float32 sum of n terms, in any order: (n - 1) eps32 sum|terms|.  With a fused
    x * scale + shift in front (one more rounding per term) 64 rows give 65 * 2^-24 * sum|a|, and the test's bound
    is TOL * max|ref| over the matrix: it holds as long as sum|a| <= 25 max|ref|, which the check below confirms
    for the distribution the GPU test draws (and a float32 sum run here stays far inside)."""
    rng = np.random.RandomState(1)
    a = rng.standard_normal((64, 2048)).astype(np.float32)
    ref = a.astype(np.float64).sum(0)
    worst_bound = 65 * 2.0 ** -24 * np.abs(a.astype(np.float64)).sum(0).max()
    assert worst_bound < R.TOL * np.abs(ref).max()
    s = np.zeros(2048, np.float32)
    for r in range(64):
        s += a[r]
    assert np.abs(s - ref).max() < R.TOL * np.abs(ref).max()


def test_dispatch_restatement_matches_the_branches_the_edge_tests_name():
    """tests/edge_refs.py restates launch_col_sums / readout_fwd_impl to label the cases: the figures the edge tests
    are built on."""
    b = R.bn_branch
    assert (b(777, 3, True)["V"], b(777, 3, True)["ry"], b(777, 3, True)["idle"]) == (1, 85, 1)
    assert (b(777, 4, True)["lpr"], b(777, 4, True)["ry"], b(777, 4, True)["round_rows"]) == (1, 256, 1024)
    assert (b(777, 76, True)["lpr"], b(777, 76, True)["ry"], b(777, 76, True)["idle"]) == (19, 13, 9)
    assert (b(777, 76, True)["round_rows"], b(777, 64, True)["round_rows"]) == (52, 64)
    assert (b(777, 100, True)["lpr"], b(777, 100, True)["ry"]) == (25, 10)
    assert (b(777, 255, True)["V"], b(777, 255, True)["lx"], b(777, 255, True)["ry"]) == (1, 255, 1)
    assert (b(777, 257, True)["V"], b(777, 257, True)["col_passes"]) == (1, 2)
    assert (b(777, 1028, True)["lpr"], b(777, 1028, True)["col_passes"]) == (257, 2)
    assert b(777, 64, False)["V"] == 1
    big = b(2048 * 512 + 1, 8, True)
    assert (big["rpb"], big["blocks"], big["last_rows"]) == (1024, 1025, 1)
    assert b(2048 * 512, 8, True)["rpb"] == 512
    assert (b(513, 64, True, 512)["blocks"], b(257, 64, True, 256)["blocks"], b(256, 64, True, 256)["blocks"]) == (2, 2, 1)
    r = R.readout_branch
    assert [r(w, 11)["pipelined"] for w in (32, 64, 128, 256, 96, 512, 2048)] == [False, True, True, True, False, False,
                                                                                False]
    assert r(32, 5)["pipelined"] and (r(75, 11)["V"], r(75, 11)["mpb"], r(75, 11)["idle"]) == (1, 3, 31)
    assert (r(2048, 11)["col_passes"], r(96, 11)["gl"], r(512, 11)["gl"]) == (2, 24, 128)
    # 300 is a multiple of 4: contiguous rows give V = 4, 75 lanes per molecule; the V = 1 column loop at this width
    # needs rows that are not 16-byte addressable (a misaligned column slice), and 301 loops in any layout
    assert (r(300, 11)["V"], r(300, 11)["gl"], r(300, 11)["mpb"], r(300, 11)["col_passes"]) == (4, 75, 3, 1)
    assert (r(300, 11, vec4=False)["V"], r(300, 11, vec4=False)["col_passes"], r(301, 11)["col_passes"]) == (1, 2, 2)
