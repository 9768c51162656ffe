"""The restatements of the persistent block kernels in tests/edge_refs.py and the case tables of
tests/test_gpu_fused_edges.py, checked without a device: block_bwd_ref, readout_dy_ref, psums_ref and bn_sums_ref against
torch autograd in float64; the any-order exactness condition of every exact case, the fp32 partial sums of the periodic
flushes included; every probe exact under the term subset its form claims and wrong with one seen term removed; and, by
emulating each form one term short, that the accuracy bounds of the GPU file would catch a kernel that lost that term."""
import numpy as np
import pytest
import torch

from tests import edge_refs as R
from tests import test_gpu_fused_edges as F
from tests import test_gpu_product_edges as P

SEGS = ((0, 0), (0, 1), (1, 38), (40, 40), (40, 111), (111, 120))  # empty, one row, ragged, a gap, empty, 125 rows
N, EPS = 125, 1e-3


def _minus(terms, t):
    return tuple(x for x in terms if x != t)


def _bn_coef(x, gamma, dy, rows):
    """[A | B | C] of the BatchNorm backward over ``rows`` of x (bn.hip: dx = A dy + B x + C), in float64."""
    b = R.bn_ref(x[rows], gamma, np.zeros_like(gamma), dy[rows], EPS)
    n = int(rows.sum())
    A = gamma * b["invstd"]
    B = -A * b["invstd"] * b["dgamma"] / n
    return np.concatenate([A, B, -A * b["dbeta"] / n - B * b["mean"]])


# ------------------------------------------------------------------------------------------------ float64 restatements
def test_block_bwd_ref_is_autograd_of_a_graphconv_block():
    """relu(S W_rel[s] + X W_self[s] + b[s]) -> BatchNorm (training) -> <., dy>: the gradients of the weights, the bias,
    S and X; one segment without neighbour term, one sharing nothing, rows outside every segment."""
    rng = np.random.default_rng(0)
    begin, end = [b for b, _ in SEGS], [e for _, e in SEGS]
    n_seg, k, W = len(SEGS), 7, 5
    cov = P._covered(begin, end, N)
    S, X = rng.standard_normal((N, k + 1)), rng.standard_normal((N, k))
    w = rng.standard_normal(n_seg * 2 * k * W)
    bias, gamma, dy = rng.standard_normal(n_seg * W), rng.standard_normal(W), rng.standard_normal((N, W))
    w_off = [[-1 if s == 1 else (2 * s) * k * W for s in range(n_seg)], [(2 * s + 1) * k * W for s in range(n_seg)]]
    b_off = [-1 if s == 4 else s * W for s in range(n_seg)]
    tS, tX, tw, tb = (torch.tensor(a, requires_grad=True) for a in (S, X, w, bias))
    pre = torch.zeros((N, W), dtype=torch.float64)
    for s in range(n_seg):
        r = slice(begin[s], end[s])
        y = tX[r, :k] @ tw[w_off[1][s]:w_off[1][s] + k * W].reshape(k, W)
        if w_off[0][s] >= 0:
            y = y + tS[r, :k] @ tw[w_off[0][s]:w_off[0][s] + k * W].reshape(k, W)
        if b_off[s] >= 0:
            y = y + tb[b_off[s]:b_off[s] + W]
        pre = pre + torch.nn.functional.pad(y, (0, 0, begin[s], N - end[s]))
    gc = torch.relu(pre)
    tcov = torch.tensor(cov)
    out = torch.nn.functional.batch_norm(gc[tcov], None, None, torch.tensor(gamma), torch.zeros(W, dtype=torch.float64), True, 0.0, EPS)
    (out * torch.tensor(dy)[tcov]).sum().backward()
    gcn = gc.detach().numpy()
    coef = _bn_coef(gcn, gamma, dy, cov)
    ref = R.block_bwd_ref(begin, end, w_off, b_off, dy, gcn, coef, [S, X], k, w, np.zeros_like(w), np.zeros_like(bias), W, False)
    scale = lambda a: np.abs(a).max()  # noqa: E731
    assert np.abs(ref["dw"] - tw.grad.numpy()).max() <= 1e-12 * scale(tw.grad.numpy())
    assert np.abs(ref["db"] - tb.grad.numpy()).max() <= 1e-12 * scale(tb.grad.numpy())
    for o, t in enumerate((tS, tX)):
        assert np.abs(ref["din"][o][cov] - t.grad.numpy()[cov, :k]).max() <= 1e-12 * scale(t.grad.numpy())
        assert np.isnan(ref["din"][o][~cov]).all()
    assert np.all(ref["din"][0][begin[1]:end[1]] == 0) and np.all(ref["S_din"][0][begin[1]:end[1]] == 0)
    assert np.all(ref["S_dw"] >= np.abs(ref["dw"]) - 1e-12) and np.all(ref["S_db"] >= np.abs(ref["db"]) - 1e-12)
    # psums: the weighting by the segment index, and the products with the block's own inputs
    seg = np.zeros(N)
    for s in range(n_seg):
        seg[begin[s]:end[s]] = s
    dS, dX = np.where(cov[:, None], ref["din"][0], 0.0), np.where(cov[:, None], ref["din"][1], 0.0)
    want = np.stack([(seg[:, None] * dS + dX).sum(0), (dS * S[:, :k] + dX * X[:, :k]).sum(0)])
    got = R.psums_ref(begin, end, ref["din"], [S, X], k, True)
    assert np.abs(got - want).max() <= 1e-12 * scale(want)
    # without coefficient vectors: relu' alone
    ref0 = R.block_bwd_ref(begin, end, w_off, b_off, dy, gcn, None, [S, X], k, w, np.zeros_like(w), None, W, False)
    assert np.array_equal(ref0["G"], np.where(gcn > 0, dy, 0.0)) and ref0["db"] is None


def test_block_bwd_ref_is_autograd_of_the_dense_block_behind_the_readout():
    """relu(P W^T + b) -> BatchNorm -> per molecule [sum | max] -> <., g2>: readout_dy_ref recomputes the gradient of
    the BatchNorm output, block_bwd_ref (nn.Linear layout) the rest; psums_ref the dense form."""
    rng = np.random.default_rng(1)
    n, k, W = 60, 6, 4
    membership, _, _ = F._readout(n, n, rng, "normal", W)
    n_mols = int(membership.max()) + 1
    Pm, w, bias, gamma = rng.standard_normal((n, k)), rng.standard_normal(W * k), rng.standard_normal(W), rng.standard_normal(W)
    beta, g2 = rng.standard_normal(W), rng.standard_normal((n_mols, 2 * W + 3))
    tP, tw, tb = (torch.tensor(a, requires_grad=True) for a in (Pm, w, bias))
    gc = torch.relu(torch.nn.functional.linear(tP, tw.reshape(W, k), tb))
    y = torch.nn.functional.batch_norm(gc, None, None, torch.tensor(gamma), torch.tensor(beta), True, 0.0, EPS)
    tm = torch.tensor(membership.astype(np.int64))
    parts = [torch.cat([y[tm == m].sum(0), y[tm == m].max(0).values]) for m in range(n_mols)]
    (torch.stack(parts) * torch.tensor(g2[:, :2 * W])).sum().backward()
    _, arg = R.readout_ref(y.detach().numpy(), membership, n_mols)
    dy, mag = R.readout_dy_ref(g2, arg, membership, W)
    assert np.array_equal(dy, R.readout_bwd_ref(g2[:, :2 * W], g2[:, :2 * W], arg, membership, False))
    assert np.all(mag >= np.abs(dy) - 1e-12)
    gcn = gc.detach().numpy()
    coef = _bn_coef(gcn, gamma, dy, np.ones(n, bool))
    ref = R.block_bwd_ref([0], [n], [[0]], [0], dy, gcn, coef, [Pm], k, w, np.zeros_like(w), np.zeros_like(bias), W, True, mag)
    for got, t in ((ref["dw"], tw), (ref["db"], tb), (ref["din"][0], tP)):
        assert np.abs(got - t.grad.numpy()).max() <= 1e-12 * np.abs(t.grad.numpy()).max()
    dP = tP.grad.numpy()
    want = np.stack([dP.sum(0), (dP * Pm).sum(0)])
    assert np.abs(R.psums_ref([0], [n], ref["din"], [Pm], k, False) - want).max() <= 1e-12 * np.abs(want).max()
    # an arg entry that names a row of ANOTHER molecule never matches
    arg2 = arg.copy()
    arg2[0, 0] = int(np.nonzero(membership == 1)[0][0])
    dy2, _ = R.readout_dy_ref(g2, arg2, membership, W)
    rows0 = membership == 0
    assert np.array_equal(dy2[rows0, 0], g2[0, 0] * np.ones(rows0.sum())) and np.array_equal(dy2[~rows0], dy[~rows0])


def test_bn_sums_and_the_accumulator_layout():
    rng = np.random.default_rng(2)
    out, cov = rng.standard_normal((9, 4)), np.array([1, 1, 0, 1, 1, 1, 0, 1, 1], bool)
    t = torch.tensor(out[cov])
    assert np.allclose(R.bn_sums_ref(out, cov), torch.stack([t.sum(0), (t * t).sum(0)]).numpy(), rtol=1e-14)
    acc = R.fresh_acc(4, -7.5)
    assert acc.size > 66 * 4 and np.array_equal(R.read_acc(acc, 4, -7.5), np.zeros((2, 4)))
    acc[8 + 3 * 8 + 4 + 1] += 2.0  # replica 3, second half (sum of squares), column 1
    acc[8 + 31 * 8 + 0] += 1.0     # replica 31, first half, column 0
    assert np.array_equal(R.read_acc(acc, 4, -7.5), [[1, 0, 0, 0], [0, 2, 0, 0]])
    for bad in (0, 7, 8 + 32 * 8):  # the first 2F doubles and the double behind the last replica
        broken = acc.copy()
        broken[bad] = 0.0
        with pytest.raises(AssertionError):
            R.read_acc(broken, 4, -7.5)


# ------------------------------------------------------------------------------------------------ exact cases
@pytest.mark.parametrize("name", list(F.FWD_INT) + list(F.FWD_LONG) + list(F.FWD_PROBE))
def test_forward_exact_cases_are_exact_in_any_order(name):
    c = {**F.FWD_INT, **F.FWD_LONG, **F.FWD_PROBE}[name]
    d = F.build_fwd(c)
    ref, S, stored = F.fwd_ref(d)
    cols = slice(d["col0"], d["col0"] + d["n_out"])
    cov, lsb = d["covered"], d["lsb"]
    for o in (1, 2):  # every operand entry is one bf16 piece in the integer cases, finite where the kernel reads it
        a = d["a%d" % o]
        if a is not None and c["kind"] == "int":
            v = a[cov, :d["k%d" % o]]
            v = v[np.isfinite(v)]  # (float rows: NaN where a term is absent)
            assert np.array_equal(R.bf16_round(v), v)
    assert R.is_multiple(ref[cov, cols], lsb) and R.any_order_exact(S, lsb), name
    assert np.array_equal(ref, stored), name + ": an exact result that bf16 does not hold"
    # the fp32 partial sums between two flushes: at most period x rows-per-thread values, and their squares
    _, _, period, per_thread = F.fwd_walk(d["shape"], d["form"])
    top = np.abs(ref[cov, cols]).max() if d["stats"] else 0.0
    assert period * per_thread * top < 2.0 ** 24 * lsb and period * per_thread * top * top < 2.0 ** 24 * lsb * lsb, name
    if c["form"] != "f32":  # fwd_bf16.hip's contract on the padding columns and on absent operands
        for o in (1, 2):
            a = d["a%d" % o]
            if a is not None:
                assert np.all(a[cov, d["k%d" % o]:] == 0) and np.isfinite(a[cov]).all() and np.isnan(a[~cov]).all()


def test_the_device_generated_long_walk_is_exact_in_any_order():
    """test_forward_exact_long_walk_bf16: operands from {-1, 0, 1}, weights and bias multiples of 0.5 of magnitude <= 1,
    128 terms + bias: |out| <= 129 in multiples of 0.5 (the test asserts < 128 on the device: eight significant bits);
    a thread's partial holds 32 tiles x 2 rows of values and of squares."""
    assert 129 < 2.0 ** 24 * 0.5 and 64 * 128 < 2.0 ** 24 * 0.5 and 64 * 128 * 128 < 2.0 ** 24 * 0.25
    assert 32 * 512 + 1 == -(-(64 * (32 * 512 - 1) + 63) // 64) + 1  # the tile count of its table


@pytest.mark.parametrize("name", list(F.BWD_INT) + list(F.BWD_LONG) + list(F.BWD_PROBE))
def test_backward_exact_cases_are_exact_in_any_order(name):
    c = {**F.BWD_INT, **F.BWD_LONG, **F.BWD_PROBE}[name]
    d = F.build_bwd(c)
    ref = F.bwd_ref(d)
    cov, k = d["covered"], d["k"]
    lsb, lsb_din, lsb_g = d["lsb"]["dw"], d["lsb"]["din"], d["lsb"]["g"]
    # both fused multiply-adds of G are exact: G formed in float32 with a rounding after every operation is G
    assert np.array_equal(R.g_float32(F.bwd_dy32(d), d["gc"], d["coef"], d["width"]).astype(np.float64)[cov], ref["G"][cov]), name
    assert R.is_multiple(ref["G"][cov], lsb_g)
    assert R.is_multiple(ref["dw"], lsb) and R.any_order_exact(ref["S_dw"], lsb), name
    if ref["db"] is not None:
        assert R.is_multiple(ref["db"], lsb_g) and R.any_order_exact(ref["S_db"], lsb_g), name
    if d["store"]:  # what is stored as bf16 is one piece
        for a in [d["gc"]] + d["ins"] + ([d["dy"].astype(np.float32)] if d["store"] == 2 and not d["dense"] else []):
            assert np.array_equal(R.bf16_round(a[cov]), a[cov]), name
    if d["ib"]:
        assert all(np.array_equal(R.bf16_round(a[cov]), a[cov]) for a in d["ins"])
    if d["dgrad"]:
        din_exact = not (c["kind"] == "probe" and d["store"] == 2 and c["variant"] == "dw")
        for o in range(d["nops"]):
            assert R.is_multiple(ref["din"][o][cov], lsb_din) and R.any_order_exact(ref["S_din"][o], lsb_din), name
            if din_exact:
                assert np.array_equal(ref["stored"][o][cov], ref["din"][o][cov]), name + ": dIn that bf16 does not hold"
    if d["psums"]:  # a thread's fp32 partial: 8 tiles x 2 rows x the operands, weighted by at most the segment index
        per = 8 * 2 * d["nops"]
        top = max(np.abs(x[cov]).max() for x in ref["stored"])
        assert per * max(d["n_seg"] - 1, 1) * top < 2.0 ** 24 * lsb_din
        assert per * top * max(np.abs(a[cov]).max() for a in d["ins"]) < 2.0 ** 24 * lsb_din


# ------------------------------------------------------------------------------------------------ probes
CLAIMS = {  # probe -> the term subsets under which a form uses it
    "a3w1": (R.SIX_TERMS,), "a2w2": (R.SIX_TERMS,), "a1w3": (R.SIX_TERMS, R.HD_TERMS, R.IB_DW_TERMS),
    "a2w1": (R.HB_DIN_TERMS,), "a1w2": (R.HB_DIN_TERMS, R.HB_DW_TERMS),
}


@pytest.mark.parametrize("probe", list(CLAIMS))
def test_probes_are_exact_under_the_claimed_subset_and_wrong_one_term_short(probe):
    pa, pw, K, lsb, seen = R.probe_spec(probe)
    a, w = R.probe_operands(probe, 40, K, 24, 5)
    ref = a.astype(np.float64) @ w.astype(np.float64)
    assert R.is_multiple(ref, lsb) and R.any_order_exact(np.abs(a.astype(np.float64)) @ np.abs(w.astype(np.float64)), lsb)
    for terms in CLAIMS[probe]:
        assert set(seen) <= set(terms)
        assert np.array_equal(R.split_product_np(a, w, terms).astype(np.float64), ref), (probe, terms)
        for t in seen:
            assert not np.array_equal(R.split_product_np(a, w, _minus(terms, t)).astype(np.float64), ref), (probe, terms, t)


@pytest.mark.parametrize("piece", [1, 2])
def test_cancelling_probes_survive_bf16_and_see_their_term(piece):
    """For the kernels that round their output to bf16: exact under the claimed subset after the rounding, and wrong
    without the term the probe is built to see -- the forward product (weight piece ``piece``) and, for piece 1, the HB
    input gradient's g1 w2 term."""
    a, w, lsb = R.cancelling_probe(np.random.default_rng(3), 40, 96, 24, piece)
    ref = a.astype(np.float64) @ w.astype(np.float64)
    assert R.is_multiple(ref, lsb) and np.abs(ref).max() < 256 * lsb
    assert np.array_equal(R.bf16_round(ref.astype(np.float32)).astype(np.float64), ref)
    claims = (R.HD_TERMS, R.HB_DIN_TERMS) if piece == 1 else (R.HD_TERMS,)
    for terms in claims:
        assert np.array_equal(R.bf16_round(R.split_product_np(a, w, terms)).astype(np.float64), ref)
        assert not np.array_equal(R.bf16_round(R.split_product_np(a, w, _minus(terms, (0, piece)))).astype(np.float64), ref)


def test_the_gb_two_piece_gradient_probe_sees_g2_w1():
    """BWD_PROBE gb_a2w1: G = +-1 + 2^-9 in the even columns from bf16 incoming gradients and the constant vector C."""
    c = F.BWD_PROBE["b2d_g_din_gb_a2w1"]
    d = F.build_bwd(c)
    r = slice(d["begin"][0], d["end"][0])
    G = R.g_float32(d["dy"], d["gc"], d["coef"], 64)[r]
    wt = np.ascontiguousarray(d["w"][d["w_off"][0][0]:d["w_off"][0][0] + d["k"] * 64].reshape(d["k"], 64).T)
    ref = G.astype(np.float64) @ wt.astype(np.float64)
    assert np.array_equal(R.bf16_round(d["dy"][r]), d["dy"][r].astype(np.float32))
    assert np.array_equal(R.bf16_round(R.split_product_np(G, wt, R.HB_DIN_TERMS)).astype(np.float64), ref)
    assert not np.array_equal(R.bf16_round(R.split_product_np(G, wt, _minus(R.HB_DIN_TERMS, (1, 0)))).astype(np.float64), ref)


# ------------------------------------------------------------------------------------------------ accuracy bounds
def _short(terms):
    return [_minus(terms, t) for t in terms]


@pytest.mark.parametrize("name", list(F.FWD_ACC))
def test_forward_accuracy_bound_catches_any_lost_term(name):
    d = F.build_fwd(F.FWD_ACC[name])
    ref, S, stored, e_ref, bound = F.fwd_accuracy_bound(d)
    cols = slice(d["col0"], d["col0"] + d["n_out"])
    claimed = R.SIX_TERMS if d["form"] == "f32" else R.HD_TERMS  # (one-piece operands: the six terms ARE these three)
    full = P.err_units(P.gemm_in_float32(d, lambda a, w, acc: R.split_product_np(a, w, claimed, acc)), ref[:, cols], S)
    print("%s: e_ref = %.2f, bound %.2f, emulated e = %.2f" % (name, e_ref, bound, full))
    assert full <= bound
    for terms in _short(claimed):
        got = P.gemm_in_float32(d, lambda a, w, acc: R.split_product_np(a, w, terms, acc)).astype(np.float64)
        if d["form"] == "h":
            got = R.bf16_round(got.astype(np.float32)).astype(np.float64)
            m = S > 0
            e = float(((np.abs(got - ref[:, cols]) - 0.5 * R.ulp(ref[:, cols], bf16=True)).clip(0)[m] / S[m]).max() / R.U24)
        else:
            e = P.err_units(got, ref[:, cols], S)
        assert e > 2.0 * bound, "%s without %s: e = %.2f against a bound of %.2f" % (name, set(claimed) - set(terms), e, bound)


@pytest.mark.parametrize("name", list(F.BWD_ACC))
def test_backward_accuracy_bound_catches_any_lost_term(name):
    d = F.build_bwd(F.BWD_ACC[name])
    ref = F.bwd_ref(d)
    bounds = F.bwd_accuracy_bounds(d, ref)
    dw_terms = R.HB_DW_TERMS if d["store"] else (R.IB_DW_TERMS if d["ib"] else R.SIX_TERMS)
    din_terms = R.HB_DIN_TERMS if d["store"] else R.SIX_TERMS

    def figures(dwt, dint):
        dw32, din32 = R.block_bwd_f32(d["begin"], d["end"], d["w_off"], F.bwd_dy32(d), d["gc"], d["coef"], d["ins"], d["k"],
                                      d["w"], d["dw0"].size, d["width"], d["dense"],
                                      lambda a, g: R.split_product_np(a, g, dwt), lambda g, w: R.split_product_np(g, w, dint))
        m = ref["S_dw"] > 0
        e_dw = float((np.abs(dw32 - ref["dw"])[m] / ref["S_dw"][m]).max() / R.U24)
        e_din = 0.0
        for o in range(d["nops"]):
            S, r64 = ref["S_din"][o], ref["din"][o]
            m = S > 0
            if not m.any():
                continue
            got = din32[o].astype(np.float64)
            err = np.abs(got - np.where(m, r64, 0.0))
            if d["store"] == 2:
                got = R.bf16_round(din32[o]).astype(np.float64)
                err = (np.abs(got - np.where(m, r64, 0.0)) - 0.5 * R.ulp(np.where(m, r64, 1.0), bf16=True)).clip(0)
            e_din = max(e_din, float((err[m] / S[m]).max() / R.U24))
        return e_dw, e_din

    e_dw, e_din = figures(dw_terms, din_terms)
    print("%s: dW e_ref %.2f bound %.2f emulated %.2f; dIn e_ref %.2f bound %.2f emulated %.2f" % (
        (name,) + bounds["dw"] + (e_dw,) + bounds["din"] + (e_din,)))
    assert e_dw <= bounds["dw"][1]
    for terms in _short(dw_terms):
        e, _ = figures(terms, din_terms)
        assert e > 2.0 * bounds["dw"][1], "%s dW without %s: e = %.2f, bound %.2f" % (name, set(dw_terms) - set(terms), e, bounds["dw"][1])
    if d["dgrad"]:
        assert e_din <= bounds["din"][1]
        for terms in _short(din_terms):
            _, e = figures(dw_terms, terms)
            assert e > 2.0 * bounds["din"][1], "%s dIn without %s: e = %.2f, bound %.2f" % (
                name, set(din_terms) - set(terms), e, bounds["din"][1])
