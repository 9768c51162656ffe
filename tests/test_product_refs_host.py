"""The product references of tests/edge_refs.py and the case tables of tests/test_gpu_product_edges.py, checked
without a device: the float64 restatements against torch in float64, the bf16 split against the bounds
csrc/split_bf16.h states, the any-order exactness condition of every exact case, and -- by emulating the split product
with one of its six terms left out -- that the probes and the accuracy bounds of the GPU file would catch a kernel
that lost that term."""
import numpy as np
import pytest
import torch

from tests import edge_refs as R
from tests import test_gpu_product_edges as G

FIVE_TERMS = {t: tuple(x for x in R.SIX_TERMS if x != t) for t in R.SIX_TERMS}
SEGS = ((0, 0), (0, 1), (1, 1), (1, 38), (40, 40), (40, 171), (171, 180))  # empty, one row, ragged, a gap, 185 rows


def _split_with(terms):
    return lambda a, w, acc: R.split_product_np(a, w, terms, acc)


# ------------------------------------------------------------------------------------------------ float64 restatements
@pytest.mark.parametrize("trans", [False, True])
@pytest.mark.parametrize("act", [0, 1, 2])
def test_seg_product_ref_is_torch_in_float64(trans, act):
    rng = np.random.default_rng(act * 2 + trans)
    begin, end = [b for b, _ in SEGS], [e for _, e in SEGS]
    n, k1, k2, n_out, n_seg = 185, 9, 5, 7, len(SEGS)
    a1, a2 = rng.standard_normal((n, k1 + 2)), rng.standard_normal((n, k2))
    w1, w2 = rng.standard_normal(3 + n_seg * k1 * n_out), rng.standard_normal(n_seg * k2 * n_out)
    bias = rng.standard_normal(n_seg * n_out)
    w1_off = [3 + s * k1 * n_out for s in range(n_seg)]
    w2_off = [(-1 if s == 3 else s * k2 * n_out) for s in range(n_seg)]
    bias_off = [(-1 if s == 5 else s * n_out) for s in range(n_seg)]
    out0 = rng.standard_normal((n, n_out))
    ref, S = R.seg_product_ref(begin, end, [(a1, w1, w1_off, k1), (a2, w2, w2_off, k2)], bias, bias_off, n_out, trans, act, out0)
    want, mag = torch.from_numpy(out0.copy()), torch.zeros((n, n_out), dtype=torch.float64)
    for s in range(n_seg):
        if end[s] == begin[s]:
            continue
        y = torch.zeros((end[s] - begin[s], n_out), dtype=torch.float64)
        m = torch.zeros_like(y)
        for a, w, off, k in ((a1, w1, w1_off, k1), (a2, w2, w2_off, k2)):
            if off[s] < 0:
                continue
            ws = torch.from_numpy(w[off[s]:off[s] + k * n_out])
            x = torch.from_numpy(a[begin[s]:end[s], :k])
            y = y + (torch.nn.functional.linear(x, ws.reshape(n_out, k)) if trans else x @ ws.reshape(k, n_out))
            m = m + (x.abs() @ (ws.reshape(n_out, k).T if trans else ws.reshape(k, n_out)).abs())
        if bias_off[s] >= 0:
            b = torch.from_numpy(bias[bias_off[s]:bias_off[s] + n_out])
            y, m = y + b, m + b.abs()
        if act == 1:
            y = torch.relu(y)
        if act == 2:
            y, m = y + want[begin[s]:end[s]], m + want[begin[s]:end[s]].abs()
        want[begin[s]:end[s]], mag[begin[s]:end[s]] = y, m
    assert np.abs(ref - want.numpy()).max() <= 1e-13 * np.abs(want.numpy()).max()
    assert np.abs(S - mag.numpy()).max() <= 1e-13 * mag.numpy().max()
    assert np.array_equal(ref[38:40], out0[38:40]) and np.array_equal(ref[180:], out0[180:]) and (S[38:40] == 0).all()
    assert (S >= np.abs(ref) - 1e-12)[S > 0].all() or act == 1


@pytest.mark.parametrize("trans", [False, True])
def test_seg_wgrad_ref_is_autograd_in_float64(trans):
    rng = np.random.default_rng(5 + trans)
    begin, end = [b for b, _ in SEGS], [e for _, e in SEGS]
    n, k, nc, n_seg = 185, 6, 5, len(SEGS)
    a, g = rng.standard_normal((n, k + 1)), rng.standard_normal((n, nc + 2))
    dw0, db0 = rng.standard_normal(n_seg * k * nc), rng.standard_normal(n_seg * nc)
    block = [0, 1, 2, 3, 4, 3, 6]  # segments 3 and 5 add into the same blocks
    dw_off = [(-1 if s == 6 else block[s] * k * nc) for s in range(n_seg)]
    db_off = [(-1 if s == 1 else block[s] * nc) for s in range(n_seg)]
    dw, db, S, Sb = R.seg_wgrad_ref(begin, end, a, g, k, nc, dw0, dw_off, db0, db_off, trans)
    want_w, want_b = dw0.copy(), db0.copy()
    for s in range(n_seg):
        w = torch.zeros((nc, k) if trans else (k, nc), dtype=torch.float64, requires_grad=True)
        b = torch.zeros(nc, dtype=torch.float64, requires_grad=True)
        x = torch.from_numpy(a[begin[s]:end[s], :k])
        y = (torch.nn.functional.linear(x, w) if trans else x @ w) + b
        (y * torch.from_numpy(g[begin[s]:end[s], :nc])).sum().backward()
        if dw_off[s] >= 0:
            want_w[dw_off[s]:dw_off[s] + k * nc] += w.grad.numpy().reshape(-1)
        if db_off[s] >= 0:
            want_b[db_off[s]:db_off[s] + nc] += b.grad.numpy()
    assert np.abs(dw - want_w).max() <= 1e-13 * np.abs(want_w).max()
    assert np.abs(db - want_b).max() <= 1e-13 * np.abs(want_b).max()
    assert np.array_equal(dw[6 * k * nc:], dw0[6 * k * nc:]) and (S >= np.abs(dw) - 1e-12).all()
    assert R.seg_wgrad_ref(begin, end, a, g, k, nc, dw0, dw_off, None, None, trans)[1] is None


def test_seq32_product_is_a_sequential_float32_chain():
    rng = np.random.default_rng(0)
    a, w = rng.standard_normal((3, 50)).astype(np.float32), rng.standard_normal((50, 2)).astype(np.float32)
    want = np.zeros((3, 2), np.float32)
    for i in range(3):
        for j in range(2):
            acc = np.float32(0)
            for kk in range(50):
                acc = np.float32(acc + np.float32(a[i, kk] * w[kk, j]))
            want[i, j] = acc
    assert np.array_equal(R.seq32_product(a, w), want)
    assert np.array_equal(R.seq32_product(a[:, 20:], w[20:], R.seq32_product(a[:, :20], w[:20])), want)


# ------------------------------------------------------------------------------------------------ the split
@pytest.mark.parametrize("kind", ["normal", "tiny", "pow2", "probe"])
def test_split3_np_meets_the_bounds_of_split_bf16_h(kind):
    rng = np.random.default_rng(1)
    x = {"normal": lambda: rng.standard_normal(100000) * 10.0 ** rng.integers(-6, 7, 100000),
         # (tiny: the smallest magnitudes whose third piece is still a normal number, |x| >= 2^-100)
         "tiny": lambda: rng.choice([-1.0, 1.0], 100000) * (1.0 + np.abs(rng.standard_normal(100000))) * 2.0 ** -100,
         "pow2": lambda: np.ldexp(rng.choice([-1.0, 1.0], 200), rng.integers(-60, 60, 200)),
         "probe": lambda: R.probe_values(rng, 100000, 3)}[kind]().astype(np.float32)
    p1, p2, p3 = (p.astype(np.float64) for p in R.split3_np(x))
    ax = np.abs(x.astype(np.float64))
    for p in (p1, p2, p3):  # every piece is a bf16 value
        assert np.array_equal(R.bf16_round(p.astype(np.float32)).astype(np.float64), p)
    assert (np.abs(x - p1) <= 2.0 ** -8 * ax).all() and (np.abs(p2) <= 2.0 ** -8 * ax).all()
    assert (np.abs(p3) <= 2.0 ** -16 * ax).all()
    assert (np.abs(x.astype(np.float64) - p1 - p2 - p3) <= 2.0 ** -24 * ax).all()
    if kind == "pow2":
        assert np.array_equal(p1, x.astype(np.float64)) and not p2.any() and not p3.any()
    if kind == "probe":  # the pieces are the three summands
        assert np.array_equal(p1 + p2 + p3, x.astype(np.float64)) and set(np.abs(p1)) == {1.0}
        assert set(np.abs(p2)) == {0.0, 2.0 ** -9, 2.0 ** -17} and set(np.abs(p3)) == {0.0, 2.0 ** -17}


# ------------------------------------------------------------------------------------------------ exactness condition
def _operand_lsbs(c):
    if c["kind"] == "probe":
        piece = {1: 1.0, 2: 2.0 ** -9, 3: 2.0 ** -17}
        return piece[R.PROBES[c["probe"]][0]], piece[R.PROBES[c["probe"]][1]]
    return (1.0, 1.0) if c["kind"] == "sign" else (0.5, 0.25)


EXACT_GEMM = [(t, n, False) for t in ("GEMM_INT", "GEMM_WIDE", "GEMM_PROBE") for n in getattr(G, t)] + \
             [(t, n, True) for t in ("HEAD_INT", "HEAD_PROBE") for n in getattr(G, t)]
EXACT_WGRAD = [(t, n) for t in ("WGRAD_INT", "WGRAD_SLABS", "WGRAD_PROBE") for n in getattr(G, t)]


@pytest.mark.parametrize("table,name,head", EXACT_GEMM)
def test_forward_exact_cases_are_exact_in_any_order(table, name, head):
    c = getattr(G, table)[name]
    d = G._head_case(c) if head else G.build_gemm(c)
    la, lw = _operand_lsbs(c)
    assert d["lsb"] == la * lw
    for o in (1, 2):
        if d["a%d" % o] is not None:
            assert R.is_multiple(d["a%d" % o], la) and R.is_multiple(d["w%d" % o], lw)
            assert np.isnan(d["a%d" % o][:, d["k%d" % o]:]).all() and np.isnan(d["a%d" % o][~d["covered"]]).all()
            if c["kind"] == "int":  # one bf16 piece each: these cases pin indexing, not the split
                assert not R.split3_np(d["w%d" % o])[1].any()
                assert not R.split3_np(np.nan_to_num(d["a%d" % o]))[1].any()
    if d["bias_v"] is not None:
        assert R.is_multiple(d["bias_v"], d["lsb"])
    cols = slice(d["col0"], d["col0"] + d["n_out"])
    assert c["act"] != 2 or R.is_multiple(d["out0"][:, cols], d["lsb"])
    ref, S = G.gemm_ref(d)
    assert R.any_order_exact(S, d["lsb"]), "sum of |terms| = %g lsb" % (S.max() / d["lsb"])
    assert np.array_equal(ref.astype(np.float32).astype(np.float64), ref)
    outside = np.ones(ref.shape, bool)
    outside[d["covered"], cols] = False
    assert np.array_equal(ref[outside], d["out0"][outside].astype(np.float64)) and (S[d["covered"]] > 0).any()
    assert (d["out0"][:, :d["col0"]] == G.SENTINEL).all() and (d["out0"][:, cols.stop:] == G.SENTINEL).all()


@pytest.mark.parametrize("table,name", EXACT_WGRAD)
def test_wgrad_exact_cases_are_exact_in_any_order(table, name):
    c = getattr(G, table)[name]
    d = G.build_wgrad(c)
    la, lg = _operand_lsbs(c)
    assert d["lsb"] == la * lg and R.is_multiple(d["a"], la) and R.is_multiple(d["g"], lg)
    assert R.is_multiple(d["dw0"], d["lsb"]) and R.is_multiple(d["g"], d["lsb_db"])
    assert np.isnan(d["a"][:, d["k"]:]).all() and np.isnan(d["g"][:, d["n"]:]).all() and np.isnan(d["a"][~d["covered"]]).all()
    dw, db, S, Sb = G.wgrad_ref(d)  # (S holds dW's starting value)
    assert R.any_order_exact(S, d["lsb"]), "sum of |terms| = %g lsb" % (S.max() / d["lsb"])
    assert np.array_equal(dw.astype(np.float32).astype(np.float64), dw)
    if db is not None:
        assert R.is_multiple(d["db0"], d["lsb_db"]) and R.any_order_exact(Sb, d["lsb_db"])
        assert np.array_equal(db.astype(np.float32).astype(np.float64), db)
    if table == "WGRAD_SLABS":  # the slab size worked out in the GPU file's docstring, from gcmi_seg_gemm_wgrad's formula
        assert _slab_rows(sum(c["sizes"]), len(c["sizes"]), c["k"], c["n"]) == {"shrink": 192, "grow": 320, "cap": 4096}[name]
    else:
        assert _slab_rows(sum(c["sizes"]), len(c["sizes"]), c["k"], c["n"]) == 128


def _slab_rows(total, n_seg, k, n, exact=False):
    kt = (k + 31) // 32
    resident = 256 * (4 if kt <= 2 else (3 if kt == 3 else 2)) - n_seg
    chunks = (kt + 3) // 4 if kt > 4 and not exact else 1
    slab = min(max((-(-total * chunks // resident) + 63) // 64 * 64, 256), 4096)
    nt = (n + 31) // 32
    groups = (nt + 3) // 4 if nt >= 3 else 1
    while slab > 128 and (-(-total // slab) + n_seg - 1) * groups * chunks < 256:
        slab -= 64
    return slab


# ------------------------------------------------------------------------------------------------ the probes bite
@pytest.mark.parametrize("probe", list(R.PROBES))
def test_probes_are_exact_with_six_terms_and_wrong_with_five(probe):
    seen = R.PROBES[probe][4]
    dropped_by_design = tuple((i, j) for i in range(3) for j in range(3) if (i, j) not in R.SIX_TERMS)
    cases = [("gemm", G.build_gemm(G.GEMM_PROBE[probe + "_N_first"])), ("gemm", G.build_gemm(G.GEMM_PROBE[probe + "_T_both"])),
             ("gemm", G._head_case(G.HEAD_PROBE[probe + "_head72"])),
             ("wgrad", G.build_wgrad(G.WGRAD_PROBE[probe + "_k20_N_one"])),
             ("wgrad", G.build_wgrad(G.WGRAD_PROBE[probe + "_k75_T_several"]))]
    for kind, d in cases:
        if kind == "gemm":
            ref, S = G.gemm_ref(d)
            run = lambda terms: G.gemm_in_float32(d, _split_with(terms)).astype(np.float64)[d["covered"]]  # noqa: E731
            ref = ref[d["covered"]]
        else:
            ref = G.wgrad_ref(d)[0]
            run = lambda terms: G.wgrad_in_float32(d, _split_with(terms)).astype(np.float64)  # noqa: E731
        assert np.array_equal(run(R.SIX_TERMS), ref)
        assert np.array_equal(run(dropped_by_design), run(())), "a term the kernels drop by design is non-zero"
        for t in R.SIX_TERMS:
            changed = float((run(FIVE_TERMS[t]) != ref).mean())
            if t in seen:
                assert changed > 0.2, "%s without term %s: only %.3f of the elements change" % (probe, t, changed)
    assert {t for p in R.PROBES.values() for t in p[4]} == set(R.SIX_TERMS)  # every term is seen by some probe


# ------------------------------------------------------------------------------------------------ the bounds bite
@pytest.mark.parametrize("name", list(G.GEMM_ACC))
def test_forward_accuracy_bound_catches_any_lost_term(name):
    d = G.build_gemm(G.GEMM_ACC[name])
    assert d["k1"] + d["k2"] <= 150
    ref, S, e_seq, bound = G.gemm_accuracy_bound(d)
    e_six = G.err_units(G.gemm_in_float32(d, _split_with(R.SIX_TERMS)), ref, S)
    e_five = {t: G.err_units(G.gemm_in_float32(d, _split_with(FIVE_TERMS[t])), ref, S) for t in R.SIX_TERMS}
    print("forward %s: e_seq32 %.2f, bound %.2f, six terms %.2f, five terms %s" % (
        name, e_seq, bound, e_six, " ".join("%.1f" % e_five[t] for t in R.SIX_TERMS)))
    assert e_six <= bound
    assert min(e_five.values()) > 2 * bound, (e_five, bound)


@pytest.mark.parametrize("name", list(G.WGRAD_ACC))
def test_wgrad_accuracy_bound_catches_any_lost_term(name):
    d = G.build_wgrad(G.WGRAD_ACC[name])
    assert max(d["sizes"]) <= 150
    ref, S, e_seq, bound = G.wgrad_accuracy_bound(d)
    e_six = G.err_units(G.wgrad_in_float32(d, _split_with(R.SIX_TERMS)), ref, S)
    e_five = {t: G.err_units(G.wgrad_in_float32(d, _split_with(FIVE_TERMS[t])), ref, S) for t in R.SIX_TERMS}
    print("wgrad %s: e_seq32 %.2f, bound %.2f, six terms %.2f, five terms %s" % (
        name, e_seq, bound, e_six, " ".join("%.1f" % e_five[t] for t in R.SIX_TERMS)))
    assert e_six <= bound
    assert min(e_five.values()) > 2 * bound, (e_five, bound)


# ------------------------------------------------------------------------------------------------ the wrapper
def test_seg_gemm_accumulate_needs_out_and_excludes_relu():
    """The checks come before anything touches a device."""
    from deepchem_amd import ops
    a, w = torch.zeros((2, 4)), torch.zeros(16)
    args = ([0], [2], a, w, [0], None, None, None, None, None, 4, False)
    with pytest.raises(ValueError, match="mutually exclusive"):
        ops.seg_gemm(*args, True, 2, 4, 0, out=torch.zeros((2, 4)), accumulate=True)
    with pytest.raises(ValueError, match="pass out"):
        ops.seg_gemm(*args, False, 2, 4, 0, accumulate=True)
