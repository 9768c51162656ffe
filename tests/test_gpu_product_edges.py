"""The segmented products (csrc/gemm.hip, csrc/gemm_split.hip, the wide head of csrc/head_bwd.hip) pinned at their tile
edges and at float32 accuracy, through ``ops.seg_gemm``, ``ops.task_head_forward`` and ``ops.seg_gemm_wgrad``, against
the float64 restatements of tests/edge_refs.py.  Three kinds of case:

  * EXACT, integer data (small integers times powers of two: one bf16 piece each, every partial sum a float32 number
    in any order -- tests/test_product_refs_host.py checks that condition for every case here).  ``np.array_equal``
    against float64 in both product modes, two launches each (fast mode reverses its grid on alternate launches), a
    sentinel in everything that must not be written, NaN in the padding columns of operand rows and in operand rows
    outside every segment.  They pin indexing, masking, offsets and the epilogues, not the split.
  * EXACT, piece probes: operands +-(1 + p 2^-9 + q 2^-17) whose products are exact only if every one of the six
    piece products is there (edge_refs.PROBES; the host test shows each five-term emulation to differ).
  * ACCURACY: standard-normal operands, contraction length <= 150, e = max |out - ref64| / S in units of 2^-24 with
    S the same product of absolute values, asserted <= 2 max(e_seq32, 1) where e_seq32 is that figure of the
    sequential float32 product of the same inputs (edge_refs.seq32_product), never of the code under test.

Which kernel a case reaches, from the dispatch predicates of ``seg_gemm`` (gemm.hip), ``launch_seg_gemm4`` /
``launch_wgrad3`` (gemm_split.hip) and ``head_fwd_wide`` (head_bwd.hip):

  ops.seg_gemm, fast mode
    one segment from row 0, first operand only, nn.Linear layout, k = 256, 33..256 outputs, no activation, 16-byte
    addressable operand rows                        -> head_fwd_wide_kernel            (HEAD cases but n_out = 32)
    else n_out % 4 == 0, ldo % 4 == 0, out 16-byte aligned -> seg_gemm4_kernel<layout, NT, AVEC>; AVEC = operand rows
      16-byte addressable (ld % 4 == 0); NT = 1 / 2 / 4 for n_out <= 32 / <= 64 / more, halved while the launch has
      fewer than 256 workgroups: every case on the short tables runs NT = 1 with ceil(n_out / 32) column groups, the
      WIDE cases (260 row tiles) run NT = 2 (n_out 36, 64) and NT = 4 (68, 100, 128; 132 and 256 with grid.y = 2)
    else (n_out % 4 != 0, out at column 1, ldo % 4 != 0) the exact-mode kernels below
  ops.seg_gemm, exact mode (and the fast-mode fall-back)
    operand rows 16-byte addressable -> seg_gemm2_kernel<layout, NT> (NT from n_out alone, grid.y = ceil(n_out / 32 NT)),
      16-byte stores when ldo % 4 == 0 and out aligned, scalar ones else
    else (k = 50 in rows of 50, k = 1, 31, 33, ... in rows of k) -> seg_gemm_kernel (64 x 64 tiles)
  act = 2 therefore runs in seg_gemm4_kernel (fast, n_out 64 / 128), seg_gemm2_kernel with 16-byte stores (exact,
    n_out 64 / 128) and with scalar ones (n_out 30; out at column 1), seg_gemm_kernel (k = 50).
  ops.task_head_forward: with a scratch and 33..256 outputs in fast mode head_prep_kernel + head_fwd_img_kernel;
    else as ops.seg_gemm of the same shape.
  ops.seg_gemm_wgrad: fast mode wgrad3_kernel<KT, layout>, KT = min(ceil(k / 32), 4), ceil(ceil(k / 32) / 4) chunks in
    grid.z (k = 129 .. 513: 2 .. 5 chunks); exact mode wgrad_kernel<KT, layout>, KT <= 8 per launch (k = 257, 300: two
    launches, 513: three; dbias from the first).  n-tiles per workgroup ntw = 1, 2, 4 for n <= 32, <= 64, more, i.e.
    4, 2, 1 row parts summed through LDS; n = 97, 128: a partly empty / full fourth tile; n = 129, 160: grid.y = 2.

Slab rows of the weight gradient, from the sizing in ``gcmi_seg_gemm_wgrad`` (resident = 256 * 4 - n_seg at k <= 64;
slab = ceil(rows * chunks / resident) rounded up to 64, at least 256, at most 4096; then, while the launch has fewer
than 256 workgroups, 64 rows less down to 128):

  every WGRAD / probe / accuracy case (<= 1 201 rows)   256 -> 128, the floor
  SLABS "shrink"   52 001 rows, 1 segment     ceil(52001 / 1023) = 51 -> 256; 204 slabs of 256 < 256, 271 of 192: 192
  SLABS "grow"    270 001 rows, 1 segment     ceil(270001 / 1023) = 264 -> 320; 844 slabs: 320
  SLABS "cap"   4 198 400 rows, 5 segments    ceil(4198400 / 1019) = 4121 -> 4160 -> 4096; segment ends at
                                              4096 m - 1, 4096 m' + 1, 4096 m'', ...: 4096

MEASURED on an MI355X.  v_mfma_f32_32x32x16_bf16 adds exactly representable sums exactly: every integer case and
every piece probe came out bit for bit equal to float64 in fast mode (both sweep directions, atomics included), so the
probe assertion is ``np.array_equal`` and not a distance.  Accuracy, e in units of 2^-24 of the element's own S:

  case                      e_seq32   bound    e fast   e exact
  seg_gemm  conv75            3.47     6.94     2.77     3.47
  seg_gemm  dense             3.68     7.36     3.67     3.68
  seg_gemm  odd               2.48     4.96     2.64     2.47
  seg_gemm  k128              3.35     6.70     2.82     3.22
  wgrad     conv75            3.75     7.50     2.21     3.60
  wgrad     dense             3.91     7.82     3.20     4.60
  wgrad     odd               1.72     3.43     1.65     1.33
  wgrad     k128              4.84     9.67     2.53     3.31
  wgrad     k130_chunks       4.25     8.49     2.88     3.38

(exact-mode forward products ARE the sequential chain but for the fused multiply-add; the weight gradient sums row
parts and slabs in another order.)  The emulated six-term product is at 1.4 .. 3.0 on these cases and every five-term
one above 21 (tests/test_product_refs_host.py prints them).  With one MFMA line taken out of seg_gemm4_kernel (the a1.b3
term) and one out of wgrad3_kernel (a2.b2) in a scratch build, the probes that see those terms and all nine accuracy
cases failed while test_seg_gemm, test_seg_gemm_wgrad and test_seg_walk still passed.
"""
import numpy as np
import pytest
import torch

from tests import edge_refs as R
from tests.test_gpu_seg_walk import SMALL as WALK_SMALL

pytestmark = pytest.mark.gpu

SENTINEL = -12345.5
MODES = ("fast", "exact")


def _up4(x):
    return (x + 3) // 4 * 4


def _bounds(sizes, gap_after=None):
    """Segments laid end to end; 5 rows that belong to no segment after segment ``gap_after`` (default: the last but
    one) and 3 after the last."""
    gap_after = len(sizes) - 2 if gap_after is None else gap_after
    begin, end, row = [], [], 0
    for s, n in enumerate(sizes):
        begin.append(row)
        end.append(row + n)
        row += n
        if s == gap_after:
            row += 5
    return begin, end, row + 3


def _covered(begin, end, n):
    c = np.zeros(n, bool)
    for b, e in zip(begin, end):
        c[b:e] = True
    return c


def _padded(values, ld, covered):
    """(n, ld) float32 with ``values`` in the leading columns of the covered rows and NaN everywhere else."""
    full = np.full((values.shape[0], ld), np.nan, np.float32)
    full[covered, :values.shape[1]] = values[covered]
    return full


# ================================================================================================ forward cases
SEGS = (0, 1, 130, 0, 37)  # empty, one row, two 128-row tiles (three of 64) with a ragged end, empty, ragged
WIDE_SEGS = (0, 1, 20000, 0, 13000)  # 1 + 157 + 102 = 260 tiles of 128 rows


def _g(**kw):
    """One forward case.  k1 / k2 = 0: that operand is absent; ld: floats per operand row (default k: dense rows);
    col0 / ldo: out is columns [col0, col0 + n_out) of a matrix with ldo columns; bias: "all", "skip" (offset -1 on
    segment 2) or None; skip1 / skip2: the segment whose first / second weight offset is -1."""
    c = dict(k1=36, ld1=0, k2=0, ld2=0, n_out=64, trans=False, act=0, sizes=SEGS, col0=0, ldo=0, bias="all",
             skip1=-1, skip2=-1, kind="int", probe=None, nnz=None, seed=0)
    c.update(kw)
    c["ld1"] = c["ld1"] or c["k1"]
    c["ld2"] = c["ld2"] or c["k2"]
    c["ldo"] = c["ldo"] or c["col0"] + c["n_out"]
    return c


GEMM_INT = {}
for _k in (1, 31, 32, 33, 63, 65, 75, 97):  # k tails of the 32-column chunk, dense rows and padded ones
    GEMM_INT["k%d" % _k] = _g(k1=_k, act=1)
    GEMM_INT["k%d_padded" % _k] = _g(k1=_k, ld1=76 if _k == 75 else _up4(_k) + 4, trans=_k % 2 == 0)
for _n in (1, 3, 4, 30, 32, 36, 64, 68, 100, 128, 132, 160, 256):  # column tails, both layouts, both operand kinds
    for _t in (False, True):
        GEMM_INT["n%d_%s" % (_n, "T" if _t else "N")] = _g(n_out=_n, trans=_t, k2=8, act=int(_n % 8 == 0))
        GEMM_INT["n%d_%s_rows50" % (_n, "T" if _t else "N")] = _g(k1=50, n_out=_n, trans=_t)
GEMM_INT.update({
    "k2_differs": _g(k1=33, ld1=36, k2=7, ld2=8, act=1),
    "k2_longer": _g(k1=20, ld1=24, k2=64, ld2=64, trans=True),
    "first_only": _g(k1=40, k2=0),
    "second_only": _g(k1=0, k2=40),
    "second_only_T": _g(k1=0, k2=33, ld2=36, trans=True, n_out=128),
    "acc64": _g(act=2), "acc128_T": _g(act=2, n_out=128, trans=True, k2=36), "acc30": _g(act=2, n_out=30),
    "acc_rows50": _g(act=2, k1=50), "acc256": _g(act=2, n_out=256, k1=65, ld1=68),
    "block": _g(col0=4, ldo=72), "block_acc": _g(col0=4, ldo=72, act=2), "block_relu_T": _g(col0=4, ldo=140, n_out=128,
                                                                                           trans=True, act=1),
    "col1": _g(col0=1, ldo=68), "col1_acc": _g(col0=1, ldo=68, act=2), "col1_rows50": _g(col0=1, ldo=68, k1=50, act=1),
    "no_bias": _g(bias=None, k2=36), "no_bias_n30": _g(bias=None, n_out=30), "no_bias_rows50": _g(bias=None, k1=50),
    "bias_skip": _g(bias="skip", k2=36), "bias_skip_n30": _g(bias="skip", n_out=30, act=1),
    "bias_skip_rows50": _g(bias="skip", k1=50),
    "w2_skip": _g(k2=36, skip2=2), "w2_skip_T_n30": _g(k2=36, skip2=4, n_out=30, trans=True),
    "w1_skip_rows50": _g(k1=50, k2=50, skip1=2),
    "walk_small": _g(k1=75, ld1=76, k2=75, ld2=76, act=1, sizes=WALK_SMALL, skip1=1),
    "walk_small_T_n100": _g(k1=64, n_out=100, trans=True, sizes=WALK_SMALL),
})
GEMM_WIDE = {"wide%d" % _n: _g(k1=4, n_out=_n, sizes=WIDE_SEGS, trans=_n in (64, 132), act=int(_n == 100), seed=_n)
             for _n in (36, 64, 68, 100, 128, 132, 256)}
GEMM_WIDE["wide128_acc"] = _g(k1=4, k2=4, n_out=128, sizes=WIDE_SEGS, act=2)
HEAD_ROWS = 70  # three workgroups of 32 rows, the last with 6
HEAD_N_OUT = (32, 33, 36, 255, 256)
HEAD_INT = {"head%d" % _n: _g(k1=256, ld1=260, n_out=_n, trans=True, sizes=(HEAD_ROWS,), col0=4, ldo=_n + 9, seed=_n)
            for _n in HEAD_N_OUT}

# piece probes: the contraction is PROBES[name][2] long (96 / 96 / 48), alone in either slot or halved over both
GEMM_PROBE = {}
for _p in R.PROBES:
    _K = R.PROBES[_p][2]
    for _t in (False, True):
        _l = "T" if _t else "N"
        GEMM_PROBE["%s_%s_first" % (_p, _l)] = _g(kind="probe", probe=_p, k1=_K, trans=_t)
        GEMM_PROBE["%s_%s_second" % (_p, _l)] = _g(kind="probe", probe=_p, k1=0, k2=_K, trans=_t, n_out=36)
        GEMM_PROBE["%s_%s_both" % (_p, _l)] = _g(kind="probe", probe=_p, k1=_K // 2, k2=_K // 2, trans=_t, n_out=128)
    GEMM_PROBE["%s_nt4" % _p] = _g(kind="probe", probe=_p, k1=_K, n_out=128, sizes=WIDE_SEGS, bias=None)
HEAD_PROBE = {"%s_head%d" % (_p, _n): _g(kind="probe", probe=_p, k1=256, ld1=260, n_out=_n, trans=True,
                                         sizes=(HEAD_ROWS,), nnz=min(64, R.PROBES[_p][2]), bias=None)
              for _p in R.PROBES for _n in (72, 256)}

# accuracy: the model's shapes, total contraction <= 150, one table with ragged and empty segments (302 rows)
ACC_SEGS = (0, 1, 64, 0, 130, 37, 70)
GEMM_ACC = {
    "conv75": _g(kind="normal", k1=75, ld1=76, k2=75, ld2=76, n_out=64, act=1, sizes=ACC_SEGS),
    "dense": _g(kind="normal", k1=64, n_out=128, trans=True, sizes=ACC_SEGS),
    "odd": _g(kind="normal", k1=33, ld1=36, k2=7, ld2=8, n_out=4, sizes=ACC_SEGS),
    "k128": _g(kind="normal", k1=128, n_out=36, sizes=ACC_SEGS),
}


def build_gemm(c):
    """The numpy side of one forward case: operands (NaN outside what may be read), flat weights and bias, offsets,
    the matrix out starts as, and ``lsb``, the power of two every term is a multiple of (None: accuracy case)."""
    begin, end, n = _bounds(c["sizes"])
    n_seg, n_out, trans = len(begin), c["n_out"], c["trans"]
    cov = _covered(begin, end, n)
    rng = np.random.default_rng(1000 * n_out + 10 * c["k1"] + c["k2"] + c["seed"])
    d = dict(c, begin=begin, end=end, n=n, n_seg=n_seg, covered=cov)

    def values(shape, lo, hi, scale):
        if c["kind"] == "normal":
            return rng.standard_normal(shape).astype(np.float32)
        return (rng.integers(lo, hi + 1, shape) * scale).astype(np.float32)

    for o, k, ld in ((1, c["k1"], c["ld1"]), (2, c["k2"], c["ld2"])):
        if not k:
            d["a%d" % o] = d["w%d" % o] = d["w%d_off" % o] = None
            continue
        if c["kind"] == "probe":  # the a of one probe for all rows, one w per segment
            Kp = c["k1"] + c["k2"]
            sl = slice(0, k) if o == 1 or not c["k1"] else slice(c["k1"], Kp)
            if "_pa" not in d:
                d["_pa"] = R.probe_operands(c["probe"], n, Kp, n_out, 77 + c["seed"], c["nnz"])[0]
                d["_pw"] = [R.probe_operands(c["probe"], 1, Kp, n_out, 78 + s + c["seed"])[1] for s in range(n_seg)]
            a, w = d["_pa"][:, sl], np.stack([pw[sl] for pw in d["_pw"]])
        else:
            a, w = values((n, k), -4, 4, 0.5), values((n_seg, k, n_out), -4, 4, 0.25)
        d["a%d" % o] = _padded(a, ld, cov)
        d["w%d" % o] = np.ascontiguousarray(w.transpose(0, 2, 1) if trans else w).reshape(-1)
        skip = c["skip1"] if o == 1 else c["skip2"]
        d["w%d_off" % o] = [-1 if s == skip else s * k * n_out for s in range(n_seg)]
    d.pop("_pa", None), d.pop("_pw", None)
    if c["bias"] is None:
        d["bias_v"], d["bias_off"] = None, None
    else:
        scale = 2.0 ** -17 if c["kind"] == "probe" and c["probe"] != "a2w2" else 0.125
        d["bias_v"] = values((n_seg, n_out), -8, 8, scale).reshape(-1)
        d["bias_off"] = [-1 if c["bias"] == "skip" and s == 2 else s * n_out for s in range(n_seg)]
    out0 = np.full((n, c["ldo"]), SENTINEL, np.float32)
    if c["act"] == 2:
        out0[:, c["col0"]:c["col0"] + n_out] = values((n, n_out), -8, 8, 0.125)
    d["out0"] = out0
    d["lsb"] = None if c["kind"] == "normal" else (R.PROBES[c["probe"]][3] if c["kind"] == "probe" else 0.125)
    return d


def gemm_operands(d):
    return [None if d["a%d" % o] is None else (d["a%d" % o], d["w%d" % o], d["w%d_off" % o], d["k%d" % o]) for o in (1, 2)]


def gemm_ref(d):
    """(float64 matrix out must equal, S of the n_out columns)."""
    cols = slice(d["col0"], d["col0"] + d["n_out"])
    ref, S = R.seg_product_ref(d["begin"], d["end"], gemm_operands(d), d["bias_v"], d["bias_off"], d["n_out"],
                               d["trans"], d["act"], d["out0"][:, cols])
    full = d["out0"].astype(np.float64)
    full[:, cols] = ref
    return full, S


def gemm_in_float32(d, product):
    """The forward contract in float32 with ``product(a, w, acc) -> acc`` as the product arithmetic: the operands in
    order into one accumulator, then the bias, then the activation (act 0 / 1).  Returns the n_out columns."""
    out = np.zeros((d["n"], d["n_out"]), np.float32)
    for s in range(d["n_seg"]):
        r = slice(d["begin"][s], d["end"][s])
        acc = np.zeros((r.stop - r.start, d["n_out"]), np.float32)
        for op in gemm_operands(d):
            if op is None or op[2][s] < 0:
                continue
            a, w, off, k = op
            blk = w[off[s]:off[s] + k * d["n_out"]]
            acc = product(a[r, :k], blk.reshape(d["n_out"], k).T if d["trans"] else blk.reshape(k, d["n_out"]), acc)
        if d["bias_v"] is not None and d["bias_off"][s] >= 0:
            acc = acc + d["bias_v"][d["bias_off"][s]:d["bias_off"][s] + d["n_out"]]
        out[r] = np.maximum(acc, np.float32(0)) if d["act"] == 1 else acc
    return out


def err_units(got, ref, S):
    """max |got - ref| / S over the elements that were computed (S > 0), in units of 2^-24."""
    m = S > 0
    return float((np.abs(got.astype(np.float64)[m] - ref[m]) / S[m]).max() / R.U24)


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _launch_gemm(d, times=2):
    """``times`` launches in each mode; {mode: [full out matrices]}."""
    import deepchem_amd as dc
    from deepchem_amd import ops
    a1, a2 = _dev(d["a1"]), _dev(d["a2"])
    w1, w2, bias = _dev(d["w1"]), _dev(d["w2"]), _dev(d["bias_v"])
    out0 = _dev(d["out0"])
    got = {}
    try:
        for mode in MODES:
            dc.set_gemm_mode(mode)
            got[mode] = []
            for _ in range(times):
                full = out0.clone()
                ops.seg_gemm(d["begin"], d["end"], None if a1 is None else a1[:, :d["k1"]], w1, d["w1_off"],
                             None if a2 is None else a2[:, :d["k2"]], w2, d["w2_off"], bias, d["bias_off"], d["n_out"],
                             d["trans"], d["act"] == 1, d["n"], d["k1"], d["k2"],
                             out=full[:, d["col0"]:d["col0"] + d["n_out"]], accumulate=d["act"] == 2)
                got[mode].append(full.cpu().numpy())
    finally:
        dc.set_gemm_mode("fast")
    return got


def _check_gemm_exact(d, what):
    ref, _ = gemm_ref(d)
    for mode, outs in _launch_gemm(d).items():
        for i, full in enumerate(outs):
            bad = np.argwhere(full.astype(np.float64) != ref)
            assert bad.size == 0, "%s %s launch %d: %d elements differ, first at %s: %r for %r" % (
                what, mode, i, len(bad), tuple(bad[0]), full[tuple(bad[0])], ref[tuple(bad[0])])


@pytest.mark.parametrize("name", list(GEMM_INT))
def test_seg_gemm_exact(name):
    """Integer data on the short tables: seg_gemm4_kernel NT = 1 (fast, n_out % 4 == 0 and an aligned out; AVEC iff
    ld % 4 == 0), else and in exact mode seg_gemm2_kernel (ld % 4 == 0) or seg_gemm_kernel -- see the module docstring."""
    _check_gemm_exact(build_gemm(GEMM_INT[name]), name)


@pytest.mark.parametrize("name", list(GEMM_WIDE))
def test_seg_gemm_exact_wide(name):
    """260 row tiles: seg_gemm4_kernel keeps NT = 2 (n_out 36: a partial column tile, 64: full) and NT = 4 (68, 100:
    partial tiles, 128: full; 132, 256: grid.y = 2 with a partial / full second group); exact mode seg_gemm2_kernel
    with the same NT."""
    _check_gemm_exact(build_gemm(GEMM_WIDE[name]), name)


def _head_forward(d, with_scratch):
    import deepchem_amd as dc
    from deepchem_amd import ops
    a, w, bias = _dev(d["a1"]), _dev(d["w1"]).reshape(d["n_out"], d["k1"]), _dev(d["bias_v"])
    scratch = torch.zeros(ops.task_head_scratch_floats(), dtype=torch.float32, device="cuda:0") if with_scratch else None
    got = {}
    try:
        for mode in MODES:
            dc.set_gemm_mode(mode)
            got[mode] = []
            for _ in range(2):
                full = _dev(d["out0"])
                ops.task_head_forward(a[:, :d["k1"]], w, bias, scratch, out=full[:, d["col0"]:d["col0"] + d["n_out"]])
                got[mode].append(full.cpu().numpy())
    finally:
        dc.set_gemm_mode("fast")
    return got


def _head_case(c):
    """A head case has one segment that is all rows: no gap, no tail."""
    d = build_gemm(dict(c, sizes=c["sizes"] + (0,)))  # (the trailing rows of _bounds are NaN rows: cut below)
    n = c["sizes"][0]
    for key in ("a1", "out0", "covered"):
        d[key] = d[key][:n]
    d.update(n=n, n_seg=1, begin=[0], end=[n], sizes=c["sizes"], w1_off=d["w1_off"][:1])
    d["w1"] = d["w1"][:c["k1"] * c["n_out"]]
    if d["bias_v"] is not None:
        d["bias_v"], d["bias_off"] = d["bias_v"][:c["n_out"]], [0]
    return d


@pytest.mark.parametrize("name", list(HEAD_INT))
def test_head_exact(name):
    """One segment from row 0, k = 256 in rows of 260, nn.Linear layout, out a column block of an odd-pitched matrix.
    ops.seg_gemm: head_fwd_wide_kernel in fast mode (n_out = 32: seg_gemm4_kernel refuses the odd pitch, so
    seg_gemm2_kernel), seg_gemm2_kernel in exact mode.  ops.task_head_forward: with scratch head_prep_kernel +
    head_fwd_img_kernel in fast mode for 33..256 outputs, else the same as ops.seg_gemm."""
    d = _head_case(HEAD_INT[name])
    ref, _ = gemm_ref(d)
    runs = {"seg_gemm": _launch_gemm(d), "head": _head_forward(d, False), "head+scratch": _head_forward(d, True)}
    for entry, got in runs.items():
        for mode, outs in got.items():
            for full in outs:
                assert np.array_equal(full.astype(np.float64), ref), "%s %s %s" % (name, entry, mode)


@pytest.mark.parametrize("name", list(GEMM_PROBE))
def test_seg_gemm_probe(name):
    """Piece probes through seg_gemm4_kernel (fast; NT = 1 on the short table, NT = 4 on the wide one) and through the
    exact-mode kernels, where they hold trivially."""
    _check_gemm_exact(build_gemm(GEMM_PROBE[name]), name)


@pytest.mark.parametrize("name", list(HEAD_PROBE))
def test_head_probe(name):
    """Piece probes through head_fwd_wide_kernel (ops.seg_gemm, ops.task_head_forward without scratch) and
    head_prep_kernel + head_fwd_img_kernel (with scratch); 64 (48) non-zero columns per 256-column row."""
    d = _head_case(HEAD_PROBE[name])
    ref, _ = gemm_ref(d)
    runs = {"seg_gemm": _launch_gemm(d), "head": _head_forward(d, False), "head+scratch": _head_forward(d, True)}
    for entry, got in runs.items():
        for mode, outs in got.items():
            for full in outs:
                assert np.array_equal(full.astype(np.float64), ref), "%s %s %s" % (name, entry, mode)


def gemm_accuracy_bound(d):
    """(ref, S, e_seq32, bound) of an accuracy case: the bound is 2 max(e_seq32, 1) with e_seq32 the figure of the
    sequential float32 product of the same inputs."""
    ref, S = gemm_ref(d)
    e_seq = err_units(gemm_in_float32(d, R.seq32_product), ref, S)
    return ref, S, e_seq, 2.0 * max(e_seq, 1.0)


@pytest.mark.parametrize("name", list(GEMM_ACC))
def test_seg_gemm_accuracy(name):
    d = build_gemm(GEMM_ACC[name])
    ref, S, e_seq, bound = gemm_accuracy_bound(d)
    cov = d["covered"]
    figures = {}
    for mode, outs in _launch_gemm(d).items():
        assert np.array_equal(outs[0], outs[1]), "%s %s: the two sweep directions differ" % (name, mode)
        assert np.all(outs[0][~cov] == SENTINEL), "%s %s: rows outside every segment were written" % (name, mode)
        figures[mode] = err_units(outs[0], ref, S)
        print("seg_gemm accuracy %s %s: e = %.2f, e_seq32 = %.2f, bound %.2f" % (name, mode, figures[mode], e_seq, bound))
    for mode, e in figures.items():
        assert e <= bound, "%s %s: e = %.2f roundings of S, bound %.2f (e_seq32 = %.2f)" % (name, mode, e, bound, e_seq)


# ================================================================================================ weight gradient
WGRAD_SEGS = (0, 1, 15, 16, 17, 127, 128, 129, 255, 256, 257)  # the 16-row step, the 32-row part, the 128-row slab


def _w(**kw):
    """One weight-gradient case.  skip_dw / skip_db: the segment whose dW / dbias offset is -1; share: segments
    (i, j) that add into the same blocks; dbias False: no bias gradient at all; start: dW and dbias start non-zero."""
    c = dict(k=33, n=33, trans=False, sizes=WGRAD_SEGS, lda=0, ldg=0, skip_dw=5, skip_db=7, share=None, dbias=True,
             start=True, kind="int", probe=None, seed=0)
    c.update(kw)
    c["lda"] = c["lda"] or _up4(c["k"]) + 4
    c["ldg"] = c["ldg"] or c["n"] + 3
    return c


WGRAD_INT = {}
for _t in (False, True):
    _l = "T" if _t else "N"
    for _k in (1, 31, 32, 33, 64, 65, 96, 97, 128, 129, 256, 257, 300, 513):
        WGRAD_INT["k%d_%s" % (_k, _l)] = _w(k=_k, trans=_t)
    for _n in (1, 31, 32, 64, 65, 96, 97, 128, 129, 160):
        WGRAD_INT["n%d_%s" % (_n, _l)] = _w(n=_n, trans=_t)
WGRAD_INT.update({
    "no_dbias": _w(dbias=False), "no_dbias_T_n64": _w(dbias=False, n=64, trans=True),
    "dense_rows": _w(k=64, lda=64, n=64, ldg=64),
    "k129_n129": _w(k=129, n=129), "from_zero_T": _w(start=False, trans=True, k=75, n=64),
})
WGRAD_SLABS = {
    "shrink": _w(k=4, n=4, sizes=(52001,), kind="sign", skip_dw=-1, skip_db=-1),
    "grow": _w(k=4, n=4, sizes=(270001,), kind="sign", skip_dw=-1, skip_db=-1, trans=True),
    "cap": _w(k=4, n=4, sizes=(4096 * 205 - 1, 4096 * 205 + 1, 4096 * 205, 4096 * 205 + 1, 4096 * 205 - 1), kind="sign",
              skip_dw=-1, skip_db=-1, lda=4, ldg=4),
}


def _probe_sizes(K, several):
    return (K // 2, 0, K // 2, 5 * K // 16, 1, 3 * K // 16) if several else (K,)


WGRAD_PROBE = {}
for _p in R.PROBES:
    for _k, _n in ((20, 36), (75, 64)):  # KT = 1 with two row parts, KT = 3 with two row parts
        for _t in (False, True):
            for _sv in (False, True):
                WGRAD_PROBE["%s_k%d_%s_%s" % (_p, _k, "T" if _t else "N", "several" if _sv else "one")] = _w(
                    kind="probe", probe=_p, k=_k, n=_n, trans=_t, sizes=_probe_sizes(R.PROBES[_p][2], _sv),
                    share=(0, 2) if _sv else None, skip_dw=-1, skip_db=-1, start=False)
ACC_WSEGS = (40, 0, 150, 97, 1, 128, 64)  # contraction lengths 40 .. 150 (and one row); the 150-row one is two slabs
WGRAD_ACC = {
    "conv75": _w(kind="normal", k=75, n=64, sizes=ACC_WSEGS),
    "dense": _w(kind="normal", k=64, n=128, trans=True, sizes=ACC_WSEGS),
    "odd": _w(kind="normal", k=33, n=4, sizes=ACC_WSEGS), "k128": _w(kind="normal", k=128, n=36, sizes=ACC_WSEGS),
    "k130_chunks": _w(kind="normal", k=130, n=36, trans=True, sizes=ACC_WSEGS),
}
for _c in WGRAD_ACC.values():
    _c.update(skip_dw=-1, skip_db=-1, start=False, dbias=False)


def build_wgrad(c):
    begin, end, rows = _bounds(c["sizes"])
    n_seg, k, n = len(begin), c["k"], c["n"]
    cov = _covered(begin, end, rows)
    rng = np.random.default_rng(1000 * n + k + c["seed"])
    d = dict(c, begin=begin, end=end, rows=rows, n_seg=n_seg, covered=cov)
    if c["kind"] == "probe":
        a, g = np.zeros((rows, k), np.float32), np.zeros((rows, n), np.float32)
        for s in range(n_seg):  # the contraction runs over the rows of a segment
            if end[s] > begin[s]:
                at, gs = R.probe_operands(c["probe"], k, end[s] - begin[s], n, 91 + s)
                a[begin[s]:end[s]], g[begin[s]:end[s]] = at.T, gs
        lsb_g = R.PROBES[c["probe"]][3] if c["probe"] != "a2w2" else 2.0 ** -9
    elif c["kind"] == "normal":
        a, g = rng.standard_normal((rows, k)).astype(np.float32), rng.standard_normal((rows, n)).astype(np.float32)
        lsb_g = None
    elif c["kind"] == "sign":
        a, g = rng.integers(-1, 2, (rows, k)).astype(np.float32), rng.integers(-1, 2, (rows, n)).astype(np.float32)
        lsb_g = 1.0
    else:
        a, g = (rng.integers(-3, 4, (rows, k)) * 0.5).astype(np.float32), (rng.integers(-3, 4, (rows, n)) * 0.25).astype(np.float32)
        lsb_g = 0.25
    d["a"], d["g"] = _padded(a, c["lda"], cov), _padded(g, c["ldg"], cov)
    block = list(range(n_seg))
    if c["share"]:
        block[c["share"][1]] = c["share"][0]
    d["dw_off"] = [-1 if s == c["skip_dw"] else block[s] * k * n for s in range(n_seg)]
    d["db_off"] = [-1 if s == c["skip_db"] else block[s] * n for s in range(n_seg)] if c["dbias"] else None
    d["lsb"] = None if c["kind"] == "normal" else (R.PROBES[c["probe"]][3] if c["kind"] == "probe" else
                                                     (1.0 if c["kind"] == "sign" else 0.125))
    d["lsb_db"] = lsb_g
    if c["start"]:
        d["dw0"] = (rng.integers(-8, 9, n_seg * k * n) * d["lsb"]).astype(np.float32)
        d["db0"] = (rng.integers(-8, 9, n_seg * n) * lsb_g).astype(np.float32) if c["dbias"] else None
    else:
        d["dw0"] = np.zeros(n_seg * k * n, np.float32)
        d["db0"] = np.zeros(n_seg * n, np.float32) if c["dbias"] else None
    return d


def wgrad_ref(d):
    return R.seg_wgrad_ref(d["begin"], d["end"], d["a"], d["g"], d["k"], d["n"], d["dw0"], d["dw_off"], d["db0"],
                           d["db_off"], d["trans"])


def wgrad_in_float32(d, product):
    """dW from zero with ``product(a^T, g, None)`` as the arithmetic of every segment (accuracy cases: no shared
    blocks)."""
    dw = np.zeros(d["n_seg"] * d["k"] * d["n"], np.float32)
    for s in range(d["n_seg"]):
        r = slice(d["begin"][s], d["end"][s])
        if d["dw_off"][s] < 0 or r.stop == r.start:
            continue
        p = product(np.ascontiguousarray(d["a"][r, :d["k"]].T), d["g"][r, :d["n"]], None)
        dw[d["dw_off"][s]:d["dw_off"][s] + d["k"] * d["n"]] += (p.T if d["trans"] else p).reshape(-1)
    return dw


def _launch_wgrad(d, times=2):
    import deepchem_amd as dc
    from deepchem_amd import ops
    a, g = _dev(d["a"]), _dev(d["g"])
    got = {}
    try:
        for mode in MODES:
            dc.set_gemm_mode(mode)
            got[mode] = []
            for _ in range(times):
                dw, db = _dev(d["dw0"]), _dev(d["db0"])
                ops.seg_gemm_wgrad(d["begin"], d["end"], a[:, :d["k"]], g[:, :d["n"]], dw, d["dw_off"], db, d["db_off"],
                                   d["trans"])
                got[mode].append((dw.cpu().numpy(), None if db is None else db.cpu().numpy()))
    finally:
        dc.set_gemm_mode("fast")
    return got


def _check_wgrad_exact(d, what):
    dw_ref, db_ref, _, _ = wgrad_ref(d)
    for mode, outs in _launch_wgrad(d).items():
        for i, (dw, db) in enumerate(outs):
            bad = np.flatnonzero(dw.astype(np.float64) != dw_ref)
            assert bad.size == 0, "%s %s launch %d: %d elements of dW differ, first at %d: %r for %r" % (
                what, mode, i, bad.size, bad[0], dw[bad[0]], dw_ref[bad[0]])
            if db_ref is not None:
                assert np.array_equal(db.astype(np.float64), db_ref), "%s %s launch %d: dbias" % (what, mode, i)


@pytest.mark.parametrize("name", list(WGRAD_INT))
def test_seg_gemm_wgrad_exact(name):
    """Integer data, 128-row slabs (the floor), operand rows padded with NaN, dW and dbias starting non-zero, segment 5
    without dW and segment 7 without dbias.  Fast: wgrad3_kernel KT 1..4 and 2..5 chunks; exact: wgrad_kernel KT 1..8
    and a second / third launch (module docstring)."""
    _check_wgrad_exact(build_wgrad(WGRAD_INT[name]), name)


@pytest.mark.parametrize("name", list(WGRAD_SLABS))
def test_seg_gemm_wgrad_slabs(name):
    """Operands in {-1, 0, 1} at k = n = 4: slabs of 192, 320 and 4096 rows (worked out in the module docstring), four
    row parts per slab, up to 206 slabs adding into one 4 x 4 block."""
    _check_wgrad_exact(build_wgrad(WGRAD_SLABS[name]), name)


@pytest.mark.parametrize("name", list(WGRAD_PROBE))
def test_seg_gemm_wgrad_probe(name):
    """Piece probes with the contraction over the rows of a segment: wgrad3_kernel KT = 1 and KT = 3, one slab and
    several (two of them adding into the same block); wgrad_kernel in exact mode."""
    _check_wgrad_exact(build_wgrad(WGRAD_PROBE[name]), name)


def wgrad_accuracy_bound(d):
    dw_ref, _, S, _ = wgrad_ref(d)
    e_seq = err_units(wgrad_in_float32(d, R.seq32_product), dw_ref, S)
    return dw_ref, S, e_seq, 2.0 * max(e_seq, 1.0)


@pytest.mark.parametrize("name", list(WGRAD_ACC))
def test_seg_gemm_wgrad_accuracy(name):
    d = build_wgrad(WGRAD_ACC[name])
    dw_ref, S, e_seq, bound = wgrad_accuracy_bound(d)
    figures = {}
    for mode, outs in _launch_wgrad(d).items():
        figures[mode] = max(err_units(dw, dw_ref, S) for dw, _ in outs)
        assert all(np.all(dw[S == 0] == 0) for dw, _ in outs), "%s %s: a block without rows was written" % (name, mode)
        print("wgrad accuracy %s %s: e = %.2f, e_seq32 = %.2f, bound %.2f" % (name, mode, figures[mode], e_seq, bound))
    for mode, e in figures.items():
        assert e <= bound, "%s %s: e = %.2f roundings of S, bound %.2f (e_seq32 = %.2f)" % (name, mode, e, bound, e_seq)
