"""The persistent forward kernels (csrc/fwd_fused.hip, csrc/fwd_bf16.hip) and the one-pass backward (csrc/bwd_fused.hip)
pinned operation by operation, through ``ops.fwd_fused_gemm``, ``ops.fused_conv_bwd`` and ``ops.fused_dense_bwd`` --
entries with NO other kernel behind them -- against the float64 restatements of tests/edge_refs.py.  Nothing here runs
a model step or collates a graph.  The three kinds of case are those of tests/test_gpu_product_edges.py:

  * EXACT, integer data: operands from {-1, 0, 1}, weights from {-1, -.5, 0, .5, 1}, coefficient vectors from powers of
    two and small integers (one bf16 piece each, both fmaf of G exact, every partial sum a float32 number in any order,
    the fp32 partials of the periodic flushes included -- tests/test_fused_refs_host.py checks that for every case).
    ``np.array_equal`` against float64 for out, dW, db, dIn and the summed replicas of stats / psums, two launches
    each with fresh outputs (the sweep direction alternates; dW, db and the sums are atomics).
  * EXACT, piece probes (edge_refs.PROBES, cancelling_probe): bit-equal at the term subset the form claims.
  * ACCURACY: standard-normal data on ACC_SEGS at the model's shapes, e = max |got - ref64| / S in units of 2^-24.

What the kernels' headers promise about their inputs, and what the cases feed them accordingly:

  fwd_fused_kernel, fwd_reg_kernel (float rows)   columns >= k_in, rows beyond a tile's end, rows outside every segment
      and the rows of an operand whose weight offset is < 0 are masked: all NaN here.
  fwd_hd_kernel (bf16 rows)   "columns [k_in, KO) of the rows are zero (or absent: ld < KO)": zeros here; an absent
      operand is NOT masked (its weight images are zero): its rows stay finite; rows outside every segment: NaN.
  fused_bwd_kernel   "what lies outside the tile is zeroed when it goes to LDS": columns >= k_in of the In rows, the
      padding columns of dy / gc and all rows outside every segment are NaN.  The In rows of an absent operand are read
      (0 x value in psums): finite.  dIn of an absent operand is written as zeros.
  Outputs start as a sentinel inside buffers with guard rows (the gap and the tail of the table) and, where the case
  says so, guard columns; accumulators start as [sentinel 2F][zeros 32 x 2F][sentinel], and the sentinels must survive.

Which instantiation a case reaches (``fwd_shape`` in csrc/common.h, ``fwd_fused_gemm``, ``fwd_h_gemm``,
``fused_conv_bwd``, ``fused_dense_bwd``):

  forward, float rows   conv   (two operands, k 33..64 -> 64)   fwd_fused_kernel<128, 2, 64, 64, false>, grid <= 256
                        dense  (one operand, k 33..64 -> 128 T) fwd_fused_kernel<64, 1, 64, 128, true>, grid <= 256
                        conv80 (two operands, k 65..80 -> 64)   wprep_kernel<false> + fwd_reg_kernel<2, 80, 64, false>, <= 512
  forward, bf16 rows    conv80 / conv / dense, bf16 out         wprep_kernel<false|true> + fwd_hd_kernel<2, 80, 64, false>,
                                                                <2, 64, 64, false>, <1, 64, 128, true>, grid <= 512
                        conv80, float out                       fwd_hd_kernel<2, 80, 64, false, true>
  backward, conv        k 33..64, dIn wanted  (``b2d``)         fused_bwd_kernel<64, 2, 2, F, F, true,  HB, GB>, grid <= 256
                        k 33..64, no dIn      (``b2``)          fused_bwd_kernel<64, 2, 2, F, F, false, HB, GB>, grid <= 512
                        k 65..96, no dIn      (``b3``)          fused_bwd_kernel<64, 3, 2, F, F, false, HB, GB>
                        k 65..96, In alone bf16 (``ib``)        fused_bwd_kernel<64, 3, 2, F, F, false, F, F, true>
  backward, dense       k 36..64 (``bd``)                       fused_bwd_kernel<128, 2, 1, T, T, true, HB, GB>, grid <= 256
  with (HB, GB) = (F, F) for float storage (``f``), (T, F) for ``act_bf16 = 1`` (``h``), (T, T) for ``act_bf16 = 2``
  (``g``): thirteen backward instantiations.  Every one of the 3 + 4 + 13 is reached by integer cases (the FWD_INT /
  BWD_INT tables carry form and shape in every case name), by a probe case (FWD_PROBE / BWD_PROBE) and by an accuracy
  case (FWD_ACC / BWD_ACC).

Tables: SMALL of tests/test_gpu_seg_walk.py (empty first / middle / last segments, one row, exactly 64 and 128 rows,
ragged ones, rows outside every segment); SIXTEEN, all sixteen segments (segment indices up to 15 in the ``deg``
weighting of psums); WALK, 99 401 rows = 1 557 tiles of 64 rows / 781 of 128, i.e. at least 3 grid_cap + 1 for both
caps, over seven non-empty segments, three of them (100, 1 and 130 rows) smaller than one workgroup's share and
separated by empty ones: the workgroups around them prefetch two tiles ahead across the boundary, rebuild the weight
images, reload the bias, run flush_w and step the cursor over an empty segment, in both sweep directions, and hold
ragged tiles.  (With at most 16 segments and 256 or more workgroups only the workgroups next to a boundary can cross
one: "every workgroup" is not attainable; all of them prefetch two ahead.)  LONG tables: flush_period x grid_cap + 1
tiles -- 2 049 of 128 rows for fwd_fused_kernel, 2 049 of 64 for fused_bwd_kernel with psums, 4 097 for
fwd_reg_kernel, 16 385 for fwd_hd_kernel (operands generated on the device, the reference in row chunks).

MEASURED on an MI355X.  All 275 integer cases and all 51 probe cases came out bit for bit equal to float64 on their first
run (both sweep directions, atomics and replica sums included), so every exact assertion is ``np.array_equal``.
Accuracy, e in units of 2^-24 of the element's own S; bound = 2 max(e_ref, 1); e_ref from seq32_product (float forms,
float-output bf16 form, IB) or split_product_np with the claimed subset (fwd_hd_kernel, HB, GB); for outputs stored as
bf16 e is the part of the error beyond half a bf16 ulp of the reference:

  case                    output      e_ref    bound        e
  f32_conv75  (fwd_reg)   out          3.17     6.34     2.40
  f32_conv76  (fwd_reg)   out          3.13     6.25     3.89
  f32_conv64  (fwd_fused) out          3.44     6.89     2.64
  f32_dense   (fwd_fused) out          3.41     6.82     3.14
  hf_conv75   (fwd_hd)    out          2.91     5.83     2.61
  h_conv75    (fwd_hd)    out bf16     1.74     3.49     0.19
  h_conv64    (fwd_hd)    out bf16     1.36     2.72     0.00
  h_dense     (fwd_hd)    out bf16     1.91     3.82     0.04
  b2d_f, b2_f             dW           3.14     6.28     2.79
                          db           3.28     6.55     2.34
  b2d_f                   dIn          2.64     5.28     2.68
  b3_f (k 75)             dW / db      3.16 / 3.04   6.33 / 6.07   2.90 / 1.95
  b3_f (k 76)             dW / db      2.62 / 3.40   5.24 / 6.81   2.61 / 1.91
  ib                      dW / db      2.98 / 3.04   5.96 / 6.07   2.90 / 1.69
  bd_f                    dW           2.59     5.17     1.05
                          db           4.68     9.36     2.11
                          dP           2.69     5.38     3.48
  b2d_h, b2_h             dW          54.34   108.68    54.34
                          db           4.09     8.18     1.95
  b2d_h                   dIn        129.31   258.62   129.31
  b3_h                    dW / db     94.23 / 3.10   188.46 / 6.20   94.23 / 1.72
  bd_h                    dW          17.98    35.95    18.30
                          db           5.99    11.99     2.22
                          dP          53.77   107.54    54.91
  b2d_g, b2_g             dW         111.45   222.89   111.45
                          db           2.72     5.43     2.48
  b2d_g                   dIn bf16    97.41   194.82    44.40
  b3_g                    dW / db     71.36 / 3.67   142.72 / 7.33   71.36 / 2.60
  bd_g                    dW          15.91    31.81    16.14
                          db           8.70    17.41     1.48
                          dP bf16     45.06    90.11    30.81

(the HB forms keep "the terms above 2^-16", as their header says: 16 .. 130 roundings, and the conv kernels reproduce the
emulated subset to the printed digit.)  stats against the float64 sums of the stored output: e <= 0.59 with bounds
2.0 .. 9.7; psums: e <= 0.15 with bounds 2.0 .. 2.5.
"""
import numpy as np
import pytest
import torch

from tests import edge_refs as R
from tests import test_gpu_product_edges as P
from tests.test_gpu_product_edges import ACC_SEGS, _bounds, _covered, err_units
from tests.test_gpu_seg_walk import SMALL

pytestmark = pytest.mark.gpu

SENTINEL = -12288.0      # exact in bf16
ACC_SENTINEL = -7.5
SIXTEEN = (3, 0, 64, 65, 1, 0, 128, 17, 0, 70, 2, 129, 0, 33, 64, 5)
WALK = (20007, 0, 100, 0, 30000, 1, 130, 0, 25663, 23500)

def _long(tiles, rows):
    """Seven segments (empty, one row, ragged, empty, whole tiles, 37 rows, ragged) of exactly ``tiles`` tiles."""
    a = b = tiles // 3
    c = tiles - 3 - a - b
    return (0, 1, rows * a + 5, 0, rows * b, 37, rows * c - 3)


def _up(x, m):
    return (x + m - 1) // m * m


def _choice(rng, vals, shape):
    return rng.choice(np.array(vals, np.float32), shape)


def _dev(a, dtype=None):
    if a is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    return t if dtype is None else t.to(dtype)


def _host(t):
    return t.float().cpu().numpy().astype(np.float64) if t.dtype == torch.bfloat16 else t.cpu().numpy().astype(np.float64)


_SCRATCH = {}


def _scratch():
    from deepchem_amd import ops
    if "t" not in _SCRATCH:
        _SCRATCH["t"] = torch.zeros(ops.fwd_fused_scratch_floats(), dtype=torch.float32, device="cuda:0")
    return _SCRATCH["t"]


def _refused(fn):
    """Runs fn; True when the entry answered GCMI_ERR_UNSUPPORTED (anything else propagates)."""
    from deepchem_amd import _lib
    try:
        fn()
    except _lib.GcmiError as e:
        assert "status -3" in str(e) and "no other kernel stands behind this entry" in str(e), str(e)
        return True
    return False


# ================================================================================================ forward
# rows = rows of a tile, cap = the largest grid, period = tiles between two flushes of the fp32 partial sums,
# per_thread = values of one column a thread adds per tile
FWD_SHAPES = {
    "conv": dict(nops=2, ko=64, n_out=64, trans=False),
    "conv80": dict(nops=2, ko=80, n_out=64, trans=False),
    "dense": dict(nops=1, ko=64, n_out=128, trans=True),
}


def fwd_walk(shape, form):
    """(rows per tile, grid cap, flush period, rows per thread and tile) of the kernel a forward case reaches."""
    if form != "f32":
        return 64, 512, 32, (2 if FWD_SHAPES[shape]["n_out"] == 64 and form == "h" else 4)
    return {"conv": (128, 256, 8, 4), "dense": (64, 256, 8, 4), "conv80": (64, 512, 8, 16)}[shape]


def _f(shape, form="f32", **kw):
    """One forward case.  form: "f32" float rows (ops.fwd_fused_gemm -> gcmi_fwd_fused_gemm), "h" bf16 rows and bf16
    out, "hf" bf16 rows and float out (gcmi_fwd_fused_gemm_h).  k / ld: columns and pitch of every operand; skip1 /
    skip2: the segment whose first / second weight offset is -1; bias "all", "skip" (offset -1 on segment 2) or None;
    col0 / ldo: out is columns [col0, col0 + n_out) of a matrix of ldo columns."""
    c = dict(FWD_SHAPES[shape], shape=shape, form=form, k=FWD_SHAPES[shape]["ko"], k2=None, ld=0, sizes=SMALL, act=1,
             skip1=-1, skip2=-1, bias="all", stats=True, col0=0, ldo=0, kind="int", probe=None, seed=0)
    c.update(kw)
    c["ld"] = c["ld"] or _up(c["k"], 4 if form == "f32" else 8)
    c["ldo"] = c["ldo"] or c["col0"] + c["n_out"]
    return c


FWD_INT = {}
for _form, _m in (("f32", 4), ("h", 8)):
    for _k in (33, 36, 63, 64):  # rows narrower than KO = 64 (the piece clamp), of 64 and wider
        for _ld in sorted({_up(_k, _m), 64, 64 + _m}):
            FWD_INT["%s_conv_k%d_ld%d" % (_form, _k, _ld)] = _f("conv", _form, k=_k, ld=_ld, skip1=1, seed=_k + _ld)
    for _k in (65, 75, 76, 80):
        for _ld in sorted({_up(_k, _m), 80, 80 + _m}):  # narrower than KO = 80 (k 65, 75, 76), of 80 and wider
            if _ld >= _k:
                FWD_INT["%s_conv80_k%d_ld%d" % (_form, _k, _ld)] = _f("conv80", _form, k=_k, ld=_ld, skip1=1, seed=_k + _ld)
    for _k in (33, 36, 64):
        FWD_INT["%s_dense_k%d" % (_form, _k)] = _f("dense", _form, k=_k, seed=_k)
        FWD_INT["%s_dense_k%d_ld%d" % (_form, _k, 64 + _m)] = _f("dense", _form, k=_k, ld=64 + _m, act=0, seed=_k + 1)
    for _shape in FWD_SHAPES:
        _two = FWD_SHAPES[_shape]["nops"] == 2
        _n = "%s_%s_" % (_form, _shape)
        FWD_INT[_n + "skip2_act0"] = _f(_shape, _form, skip1=1 if _two else -1, skip2=7 if _two else -1, act=0, seed=1)
        FWD_INT[_n + "bias_skip"] = _f(_shape, _form, bias="skip", seed=2)
        FWD_INT[_n + "no_bias_no_stats"] = _f(_shape, _form, bias=None, stats=False, act=0, seed=3)
        FWD_INT[_n + "block"] = _f(_shape, _form, col0=8, ldo=FWD_SHAPES[_shape]["n_out"] + 24, skip1=4 if _two else -1, seed=4)
        FWD_INT[_n + "sixteen"] = _f(_shape, _form, sizes=SIXTEEN, skip1=0 if _two else -1, skip2=9 if _two else -1, seed=5)
        FWD_INT[_n + "walk"] = _f(_shape, _form, sizes=WALK, skip1=2 if _two else -1, k=FWD_SHAPES[_shape]["ko"] - 4, seed=6)
FWD_INT["hf_conv80_k65_ld72"] = _f("conv80", "hf", k=65, ld=72, skip1=1, seed=7)
FWD_INT["hf_conv80_k75_ld80"] = _f("conv80", "hf", k=75, ld=80, skip2=7, act=0, seed=8)
FWD_INT["hf_conv80_k80_ld88_block"] = _f("conv80", "hf", k=80, ld=88, col0=8, ldo=80, bias="skip", seed=9)
FWD_INT["hf_conv80_sixteen"] = _f("conv80", "hf", k=76, ld=80, sizes=SIXTEEN, skip1=0, bias=None, seed=10)
FWD_INT["hf_conv80_walk"] = _f("conv80", "hf", k=76, ld=80, sizes=WALK, skip1=2, seed=11)
FWD_LONG = {
    "f32_conv_long": _f("conv", "f32", sizes=_long(2049, 128), skip1=1, seed=12),
    "f32_conv80_long": _f("conv80", "f32", k=76, ld=76, sizes=_long(4097, 64), skip1=1, seed=13),
}

# probes: the probe's contraction (PROBES[name][2] columns, split evenly over the operands) sits in the leading columns of
# every operand; the columns behind it are zero in the operands
FWD_PROBE = {}
for _shape in FWD_SHAPES:
    for _p in ("a3w1", "a1w3", "a2w2"):
        FWD_PROBE["f32_%s_%s" % (_shape, _p)] = _f(_shape, "f32", kind="probe", probe=_p, sizes=ACC_SEGS, stats=False)
    FWD_PROBE["h_%s_cancel1" % _shape] = _f(_shape, "h", kind="probe", probe="cancel1", sizes=ACC_SEGS, stats=False, act=0, bias=None)
    FWD_PROBE["h_%s_cancel2" % _shape] = _f(_shape, "h", kind="probe", probe="cancel2", sizes=ACC_SEGS, stats=False, act=0, bias=None)
FWD_PROBE["hf_conv80_a1w3"] = _f("conv80", "hf", kind="probe", probe="a1w3", sizes=ACC_SEGS, stats=False)

FWD_ACC = {}
for _form in ("f32", "h"):  # (seeds: see tests/test_fused_refs_host.py on the lost-term margin)
    FWD_ACC[_form + "_conv75"] = _f("conv80", _form, kind="normal", k=75, sizes=ACC_SEGS)
    FWD_ACC[_form + "_conv64"] = _f("conv", _form, kind="normal", sizes=ACC_SEGS)
    FWD_ACC[_form + "_dense"] = _f("dense", _form, kind="normal", sizes=ACC_SEGS)
FWD_ACC["f32_conv76"] = _f("conv80", "f32", kind="normal", k=76, sizes=ACC_SEGS)
FWD_ACC["hf_conv75"] = _f("conv80", "hf", kind="normal", k=75, sizes=ACC_SEGS)
for _c in FWD_ACC.values():
    _c["seed"] = 1


def build_fwd(c):
    """The numpy side of one forward case, with the keys of test_gpu_product_edges.build_gemm (so that its gemm_ref and
    gemm_in_float32 serve here too): operands as float32 arrays holding bf16-exact values where the form stores bf16."""
    begin, end, n = _bounds(c["sizes"])
    n_seg, n_out, trans, k, ld, nops = len(begin), c["n_out"], c["trans"], c["k"], c["ld"], c["nops"]
    half = c["form"] != "f32"
    cov = _covered(begin, end, n)
    rng = np.random.default_rng(7919 * c["seed"] + 31 * k + ld + n_out)
    d = dict(c, begin=begin, end=end, n=n, n_seg=n_seg, covered=cov, k1=k, k2=(c["k2"] or k) if nops == 2 else 0, ld1=ld, ld2=ld)
    lsb = None
    if c["kind"] == "probe":
        a_all, w_all, lsb, Kp = _fwd_probe_operands(c, n, n_seg, rng)
    for o in range(nops):
        ko = d["k1"] if o == 0 else d["k2"]
        if c["kind"] == "int":
            a, w = _choice(rng, (-1, 0, 1), (n, ko)), _choice(rng, (-1, -.5, 0, .5, 1), (n_seg, ko, n_out))
            lsb = 0.5
        elif c["kind"] == "normal":
            a, w = rng.standard_normal((n, ko)).astype(np.float32), rng.standard_normal((n_seg, ko, n_out)).astype(np.float32)
            a = R.bf16_round(a) if half else a
        else:
            per = Kp // nops
            a = np.zeros((n, ko), np.float32)
            a[:, :per] = a_all[:, o * per:(o + 1) * per]
            w = _choice(rng, (-1, 1), (n_seg, ko, n_out))
            w[:, :per] = w_all[:, o * per:(o + 1) * per]
        skip = c["skip1"] if o == 0 else c["skip2"]
        full = np.full((n, ld), np.nan, np.float32)
        full[cov, :ko] = a[cov]
        if half:
            full[cov, ko:] = 0.0  # fwd_bf16.hip: the padding columns of the rows are zero
        elif skip >= 0:
            full[begin[skip]:end[skip]] = np.nan  # masked with the absent term
        d["a%d" % (o + 1)] = full
        d["w%d" % (o + 1)] = np.ascontiguousarray(w.transpose(0, 2, 1) if trans else w).reshape(-1)
        d["w%d_off" % (o + 1)] = [-1 if s == skip else s * ko * n_out for s in range(n_seg)]
    if nops == 1:
        d["a2"] = d["w2"] = d["w2_off"] = None
    if c["bias"] is None:
        d["bias_v"], d["bias_off"] = None, None
    else:
        if c["kind"] == "int":
            bias = _choice(rng, (-1, -.5, 0, .5, 1), (n_seg, n_out))
        elif c["kind"] == "normal":
            bias = rng.standard_normal((n_seg, n_out)).astype(np.float32)
        else:
            bias = (rng.integers(-8, 9, (n_seg, n_out)) * lsb).astype(np.float32)
        d["bias_v"] = bias.reshape(-1)
        d["bias_off"] = [-1 if c["bias"] == "skip" and s == 2 else s * n_out for s in range(n_seg)]
    d["out0"] = np.full((n, c["ldo"]), SENTINEL, np.float32)
    d["lsb"] = None if c["kind"] == "normal" else lsb
    return d


def _fwd_probe_operands(c, n, n_seg, rng):
    nops, n_out = c["nops"], c["n_out"]
    if c["probe"].startswith("cancel"):
        Kp = 96 if nops == 2 else 64
        piece = int(c["probe"][-1])
        a, _, lsb = R.cancelling_probe(rng, n, Kp, n_out, piece)
        w = np.stack([R.cancelling_probe(np.random.default_rng(500 + s), 1, Kp, n_out, piece)[1] for s in range(n_seg)])
        return a, w, lsb, Kp
    Kp = min(R.probe_spec(c["probe"])[2], c["ko"] * nops)
    Kp = Kp if nops == 2 else min(Kp, 64)
    a = R.probe_operands(c["probe"], n, Kp, n_out, 77 + c["seed"])[0]
    w = np.stack([R.probe_operands(c["probe"], 1, Kp, n_out, 78 + s + c["seed"])[1] for s in range(n_seg)])
    return a, w, R.probe_spec(c["probe"])[3], Kp


def fwd_ref(d):
    """(the float64 matrix out must equal where nothing is rounded, S of the n_out columns, the stored values: rounded to
    bf16 under form "h")."""
    full, S = P.gemm_ref(d)
    if d["form"] == "h":
        cols = slice(d["col0"], d["col0"] + d["n_out"])
        stored = full.copy()
        stored[d["covered"], cols] = R.bf16_round(full[d["covered"], cols].astype(np.float32))
        return full, S, stored
    return full, S, full


def _launch_fwd(d, times=2):
    """``times`` launches with fresh outputs; [(full out matrix as float64, (2, n_out) sums or None)]."""
    from deepchem_amd import ops
    half = d["form"] != "f32"
    adt = torch.bfloat16 if half else None
    a1, a2 = _dev(d["a1"], adt), _dev(d["a2"], adt)
    w1, w2, bias = _dev(d["w1"]), _dev(d["w2"]), _dev(d["bias_v"])
    got = []
    for _ in range(times):
        full = _dev(d["out0"], torch.bfloat16 if d["form"] == "h" else None)
        acc = _dev(R.fresh_acc(d["n_out"], ACC_SENTINEL)) if d["stats"] else None
        ops.fwd_fused_gemm(d["begin"], d["end"], a1[:, :d["k1"]], w1, d["w1_off"], None if a2 is None else a2[:, :d["k2"]],
                           w2, d["w2_off"], bias, d["bias_off"], d["n_out"], d["trans"], d["act"] == 1, d["n"], d["k1"],
                           d["k2"], full[:, d["col0"]:d["col0"] + d["n_out"]], stats=acc, scratch=_scratch())
        got.append((_host(full), None if acc is None else R.read_acc(acc.cpu().numpy(), d["n_out"], ACC_SENTINEL)))
    return got


def _check_fwd_exact(d, what):
    _, _, stored = fwd_ref(d)
    cols = slice(d["col0"], d["col0"] + d["n_out"])
    sums_ref = R.bn_sums_ref(stored[:, cols], d["covered"])
    for i, (full, sums) in enumerate(_launch_fwd(d)):
        bad = np.argwhere(full != stored)
        assert bad.size == 0, "%s launch %d: %d elements differ, first at %s: %r for %r" % (
            what, i, len(bad), tuple(bad[0]), full[tuple(bad[0])], stored[tuple(bad[0])])
        if sums is not None:
            assert np.array_equal(sums, sums_ref), "%s launch %d: the BatchNorm sums differ" % (what, i)


@pytest.mark.parametrize("name", list(FWD_INT))
def test_forward_exact(name):
    _check_fwd_exact(build_fwd(FWD_INT[name]), name)


@pytest.mark.parametrize("name", list(FWD_LONG))
def test_forward_exact_long_walk(name):
    """flush_period x grid_cap + 1 tiles: some workgroup flushes its fp32 partial sums in the middle of its walk."""
    _check_fwd_exact(build_fwd(FWD_LONG[name]), name)


def test_forward_exact_long_walk_bf16():
    """fwd_hd_kernel<2, 64, 64, false>, 32 x 512 + 1 tiles of 64 rows (1 048 640 rows, one segment plus a one-row one):
    operands from {-1, 0, 1} generated on the device, the float64 reference in chunks of 65 536 rows."""
    from deepchem_amd import ops
    n_big = 64 * (32 * 512 - 1) + 63
    begin, end = [0, n_big], [n_big, n_big + 1]
    n = n_big + 1
    gen = torch.Generator(device="cuda:0").manual_seed(5)
    a = [(torch.randint(-1, 2, (n, 64), generator=gen, device="cuda:0", dtype=torch.int8)).to(torch.bfloat16) for _ in range(2)]
    w = (torch.randint(-2, 3, (2, 2, 64, 64), generator=gen, device="cuda:0", dtype=torch.int8)).to(torch.float32) * 0.5
    bias = (torch.randint(-2, 3, (2, 64), generator=gen, device="cuda:0", dtype=torch.int8)).to(torch.float32) * 0.5
    ref_sums = torch.zeros((2, 64), dtype=torch.float64, device="cuda:0")
    refs = []
    for r0 in range(0, n, 65536):
        r1 = min(r0 + 65536, n)
        parts = []
        for s in range(2):
            lo, hi = max(r0, begin[s]), min(r1, end[s])
            if hi > lo:
                y = a[0][lo:hi].double() @ w[s, 0].double() + a[1][lo:hi].double() @ w[s, 1].double() + bias[s].double()
                parts.append(torch.relu(y))
        y = torch.cat(parts)
        assert float(y.abs().max()) < 128.0  # multiples of 0.5 below 128: exact in bf16
        ref_sums[0] += y.sum(0)
        ref_sums[1] += (y * y).sum(0)
        refs.append(y.to(torch.bfloat16))
    ref = torch.cat(refs)
    off = [0, 2 * 64 * 64]
    for i in range(2):
        out = torch.full((n, 64), SENTINEL, dtype=torch.bfloat16, device="cuda:0")
        acc = _dev(R.fresh_acc(64, ACC_SENTINEL))
        ops.fwd_fused_gemm(begin, end, a[0], w.reshape(-1), off, a[1], w.reshape(-1), [o + 64 * 64 for o in off],
                           bias.reshape(-1), [0, 64], 64, False, True, n, 64, 64, out, stats=acc, scratch=_scratch())
        assert torch.equal(out, ref), "launch %d" % i
        assert np.array_equal(R.read_acc(acc.cpu().numpy(), 64, ACC_SENTINEL), ref_sums.cpu().numpy()), "launch %d: sums" % i


@pytest.mark.parametrize("name", list(FWD_PROBE))
def test_forward_probe(name):
    _check_fwd_exact(build_fwd(FWD_PROBE[name]), name)


def fwd_accuracy_bound(d):
    """(ref, S, stored, e_ref, bound): e_ref is the figure of the sequential float32 product of the same inputs (float
    rows, and bf16 rows with float out) or of the emulated product of the stored operand piece with three weight
    pieces (bf16 out); bound = 2 max(e_ref, 1)."""
    ref, S, stored = fwd_ref(d)
    if d["form"] == "h":
        product = lambda a, w, acc: R.split_product_np(a, w, R.HD_TERMS, acc)  # noqa: E731
    else:
        product = R.seq32_product
    cols = slice(d["col0"], d["col0"] + d["n_out"])
    e_ref = err_units(P.gemm_in_float32(d, product), ref[:, cols], S)
    return ref, S, stored, e_ref, 2.0 * max(e_ref, 1.0)


def sums_check(what, sums, got_stored, ref_stored, elem_bound, chunk, covered):
    """The (2, F) sums of an accuracy case.  (i) Against the float64 sums of the values THE KERNEL stored, which is what
    the headers promise: only the summation differs, bound 2 max(e_seq, 1) roundings of the sum of absolute values, e_seq
    the figure of a float32 chain over ``chunk`` rows (the fp32 partial of one thread between two flushes) of the
    REFERENCE values.  (ii) Against the float64 sums of the reference values as stored: the same bound plus what the
    per-element bound ``elem_bound`` (an array) lets the stored values differ by."""
    g, r, b = got_stored[covered], ref_stored[covered], elem_bound[covered]
    figures = []
    for m, (gv, rv, bv) in enumerate(((g, r, b), (g * g, r * r, b * (2 * np.abs(r) + b)))):
        mag = np.abs(rv).sum(0)
        ok = mag > 0
        seq = R.seq32_colsum(r, chunk) if m == 0 else R.seq32_colsum(r, chunk, other=r)
        e_seq = float((np.abs(seq - rv.sum(0))[ok] / mag[ok]).max() / R.U24)
        bound = 2.0 * max(e_seq, 1.0)
        e_own = float((np.abs(sums[m] - gv.sum(0))[ok] / np.abs(gv).sum(0)[ok]).max() / R.U24)
        slack = bound * R.U24 * mag + bv.sum(0)
        worst = float((np.abs(sums[m] - rv.sum(0))[ok] / slack[ok]).max())
        print("%s sums[%d]: e_own = %.2f, e_seq32 = %.2f, bound %.2f; against the reference %.3f of its bound" % (
            what, m, e_own, e_seq, bound, worst))
        figures.append((e_own, bound, worst))
    for m, (e_own, bound, worst) in enumerate(figures):
        assert e_own <= bound, "%s sums[%d]: e = %.2f, bound %.2f" % (what, m, e_own, bound)
        assert worst <= 1.0, "%s sums[%d] against the reference: %.3f of the bound" % (what, m, worst)


@pytest.mark.parametrize("name", list(FWD_ACC))
def test_forward_accuracy(name):
    d = build_fwd(FWD_ACC[name])
    ref, S, stored, e_ref, bound = fwd_accuracy_bound(d)
    cols = slice(d["col0"], d["col0"] + d["n_out"])
    cov = d["covered"]
    outs = _launch_fwd(d)
    assert np.array_equal(outs[0][0], outs[1][0]), name + ": the two sweep directions differ"
    full, sums = outs[0]
    assert np.all(full[~cov] == SENTINEL), name + ": rows outside every segment were written"
    err = np.abs(full[:, cols] - ref[:, cols])
    if d["form"] == "h":  # stored rounded: half a bf16 ulp of the reference on top of the product's bound
        allowed = 0.5 * R.ulp(ref[:, cols], bf16=True) + bound * S * R.U24
        m = S > 0
        worst = float((err[m] / allowed[m]).max())
        e = float(((err[m] - 0.5 * R.ulp(ref[:, cols], bf16=True)[m]).clip(0) / S[m]).max() / R.U24)
        print("forward accuracy %s: e beyond half a bf16 ulp = %.2f, e_ref = %.2f, bound %.2f, worst %.3f of allowed" % (
            name, e, e_ref, bound, worst))
        assert worst <= 1.0, "%s: %.3f of half a bf16 ulp + %.2f roundings of S (e_ref = %.2f)" % (name, worst, bound, e_ref)
        elem = R.ulp(ref[:, cols], bf16=True) + bound * S * R.U24
    else:
        e = err_units(full[:, cols], ref[:, cols], S)
        print("forward accuracy %s: e = %.2f, e_ref = %.2f, bound %.2f" % (name, e, e_ref, bound))
        assert e <= bound, "%s: e = %.2f roundings of S, bound %.2f (e_ref = %.2f)" % (name, e, bound, e_ref)
        elem = bound * S * R.U24
    _, _, period, per_thread = fwd_walk(d["shape"], d["form"])
    sums_check("forward accuracy " + name, sums, full[:, cols], stored[:, cols], elem, period * per_thread, cov)


def _fwd_refusal_cases():
    c = {
        "n_out60": _f("conv", n_out=60),
        "k1_ne_k2": _f("conv", k=64, k2=60),
        "k32": _f("conv", k=32), "k81": _f("conv80", k=81, ld=84),
        "misaligned_out": _f("conv", col0=1, ldo=68),
        "ldo_mod4": _f("conv", ldo=66),
        "accumulate_shape": _f("dense", trans=False),  # 64 -> 128 in k x n layout: no such persistent kernel
        "h_ld_mod8": _f("conv", "h", ld=68),
        "h_k32": _f("conv", "h", k=32), "h_k81": _f("conv80", "h", k=81, ld=88),
        "hf_conv": _f("conv", "hf"), "hf_dense": _f("dense", "hf"),
        "h_ldo_mod8": _f("conv", "h", ldo=68),
    }
    return c


@pytest.mark.parametrize("name", ["exact_mode_f32", "exact_mode_h", "fused_off_f32"] + list(_fwd_refusal_cases()))
def test_forward_refusals(name):
    """GCMI_ERR_UNSUPPORTED with an error text, nothing launched (so nothing written): out keeps its sentinel."""
    import deepchem_amd as dc
    from deepchem_amd import _lib, ops
    exact, off = name.startswith("exact_mode"), name.startswith("fused_off")
    c = _f("conv", "h" if name.endswith("_h") else "f32") if exact or off else _fwd_refusal_cases()[name]
    d = build_fwd(dict(c, sizes=ACC_SEGS))
    half = d["form"] != "f32"
    a1, a2 = _dev(d["a1"], torch.bfloat16 if half else None), _dev(d["a2"], torch.bfloat16 if half else None)
    full = _dev(d["out0"], torch.bfloat16 if d["form"] == "h" else None)
    acc = _dev(R.fresh_acc(d["n_out"], ACC_SENTINEL))
    before = acc.clone()
    try:
        if exact:
            dc.set_gemm_mode("exact")
        if off:  # GCMI_OPT_FUSED_BWD: the switch of the one-pass kernels, forward and backward
            _lib.call("gcmi_set_option", _lib.GCMI_OPT_FUSED_BWD, 0)
        assert _refused(lambda: ops.fwd_fused_gemm(
            d["begin"], d["end"], a1[:, :d["k1"]], _dev(d["w1"]), d["w1_off"], None if a2 is None else a2[:, :d["k2"]],
            _dev(d["w2"]), d["w2_off"], _dev(d["bias_v"]), d["bias_off"], d["n_out"], d["trans"], True, d["n"], d["k1"],
            d["k2"], full[:, d["col0"]:d["col0"] + d["n_out"]], stats=acc, scratch=_scratch())), name + ": not refused"
    finally:
        dc.set_gemm_mode("fast")
        _lib.call("gcmi_set_option", _lib.GCMI_OPT_FUSED_BWD, 1)
    torch.cuda.synchronize()
    assert bool((full == SENTINEL).all()) and torch.equal(acc, before), name + ": a refusal wrote something"


# ================================================================================================ backward
# form -> (block, 32-column tiles of In, input gradients, act_bf16, in_bf16); the instantiation is in the module docstring
BWD_FORMS = {}
for _s, _l in ((0, "f"), (1, "h"), (2, "g")):
    BWD_FORMS["b2d_" + _l] = ("conv", 2, True, _s, 0)
    BWD_FORMS["b2_" + _l] = ("conv", 2, False, _s, 0)
    BWD_FORMS["b3_" + _l] = ("conv", 3, False, _s, 0)
    BWD_FORMS["bd_" + _l] = ("dense", 2, True, _s, 0)
BWD_FORMS["ib"] = ("conv", 3, False, 0, 1)
DENSE_ROWS = 700
MOL_SIZES = (1, 1, 7, 58, 3, 130, 12, 1)  # one-row molecules; the 58-row one holds rows 9..66, the 130-row one three tiles


def _b(form, **kw):
    """One backward case.  k / ld: columns and pitch of the In rows; skip_rel / skip_self: the segment whose first /
    second weight offset is -1; db "all", "skip" (offset -1 on segment 2) or None; share (i, j): segment j adds into
    the dW / db blocks of segment i; coef False: no coefficient vectors (conv); psums: with input gradients only;
    pad: dy / gc / g2 rows and the input-gradient rows 4 columns wider than needed (guard columns); rows: the dense
    block's row count."""
    block, kt, dgrad, store, ib = BWD_FORMS[form]
    c = dict(form=form, block=block, kt=kt, dgrad=dgrad, store=store, ib=ib, width=128 if block == "dense" else 64,
             nops=1 if block == "dense" else 2, k=64 if kt == 2 else 76, ld=0, sizes=SMALL, rows=DENSE_ROWS, coef=True,
             skip_rel=1 if block == "conv" else -1, skip_self=-1, db="all", share=None, psums=True, pad=0, kind="int",
             probe=None, variant=None, seed=0)
    c.update(kw)
    c["ld"] = c["ld"] or _up(c["k"], 4)
    c["psums"] = c["psums"] and dgrad
    return c


BWD_INT = {}
for _form, (_block, _kt, _dgrad, _store, _ib) in BWD_FORMS.items():
    if _block == "dense" or _dgrad:
        _widths = ((36, 36), (36, 64), (64, 64), (64, 68))  # input gradients: k_in % 4 == 0
    elif _kt == 2:
        _widths = ((33, 36), (33, 64), (36, 36), (36, 68), (63, 64), (64, 64), (64, 68))
    else:
        _widths = ((65, 68), (65, 80), (75, 76), (76, 76), (76, 80), (80, 80), (80, 84), (81, 84), (95, 96), (96, 96), (96, 100))
    for _k, _ld in _widths:
        BWD_INT["%s_k%d_ld%d" % (_form, _k, _ld)] = _b(_form, k=_k, ld=_ld, seed=_k + _ld)
    _conv = _block == "conv"
    BWD_INT[_form + "_db_skip_pad"] = _b(_form, db="skip", pad=4, skip_self=7 if _conv else -1, seed=1)
    BWD_INT[_form + "_bare"] = _b(_form, db=None, psums=False, coef=not _conv, seed=2)
    BWD_INT[_form + "_sixteen"] = _b(_form, sizes=SIXTEEN, rows=1000, skip_rel=0 if _conv else -1, skip_self=9 if _conv else -1,
                                     share=(2, 6) if _conv else None, seed=3)
    BWD_INT[_form + "_walk"] = _b(_form, sizes=WALK, rows=sum(WALK), skip_rel=2 if _conv else -1, seed=4,
                                  k=60 if _kt == 2 else 92)
BWD_LONG = {"b2d_f_long": _b("b2d_f", sizes=_long(2049, 64), seed=5)}

PROBE_SEGS = (24, 0, 24, 15, 1, 9)  # at most 48 rows per segment: within every probe's contraction length
BWD_PROBE = {}
for _form, (_block, _kt, _dgrad, _store, _ib) in BWD_FORMS.items():
    if _store == 0 and not _ib:
        _list = [(p, "dw") for p in ("a3w1", "a1w3", "a2w2")] + ([(p, "din") for p in ("a3w1", "a1w3", "a2w2")] if _dgrad else [])
    elif _ib:
        _list = [("a1w3", "dw")]
    elif _store == 1:
        _list = [("a1w2", "dw")] + ([("a2w1", "din"), ("a1w2", "din")] if _dgrad else [])
    else:
        _list = [("a1w2", "dw")] + ([("gb_a2w1", "din"), ("gb_a1w2", "din")] if _dgrad else [])
    for _p, _v in _list:
        BWD_PROBE["%s_%s_%s" % (_form, _v, _p)] = _b(_form, kind="probe", probe=_p, variant=_v, sizes=PROBE_SEGS, rows=48,
                                                     psums=False, skip_rel=-1, seed=len(_p) + len(_v))

BWD_ACC = {}
for _form, (_block, _kt, _dgrad, _store, _ib) in BWD_FORMS.items():
    BWD_ACC[_form] = _b(_form, kind="normal", sizes=ACC_SEGS, rows=302, k=64 if _kt == 2 else 75, skip_rel=1 if _block == "conv" else -1)
BWD_ACC["b3_f_k76"] = _b("b3_f", kind="normal", sizes=ACC_SEGS, k=76)
for _c in BWD_ACC.values():
    _c["seed"] = 1


def _readout(rows, n, rng, kind, width):
    """(membership (n,), g2 (n_mols, 2 width), arg (n_mols, width)): molecules of MOL_SIZES rows in turn; arg names the
    first row of the molecule (f % 4 == 0), its last row (1), nothing (2: -1) or the first row of the NEXT molecule,
    which no row of this one equals (3)."""
    sizes = []
    while sum(sizes) < rows:
        sizes.append(min(MOL_SIZES[len(sizes) % len(MOL_SIZES)], rows - sum(sizes)))
    n_mols = len(sizes)
    membership = np.zeros(n, np.int32)
    membership[:rows] = np.repeat(np.arange(n_mols), sizes)
    first = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    last = np.cumsum(sizes) - 1
    f = np.arange(width) % 4
    arg = np.where(f == 0, first[:, None], np.where(f == 1, last[:, None], np.where(f == 2, -1, np.roll(first, -1)[:, None])))
    g2 = rng.standard_normal((n_mols, 2 * width)).astype(np.float32) if kind == "normal" else _choice(rng, (-1, 0, 1), (n_mols, 2 * width))
    return membership, g2, arg.astype(np.int32)


def _bwd_probe_data(c, begin, end, n, rng):
    """(G, C, ins, w (n_seg, nops, k, width), lsb) of a probe case: G = dy + C with C a per-column constant (non-zero
    only where the incoming gradients are bf16 and G needs a second piece), gc = 1, A = 1, B = 0.  lsb: the power of two
    every term of dW, of dIn and every entry of G is a multiple of.  Where the contraction over the columns of G would be
    longer than 96 (the dense block's 128) the columns from 96 on are zero."""
    W, nops, k, name, variant = c["width"], c["nops"], c["k"], c["probe"], c["variant"]
    n_seg = len(begin)
    G, C = np.zeros((n, W), np.float32), np.zeros(W, np.float32)
    ins = [_choice(rng, (-1, 1), (n, k)) for _ in range(nops)]
    w = _choice(rng, (-1, 1), (n_seg, nops, k, W))
    gb_conv = c["store"] == 2 and c["block"] == "conv"
    if name == "gb_a2w1" or (gb_conv and variant == "dw"):
        # two-piece G from one-piece incoming gradients: +-1 (equal in adjacent column pairs) plus 2^-9 in the even columns
        # (dw: in random columns)
        bits = (np.arange(W) % 2 == 0) if name == "gb_a2w1" else rng.integers(0, 2, W).astype(bool)
        C = (bits * 2.0 ** -9).astype(np.float32)
    for s in range(n_seg):
        rows = end[s] - begin[s]
        r = slice(begin[s], end[s])
        if rows == 0:
            continue
        if name == "gb_a2w1":
            sg = np.repeat(_choice(rng, (-1, 1), (rows, W // 2)), 2, axis=1)
            G[r] = sg + C
            for o in range(nops):
                t = np.repeat(_choice(rng, (-1, 1), (k, W // 2)), 2, axis=1)
                t[:, 1::2] *= -1.0
                w[s, o] = t
        elif name == "gb_a1w2":
            Wc = min(W, 96)
            for o in range(nops):
                a, wc, _ = R.cancelling_probe(np.random.default_rng(900 + 7 * s), rows, Wc, k, 1)
                G[r, :Wc] = a  # (the same generator state for both operands: the same G)
                wc2 = R.cancelling_probe(np.random.default_rng(950 + 7 * s + o), 1, Wc, k, 1)[1]
                w[s, o][:, :Wc] = wc2.T
        elif variant == "dw":
            pa, pw = R.probe_spec(name)[:2]
            for o in range(nops):
                ins[o][r] = R.probe_values(rng, (rows, k), pa)
            if gb_conv:
                G[r] = _choice(rng, (-1, 1), (rows, W)) + C
            else:
                G[r] = R.probe_values(rng, (rows, W), pw)
            G[r, 96:] = 0.0
        else:  # din: G is the probe's left operand, W^T (width x k) its right one
            K = R.probe_spec(name)[2]
            for o in range(nops):
                a, wt = R.probe_operands(name, rows, W, k, 300 + 11 * s + o, nnz=K if K < W else None)
                if o == 0:
                    G[r] = a
                w[s, o] = wt.T
    piece_lsb = {1: 1.0, 2: 2.0 ** -9, 3: 2.0 ** -17}
    if name.startswith("gb_"):
        lsb = dict(g=2.0 ** -9 if name == "gb_a2w1" else 1.0, din=2.0 ** -9)
        lsb["dw"] = lsb["g"]
    elif variant == "dw":
        lsb = dict(dw=R.probe_spec(name)[3], g=piece_lsb[R.probe_spec(name)[1]])
        lsb["din"] = lsb["g"]
    else:
        lsb = dict(din=R.probe_spec(name)[3], g=piece_lsb[R.probe_spec(name)[0]])
        lsb["dw"] = lsb["g"]
    return G, C, ins, w, lsb


def build_bwd(c):
    """The numpy side of one backward case: float32 arrays holding bf16-exact values where the form stores bf16."""
    dense = c["block"] == "dense"
    W, nops, k, ld, store = c["width"], c["nops"], c["k"], c["ld"], c["store"]
    if dense:
        begin, end, n = [0], [c["rows"]], c["rows"] + 3
    else:
        begin, end, n = _bounds(c["sizes"])
    n_seg = len(begin)
    cov = _covered(begin, end, n)
    rng = np.random.default_rng(104729 * c["seed"] + 17 * k + ld + W + 3 * store)
    d = dict(c, begin=begin, end=end, n=n, n_seg=n_seg, covered=cov, dense=dense)
    rnd = (lambda a: R.bf16_round(a)) if c["kind"] == "normal" else (lambda a: a)
    coef = None
    d["lsb"] = dict(dw=0.25, din=0.25, g=0.25)
    if c["kind"] == "probe":
        G, C, ins, w, d["lsb"] = _bwd_probe_data(c, begin, end, n, rng)
        dy, gc = G - C, np.ones((n, W), np.float32)
        if dense or C.any():
            coef = np.concatenate([np.ones(W), np.zeros(W), C]).astype(np.float32)
        if dense:  # one molecule per row, nothing through the max part
            d["membership"], d["arg"] = np.arange(n, dtype=np.int32), np.full((n, W), -1, np.int32)
            d["g2"] = np.concatenate([dy, np.zeros((n, W), np.float32)], 1)
    else:
        normal = c["kind"] == "normal"
        if dense:
            d["membership"], d["g2"], d["arg"] = _readout(c["rows"], n, rng, c["kind"], W)
            dy = None
        else:
            dy = rng.standard_normal((n, W)).astype(np.float32) if normal else _choice(rng, (-1, 0, 1), (n, W))
            dy = rnd(dy) if store == 2 else dy
        gc = rng.standard_normal((n, W)).astype(np.float32) if normal else _choice(rng, (-.5, 0, .5, 1), (n, W))
        gc = rnd(gc) if store else gc
        ins = [rng.standard_normal((n, k)).astype(np.float32) if normal else _choice(rng, (-1, 0, 1), (n, k)) for _ in range(nops)]
        ins = [rnd(a) if (store or c["ib"]) else a for a in ins]
        w = rng.standard_normal((n_seg, nops, k, W)).astype(np.float32) if normal else _choice(rng, (-1, 0, 1), (n_seg, nops, k, W))
        if c["coef"]:
            if normal:
                coef = rng.standard_normal(3 * W).astype(np.float32)
            else:
                A, B, C = _choice(rng, (0, 1, 2, -1), W), _choice(rng, (0, .5, -.5), W), _choice(rng, (0, .25, -.25), W)
                A[0], B[1], C[1] = 0, 0, 0  # a column without dy, a column of A dy alone
                A[1] = 2
                coef = np.concatenate([A, B, C])
    d["coef"] = coef
    if dense:
        d["dy"], d["dy_mag"] = R.readout_dy_ref(d["g2"], d["arg"], d["membership"], W)
    else:
        d["dy"], d["dy_mag"] = dy, None
    d["gc"], d["ins"] = gc, ins
    wd = np.ascontiguousarray(w.transpose(0, 1, 3, 2)) if dense else w
    d["w"] = wd.reshape(-1)
    block = list(range(n_seg))
    if c["share"]:
        block[c["share"][1]] = c["share"][0]
    skips = (c["skip_rel"], c["skip_self"])
    d["w_off"] = [[-1 if s == skips[o] else (block[s] * nops + o) * k * W for s in range(n_seg)] for o in range(nops)]
    d["b_off"] = None if c["db"] is None else [-1 if (c["db"] == "skip" and s == 2) else block[s] * W for s in range(n_seg)]
    if c["kind"] == "int":
        d["dw0"] = (rng.integers(-8, 9, w.size) * 0.25).astype(np.float32)
        d["db0"] = None if c["db"] is None else (rng.integers(-8, 9, n_seg * W) * 0.25).astype(np.float32)
    else:
        d["dw0"] = np.zeros(w.size, np.float32)
        d["db0"] = None if c["db"] is None else np.zeros(n_seg * W, np.float32)
    return d


def bwd_ref(d):
    """block_bwd_ref of the case, plus ``stored``: the input gradients as the kernel stores them (rounded to bf16 when
    the gradient streams are bf16) and ``psums`` of those."""
    ref = R.block_bwd_ref(d["begin"], d["end"], d["w_off"], d["b_off"] or [-1] * d["n_seg"], d["dy"], d["gc"], d["coef"],
                          d["ins"], d["k"], d["w"], d["dw0"], d["db0"], d["width"], d["dense"], d["dy_mag"])
    stored = []
    for x in ref["din"]:
        y = x.copy()
        if d["store"] == 2:
            y[d["covered"]] = R.bf16_round(x[d["covered"]].astype(np.float32))
        stored.append(y)
    ref["stored"] = stored
    ref["psums"] = R.psums_ref(d["begin"], d["end"], stored, d["ins"], d["k"], not d["dense"])
    return ref


def _pad_rows(values, ld, covered, fill=np.nan):
    full = np.full((values.shape[0], ld), fill, np.float32)
    full[covered, :values.shape[1]] = values[covered]
    return full


def _launch_bwd(d, times=2, expect_launch=True):
    """``times`` launches with fresh outputs; [dict(dw, db, din: full matrices, psums)].  The launch counter moves by
    one per call."""
    from deepchem_amd import ops
    st, W, k, cov, pad = d["store"], d["width"], d["k"], d["covered"], d["pad"]
    bf = torch.bfloat16
    gc = _dev(_pad_rows(d["gc"], W + pad, cov), bf if st else None)
    ins = [_dev(_pad_rows(a, d["ld"], cov), bf if (st or d["ib"]) else None) for a in d["ins"]]
    coef, w = _dev(d["coef"]), _dev(d["w"])
    if d["dense"]:
        g2 = _dev(_pad_rows(d["g2"], 2 * W + pad, np.ones(d["g2"].shape[0], bool)))
        membership, arg = _dev(d["membership"]), _dev(d["arg"])
    else:
        dy = _dev(_pad_rows(d["dy"], W + pad, cov), bf if st == 2 else None)
    ldd = _up(k, 4) + pad
    got = []
    for _ in range(times):
        dw, db = _dev(d["dw0"]), _dev(d["db0"])
        douts = [torch.full((d["n"], ldd), SENTINEL, dtype=bf if st == 2 else torch.float32, device="cuda:0")
                 for _ in d["ins"]] if d["dgrad"] else [None, None]
        acc = _dev(R.fresh_acc(k, ACC_SENTINEL)) if d["psums"] else None
        before = ops.fused_bwd_launches()
        if d["dense"]:
            ops.fused_dense_bwd(d["begin"], d["end"], d["w_off"][0], d["b_off"], membership, g2[:, :2 * W], arg, gc[:, :W],
                                coef, ins[0][:, :k], w, dw, db, douts[0][:, :k], psums=acc, act_bf16=st)
        else:
            ops.fused_conv_bwd(d["begin"], d["end"], d["w_off"][0], d["w_off"][1], d["b_off"], dy[:, :W], gc[:, :W], coef,
                               ins[0][:, :k], ins[1][:, :k], w, dw, db, None if douts[0] is None else douts[0][:, :k],
                               None if douts[1] is None else douts[1][:, :k], psums=acc, act_bf16=st, in_bf16=d["ib"])
        assert ops.fused_bwd_launches() == before + 1, "the launch counter did not move by one"
        got.append(dict(dw=dw.cpu().numpy().astype(np.float64), db=None if db is None else db.cpu().numpy().astype(np.float64),
                        din=[_host(t) for t in douts if t is not None],
                        psums=None if acc is None else R.read_acc(acc.cpu().numpy(), k, ACC_SENTINEL)))
    return got


def din_full(d, values, ldd):
    """The matrix an input-gradient buffer must equal: ``values`` in columns [0, k) of the covered rows, the sentinel in
    the guard columns and in the rows outside every segment."""
    full = np.full((d["n"], ldd), SENTINEL, np.float64)
    full[d["covered"], :d["k"]] = values[d["covered"]]
    return full


def _check_bwd_exact(d, what, check_din=True):
    ref = bwd_ref(d)
    for i, g in enumerate(_launch_bwd(d)):
        bad = np.flatnonzero(g["dw"] != ref["dw"])
        assert bad.size == 0, "%s launch %d: %d elements of dW differ, first at %d: %r for %r" % (
            what, i, bad.size, bad[0], g["dw"][bad[0]], ref["dw"][bad[0]])
        if ref["db"] is not None:
            assert np.array_equal(g["db"], ref["db"]), "%s launch %d: db" % (what, i)
        for o, full in enumerate(g["din"]):
            want = din_full(d, ref["stored"][o], full.shape[1])
            if not check_din:
                want[d["covered"], :d["k"]] = full[d["covered"], :d["k"]]  # (guards and uncovered rows only)
            bad = np.argwhere(full != want)
            assert bad.size == 0, "%s launch %d: dIn[%d] differs in %d places, first at %s: %r for %r" % (
                what, i, o, len(bad), tuple(bad[0]), full[tuple(bad[0])], want[tuple(bad[0])])
        if g["psums"] is not None:
            assert np.array_equal(g["psums"], ref["psums"]), "%s launch %d: psums" % (what, i)


@pytest.mark.parametrize("name", list(BWD_INT))
def test_backward_exact(name):
    _check_bwd_exact(build_bwd(BWD_INT[name]), name)


@pytest.mark.parametrize("name", list(BWD_LONG))
def test_backward_exact_long_walk(name):
    """8 x 256 + 1 tiles with psums: some workgroup runs flush_psums in the middle of its walk."""
    _check_bwd_exact(build_bwd(BWD_LONG[name]), name)


@pytest.mark.parametrize("name", list(BWD_PROBE))
def test_backward_probe(name):
    """dw: the contraction runs over the rows of a segment (<= 48); din: over the columns of G.  A "dw" case whose input
    gradients are rounded to bf16 compares only dW and db (and the guards of dIn)."""
    c = BWD_PROBE[name]
    _check_bwd_exact(build_bwd(c), name, check_din=not (c["store"] == 2 and c["variant"] == "dw"))


def bwd_products(d):
    """(dW product, dIn product) in float32 by the rule of the module docstring: the sequential float32 chain for the
    forms that keep all six terms (and the IB form, whose one-piece In and three-piece G lose nothing), the emulated
    term subsets for the HB forms."""
    if d["store"]:
        return (lambda a, g: R.split_product_np(a, g, R.HB_DW_TERMS)), (lambda g, w: R.split_product_np(g, w, R.HB_DIN_TERMS))
    return (lambda a, g: R.seq32_product(a, g)), (lambda g, w: R.seq32_product(g, w))


def bwd_dy32(d):
    if not d["dense"]:
        return d["dy"].astype(np.float32)
    W, m = d["width"], d["membership"].astype(np.int64)
    hit = d["arg"][m] == np.arange(d["n"])[:, None]
    return (d["g2"][m, :W] + np.where(hit, d["g2"][m, W:], np.float32(0))).astype(np.float32)


def bwd_accuracy_bounds(d, ref):
    """{output: (e_ref, bound)} for dw, db and din."""
    dwp, dinp = bwd_products(d)
    dw32, din32 = R.block_bwd_f32(d["begin"], d["end"], d["w_off"], bwd_dy32(d), d["gc"], d["coef"], d["ins"], d["k"], d["w"],
                                  d["dw0"].size, d["width"], d["dense"], dwp, dinp)
    out = {}
    m = ref["S_dw"] > 0
    out["dw"] = float((np.abs(dw32.astype(np.float64) - ref["dw"])[m] / ref["S_dw"][m]).max() / R.U24)
    worst = 0.0
    for o in range(len(d["ins"])):
        m = ref["S_din"][o] > 0
        if m.any():
            worst = max(worst, float((np.abs(din32[o].astype(np.float64) - ref["din"][o])[m] / ref["S_din"][o][m]).max() / R.U24))
    out["din"] = worst
    if ref["db"] is not None:  # db: a float32 chain down the rows of every segment
        G32 = R.g_float32(bwd_dy32(d), d["gc"], d["coef"], d["width"])
        db32 = np.zeros(ref["db"].size)
        for s in range(d["n_seg"]):
            if d["b_off"][s] >= 0 and d["end"][s] > d["begin"][s]:
                r = slice(d["begin"][s], d["end"][s])
                db32[d["b_off"][s]:d["b_off"][s] + d["width"]] += R.seq32_product(np.ones((1, r.stop - r.start), np.float32), G32[r])[0]
        m = ref["S_db"] > 0
        out["db"] = float((np.abs(db32 - ref["db"])[m] / ref["S_db"][m]).max() / R.U24)
    return {key: (e, 2.0 * max(e, 1.0)) for key, e in out.items()}


@pytest.mark.parametrize("name", list(BWD_ACC))
def test_backward_accuracy(name):
    d = build_bwd(BWD_ACC[name])
    ref = bwd_ref(d)
    bounds = bwd_accuracy_bounds(d, ref)
    cov, k = d["covered"], d["k"]
    figures = []
    for g in _launch_bwd(d):
        m = ref["S_dw"] > 0
        figures.append(("dw", float((np.abs(g["dw"] - ref["dw"])[m] / ref["S_dw"][m]).max() / R.U24)) + bounds["dw"])
        assert np.all(g["dw"][~m] == 0), name + ": a dW block without rows or term was written"
        if ref["db"] is not None:
            mb = ref["S_db"] > 0
            e_db = float((np.abs(g["db"] - ref["db"])[mb] / ref["S_db"][mb]).max() / R.U24)
            figures.append(("db", e_db) + bounds["db"])
        for o, full in enumerate(g["din"]):
            assert np.all(full[~cov] == SENTINEL), name + ": rows outside every segment were written"
            S, r64 = ref["S_din"][o], ref["din"][o]
            m = S > 0
            err = np.abs(full[:, :k] - np.where(m, r64, 0.0))
            e_ref, bound = bounds["din"]
            if d["store"] == 2:
                half = 0.5 * R.ulp(np.where(m, r64, 1.0), bf16=True)
                figures.append(("din%d beyond half a bf16 ulp" % o, float(((err - half).clip(0)[m] / S[m]).max() / R.U24), e_ref, bound))
                elem = 2.0 * half + bound * S * R.U24
            else:
                figures.append(("din%d" % o, float((err[m] / S[m]).max() / R.U24), e_ref, bound))
                elem = bound * S * R.U24
            assert np.all(full[cov, :k][~m[cov]] == 0), name + ": dIn of an absent term is not zero"
        if g["psums"] is not None:
            _psums_check(name, d, g, ref)
    for what, e, e_ref, bound in figures:
        print("backward accuracy %s %s: e = %.2f, e_ref = %.2f, bound %.2f" % (name, what, e, e_ref, bound))
    for what, e, e_ref, bound in figures:
        assert e <= bound, "%s %s: e = %.2f roundings of S, bound %.2f (e_ref = %.2f)" % (name, what, e, bound, e_ref)


def _psums_check(name, d, g, ref):
    """psums against the float64 sums of the input gradients the kernel stored (the header: "the sums describe the
    stored values"): what differs is the summation -- fp32 partials of 8 tiles x 2 rows per thread (conv: both operands
    into one partial), then float64.  Bound 2 max(e_seq, 1) roundings of the sum of absolute values, e_seq from a
    float32 chain over 32 reference values at a time."""
    k, conv = d["k"], not d["dense"]
    got = [np.where(d["covered"][:, None], x[:, :k], 0.0) for x in g["din"]]
    own = R.psums_ref(d["begin"], d["end"], got, d["ins"], k, conv)
    mag = R.psums_mag(d["begin"], d["end"], got, d["ins"], k, conv)
    refs = [np.where(d["covered"][:, None], x, 0.0) for x in ref["stored"]]
    seg = np.zeros(d["n"])
    for s in range(d["n_seg"]):
        seg[d["begin"][s]:d["end"][s]] = s
    for m in range(2):
        seq = np.zeros(k)
        for o, (x, a) in enumerate(zip(refs, d["ins"])):
            a0 = np.where(d["covered"][:, None], a[:, :k], 0.0)
            seq += R.seq32_colsum(x, 32, weights=seg if (conv and o == 0) else None) if m == 0 else R.seq32_colsum(x, 32, other=a0)
        rmag = R.psums_mag(d["begin"], d["end"], refs, d["ins"], k, conv)[m]
        ok = rmag > 0
        e_seq = float((np.abs(seq - ref["psums"][m])[ok] / rmag[ok]).max() / R.U24)
        bound = 2.0 * max(e_seq, 1.0)
        e = float((np.abs(g["psums"][m] - own[m])[mag[m] > 0] / mag[m][mag[m] > 0]).max() / R.U24)
        print("backward accuracy %s psums[%d]: e = %.2f, e_seq32 = %.2f, bound %.2f" % (name, m, e, e_seq, bound))
        assert e <= bound, "%s psums[%d]: e = %.2f, bound %.2f" % (name, m, e, bound)


def _bwd_refusal_cases():
    return {
        "k32": _b("b2_f", k=32), "k97": _b("b3_f", k=97, ld=100), "k35_dgrad": _b("b2d_f", k=35, ld=36),
        "k68_dgrad": _b("b2d_f", k=68), "ib_k64": _b("ib", k=64), "ib_with_dout": dict(_b("b3_f", k=76), ib=1, dgrad=True),
        "dense_no_coef": _b("bd_f", coef=False), "dense_k33": _b("bd_f", k=33, ld=36), "dense_k68": _b("bd_f", k=68),
        "dense_begin": dict(_b("bd_f"), begin0=4),
    }


@pytest.mark.parametrize("name", ["exact_mode_conv", "exact_mode_dense", "fused_off_conv"] + list(_bwd_refusal_cases()))
def test_backward_refusals(name):
    """GCMI_ERR_UNSUPPORTED with an error text; dW, db, dIn and psums keep what they held and the launch counter stays."""
    import deepchem_amd as dc
    from deepchem_amd import _lib, ops
    special = name.startswith("exact_mode") or name.startswith("fused_off")
    c = _b("bd_f" if name.endswith("dense") else "b2d_f") if special else _bwd_refusal_cases()[name]
    d = build_bwd(dict(c, sizes=ACC_SEGS, rows=302))
    if c.get("begin0"):
        d["begin"] = [c["begin0"]]
    W, k, cov = d["width"], d["k"], d["covered"]
    bf = torch.bfloat16
    gc = _dev(_pad_rows(d["gc"], W, cov))
    ins = [_dev(_pad_rows(a, d["ld"], cov), bf if d["ib"] else None) for a in d["ins"]]
    dw, db = _dev(d["dw0"]), _dev(d["db0"])
    douts = [torch.full((d["n"], _up(k, 4)), SENTINEL, dtype=torch.float32, device="cuda:0") for _ in d["ins"]] if d["dgrad"] else [None, None]
    acc = _dev(R.fresh_acc(k, ACC_SENTINEL)) if d["dgrad"] else None
    before = ops.fused_bwd_launches()
    try:
        if name.startswith("exact_mode"):
            dc.set_gemm_mode("exact")
        if name.startswith("fused_off"):
            _lib.call("gcmi_set_option", _lib.GCMI_OPT_FUSED_BWD, 0)
        if d["dense"]:
            call = lambda: ops.fused_dense_bwd(d["begin"], d["end"], d["w_off"][0], d["b_off"], _dev(d["membership"]), _dev(d["g2"]),  # noqa: E731
                                               _dev(d["arg"]), gc, _dev(d["coef"]), ins[0][:, :k], _dev(d["w"]), dw, db,
                                               douts[0][:, :k], psums=acc)
        else:
            call = lambda: ops.fused_conv_bwd(d["begin"], d["end"], d["w_off"][0], d["w_off"][1], d["b_off"],  # noqa: E731
                                              _dev(_pad_rows(d["dy"], W, cov)), gc, _dev(d["coef"]), ins[0][:, :k], ins[1][:, :k],
                                              _dev(d["w"]), dw, db, None if douts[0] is None else douts[0][:, :k],
                                              None if douts[1] is None else douts[1][:, :k], psums=acc, in_bf16=d["ib"])
        assert _refused(call), name + ": not refused"
    finally:
        dc.set_gemm_mode("fast")
        _lib.call("gcmi_set_option", _lib.GCMI_OPT_FUSED_BWD, 1)
    torch.cuda.synchronize()
    assert ops.fused_bwd_launches() == before, name + ": the launch counter moved"
    assert torch.equal(dw, _dev(d["dw0"])) and torch.equal(db, _dev(d["db0"])), name + ": a refusal wrote dW / db"
    for t in douts:
        assert t is None or bool((t == SENTINEL).all()), name + ": a refusal wrote dIn"
    assert acc is None or torch.equal(acc, _dev(R.fresh_acc(k, ACC_SENTINEL))), name + ": a refusal wrote psums"
