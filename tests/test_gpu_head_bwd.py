"""The per-molecule head backward kernels (csrc/head_bwd.hip: head_bwd_kernel; head_prep_kernel's backward image +
head_bwd_wide_kernel + head_wgrad_wide_kernel), which the suite reached only through whole model steps with every row
carrying a loss, weights always present and ldfp = ldg2 = 256, pinned operation by operation through
``ops.head_backward`` (gcmi_head_backward: no other kernel behind it) against the float64 restatement
``tests.edge_refs.head_bwd_ref``.  Inputs are generated directly -- fingerprint, logits, labels, weights, runs, arg,
rawsum, mean, invstd -- no graph is collated and no model step runs.

Guards, in every case.  g2 sits in a buffer with two guard rows and guard columns (ldg2 = 264), dW, db, the 16 loss
replicas and dl_scratch between sentinel words, the BatchNorm accumulator as [sentinel 2F][start 32 x 2F][sentinel]
(edge_refs.fresh_acc): the sentinels must survive.  Every case asserts the route it claims.  What the kernels must not
use is NaN: logits, labels and weights of the rows >= n_rows, the fingerprint's guard columns (ldfp = 257 narrow, 260
wide), rawsum's max half where arg < 0, and dl_scratch / img_scratch before the call (what a forward left there must
not matter; on route 0 both must still be all NaN afterwards).  The fingerprint rows of PADDING molecules stay finite:
the kernels read them and multiply them by a zero gradient.

Which kernel a case reaches (head_bwd_fused):
  outputs <= 32            head_bwd_kernel, 256 threads, 32 molecules a round, grid min(768, ceil(n_mols / 32)), molecule
                           ranges b n_mols / grid; sums into replica block % 32, loss into replica 0        route 0
  33..256 outputs          head_prep_kernel (W split once; the backward image is read), head_bwd_wide_kernel (512
  (GCMI_HEAD_WIDE_MIN=1:   threads, one workgroup per 32 molecules; L2 and two classes: the unrolled rounds of 128
   1..256)                 tasks with the one-exponential softmax; other class counts: the general loop), then
                           head_wgrad_wide_kernel, grid (slabs, ceil(outputs / 64), 4), slabs of a multiple of 32
                           molecules, at least 64                                                         route 1

Three kinds of case, as in tests/test_gpu_product_edges.py:
  int   L2 with small-integer logits - labels, fp in {0, +-0.5, +-1}, W in {-1, -0.5, 0, 0.5, 1}, dyadic mean / invstd /
        rawsum, weights None where n_rows n_tasks is a power of two and otherwise count x {0, 0.5, 1} (the float32
        product count x float32(1 / count) rounds to exactly 1 for every count used, which tests/test_head_refs_host.py
        checks, so d logits are powers of two whatever the count); on the wide route also two-class cross-entropy with
        equal logits per task (p = 0.5 exactly in the one-exponential form), one-hot and all-zero label rows.  Two
        launches; g2, dW, db, dl_scratch, the summed loss replicas and the summed sums replicas must be
        np.array_equal to float64.  (The cross-entropy LOSS of those cases is (sum of w over the one-hot rows) x
        logf(2): one device logarithm, held to (1 + T) 2^-24 of its value instead.)
  acc   standard-normal logits and W, fp = tanh(normal).  e = max |got - ref64| / S in units of 2^-24, S = the sum of
        the absolute values of the terms (floored at 2^-102: below it float32 leaves its normal range); bound
        2 max(e_ref, 1) + T with e_ref of edge_refs.head_bwd_f32 on the same inputs and T the allowance for the device's
        expf / logf, which are not numpy's.  No device-math accuracy table ships with the ROCm toolchain, so T = 4 is an
        ASSUMPTION (the usual 1..4 ulp the OpenCL / HIP documentation gives for these functions).  T is granted to the loss, to d
        logits and to everything linear in them; L2 cases call no such function and get T = 0.  On the wide route g2, dW
        and db are ALSO held to float64 computed from the d logits the kernel returned in dl_scratch, bound
        2 max(e_ref, 1) without T: a loss error and a product error show separately.  The BatchNorm sums are fp64 on the
        device: e in units of 2^-53 of S against the extended-precision sums of the g2 THE KERNEL RETURNED (float32 g2
        feeds them; g2 is checked on its own), bound 2 max(e_ref, 1) with e_ref of a sequential float64 sum in reversed
        order.
  sat   accuracy cases with logit gaps of +-30 and +-100 (p underflows, 1 + e^d rounds to 1), exactly equal logits, the
        larger logit in either class position (both branches of the wide two-class ``first`` select) and label rows that
        are not one-hot (ysum 0, 0.3 and 2).

Measured on an MI355X (gfx950, the default -O3 build), per group of cases; the bound is per case.  Units: 2^-24 of S
(2^-53 for the sums).
Each entry: largest e / largest e_ref (largest e / bound of any case of the row).
  route 0, L2            loss 0.12/0.12 (0.06)  g2 4.57/4.57 (0.50)  dW 2.58/2.64 (0.62)  db 0.77/1.20 (0.39)  sums 1.74/1.74 (0.50)
  route 0, CE            loss 0.36/0.41 (0.06)  g2 5.07/5.07 (0.36)  dW 4.28/4.50 (0.33)  db 1.35/1.97 (0.23)  sums 1.71/1.16 (0.85)
  route 0, CE saturated  loss 0.12/0.12 (0.02)  g2 2.02/2.02 (0.25)  dW 3.77/3.77 (0.33)  db 0.64/0.64 (0.11)
  route 1, L2            loss 0.48/0.48 (0.24)  dl 3.09/3.09 (0.50)  g2 4.12/4.12 (0.50)  dW 3.16/2.68 (0.60)  db 1.63/1.63 (0.50)
                         from the returned dl: g2 6.84/6.84 (0.50)  dW 3.22/3.53 (0.84)  db 1.40/2.23 (0.39);  sums 1.40/1.70 (0.50)
  route 1, CE            loss 0.26/0.11 (0.04)  dl 9.19/8.78 (0.47)  g2 2.39/2.39 (0.27)  dW 1.94/1.90 (0.26)  db 0.96/1.29 (0.16)
                         from the returned dl: g2 3.60/3.54 (0.55)  dW 2.71/3.29 (0.50)  db 1.59/2.41 (0.50);  sums 0.60/1.82 (0.28)
  route 1, CE saturated  loss 0.24/0.24 (0.04)  dl 23.92/22.90 (0.48)  g2 2.60/2.60 (0.28)  dW 2.39/2.39 (0.27)  db 0.73/0.99 (0.12)
                         from the returned dl: g2 3.63/3.63 (0.50)  dW 3.88/3.88 (0.50)  db 1.32/1.51 (0.46)
  GCMI_HEAD_WIDE_MIN=1   loss 0.29/0.10 (0.05)  dl 6.15/5.21 (0.50)  g2 2.64/2.56 (0.50)  dW 2.63/2.37 (0.37)  db 1.24/1.41 (0.18)
                         from the returned dl: g2 2.83/2.83 (0.59)  dW 2.94/2.94 (0.50)  db 1.33/2.04 (0.56);  sums 0.88/1.84 (0.32)
(The d logits of the saturated cases: float32 rounds a logit difference of 30 to 2^-20, which is 16 units of the small
probability; the reference chain does the same.)

Found while measuring.  With e_ref from one rounding per 16-wide product step (split_product_np as tests/
test_gpu_product_edges.py uses it) the 256-output, 2 081-molecule L2 case gave g2-from-returned-dl e = 6.84 against
e_ref 3.33, bound 6.65; six other cases sat at 1.0..1.8 e_ref.  The kernel is not at fault: emulating its g2 from the d
logits it returned reproduces 86 % of 76 000 outputs bit for bit (1.2 ulp apart on average) when the 16 products of
a v_mfma_f32_32x32x16_bf16 enter the accumulator as TWO exact sums of 8 with a rounding after each, and 15 % (53 ulp)
with one rounding per step; sums of 4, 2, 1 and truncation fit worse.  head_bwd_f32 therefore states the instruction's
two roundings (edge_refs.MFMA_GROUP = 8); the same case then measures e = e_ref = 6.84.
"""
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest
import torch

from tests import edge_refs as R

pytestmark = pytest.mark.gpu

SENTINEL = -12288.0
ACC_SENTINEL = -7.5
T_DEVICE_MATH = 4.0  # an assumption: see the module docstring
U53 = 2.0 ** -53
F = R.HEAD_K // 2


def C(data, kind, tasks, classes, mols, rows=None, weights=False, db=True, sums=None, empties=(), starts=False, wide=None,
      ldfp=None, ldg2=264):
    """One case.  kind 0 cross-entropy / 1 L2; rows: molecules with a loss (None: all); weights: False = NULL, True =
    present with zeros; sums: n_deg or None; empties: molecules without atoms; starts: dW, db, loss and sums start
    non-zero; wide: the route claimed (None: by the output count)."""
    tc = tasks * (classes if kind == 0 else 1)
    wide = tc > 32 if wide is None else wide
    return dict(data=data, kind=kind, tasks=tasks, classes=classes if kind == 0 else 1, mols=mols,
                rows=mols if rows is None else rows, weights=weights, db=db, sums=sums, empties=tuple(empties),
                starts=starts, wide=wide, ldfp=(260 if wide else 257) if ldfp is None else ldfp, ldg2=ldg2, tc=tc)


def case_id(c):
    s = "%s-%s-%dx%d-m%d-r%d" % (c["data"], "ce" if c["kind"] == 0 else "l2", c["tasks"], c["classes"], c["mols"], c["rows"])
    s += ("-w" if c["weights"] else "") + ("" if c["db"] else "-nodb") + ("-s%d" % c["sums"] if c["sums"] else "")
    return s + ("-e" if c["empties"] else "") + ("-st" if c["starts"] else "") + ("-wide" if c["wide"] else "-narrow")


CAP = 768 * 32
NARROW = [
    # ---- exact integer cases: every mechanism of head_bwd_kernel
    C("int", 1, 1, 1, 1, sums=11),                                    # Delaney's shape, one molecule
    C("int", 1, 7, 1, 31, weights=True, sums=5, empties=(0, 14, 30)),  # a partial round; empty first, middle, last
    C("int", 1, 31, 1, 32, rows=21, weights=True, db=False),          # a whole round, padding molecules, no db
    C("int", 1, 32, 1, 33, rows=1, sums=1, starts=True),              # two workgroups of 16 and 17; one row with a loss
    C("int", 1, 32, 1, 75, rows=64, sums=11, empties=(0, 37, 74)),    # three workgroups of 25
    C("int", 1, 32, 1, CAP + 1, rows=16384, sums=11, empties=(0, 31, CAP)),  # the grid cap: one workgroup's second round
    C("int", 1, 7, 1, CAP + 33, rows=CAP + 22, weights=True, sums=5, starts=True),  # ... of 33 workgroups
    # ---- accuracy: every output shape
    C("acc", 1, 1, 1, 75, sums=11, empties=(3,)),
    C("acc", 1, 7, 1, 33, rows=22, weights=True, sums=5, starts=True),
    C("acc", 1, 31, 1, 31, db=False),
    C("acc", 1, 32, 1, 1, sums=1),
    C("acc", 0, 1, 2, 32, sums=11, empties=(31,)),
    C("acc", 0, 12, 2, 75, rows=64, weights=True, sums=11, empties=(0, 40, 74)),
    C("acc", 0, 16, 2, 33, rows=1),
    C("acc", 0, 5, 3, 31, weights=True),
    C("acc", 0, 10, 3, 75, sums=5),
    C("acc", 0, 8, 4, 33, rows=22, sums=11, starts=True),            # exactly kHT = 32 outputs
    C("acc", 0, 1, 32, 32, db=False),
    C("acc", 0, 1, 1, 75, weights=True),                              # one class: p = 1, a zero gradient from cancellation
    C("acc", 1, 32, 1, CAP + 1, weights=True, sums=11, empties=(5, CAP)),
    C("acc", 0, 16, 2, CAP + 33, rows=CAP + 22, sums=5),
    C("sat", 0, 12, 2, 33, weights=True),
    C("sat", 0, 5, 3, 32, rows=21),
]
WIDE = [
    # ---- exact integer cases: L2
    C("int", 1, 33, 1, 1, weights=True, sums=11),                     # the smallest wide shape, TCP 48
    C("int", 1, 49, 1, 31, rows=21, weights=True, db=False, sums=5, empties=(0, 15, 30)),
    C("int", 1, 64, 1, 32, sums=11),
    C("int", 1, 65, 1, 33, rows=1, weights=True),                     # a second 64-block of dW with one live row
    C("int", 1, 129, 1, 63, rows=62, weights=True, sums=1, empties=(31, 32)),  # one lane of the second loss round
    C("int", 1, 200, 1, 64, rows=53, weights=True),
    C("int", 1, 256, 1, 65, rows=64, sums=11, starts=True),           # one slab with a tail of one molecule
    C("int", 1, 256, 1, 97, rows=96, weights=True, db=False, sums=5),          # two slabs of 64; the second: a round and a tail of 1
    C("int", 1, 256, 1, 2081, rows=2048, sums=11, empties=(0, 1000, 2080)),  # 22 slabs, tail 65; 66 workgroups
    # ---- exact integer cases: two classes, equal logits
    C("int", 0, 17, 2, 2081, rows=2070, weights=True, sums=5, starts=True),  # 34 outputs padded to 48; 33 slabs of 64
    C("int", 0, 24, 2, 97, weights=True),
    C("int", 0, 128, 2, 65, rows=64, sums=11, empties=(64,)),
    # ---- accuracy
    C("acc", 1, 33, 1, 33, rows=22, weights=True, sums=11, starts=True),
    C("acc", 1, 49, 1, 1),
    C("acc", 1, 64, 1, 31, db=False, sums=5, empties=(0, 30)),
    C("acc", 1, 65, 1, 97, weights=True),
    C("acc", 1, 129, 1, 65, rows=1, sums=1),
    C("acc", 1, 200, 1, 63, weights=True, sums=11),
    C("acc", 1, 256, 1, 2081, rows=2070, weights=True, sums=11, empties=(7, 2080)),
    C("acc", 0, 17, 2, 64, sums=5),
    C("acc", 0, 24, 2, 32, rows=21, weights=True, db=False),
    C("acc", 0, 128, 2, 97, weights=True, sums=11, empties=(96,)),
    C("acc", 0, 11, 3, 65, weights=True, sums=11),                    # the general loop at the smallest wide size
    C("acc", 0, 85, 3, 33, rows=22),
    C("acc", 0, 64, 4, 63, sums=5, starts=True),
    C("acc", 0, 17, 2, 2081, weights=True, sums=11),
    C("sat", 0, 24, 2, 33, weights=True),
    C("sat", 0, 128, 2, 32, rows=21),
    C("sat", 0, 11, 3, 31, weights=True),
]
# GCMI_HEAD_WIDE_MIN=1: the wide pair at 1, 2, 15, 16, 17 and 32 outputs (TCP 16 or 32, one or two k-steps, most of the
# image padding)
SWITCHED = [
    C("int", 1, 1, 1, 33, rows=32, sums=11, wide=True),
    C("int", 1, 2, 1, 65, rows=64, sums=5, wide=True),
    C("int", 1, 15, 1, 31, weights=True, wide=True),
    C("int", 0, 8, 2, 64, sums=11, wide=True),
    C("int", 1, 17, 1, 97, weights=True, sums=1, empties=(96,), wide=True),
    C("int", 1, 32, 1, 32, db=False, wide=True),
    C("acc", 0, 1, 1, 33, weights=True, wide=True),
    C("acc", 0, 1, 2, 65, sums=11, wide=True),
    C("acc", 0, 5, 3, 31, weights=True, sums=5, wide=True),
    C("acc", 0, 8, 2, 64, rows=53, wide=True),
    C("acc", 1, 17, 1, 97, sums=11, wide=True),
    C("acc", 0, 8, 4, 33, weights=True, sums=1, wide=True),
    C("sat", 0, 1, 2, 32, wide=True),
]


# ================================================================================================ inputs
def _pow2(n):
    return n & (n - 1) == 0


def _logits_labels(c, rng):
    """float32 logits and labels of all n_mols rows (the caller NaNs the padding rows) and, for the integer kind, the
    scale of the weights."""
    kind, data = c["kind"], c["data"]
    shape = (c["mols"], c["tasks"]) + ((c["classes"],) if kind == 0 else ())
    if data == "int" and kind == 1:
        y = rng.integers(-3, 4, shape)
        return (y + rng.choice(np.array([-2, -1, 0, 1, 2]), shape)).astype(np.float32), y.astype(np.float32)
    if data == "int":  # two classes, equal logits; label rows [1, 0], [0, 1], [0, 0]
        assert c["classes"] == 2
        x = np.repeat(rng.integers(-3, 4, shape[:2])[..., None], 2, -1)
        cls = rng.integers(0, 3, shape[:2])
        return x.astype(np.float32), np.stack([cls == 0, cls == 1], -1).astype(np.float32)
    if kind == 1:
        return rng.standard_normal(shape).astype(np.float32), rng.standard_normal(shape).astype(np.float32)
    x = rng.standard_normal(shape)
    nc = c["classes"]
    hot = np.eye(nc)[rng.integers(0, nc, shape[:2])]
    if data == "acc":
        return x.astype(np.float32), hot.astype(np.float32)
    # saturation: one class of every item moved by a gap (its position decides the branch of the two-class select)
    gap = rng.choice(np.array([30.0, -30.0, 100.0, -100.0, 0.0, 0.0]), shape[:2])
    x = np.repeat(x[..., :1], nc, -1)  # exactly equal logits to start from
    pos = rng.integers(0, nc, shape[:2])
    np.put_along_axis(x, pos[..., None], np.take_along_axis(x, pos[..., None], -1) + gap[..., None], -1)
    jitter = rng.integers(0, 2, shape[:2]).astype(bool) & (gap != 0.0)  # half of the moved items: unequal others too
    x = np.where(jitter[..., None], x + 0.25 * rng.standard_normal(shape), x)
    style = rng.integers(0, 4, shape[:2])  # one-hot, all zero (ysum 0), 0.3 in one place, two ones (ysum 2)
    y = hot.copy()
    y[style == 1] = 0.0
    y[style == 2] *= 0.3
    y[style == 3] = np.maximum(hot, np.roll(hot, 1, -1))[style == 3]
    return x.astype(np.float32), y.astype(np.float32)


def build(c):
    """Every operand of one case as numpy arrays, the float64 reference with the starts folded in, and the buffers'
    initial contents."""
    rng = np.random.default_rng(zlib.crc32(case_id(c).encode()))
    f32 = np.float32
    kind, mols, rows, tasks, tc, data = c["kind"], c["mols"], c["rows"], c["tasks"], c["tc"], c["data"]
    integer = data == "int"
    d = dict(c=c)
    x, y = _logits_labels(c, rng)
    count = rows * tasks
    if not c["weights"]:
        assert not integer or _pow2(count), "integer data without weights needs a power-of-two count"
        w = None
    elif integer:
        w = (count * rng.choice(np.array([0.0, 0.5, 1.0]), (mols, tasks))).astype(f32)
    else:
        w = ((0.5 + rng.random((mols, tasks))) * (rng.random((mols, tasks)) < 0.75)).astype(f32)
    x[rows:], y[rows:] = np.nan, np.nan
    if w is not None:
        w[rows:] = np.nan
    d.update(logits=x, labels=y, weights=w)
    fp = np.full((mols, c["ldfp"]), np.nan, f32)
    if integer:
        fp[:, :256] = rng.choice(np.array([0.0, 0.5, -0.5, 1.0, -1.0]), (mols, 256))
        W = rng.choice(np.array([-1.0, -0.5, 0.0, 0.5, 1.0]), (tc, 256)).astype(f32)
    else:
        fp[:, :256] = np.tanh(rng.standard_normal((mols, 256)))
        W = rng.standard_normal((tc, 256)).astype(f32)
    d.update(fp=fp, w=W)
    si = None
    if c["sums"]:
        n_deg = c["sums"]
        length = rng.integers(0, 4, (mols, n_deg))
        length[:, rng.integers(0, n_deg)] += 1  # no accidental empty molecule
        length[list(c["empties"])] = 0
        begin = rng.integers(0, 1000, (mols, n_deg))
        runs = np.stack([begin, begin + length], -1).astype(np.int32)
        arg = rng.integers(0, 1 << 20, (mols, F)).astype(np.int32)
        arg[list(c["empties"])] = -1
        if integer:
            rawsum = (rng.integers(-16, 17, (mols, 256)) / 4.0).astype(f32)
            mean, invstd = (rng.integers(-8, 9, F) / 4.0).astype(f32), rng.choice(np.array([0.25, 0.5, 1.0, 2.0]), F).astype(f32)
        else:
            rawsum = (rng.standard_normal((mols, 256)) * 3.0).astype(f32)
            mean, invstd = rng.standard_normal(F).astype(f32), (0.5 + rng.random(F)).astype(f32)
        rawsum[:, F:][arg < 0] = np.nan
        si = dict(runs=runs, arg=arg, rawsum=rawsum, mean=mean, invstd=invstd)
    else:
        assert not c["empties"]
    d["si"] = si
    if c["starts"]:
        d["dw0"] = rng.integers(-4, 5, (tc, 256)).astype(f32) if integer else rng.standard_normal((tc, 256)).astype(f32)
        d["db0"] = rng.integers(-4, 5, tc).astype(f32) if integer else rng.standard_normal(tc).astype(f32)
        d["loss0"] = rng.integers(-4, 5, R.LOSS_REPLICAS).astype(np.float64)
        d["sums0"] = rng.integers(-4, 5, (R.BN_REPLICAS, 2, F)).astype(np.float64)
    else:
        d["dw0"], d["db0"] = np.zeros((tc, 256), f32), np.zeros(tc, f32)
        d["loss0"], d["sums0"] = np.zeros(R.LOSS_REPLICAS), np.zeros((R.BN_REPLICAS, 2, F))
    ref = R.head_bwd_ref(kind, x, y, w, rows, fp[:, :256], W, si)
    ref["dw"], ref["S_dw"] = ref["dw"] + d["dw0"], ref["S_dw"] + np.abs(d["dw0"])
    ref["db"], ref["S_db"] = ref["db"] + d["db0"], ref["S_db"] + np.abs(d["db0"])
    ref["loss"], ref["S_loss"] = ref["loss"] + d["loss0"].sum(), ref["S_loss"] + np.abs(d["loss0"]).sum()
    d["ref"] = ref
    return d


def exactness_failures(d):
    """What has to hold for an integer case to be exact on any kernel that computes the right thing in any order: every
    d logit a power of two (or zero) that float32 arithmetic reproduces (count x float32(1 / count) == 1), every operand
    of the products one bf16 piece, every partial sum of dfp, dW and db in any order a float32 number, g2 = dfp x
    {0, 0.75, 1} a float32 number, the loss a multiple of 0.5 below 2^52 (L2), the sums exact in float64 in any order.  Returns
    the list of what does not hold."""
    c, ref = d["c"], d["ref"]
    bad = []
    fp, W, rows = d["fp"][:, :256], d["w"], c["rows"]
    dl = ref["dl"]
    nz = np.abs(dl[dl != 0])
    if nz.size == 0:
        return ["no gradient at all"]
    if not np.all(np.log2(nz) == np.round(np.log2(nz))):
        bad.append("a d logit is no power of two")
    lsb = float(nz.min())
    for wide in ((False, True) if c["kind"] == 1 else (True,)):  # (p = 0.5 exactly in the one-exponential form only)
        loss32, dl32 = R.head_dl_f32(c["kind"], d["logits"], d["labels"], d["weights"], rows, wide)
        if not np.array_equal(dl32.astype(np.float64), dl[:rows]):
            bad.append("float32 d logits differ from float64 (wide=%s)" % wide)
        if c["kind"] == 1 and loss32 + d["loss0"].sum() != ref["loss"]:
            bad.append("float32 loss terms differ from float64")
    for name, v in (("dl", dl.astype(np.float32)), ("fp", fp), ("w", W)):
        if not np.array_equal(R.bf16_round(v), v):
            bad.append(name + " is not one bf16 piece")
    a = np.abs(dl)
    if not (R.is_multiple(W, 0.5) and R.is_multiple(fp, 0.5) and R.is_multiple(d["dw0"], 1.0) and R.is_multiple(d["db0"], 1.0)):
        bad.append("an operand is no multiple of 0.5 / a start no integer")
    if not R.any_order_exact(a @ np.abs(W), lsb / 2):
        bad.append("dfp")
    if not (R.is_multiple(ref["g2"], lsb / 8) and R.any_order_exact(np.abs(ref["g2"]), lsb / 8)):
        bad.append("g2")
    if not R.any_order_exact(a.T @ np.abs(fp) + np.abs(d["dw0"]), min(lsb / 2, 1.0)):
        bad.append("dW")
    if not R.any_order_exact(a.sum(0) + np.abs(d["db0"]), min(lsb, 1.0)):
        bad.append("db")
    if c["kind"] == 1 and not (R.is_multiple(ref["loss"], 0.5) and ref["S_loss"] < 2.0 ** 52):
        bad.append("loss")
    if d["si"] is not None:
        sums, S = ref["sums"], ref["S_sums"]
        lsb_s = lsb / 8 / 16  # g2 times multiples of 1/4 times multiples of 1/4
        if not (float(S.max()) + 4.0 * R.BN_REPLICAS < 2.0 ** 53 * lsb_s and R.is_multiple(sums.astype(np.float64), lsb_s) and
                np.array_equal(sums.astype(np.float64), R.head_sums_seq64(ref["g2"], d["si"])) and
                np.array_equal(sums.astype(np.float64), R.head_sums_seq64(ref["g2"], d["si"], reverse=False))):
            bad.append("sums")
    return bad


# ================================================================================================ launch
def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _guarded(values, pad=64):
    """[pad sentinels][values][pad sentinels] on the device, and the view of the middle."""
    v = np.asarray(values)
    buf = np.full(v.size + 2 * pad, SENTINEL, v.dtype)
    buf[pad:pad + v.size] = v.reshape(-1)
    t = _dev(buf)
    return t, t[pad:pad + v.size]


def _buffers(d):
    """Fresh device buffers of one launch."""
    from deepchem_amd import ops
    c = d["c"]
    mols, tc = c["mols"], c["tc"]
    b = dict(g2=torch.full((mols + 2, c["ldg2"]), SENTINEL, dtype=torch.float32, device="cuda:0"))
    b["dw_all"], b["dw"] = _guarded(d["dw0"])
    b["db_all"], b["db"] = _guarded(d["db0"]) if c["db"] else (None, None)
    b["loss_all"], b["loss"] = _guarded(d["loss0"], pad=8)
    b["dl_all"], b["dl"] = _guarded(np.full(mols * tc, np.nan, np.float32))
    b["img"] = torch.full((ops.task_head_scratch_floats(),), float("nan"), dtype=torch.float32, device="cuda:0")
    if d["si"] is not None:
        acc = R.fresh_acc(F, ACC_SENTINEL)
        acc[2 * F:2 * F * (1 + R.BN_REPLICAS)] = d["sums0"].reshape(-1)
        b["sums"] = _dev(acc)
    else:
        b["sums"] = None
    return b


def _call(d, b, ins, **override):
    from deepchem_amd import ops
    c = d["c"]
    a = dict(kind=c["kind"], logits=ins["logits"], labels=ins["labels"], weights=ins["weights"], n_rows=c["rows"],
             n_tasks=c["tasks"], n_classes=c["classes"], fp=ins["fp"][:, :256], w=ins["w"], dw=b["dw"], db=b["db"],
             g2=b["g2"][1:1 + c["mols"], :256], loss_acc=b["loss"], sums=b["sums"], dl_scratch=b["dl"], img_scratch=b["img"])
    if d["si"] is not None:
        a.update(runs=ins["runs"], arg=ins["arg"], rawsum=ins["rawsum"], mean=ins["mean"], invstd=ins["invstd"])
    a.update(override)
    return ops.head_backward(**a)


def _inputs(d):
    ins = {k: _dev(d[k]) for k in ("logits", "labels", "weights", "fp", "w")}
    if d["si"] is not None:
        ins.update({k: _dev(v) for k, v in d["si"].items()})
    return ins


def _read_sums(acc):
    """read_acc of edge_refs with the replicas added in extended precision (the sum of 32 doubles adds no rounding)."""
    acc = acc.cpu().numpy()
    R.read_acc(acc, F, ACC_SENTINEL)  # the sentinels
    return acc[2 * F:2 * F * (1 + R.BN_REPLICAS)].reshape(R.BN_REPLICAS, 2, F).astype(np.longdouble).sum(0)


def launch(d, times):
    """``times`` launches on fresh buffers; the guards and the route are checked here.  Returns the outputs per launch."""
    c = d["c"]
    mols, tc = c["mols"], c["tc"]
    ins = _inputs(d)
    outs = []
    for i in range(times):
        b = _buffers(d)
        route = _call(d, b, ins)
        torch.cuda.synchronize()
        what = "%s launch %d" % (case_id(c), i)
        assert route == (1 if c["wide"] else 0), what + ": route %d" % route
        g2 = b["g2"].cpu().numpy()
        assert np.all(g2[0] == SENTINEL) and np.all(g2[1 + mols:] == SENTINEL) and np.all(g2[:, 256:] == SENTINEL), \
            what + ": g2 guard rows or columns were written"
        o = dict(g2=g2[1:1 + mols, :256])
        for name, pad in (("dw", 64), ("db", 64), ("loss", 8), ("dl", 64)):
            if b[name + "_all"] is None:
                continue
            full = b[name + "_all"].cpu().numpy()
            assert np.all(full[:pad] == SENTINEL) and np.all(full[-pad:] == SENTINEL), what + ": guards of " + name
            o[name] = full[pad:-pad]
        o["dw"] = o["dw"].reshape(tc, 256)
        o["dl"] = o["dl"].reshape(mols, tc)
        if c["wide"]:
            assert not np.isnan(o["dl"]).any(), what + ": dl_scratch keeps NaN"
        else:  # route 0 touches neither scratch
            assert np.isnan(o["dl"]).all() and bool(torch.isnan(b["img"]).all()), what + ": route 0 wrote a scratch"
        o["loss_rep"] = o["loss"].astype(np.float64)
        o["loss"] = float(o["loss"].astype(np.longdouble).sum())
        o["sums"] = None if b["sums"] is None else _read_sums(b["sums"])
        o["sums_rep"] = None if b["sums"] is None else \
            b["sums"].cpu().numpy()[2 * F:2 * F * (1 + R.BN_REPLICAS)].reshape(R.BN_REPLICAS, 2, F)
        outs.append(o)
    return outs


# ================================================================================================ checks
def replicas_of(c):
    """(sums replica, loss replica) of every molecule, as the two routes place them: head_bwd_kernel -- workgroup b of
    grid = min(768, ceil(n_mols / 32)) takes the molecules [b n_mols / grid, (b + 1) n_mols / grid), its sums go to
    replica b % 32 and all loss to replica 0; the wide kernel -- workgroup b takes 32 molecules, wave v four of them,
    sums to replica b % 32, loss to replica (8 b + v) % 16."""
    m = np.arange(c["mols"])
    if c["wide"]:
        return (m // 32) % R.BN_REPLICAS, (8 * (m // 32) + (m % 32) // 4) % R.LOSS_REPLICAS
    grid = min(768, (c["mols"] + 31) // 32)
    block = np.searchsorted(np.arange(1, grid + 1) * c["mols"] // grid, m, side="right")
    return block % R.BN_REPLICAS, np.zeros(c["mols"], np.int64)


def replica_refs(d):
    """The exact contents of every replica of an integer case: (sums (32, 2, F) or None, loss (16,) or None for
    cross-entropy)."""
    c, ref = d["c"], d["ref"]
    rs, rl = replicas_of(c)
    sums = loss = None
    if d["si"] is not None:
        (a1, b1, a2, b2), _ = R._head_sums_terms(ref["g2"], d["si"], np.float64)
        sums = d["sums0"].copy()
        np.add.at(sums[:, 0], rs, a1 + b1)
        np.add.at(sums[:, 1], rs, a2 + b2)
    if c["kind"] == 1:
        rows = c["rows"]
        x, y = R.f64(d["logits"])[:rows], R.f64(d["labels"])[:rows]
        w = 1.0 if d["weights"] is None else R.f64(d["weights"])[:rows]
        loss = d["loss0"].copy()
        np.add.at(loss, rl[:rows], (w * (x - y) ** 2).sum(1))
    return sums, loss


def check_exact(d):
    c, ref = d["c"], d["ref"]
    for i, o in enumerate(launch(d, 2)):
        what = "%s launch %d: " % (case_id(c), i)
        assert np.array_equal(o["g2"], ref["g2"]), what + "g2"
        assert np.array_equal(o["dw"], ref["dw"]), what + "dW"
        if c["db"]:
            assert np.array_equal(o["db"], ref["db"]), what + "db"
        if c["wide"]:
            assert np.array_equal(o["dl"], ref["dl"]), what + "dl_scratch"
        if c["kind"] == 1:
            assert o["loss"] == ref["loss"], what + "loss %r != %r" % (o["loss"], ref["loss"])
        else:  # (sum of w over the one-hot rows) x logf(2): see the module docstring
            assert abs(o["loss"] - ref["loss"]) <= (1.0 + T_DEVICE_MATH) * R.U24 * ref["S_loss"], what + "loss"
        if d["si"] is not None:
            assert np.array_equal(o["sums"].astype(np.float64), (ref["sums"] + d["sums0"].sum(0)).astype(np.float64)), what + "sums"
        # ... and replica by replica: the layout the kernels spread their atomics by
        sums_rep, loss_rep = replica_refs(d)
        if sums_rep is not None:
            assert np.array_equal(o["sums_rep"], sums_rep), what + "the replicas of the sums"
        if loss_rep is not None:
            assert np.array_equal(o["loss_rep"], loss_rep), what + "the replicas of the loss"


def _bound(e_ref, T=0.0):
    return 2.0 * max(e_ref, 1.0) + T


def check_accuracy(d):
    """Returns the figures {name: (e, e_ref, bound)} after asserting each e <= bound."""
    c, ref = d["c"], d["ref"]
    name = case_id(c)
    fp, W = d["fp"][:, :256], d["w"]
    o = launch(d, 1)[0]
    f32r = R.head_bwd_f32(c["kind"], d["logits"], d["labels"], d["weights"], c["rows"], fp, W, c["wide"])
    f32r["dw"], f32r["db"] = f32r["dw"] + d["dw0"], f32r["db"] + d["db0"]
    f32r["loss"] += d["loss0"].sum()
    T = T_DEVICE_MATH if c["kind"] == 0 else 0.0
    fig = {}
    keys = ["g2", "dw"] + (["db"] if c["db"] else []) + (["dl"] if c["wide"] else [])
    for k in keys:
        e_ref = R.head_err_units(f32r[k], ref[k], ref["S_" + k])
        fig[k] = (R.head_err_units(o[k], ref[k], ref["S_" + k]), e_ref, _bound(e_ref, T))
    S_loss = max(ref["S_loss"], R.TINY32)
    e_ref = abs(f32r["loss"] - ref["loss"]) / S_loss / R.U24
    fig["loss"] = (abs(o["loss"] - ref["loss"]) / S_loss / R.U24, e_ref, _bound(e_ref, T))
    if c["wide"]:  # the products alone: float64 from the d logits the kernel returned, no allowance
        lin = R.head_linear_ref(o["dl"], np.abs(o["dl"]), fp, W)
        l32 = R.head_linear_f32(o["dl"], fp, W, True)
        for k in ("g2", "dw") + (("db",) if c["db"] else ()):
            start = 0.0 if k == "g2" else d[k + "0"]
            r, S = lin[k] + start, lin["S_" + k] + np.abs(start)
            e_ref = R.head_err_units(l32[k] + start, r, S)
            fig[k + "|dl"] = (R.head_err_units(o[k], r, S), e_ref, _bound(e_ref))
    if d["si"] is not None:  # from the g2 the kernel returned
        sums, S = R.head_sums_ref(o["g2"], d["si"])
        sums, S = sums + d["sums0"].sum(0), S + np.abs(d["sums0"]).sum(0)
        seq = R.head_sums_seq64(o["g2"], d["si"]) + d["sums0"].sum(0)
        e_ref = R.head_err_units(seq, sums, S, U53)
        fig["sums"] = (R.head_err_units(o["sums"], sums, S, U53), e_ref, _bound(e_ref))
    print("head backward %s: " % name + "; ".join("%s e %.2f e_ref %.2f bound %.2f" % ((k,) + v) for k, v in fig.items()))
    over = {k: v for k, v in fig.items() if not v[0] <= v[2]}
    assert not over, "%s: above the bound: %r" % (name, over)
    return fig


def run_case(c):
    d = build(c)
    if c["data"] == "int":
        assert not exactness_failures(d), exactness_failures(d)
        check_exact(d)
    else:
        check_accuracy(d)


@pytest.mark.parametrize("c", NARROW, ids=case_id)
def test_narrow_route(c):
    run_case(c)


@pytest.mark.parametrize("c", WIDE, ids=case_id)
def test_wide_route(c):
    run_case(c)


# ================================================================================================ refusals
REFUSALS = {
    "exact_mode_33_outputs": (C("acc", 1, 33, 1, 33, sums=11), {}),
    "ldfp_257_with_40_outputs": (C("acc", 0, 20, 2, 33, ldfp=257), {}),
    "scratch_missing": (C("acc", 1, 64, 1, 33), dict(dl_scratch=None)),
    "image_scratch_missing": (C("acc", 1, 64, 1, 33), dict(img_scratch=None)),
    "257_outputs": (C("acc", 1, 257, 1, 33), {}),
    "sums_without_runs": (C("acc", 1, 7, 1, 33, sums=11), dict(runs=None)),
    "one_pass_kernels_off": (C("acc", 1, 7, 1, 33, sums=11), {}),
}


@pytest.mark.parametrize("name", list(REFUSALS))
def test_refusal_writes_nothing(name):
    """GCMI_ERR_UNSUPPORTED with an error text and nothing launched: every buffer keeps its contents, sentinels, starts
    and the NaN of the two scratches included."""
    import deepchem_amd as dc
    from deepchem_amd import _lib
    c, override = REFUSALS[name]
    d = build(dict(c, starts=True))
    ins, b = _inputs(d), _buffers(d)
    before = {k: v.clone() for k, v in b.items() if v is not None}
    try:
        if name.startswith("exact_mode"):
            dc.set_gemm_mode("exact")
        if name == "one_pass_kernels_off":
            _lib.call("gcmi_set_option", _lib.GCMI_OPT_FUSED_BWD, 0)
        with pytest.raises(_lib.GcmiError) as err:
            _call(d, b, ins, **override)
        assert "status -3" in str(err.value) and "no other kernel stands behind this entry" in str(err.value)
    finally:
        dc.set_gemm_mode("fast")
        _lib.call("gcmi_set_option", _lib.GCMI_OPT_FUSED_BWD, 1)
    torch.cuda.synchronize()
    for k, v in before.items():
        assert torch.equal(torch.nan_to_num(b[k], nan=1234.5), torch.nan_to_num(v, nan=1234.5)), name + ": " + k + " was written"


# ================================================================================================ environment switch
def run_switched():
    for c in SWITCHED:
        run_case(c)


def test_wide_pair_below_33_outputs():
    """GCMI_HEAD_WIDE_MIN=1 is read once per process: one child (one GPU process at a time) runs the wide pair at 1, 2,
    15, 16, 17 and 32 outputs -- TCP = 16 or 32, one or two k-steps, most of the image padding -- with the same case
    builder and the same checks."""
    code = "from tests.test_gpu_head_bwd import run_switched\nrun_switched()\nprint('ok')\n"
    env = dict(os.environ)
    env.pop("GCMI_HEAD_WIDE", None)
    env["GCMI_HEAD_WIDE_MIN"] = "1"
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300,
                         cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    print(out.stdout[-6000:])
    assert out.returncode == 0 and "ok" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]
