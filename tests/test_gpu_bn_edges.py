"""The BatchNorm kernels (csrc/bn.hip: bn_stats, bn_apply, bn_bwd with and without relu_mask, bn_fold_eval) and
relu_bwd_ (csrc/gemm.hip) at every shape and layout their host code dispatches on, each case against the float64
restatement of tests/edge_refs.py (checked on the CPU by tests/test_edge_refs_host.py).

Every case id spells the branch it reaches, computed by ``edge_refs.bn_branch`` -- a restatement of launch_col_sums
and of the dx launch in bn_bwd_impl: ``sumsV / dxV`` the vector width of the column-sum and of the dx kernel (4 only
if every operand of that launch is 16-byte aligned, has ld % 4 == 0 and n_feat % 4 == 0), ``lx`` column lanes,
``ry = 256 / lx`` row lanes, ``idle`` threads with ty >= ry, ``colpasses`` trips of the column loop, ``wg`` workgroups
and ``lastrows`` rows of the last workgroup of the sums launch + of the dx launch (shares of at least 512 and 256
rows, rounded up to a multiple of the 4 ry rows of one round).

Every case runs TWICE in a row: next_sweep_direction() flips with every launch and a run makes five of them, so the
second run takes every kernel in the other sweep direction.

Bounds: TOL = 1e-4 relative to the largest reference magnitude for the per-column vectors and the running
statistics, 1e-4 * max(1, max|ref|) absolute for y and dx (tests/test_gpu_kernels.py).  The ReLU mask and untouched
memory are exact.  The ill-conditioned case has its own bound, from the float32 restatement (see that test).
"""
import numpy as np
import pytest
import torch

from oracle.edge_checks import DEV, SENTINEL, wide
from oracle.edge_checks import to_dev as _dev
from oracle.edge_checks import to_np as _np
from tests import edge_refs as R

pytestmark = pytest.mark.gpu
TOL = R.TOL

# where an operand lives: (columns left of it, columns right of it) in a sentinel-filled matrix, None = contiguous
PLACES = {
    "c": None,        # contiguous: aligned, ld = n_feat
    "a4": (4, 4),     # columns [4 : 4+f] of a matrix f + 8 wide: aligned, ld % 4 == 0, ld > n_feat -> V = 4
    "m1": (1, 7),     # columns [1 : 1+f] of the same matrix: the pointer is 4 bytes off -> V = 1 at any width
    "odd": (0, 1),    # columns [: f] of a matrix f + 1 wide: ld % 4 != 0 -> V = 1
}


def _vec4(place, f):
    return place in ("c", "a4") and f % 4 == 0


def _case(n, f, x_place="c", dy_place="c"):
    """stats sums and bn_apply read x alone; the backward sums read dy and x; the dx kernel dy, x and a contiguous
    dx: with dy and x in different places the sums and the dx kernel must EACH fall back to V = 1."""
    layout = x_place if x_place == dy_place else "x_%s_dy_%s" % (x_place, dy_place)
    both = _vec4(x_place, f) and _vec4(dy_place, f)
    return pytest.param(n, f, x_place, dy_place, id=R.bn_case_id(n, f, layout, both, both) +
                        ("-statsV%d" % (4 if _vec4(x_place, f) else 1) if not both else ""))


CASES = (
    # widths (contiguous).  1, 2: V = 1; 3: ry = 85, one idle thread; 4: lpr = 1, ry = 256, rounds of 1024 rows;
    # 76: lpr = 19, ry = 13, 9 idle; 100: lpr = 25, ry = 10; 255: V = 1, lx = 255, ry = 1; 257: V = 1, a second column
    # pass of one column; 1028: V = 4, lpr = 257, second column pass
    [_case(777, f) for f in (1, 2, 3, 4, 8, 76, 100, 255, 257, 1028)] +
    # row counts at width 64 (ry = 16, rounds of 64 rows): one round on and off its edge, the dx share of 256 and the
    # sums share of 512 rows on and off theirs, three workgroups
    [_case(n, 64) for n in (1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1025)] +
    # row counts at width 76 (one round = 4 * 13 = 52 rows; 520 = ten rounds = the rounded-up share)
    [_case(n, 76) for n in (52, 53, 520, 521)] +
    # the raised share: ceil(n / 2048) = 513 rows, rounded up to 1024 (ry = 128); the last workgroup has one row
    [_case(2048 * 512 + 1, 8)] +
    # layouts, 777 rows
    [_case(777, 64)] + [_case(777, f, p, p) for f in (64, 76) for p in ("a4", "m1", "odd")] +
    # dy aligned and x misaligned, and the reverse
    [_case(777, f, xp, dp) for f in (64, 76) for xp, dp in (("m1", "a4"), ("a4", "m1"))] +
    [_case(1, 76), _case(1, 3), _case(1, 64, "a4", "a4")])


def _place(a, place):
    if PLACES[place] is None:
        return _dev(a), None
    return wide(a, *PLACES[place])


def _err(got, ref, floor_one):
    """largest |got - ref| relative to max|ref| (``floor_one``: to max(1, max|ref|))."""
    got, ref = _np(got), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert np.isfinite(got).all()
    scale = float(np.abs(ref).max()) if ref.size else 0.0
    if floor_one:
        scale = max(scale, 1.0)
    worst = float(np.abs(got - ref).max()) if ref.size else 0.0
    if scale == 0.0:  # an all-zero reference: only zeros will do
        return 0.0 if worst == 0.0 else float("inf")
    return worst / scale


MATRICES = ("y", "y_eval", "dx", "dx_relu")


def _bn_inputs(n, f, x=None, seed=0):
    rng = np.random.RandomState(1000 * f + n % 1000 + seed)
    if x is None:
        x = (rng.standard_normal((n, f)) * 2 + 1).astype(np.float32)  # a fifth of the entries negative: the ReLU mask
    dy = rng.standard_normal((n, f)).astype(np.float32)
    gamma = (rng.rand(f) + 0.5).astype(np.float32)
    beta = rng.standard_normal(f).astype(np.float32)
    rm0, rv0 = rng.standard_normal(f).astype(np.float32), (rng.rand(f) + 0.5).astype(np.float32)
    return x, dy, gamma, beta, rm0, rv0


def run_bn(n, f, x_place, dy_place, x=None, allowed=None):
    """Two runs of stats / apply / backward / masked backward / eval fold on one input.  ``allowed``: per output, the
    permitted error (default TOL everywhere).  Returns the largest error of every output over both runs."""
    from deepchem_amd import ops
    x, dy, gamma, beta, rm0, rv0 = _bn_inputs(n, f, x)
    ref = R.bn_ref(x, gamma, beta, dy)
    xg, xw = _place(x, x_place)
    dyg, dyw = _place(dy, dy_place)
    before = [(w, w.clone()) for w in (xw, dyw) if w is not None]
    g, b, rm, rv = _dev(gamma), _dev(beta), _dev(rm0.copy()), _dev(rv0.copy())
    worst = {}

    def check(run, name, got, want):
        e = _err(got, want, name in MATRICES)
        lim = TOL if allowed is None else allowed[name]
        print("bn n=%d f=%d x:%s dy:%s run %d %-12s err %.3e allowed %.3e" % (n, f, x_place, dy_place, run, name, e, lim))
        worst[name] = max(worst.get(name, 0.0), e)
        assert e <= lim, "%s (run %d): error %.3e, allowed %.3e" % (name, run, e, lim)

    for run in (1, 2):
        mean, invstd, scale, shift = ops.bn_stats(xg, g, b, rm, rv, R.BN_EPS, R.BN_MOMENTUM)
        y = ops.bn_apply(xg, scale, shift)
        dgamma, dbeta, dx = ops.bn_bwd(dyg, xg, g, mean, invstd, True)
        dgamma_m, dbeta_m, dx_m = ops.bn_bwd(dyg, xg, g, mean, invstd, True, relu_mask=True)
        for name, got in (("mean", mean), ("invstd", invstd), ("scale", scale), ("shift", shift), ("y", y),
                          ("dgamma", dgamma), ("dbeta", dbeta), ("dx", dx), ("dx_relu", dx_m), ("dgamma", dgamma_m),
                          ("dbeta", dbeta_m)):
            check(run, name, got, ref[name])
        check(run, "running_mean", rm, R.bn_running_ref(rm0, ref["mean"], run))
        check(run, "running_var", rv, R.bn_running_ref(rv0, ref["unbiased"], run))
        # the mask is x > 0 on the kernel's own dx, exactly (the parameter gradients do not depend on it)
        assert torch.equal(dx_m, torch.where(xg > 0, dx, torch.zeros_like(dx)))
        # eval fold of the running statistics the device now holds
        s2, h2 = ops.bn_fold_eval(g, b, rm, rv, R.BN_EPS)
        rs, rh = R.bn_fold_eval_ref(gamma, beta, _np(rm), _np(rv))
        check(run, "scale_eval", s2, rs)
        check(run, "shift_eval", h2, rh)
        check(run, "y_eval", ops.bn_apply(xg, s2, h2), x.astype(np.float64) * rs + rh)
    # (outside the two runs: a sixth launch per run would bring the second run back to the first one's directions)
    dgamma, dbeta, none = ops.bn_bwd(dyg, xg, g, mean, invstd, False)
    assert none is None
    check(3, "dgamma", dgamma, ref["dgamma"])
    check(3, "dbeta", dbeta, ref["dbeta"])
    for w, was in before:  # the kernels only read their inputs: block and sentinel columns alike
        assert torch.equal(w, was), "an input matrix was written"
        assert bool((w[:, -1] == SENTINEL).all())
    return worst


@pytest.mark.parametrize("n,f,x_place,dy_place", CASES)
def test_bn_shapes_and_layouts(n, f, x_place, dy_place):
    run_bn(n, f, x_place, dy_place)


def test_bn_constant_column_has_zero_variance_and_finite_dx():
    """var = 0 exactly (the fp64 sums of n copies of 2.5 and of 6.25 are exact), invstd = 1 / sqrt(eps)."""
    from deepchem_amd import ops
    rng = np.random.RandomState(5)
    x = (rng.standard_normal((777, 64)) * 2 + 1).astype(np.float32)
    x[:, 5] = 2.5
    x[:, 63] = -0.75
    run_bn(777, 64, "c", "c", x=x)
    xg, f = _dev(x), 64
    ones = torch.ones(f, device=DEV)
    mean, invstd, scale, shift = ops.bn_stats(xg, ones, torch.zeros(f, device=DEV), torch.zeros(f, device=DEV),
                                              ones.clone(), R.BN_EPS, R.BN_MOMENTUM)
    want = np.float32(1.0 / np.sqrt(np.float64(np.float32(1e-3))))
    assert float(invstd[5]) == float(want) and float(invstd[63]) == float(want)
    assert float(mean[5]) == 2.5 and float(mean[63]) == -0.75
    _, _, dx = ops.bn_bwd(_dev(rng.standard_normal((777, 64)).astype(np.float32)), xg, ones, mean, invstd, True)
    assert bool(torch.isfinite(dx).all())


def test_bn_ill_conditioned_columns_stay_within_four_times_float32():
    """Column means near 1e3, standard deviation near 1e-1, n = 4099, f = 64.  float32 holds a mean near 1e3 to
    3e-5, which is 3e-4 standard deviations, and shift = beta - mean * scale (~1e4) to 5e-4: no float32 BatchNorm
    reaches 1e-4 here, so the bound is not fixed in advance.  It is measured: ``edge_refs.bn_ref_f32`` (the same
    formulas with float32 vectors and float32 per-element arithmetic, float64 column sums as the kernel has) against
    ``edge_refs.bn_ref`` on the same input, per output; the kernel may be four times that (it rounds
    scale * x + shift once, as a fused multiply-add, where the restatement rounds twice), never less than TOL.

    Measured (float32 restatement on the CPU | kernel on MI355X; relative to max|ref|, for y and dx to
    max(1, max|ref|)):
        mean   4.9e-08 | 4.9e-08    invstd 6.0e-07 | 6.4e-08    scale  5.0e-07 | 5.1e-08    shift 5.1e-07 | 8.8e-08
        y      2.8e-04 | 1.5e-04    dgamma 3.0e-04 | 3.0e-04    dbeta  3.9e-08 | 3.9e-08
        dx     8.8e-06 | 8.9e-06    dx with the ReLU mask 9.4e-06 | 6.9e-06     eval fold: y 1.7e-04 | 5.9e-05
    so y may be off by 1.14e-03, dgamma by 1.19e-03, the eval-mode y by 6.8e-04, everything else by TOL.
    """
    n, f = 4099, 64
    rng = np.random.RandomState(7)
    centre = (1e3 * (1 + 0.2 * rng.rand(f)) * rng.choice([-1.0, 1.0], size=f))
    x = (centre + 0.1 * rng.standard_normal((n, f))).astype(np.float32)
    x, dy, gamma, beta, rm0, rv0 = _bn_inputs(n, f, x)
    ref, f32 = R.bn_ref(x, gamma, beta, dy), R.bn_ref_f32(x, gamma, beta, dy)
    measured = {k: _err(f32[k], ref[k], k in MATRICES) for k in ("mean", "invstd", "scale", "shift", "y", "dgamma",
                                                                   "dbeta", "dx", "dx_relu")}
    # the eval fold of the running statistics after one and after two updates (running_mean ~ 990, then ~ 999.9:
    # x * scale + shift cancels there as well), restated in float32 on the reference's running statistics
    f32t = np.float32
    for k in ("scale_eval", "shift_eval", "y_eval"):
        measured[k] = 0.0
    for times in (1, 2):
        rm = R.bn_running_ref(rm0, ref["mean"], times).astype(f32t)
        rv = R.bn_running_ref(rv0, ref["unbiased"], times).astype(f32t)
        rs, rh = R.bn_fold_eval_ref(gamma, beta, rm, rv)
        sc = gamma * (f32t(1) / np.sqrt(rv + f32t(R.BN_EPS)))
        sh = beta - rm * sc
        assert sc.dtype == f32t and sh.dtype == f32t
        for k, got, want in (("scale_eval", sc, rs), ("shift_eval", sh, rh), ("y_eval", x * sc + sh, x.astype(np.float64) * rs + rh)):
            measured[k] = max(measured[k], _err(got, want, k in MATRICES))
    allowed = {k: max(4.0 * e, TOL) for k, e in measured.items()}
    # (momentum updates of the mean and the variance: errors of the size of theirs, nothing cancels)
    allowed["running_mean"], allowed["running_var"] = allowed["mean"], TOL
    for k in sorted(measured):
        print("ill-conditioned: float32 restatement %-8s err %.3e -> allowed %.3e" % (k, measured[k], allowed[k]))
    worst = run_bn(n, f, "c", "c", x=x, allowed=allowed)
    for k in sorted(measured):
        print("ill-conditioned: kernel              %-8s err %.3e" % (k, worst[k]))


def test_bn_refusals_launch_nothing():
    """ldx < n_feat and zero rows are refused before any launch: nothing the call could write has changed."""
    import ctypes
    from deepchem_amd import _lib, ops
    f, n = 8, 16
    x = torch.randn((n, f), device=DEV)
    vec = lambda v: torch.full((f,), v, device=DEV)  # noqa: E731
    g, b, rm, rv = vec(1.0), vec(0.0), vec(0.25), vec(0.75)
    with pytest.raises(ValueError):
        ops.bn_stats(x[:0], g, b, rm, rv, R.BN_EPS, R.BN_MOMENTUM)
    # a hand-made view whose rows overlap (row stride f - 1): the wrapper must not turn it into ld = f
    overlap = torch.as_strided(x, (n, f), (f - 1, 1))
    mean, invstd = vec(0.0), vec(1.0)
    with pytest.raises(ValueError):
        ops.bn_stats(overlap, g, b, rm, rv, R.BN_EPS, R.BN_MOMENTUM)
    with pytest.raises(ValueError):
        ops.bn_apply(overlap, g, b)
    with pytest.raises(ValueError):
        ops.bn_bwd(overlap, x, g, mean, invstd, True)
    with pytest.raises(ValueError):
        ops.bn_bwd(x, overlap, g, mean, invstd, True)
    with pytest.raises(ValueError):
        ops.relu_bwd_(overlap, x)
    # the C entry points themselves
    out = [vec(SENTINEL) for _ in range(4)]
    acc = torch.full((_lib.bn_acc_doubles(f),), SENTINEL, dtype=torch.float64, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for ldx, rows in ((f - 1, n), (f, 0)):
        with pytest.raises(_lib.GcmiError):
            _lib.call("gcmi_bn_stats", p(x), ldx, rows, f, p(g), p(b), R.BN_EPS, R.BN_MOMENTUM, p(rm), p(rv),
                      p(out[0]), p(out[1]), p(out[2]), p(out[3]), p(acc), st)
    y = torch.full((n, f), SENTINEL, device=DEV)
    with pytest.raises(_lib.GcmiError):
        _lib.call("gcmi_bn_apply", p(x), f - 1, n, f, p(g), p(b), p(y), f, st)
    with pytest.raises(_lib.GcmiError):
        _lib.call("gcmi_bn_apply", p(x), f, n, f, p(g), p(b), p(y), f - 1, st)
    dx = torch.full((n, f), SENTINEL, device=DEV)
    for lddy, ldx, lddx, rows in ((f - 1, f, f, n), (f, f - 1, f, n), (f, f, f - 1, n), (f, f, f, 0)):
        with pytest.raises(_lib.GcmiError):
            _lib.call("gcmi_bn_bwd", p(x), lddy, p(x), ldx, rows, f, p(g), p(mean), p(invstd), p(out[0]), p(out[1]), p(dx),
                      lddx, 0, p(acc), st)
    torch.cuda.synchronize()
    for t in out + [acc, y, dx]:
        assert bool((t == SENTINEL).all())
    assert bool((rm == 0.25).all()) and bool((rv == 0.75).all())


# ------------------------------------------------------------------------------------------------ relu_bwd_
def _relu_case(n, f, g_place, y_place):
    v = 4 if (_vec4(g_place, f) and _vec4(y_place, f)) else 1
    return pytest.param(n, f, g_place, y_place, id="n%d-f%d-g_%s-y_%s-V%d-%s" % (
        n, f, g_place, y_place, v, "stride" if n * (f // v) > 8192 * 256 else "nostride"))


RELU_CASES = ([_relu_case(n, f, "c", "c") for f in (1, 3, 64, 76, 300) for n in (1, 333, 70001)] +
              [_relu_case(n, f, gp, yp) for f in (3, 64, 76) for n in (1, 333)
               for gp, yp in (("a4", "a4"), ("m1", "m1"), ("a4", "m1"), ("m1", "a4"), ("odd", "c"))] +
              [_relu_case(70001, 64, "a4", "m1"), _relu_case(70001, 76, "a4", "a4")])


@pytest.mark.parametrize("n,f,g_place,y_place", RELU_CASES)
def test_relu_bwd_inplace(n, f, g_place, y_place):
    """g <- g where y > 0, else 0, in place: exact, -0.0 and 0.0 in y both close the gate, and nothing outside the
    column block of g (nor anything of y) is written.  V = 4 only if g and y are both 16-byte addressable; the
    grid-stride loop (grid_for caps the grid at 8192 workgroups of 256 slots) runs at 70 001 x 300 only."""
    from deepchem_amd import ops
    rng = np.random.RandomState(n + f)
    g = rng.standard_normal((n, f)).astype(np.float32)
    y = rng.standard_normal((n, f)).astype(np.float32)
    flat = y.reshape(-1)
    flat[::5] = 0.0
    flat[2::7] = -0.0
    assert n * f < 3 or (np.signbit(flat[2]) and flat[2] == 0)
    gg, gw = _place(g, g_place)
    yg, yw = _place(y, y_place)
    y_before = None if yw is None else yw.clone()
    out = ops.relu_bwd_(gg, yg)
    assert out.data_ptr() == gg.data_ptr()
    want = torch.where(torch.from_numpy(y) > 0, torch.from_numpy(g), torch.zeros(()))
    mism = int((out.cpu() != want).sum())
    print("relu_bwd n=%d f=%d g:%s y:%s mismatches %d" % (n, f, g_place, y_place, mism))
    assert mism == 0 and torch.equal(out.cpu(), want)
    if gw is not None:
        lo = PLACES[g_place][0]
        outside = gw.clone()
        outside[:, lo:lo + f] = SENTINEL
        assert bool((outside == SENTINEL).all()), "columns outside the block of g were written"
    if yw is not None:
        assert torch.equal(yw, y_before)
