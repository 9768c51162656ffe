"""The readout kernels (csrc/readout.hip: ops.readout, ops.readout_bwd) at every width, layout and batch shape
readout_fwd_impl / gcmi_readout_bwd dispatch on, against the float64 restatement of tests/edge_refs.py (checked on
the CPU, also against the oracle's GraphGather, by tests/test_edge_refs_host.py).

Every case id spells the branch it reaches (``edge_refs.readout_branch``, a restatement of readout_fwd_impl): ``V``
the vector width (4 only for 16-byte addressable rows and n_feat % 4 == 0), ``gl`` lanes per molecule, ``mpb``
molecules per workgroup, ``idle`` threads of no lane group, ``colpasses`` trips of the column loop, ``pipelined`` /
``plain`` the walk (pipelined only for V = 4, gl = n_feat / 4 a power of two with n_deg <= gl <= 64), ``lastwg`` the
molecules of the last workgroup (fewer than mpb: absent groups).

The batches are built by hand (``edge_refs.readout_batch``): molecules without atoms at the front, in the middle and
at the end, 1, 3, 4, 5, 8, 9, 12, 13 and 25 atoms (the four-row rounds and the three rounds in flight on and off
their boundaries), all rows in one degree block, one row in each block (every round crosses run boundaries), rows in
the first and last block only, 64 atoms at the most.  ``A40`` / ``A43``: max_deg 10 (n_deg = 11), 40 and 43
molecules; ``B37``: max_deg 4 (n_deg = 5, which makes width 32 pipelined), 37 molecules.

Bounds: TOL = 1e-4 relative to the largest finite reference magnitude for real-valued features; with small-integer
features, signed power-of-two scales and integer shifts every a = x * scale + shift and every sum is exact in
float32 (host test), so sums, maxima and arg-max rows must EQUAL the reference.  Molecules without atoms: sum 0, max
-inf, arg-max -1; with tanh 0 and -1.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from oracle.edge_checks import DEV, SENTINEL, wide
from oracle.edge_checks import to_dev as _dev
from oracle.edge_checks import to_np as _np
from tests import edge_refs as R

pytestmark = pytest.mark.gpu
TOL = R.TOL

BATCHES = {"A40": (11, 20, 1), "A43": (11, 23, 2), "B37": (5, 17, 3)}  # n_deg, random molecules, seed
PLACES = {"c": None, "a4": (4, 4), "m1": (1, 7)}  # as tests/test_gpu_bn_edges.py: contiguous, aligned slice, misaligned
# width, where x lives.  1, 3: V = 1, one and three lanes per molecule; 75: V = 1, mpb = 3, 31 idle threads; 300 is a
# multiple of 4: contiguous rows give V = 4 with 75 lanes (mpb = 3), the V = 1 column loop at this width needs rows
# that are not 16-byte addressable (300-m1), and 301 loops in any layout; 32: plain at max_deg 10 (gl = 8 < 11),
# pipelined at max_deg 4; 64, 128, 256: pipelined; 96 (gl = 24, no power of two) and 512 (gl = 128 > 64): plain;
# 2048: V = 4 column loop; 64-a4 / 64-m1: x a column slice, V = 4 with ld > n_feat and V = 1
WIDTHS = [(1, "c"), (3, "c"), (75, "c"), (300, "c"), (300, "m1"), (301, "c"), (32, "c"), (64, "c"), (128, "c"),
          (256, "c"), (96, "c"), (512, "c"), (2048, "c"), (64, "a4"), (64, "m1")]
CASES = [pytest.param(f, place, b, id=R.readout_case_id(f, BATCHES[b][0], 20 + BATCHES[b][1], place + "-" + b,
                                                         place != "m1"))
         for f, place in WIDTHS for b in BATCHES]


@functools.lru_cache(maxsize=None)
def batch(name):
    """(BatchGraph on the GPU, membership, atoms per molecule): the readout reads the degree blocks and membership
    only, the neighbour table is all zeros."""
    from deepchem_amd.graph import BatchGraph
    n_deg, n_fill, seed = BATCHES[name]
    counts = R.readout_batch(n_deg, n_fill, seed)
    deg_counts, membership = R.hand_batch(counts)
    n_edges = sum(d * c for d, c in enumerate(deg_counts))
    g = BatchGraph(deg_counts, torch.zeros(n_edges, dtype=torch.int32, device=DEV), _dev(membership))
    assert g.max_deg + 1 == n_deg and g.n_atoms == len(membership)
    return g, membership, counts.sum(1)


@functools.lru_cache(maxsize=None)
def features(name, f, ints):
    """(x, scale, shift) float32.  ``ints``: x in [-3, 3], scale a signed power of two in [1/2, 4] with one zero,
    shift an integer in [-2, 2] -- exact in float32, ties everywhere."""
    n_atoms = len(batch(name)[1])
    rng = np.random.RandomState(f + 7 * len(name) + (1 if ints else 0))
    if ints:
        x = rng.randint(-3, 4, size=(n_atoms, f))
        scale = rng.choice([-1.0, 1.0], size=f) * 2.0 ** rng.randint(-1, 3, size=f)
        scale[0] = -2.0  # at least one negative scale: the maximum is then the minimum of x
        if f > 1:
            scale[1] = 0.0  # every row ties: the first row of the molecule must win
        shift = rng.randint(-2, 3, size=f)
    else:
        x, scale, shift = rng.standard_normal((n_atoms, f)), rng.standard_normal(f), rng.standard_normal(f)
    return tuple(a.astype(np.float32) for a in (x, scale, shift))


def _place(a, place):
    if PLACES[place] is None:
        return _dev(a), None
    return wide(a, *PLACES[place])


def run_readout(g, x, n_mols, scale, shift, tanh, eligible):
    """ops.readout; where the pipelined walk is eligible, with GCMI_OPT_READOUT_PIPELINED on and off: both walks
    take the rows in the same order, outputs and arg-max must be bit-identical."""
    from deepchem_amd import _lib, ops
    if not eligible:
        return ops.readout(g, x, n_mols, scale, shift, tanh)
    was = ctypes.c_int32(-1)
    _lib.call("gcmi_get_option", _lib.GCMI_OPT_READOUT_PIPELINED, ctypes.byref(was))
    assert was.value in (0, 1)
    got = {}
    try:
        for mode in (1, 0):
            _lib.call("gcmi_set_option", _lib.GCMI_OPT_READOUT_PIPELINED, mode)
            out, arg = ops.readout(g, x, n_mols, scale, shift, tanh)
            got[mode] = (out.clone(), arg.clone())
    finally:
        _lib.call("gcmi_set_option", _lib.GCMI_OPT_READOUT_PIPELINED, was.value)
    assert torch.equal(got[1][0], got[0][0]), "pipelined and plain walk differ in the outputs"
    assert torch.equal(got[1][1], got[0][1]), "pipelined and plain walk differ in the arg-max"
    return got[1]


def _rel(got, ref):
    """largest error over the finite entries of ref, relative to their largest magnitude."""
    fin = np.isfinite(ref)
    assert np.isfinite(got[fin]).all()
    scale = float(np.abs(ref[fin]).max()) if fin.any() else 0.0
    worst = float(np.abs(got[fin] - ref[fin]).max()) if fin.any() else 0.0
    return worst / scale if scale > 0 else (0.0 if worst == 0 else float("inf"))


def check_empty(out, arg, sizes, f, tanh, what):
    empty = sizes == 0
    assert empty[0] and empty[-1] and empty[1:-1].any()
    assert (out[empty, :f] == 0).all(), what + ": sum of a molecule without atoms"
    assert (out[empty, f:] == (-1.0 if tanh else -np.inf)).all(), what + ": max of a molecule without atoms"
    assert (arg[empty] == -1).all() and (arg[~empty] >= 0).all(), what + ": arg-max of a molecule without atoms"


@pytest.mark.parametrize("f,place,name", CASES)
def test_readout_forward(f, place, name):
    g, membership, sizes = batch(name)
    n_mols = len(sizes)
    n_deg = BATCHES[name][0]
    eligible = R.readout_branch(f, n_deg, place != "m1")["pipelined"]
    for ints in (False, True):
        x, scale, shift = features(name, f, ints)
        xg, xw = _place(x, place)
        x_before = None if xw is None else xw.clone()
        sg, hg = _dev(scale), _dev(shift)
        for bn in (False, True):
            for tanh in (False, True):
                what = "readout f=%d %s %s %s bn=%d tanh=%d" % (f, place, name, "int" if ints else "real", bn, tanh)
                out_g, arg_g = run_readout(g, xg, n_mols, sg if bn else None, hg if bn else None, tanh, eligible)
                assert tuple(out_g.shape) == (n_mols, 2 * f) and tuple(arg_g.shape) == (n_mols, f)
                out, arg = _np(out_g), arg_g.cpu().numpy().astype(np.int64)
                ref, ref_arg = R.readout_ref(x, membership, n_mols, scale if bn else None, shift if bn else None, tanh)
                check_empty(out, arg, sizes, f, tanh, what)
                err = _rel(out, ref)
                exact = ints and not tanh
                print("%s: err %.3e allowed %.3e, arg-max mismatches %d" % (what, err, 0.0 if exact else TOL,
                                                                            int((arg != ref_arg).sum())))
                if exact:
                    assert np.array_equal(out, ref), what + ": integer sums and maxima must be exact"
                else:
                    assert err <= TOL, what
                    assert np.array_equal(np.isfinite(out), np.isfinite(ref))
                if ints or not bn:
                    # a is exact in float32 (integers) or x itself: the lowest row attaining the maximum, exactly
                    assert np.array_equal(arg, ref_arg), what + ": arg-max"
                else:
                    # real features under a real scale: a near-tie may fall either way in float32; the winner must be
                    # a row of the molecule whose float64 value is the maximum to within TOL
                    a64 = x.astype(np.float64) * scale + shift
                    has = sizes > 0
                    rows = arg[has]
                    assert (membership[rows] == np.nonzero(has)[0][:, None]).all(), what + ": arg-max row of another molecule"
                    top = np.take_along_axis(a64, rows, 0)
                    mx = R.readout_ref(x, membership, n_mols, scale, shift, False)[0][has, f:]
                    assert (mx - top <= TOL * np.abs(mx).max()).all(), what + ": arg-max row is not a maximum"
                if place != "c":
                    # same rows in the same order whatever the vector width: bit-equal to the contiguous run
                    out_c, arg_c = run_readout(g, _dev(x), n_mols, sg if bn else None, hg if bn else None, tanh,
                                               R.readout_branch(f, n_deg)["pipelined"])
                    assert torch.equal(out_g, out_c) and torch.equal(arg_g, arg_c), what + ": strided != contiguous"
        if xw is not None:
            assert torch.equal(xw, x_before) and bool((xw[:, -1] == SENTINEL).all())


@pytest.mark.parametrize("f,place,name", CASES)
def test_readout_backward(f, place, name):
    """dx of <out, dout> for random dout: every row gets its molecule's sum gradient, the arg-max row the max gradient
    on top, with tanh both times 1 - out^2 of the saved output.  (V = 4 iff n_feat % 4 == 0 here: dout, out, arg and
    dx are contiguous; ``place`` only moves x of the forward that produces out and arg.)"""
    from deepchem_amd import ops
    g, membership, sizes = batch(name)
    n_mols = len(sizes)
    x, _, _ = features(name, f, False)
    xg, _ = _place(x, place)
    rng = np.random.RandomState(f)
    dout = rng.standard_normal((n_mols, 2 * f)).astype(np.float32)
    for tanh in (False, True):
        out_g, arg_g = ops.readout(g, xg, n_mols, tanh=tanh)
        ref_out, ref_arg = R.readout_ref(x, membership, n_mols, tanh=tanh)
        assert np.array_equal(arg_g.cpu().numpy(), ref_arg)
        dx = ops.readout_bwd(g, _dev(dout), out_g, arg_g, tanh)
        ref = R.readout_bwd_ref(dout, np.where(np.isfinite(ref_out), ref_out, 0.0), ref_arg, membership, tanh)
        err = _rel(_np(dx), ref)
        print("readout_bwd f=%d %s %s tanh=%d: err %.3e allowed %.3e" % (f, place, name, tanh, err, TOL))
        assert err <= TOL


# dout / out as column slices of wider matrices at width 64.  gcmi_readout_bwd: V = 4 iff dx, dout, arg and -- with
# tanh only -- out are 16-byte addressable
@pytest.mark.parametrize("dout_place,out_place,tanh,v", [("a4", "a4", True, 4), ("a4", "m1", True, 1), ("m1", "a4", True, 1),
                                                        ("a4", "m1", False, 4), ("m1", "a4", False, 1),
                                                        ("a4", "a4", False, 4)],
                         ids=lambda p: str(p))
def test_readout_backward_sliced_gradients(dout_place, out_place, tanh, v):
    from deepchem_amd import ops
    f, name = 64, "A43"
    g, membership, sizes = batch(name)
    n_mols = len(sizes)
    x, _, _ = features(name, f, False)
    out_c, arg_g = ops.readout(g, _dev(x), n_mols, tanh=tanh)
    out_np = out_c.cpu().numpy()
    out_np[~np.isfinite(out_np)] = 0.0  # (-inf of the molecules without atoms: no row reads them)
    dout = np.random.RandomState(11).standard_normal((n_mols, 2 * f)).astype(np.float32)
    dg, dw = _place(dout, dout_place)
    og, ow = _place(out_np, out_place)
    kept = [(w, w.clone()) for w in (dw, ow)]
    dx = ops.readout_bwd(g, dg, og, arg_g, tanh)
    ref_out, ref_arg = R.readout_ref(x, membership, n_mols, tanh=tanh)
    ref = R.readout_bwd_ref(dout, np.where(np.isfinite(ref_out), ref_out, 0.0), ref_arg, membership, tanh)
    err = _rel(_np(dx), ref)
    print("readout_bwd sliced dout:%s out:%s tanh=%d (V = %d): err %.3e allowed %.3e" % (dout_place, out_place, tanh, v,
                                                                                      err, TOL))
    assert err <= TOL
    # the vector width changes nothing in the arithmetic: bit-equal to the contiguous call
    assert torch.equal(dx, ops.readout_bwd(g, _dev(dout), _dev(out_np), arg_g, tanh))
    for w, was in kept:
        assert torch.equal(w, was)
