"""The lattice-convolution kernels (csrc/lcnn.hip) at the sizes their launch arithmetic depends on, the four ops called
directly: ``ops.lc_site_fwd``, ``lc_site_bwd``, ``lc_rev_sum`` and ``lc_running``, one after the other from a Y drawn
N(0, 1) (no product ahead of them), in training and in eval mode.

Bar: ``bar`` of tests/test_gpu_lcnn.py, unchanged: the error against the float64 restatement (tests/lcnn_refs.py:
``site_fwd_ref``, ``site_bwd_ref``, ``rev_sum_ref``, ``running_ref``) is at most 4 times ``e32``, the larger error of
the float32 restatements in the two slot orders, with a floor of one float32 ulp of the tensor's largest entry.  For the
running statistics the float64 reference is the literal loop of the N per-site updates, ``e32`` the float32 loop.  The
two slot orders lie within 4 times of each other for every tensor of every case (tests/test_conv_edge_refs_host.py
asserts it on the CPU; no case was reseeded).  Where two launches differ only in leading dimension, column offset,
optional argument or tiling the assertion is ``torch.equal``: no atomics, fixed summation orders.

Cases (O, P, K, n_sites) and what each pins (a workgroup of 256 threads takes 256 // O sites; lc_site_bwd leaves one
partial row per workgroup of a grid cut to 1024; lc_sums_finish gives lane l the partials l, l + 64, ...):
* (64, 2, 1, n), n = 256 | 257: 64 | 65 partials, the first second partial of a lane of lc_sums_finish;
  n = 4096 | 4097: 1024 | 1025 site groups, the cap of the partial grid: lc_site_bwd takes a second turn of its loop.
* (64, 2, 8, 4097): 32 776 reverse rows = 8194 row groups of lc_rev_sum, past the 8192 workgroups of ``grid_for``.
* (19, 6, 3, n), n = 255 | 256 | 257: lc_running's 256 threads start to stride (k += 256); n = 2047 | 2048 | 2049: its
  cut at kLcRunWindow = 2048 sites.
* (O, 3, 3, 20), O = 2, 3 (128 and 85 sites per workgroup, 0 and 1 idle threads), 36 | 37 and 42 | 43 (256 // O steps
  7 -> 6 and 6 -> 5), 63 (4 sites, 4 idle threads).
* (19, P, 3, 20), P = 3, 4, 5, 7: the ``p < P`` predicates of the loops unrolled over kLcMaxP = 8.
* lc_running alone on the cut cases, momentum 0.1 (the bound the window is derived for), 0.5 and 1.0 (only the last
  site counts, (1 - m)^N = 0), from running statistics of size up to 1e30, on N(0, 1) rows and on rows whose sites further
  back than 256 from the last are 1e12 times louder (so the sites between 256 and 2048 back carry the result, and what
  the window skips must still stay under the floor: the claim of the comment at kLcRunWindow).
* views: Y as the columns [3, 3 + K O) of a NaN matrix 5 columns wider, dOut as the columns [1, 1 + O) of a NaN matrix;
  mask = None against ones, bias = None against zeros, want_x = False: the same bits.
* tiling: (64, 2, 8, 4097) nine times in one LcBatch, 36 873 sites = 9219 site groups of lc_site_fwd and 73 746 row
  groups of lc_rev_sum, past 8192 workgroups: every copy's rows of out, X, dX and dY equal the single copy's.

Measured on an MI355X (worst ratio error / e32, training / eval): the grid cases 1.02 / 1.03, the lc_running sizes 1.58 /
1.36, the widths 1.30 / 0.95, the permutation counts 1.62 / 1.02; lc_running alone 2.07 (n = 2047, momentum 0.1).  Worst
of the family: 2.07.  No case was reseeded.  One finding, fixed in csrc/lcnn.hip: at (2, 3, 3, 20) in eval mode db, then
the sum of the float32 dX, stood at 5.42 (1.2 ulp); it is now (gamma * invstd) * dbeta in double (LCNN,
"edges pinned").
"""
import numpy as np
import pytest
import torch

from deepchem_amd import ops
from tests import lcnn_refs as R
from tests.test_gpu_lcnn import bar

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")

GRID_CASES = [(64, 2, 1, n) for n in (256, 257, 4096, 4097)] + [(64, 2, 8, 4097)]
RUNNING_CASES = [(19, 6, 3, n) for n in (255, 256, 257, 2047, 2048, 2049)]
WIDTH_CASES = [(O, 3, 3, 20) for O in (2, 3, 36, 37, 42, 43, 63)]
PERM_CASES = [(19, P, 3, 20) for P in (3, 4, 5, 7)]
OP_CASES = GRID_CASES + RUNNING_CASES + WIDTH_CASES + PERM_CASES
TILED_CASE, COPIES = (64, 2, 8, 4097), 9
CUT_SITES = (2047, 2048, 2049, 4097)
MOMENTA = (0.1, 0.5, 1.0)
LOUD, LOUD_FROM = 1e12, 256


def tables_of(c):
    return ops.lc_graph_tables(c["graph"].edge_index, c["N"], c["P"], c["K"])


def tiled_batch(c, copies, device):
    """``copies`` times the graph of a case in one LcBatch."""
    return ops.LcBatch([tables_of(c)] * copies, c["P"], c["K"], device)


def dev(a):
    return None if a is None else torch.as_tensor(a, device=DEV)


def run_ops(c, batch=None, copies=1, y=None, cot=None, mask="case", bias="case", want_x=True, running=True):
    """The four ops one after the other on a case (tiled ``copies`` times); tensors on the device by name."""
    b = batch or tiled_batch(c, copies, DEV)
    rep = lambda a: dev(np.tile(a, (copies,) + (1,) * (a.ndim - 1)))  # noqa: E731
    y = rep(c["Y"]) if y is None else y
    cot = rep(c["cot"]) if cot is None else cot
    mask = rep(c["mask"]) if isinstance(mask, str) else mask
    bias = dev(c["b"]) if isinstance(bias, str) else bias
    gamma, beta = dev(c["gamma"]), dev(c["beta"])
    stats = {} if c["training"] else dict(mean=dev(c["rm"]), var=dev(c["rv"]))
    out, x = ops.lc_site_fwd(b, y, bias, gamma, beta, eps=R.EPS, mask=mask, want_x=want_x, **stats)
    res = {"out": out}
    if x is not None:
        dx, sums = ops.lc_site_bwd(b, x, cot, gamma, eps=R.EPS, mask=mask, **stats)
        O = c["O"]
        res.update(X=x, dX=dx, dgamma=sums[:O], dbeta=sums[O:2 * O], db=sums[2 * O:], dY=ops.lc_rev_sum(b, dx))
        rm, rv = dev(c["rm"]).clone(), dev(c["rv"]).clone()
        tracked = torch.zeros((), dtype=torch.int64, device=DEV)
        if c["training"] and running:
            ops.lc_running(b, x, rm, rv, tracked, R.MOMENTUM)
        res.update(rm=rm, rv=rv, tracked=tracked)
    torch.cuda.synchronize()
    return res


def shaped(c, name, t):
    return t.reshape(c["N"], -1) if name in ("X", "dX") else t


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("O,P,K,n", OP_CASES)
def test_ops_against_float64(O, P, K, n, training):
    c = R.op_case(O, P, K, n, training)
    want, e32, spread = R.op_references(c)
    got = run_ops(c)
    label = "O%d P%d K%d n%d %s" % (O, P, K, n, "train" if training else "eval")
    worst = max(bar(got[k].cpu().numpy().reshape(want[k].shape), want[k], e32[k], "%s %s" % (label, k)) for k in R.OP_NAMES)
    print("%s: worst ratio %.2f, slot-order spread %.2f" % (label, worst, spread))
    assert int(got["tracked"]) == (n if training else 0)
    again = run_ops(c)
    for k in got:
        assert torch.equal(got[k], again[k]), k  # bit for bit


def running_rows(n, loud):
    """X (n, 6, 19) N(0, 1); ``loud``: the sites further back than LOUD_FROM from the last times LOUD."""
    rng = np.random.RandomState(n + int(loud))
    x = rng.normal(0, 1, (n, 6, 19))
    if loud:
        x[:max(n - LOUD_FROM, 0)] *= LOUD
    return x.astype(np.float32)


def running_start(n):
    """rm0, rv0 (19,): sizes from 1 to 1e30, both signs for the mean."""
    rng = np.random.RandomState(3 * n)
    size = 10.0 ** rng.uniform(0, 30, (2, 19))
    size[:, 0] = 1e30
    return (size[0] * rng.choice([-1.0, 1.0], 19)).astype(np.float32), size[1].astype(np.float32)


@pytest.mark.parametrize("loud", [False, True], ids=["plain", "loud"])
@pytest.mark.parametrize("n", CUT_SITES)
def test_running_statistics_at_the_window(n, loud):
    """lc_running alone against the N sequential updates it replaces, either side of its window of 2048 sites."""
    c = R.op_case(19, 6, 3, n, True)
    b = tiled_batch(c, 1, DEV)
    x = running_rows(n, loud)
    rm0, rv0 = running_start(n)
    worst = 0.0
    for m in MOMENTA:
        want = R.running_ref(x, rm0, rv0, m, torch.float64)
        f32 = R.running_ref(x, rm0, rv0, m, torch.float32)
        rm, rv = dev(rm0).clone(), dev(rv0).clone()
        tracked = torch.full((), 5, dtype=torch.int64, device=DEV)
        ops.lc_running(b, dev(x), rm, rv, tracked, m)
        assert int(tracked) == 5 + n
        for name, got, w, f in (("rm", rm, want[0], f32[0]), ("rv", rv, want[1], f32[1])):
            w = w.numpy()
            e32 = float(np.max(np.abs(f.double().numpy() - w)))
            worst = max(worst, bar(got.cpu().numpy(), w, e32, "n%d %s momentum %g %s" % (n, "loud" if loud else "plain", m, name)))
    print("n%d %s: worst ratio %.2f" % (n, "loud" if loud else "plain", worst))


def padded(a, ld, col0):
    """``a`` as the columns [col0, col0 + width) of a NaN matrix with ``ld`` columns."""
    a = dev(a)
    t = torch.full((a.shape[0], ld), NAN, dtype=torch.float32, device=DEV)
    t[:, col0:col0 + a.shape[1]] = a
    return t[:, col0:col0 + a.shape[1]]


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("O,P,K,n", [(19, 6, 3, 257), (63, 3, 3, 20), (64, 2, 8, 4097)])
def test_views_and_optional_arguments(O, P, K, n, training):
    c = R.op_case(O, P, K, n, training)
    b = tiled_batch(c, 1, DEV)
    dense = run_ops(c, b)
    # ldy = K O + 5 from column 3, lddo = O + 3 from column 1
    views = run_ops(c, b, y=padded(c["Y"], K * O + 5, 3), cot=padded(c["cot"], O + 3, 1))
    for k in dense:
        assert torch.equal(dense[k], views[k]), "padded views: %s differs" % k
    assert torch.equal(run_ops(c, b, want_x=False)["out"], dense["out"])
    ones = dict(c, mask=np.ones_like(c["mask"]))
    zero = dict(c, b=np.zeros_like(c["b"]))
    for what, with_it, without in (("mask", run_ops(ones, b), run_ops(c, b, mask=None)),
                                   ("bias", run_ops(zero, b), run_ops(c, b, bias=None))):
        for k in with_it:
            assert torch.equal(with_it[k], without[k]), "%s = None: %s differs" % (what, k)
        assert not bool(torch.isnan(without["out"]).any())


def test_tiling_past_the_grid_cap():
    """Nine copies of a case in one batch: every per-site result of every copy has the single copy's bits."""
    c = R.op_case(*TILED_CASE, True)
    one = run_ops(c, running=False)
    b = tiled_batch(c, COPIES, DEV)
    n = c["N"]
    assert b.n_sites == COPIES * n == 36873 and -(-b.n_sites // (256 // c["O"])) > 8192
    many = run_ops(c, b, copies=COPIES, running=False)
    for k in ("out", "X", "dX", "dY"):
        rows = many[k].reshape(COPIES, *one[k].shape)
        for i in range(COPIES):
            assert torch.equal(rows[i], one[k]), "%s of copy %d" % (k, i)
