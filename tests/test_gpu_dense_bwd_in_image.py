"""The prepared In image of the dense fp32 backward (csrc/bwd_fused.hip, fused_bwd_kernel<128, 2, 1, T, T, T>): phase (a)
transposes the pooled rows across the lanes of a wave, splits them once per tile and stores the three bf16 pieces as
[piece][column][row] in LDS; the four weight-gradient waves read their In fragments from there.  Everything goes
through ``ops.fused_dense_bwd`` with the builders of tests/test_gpu_fused_edges.py (NaN outside the tile, sentinels,
two launches for the two sweep directions) and every assertion is ``np.array_equal`` against float64:

  * ADDRESS PROBE.  G has a single 1 at (r*, c*): coef = (1, 0, 0), gc = 1 everywhere, dsum = 0 and dmax one-hot with
    arg naming r* (one molecule per row).  In[r][c] = (128 + r mod 128) 2^(c - 32): the seven mantissa bits below the leading
    one name the row, the exponent the column, and the value is ONE bf16 piece, so dW[c*][:] = In[r*][:k] whichever
    image entry the wave read -- a wrong row, column, lane row, half of an 8-row entry or k-step shows as another
    value.  r* over both passes of phase (a) (rows < 32 / >= 32), all four lane rows (r* mod 4), both halves of an entry
    (r* mod 8 < 4 / >= 4) and every 16-row k-step, in two tiles; c* in both halves of every 32-column group of G.
  * RAGGED TILES, integer data: 64 + v rows (v = 1 .. 9, 63) and v rows alone (1, 2, 7, 8): ``valid`` inside an
    8-row entry, on its edge, odd and even.
  * WIDTHS (k, ld) = (40, 44), (60, 64), (60, 68) besides those of BWD_INT: masked columns inside a 32-column group.
  * THREE-PIECE In: +-(1 + 2^-9 + 2^-17) against G from {-1, 0, 1} over one tile: every product is exact and every
    partial sum of at most 64 of them (and of the multiples of 1/4 dW starts from) is a multiple of 2^-17 below 128,
    a float32 number: dW is exact only if all three pieces of In arrive, each in its place.
  * IMAGE OVERWRITTEN: 2 x 256 + 1 tiles and five rows (integer data, random per tile): one workgroup walks three
    tiles and rewrites the image between them.
"""
import numpy as np
import pytest

from tests import edge_refs as R
from tests.test_gpu_fused_edges import _b, _check_bwd_exact, _launch_bwd, build_bwd, bwd_ref

pytestmark = pytest.mark.gpu

W = 128
PROBE_ROWS = tuple(t + r for t in (0, 64) for r in (0, 1, 3, 4, 7, 8, 15, 16, 31, 32, 35, 36, 63))
PROBE_COLS = (0, 31, 32, 127)


def _probe_case(k):
    """The parts of an address probe that do not depend on (r*, c*)."""
    d = build_bwd(_b("bd_f", rows=128, k=k, psums=False, seed=k))
    n = d["n"]
    r, c = np.arange(n)[:, None], np.arange(k)[None, :]
    d["ins"] = [((128 + r % 128) * 2.0 ** (c - 32)).astype(np.float32)]
    assert np.array_equal(R.bf16_round(d["ins"][0]), d["ins"][0]), "the probe values must be one bf16 piece"
    d["gc"] = np.ones((n, W), np.float32)
    d["coef"] = np.concatenate([np.ones(W), np.zeros(2 * W)]).astype(np.float32)
    d["membership"] = np.arange(n, dtype=np.int32)
    d["dw0"], d["db0"] = np.zeros_like(d["dw0"]), np.zeros_like(d["db0"])
    return d


@pytest.mark.parametrize("cstar", PROBE_COLS)
@pytest.mark.parametrize("k", (64, 36))
def test_address_probe(k, cstar):
    d = _probe_case(k)
    n = d["n"]
    for rstar in PROBE_ROWS:
        d["g2"] = np.zeros((n, 2 * W), np.float32)
        d["g2"][rstar, W + cstar] = 1.0
        d["arg"] = np.full((n, W), -1, np.int32)
        d["arg"][rstar, cstar] = rstar
        d["dy"], d["dy_mag"] = R.readout_dy_ref(d["g2"], d["arg"], d["membership"], W)
        what = "probe k %d, G[%d][%d]" % (k, rstar, cstar)
        for i, g in enumerate(_launch_bwd(d)):
            dw = g["dw"].reshape(W, k)
            assert np.array_equal(dw[cstar], d["ins"][0][rstar, :k].astype(np.float64)), "%s launch %d: dW[c*] is %r" % (
                what, i, dw[cstar])
            assert np.count_nonzero(np.delete(dw, cstar, 0)) == 0, "%s launch %d: dW outside row c*" % (what, i)
        _check_bwd_exact(d, what)


RAGGED = tuple(64 + v for v in (1, 2, 3, 4, 5, 6, 7, 8, 9, 63)) + (1, 2, 7, 8)


@pytest.mark.parametrize("rows", RAGGED)
def test_ragged_tiles(rows):
    _check_bwd_exact(build_bwd(_b("bd_f", rows=rows, seed=100 + rows)), "bd_f rows %d" % rows)


@pytest.mark.parametrize("k,ld", ((40, 44), (60, 64), (60, 68)))
def test_widths(k, ld):
    _check_bwd_exact(build_bwd(_b("bd_f", k=k, ld=ld, seed=k + ld)), "bd_f k %d ld %d" % (k, ld))


def test_three_piece_in():
    d = build_bwd(_b("bd_f", rows=64, psums=False, seed=7))
    rng = np.random.default_rng(7)
    n = d["n"]
    v = np.float32(1.0 + 2.0 ** -9 + 2.0 ** -17)
    p1, p2, p3 = (float(p[0]) for p in R.split3_np(np.array([v], np.float32)))
    assert p2 != 0 and p3 != 0 and p1 + p2 + p3 == float(v), "the value must need exactly three pieces"
    d["ins"] = [(rng.choice(np.array([-1.0, 1.0], np.float32), (n, d["k"])) * v).astype(np.float32)]
    d["g2"][:, W:] = 0.0  # dy = dsum, from {-1, 0, 1}
    d["gc"] = rng.choice(np.array([-0.5, 0.0, 0.5, 1.0], np.float32), (n, W))
    d["coef"] = np.concatenate([np.ones(W), np.zeros(2 * W)]).astype(np.float32)
    d["dy"], d["dy_mag"] = R.readout_dy_ref(d["g2"], d["arg"], d["membership"], W)
    G = bwd_ref(d)["G"][:64]
    assert set(np.unique(G)) == {-1.0, 0.0, 1.0}
    _check_bwd_exact(d, "three-piece In")


def test_image_overwritten_between_tiles():
    rows = 64 * (2 * 256 + 1) + 5
    _check_bwd_exact(build_bwd(_b("bd_f", rows=rows, seed=11)), "bd_f %d rows" % rows)
