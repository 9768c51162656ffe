"""The Weave kernels (csrc/weave.hip) at their block seams, widths and dispatch edges, every case against a FLOAT64
restatement written here from the kernels' header comments.

Tolerances (none of them is tuned against a kernel's output):

* Sums and products (weave_pair_to_atom, weave_pair_features, fold_affine, weave_gather without the expansion):
  per element ``|got - ref| <= (n_terms + 2) * eps32 * sum|terms|`` with ``sum|terms|`` from the float64 restatement
  run on the absolute values of its inputs (relu of a non-negative sum is the sum) and eps32 = 2^-23.  n_terms:
  ``fp + 1 + pairs`` per atom for pair_to_atom (a product of fp terms plus the bias per pair, then the pairs added
  up, in partial sums that the atomics add in any order: a chain of at most ``pairs`` additions), 6 for an atom-pair column of pair_features
  (two three-term sums and their sum), ``fp + 1`` for a pair-pair column, 2 for fold_affine, the atoms of the
  molecule for the plain gather.
* expf / tanhf kernels (the Gaussian histogram of weave_gather, tanh_): the same formula is run on the CPU in torch
  float32 on the test's own inputs; ``E`` is its largest error over ALL cases of the family, relative to
  ``max(|ref|, 1)`` per element, and the kernel gets ``max(4 E, 8 eps32) * max(|ref|, 1)`` per element.  Measured on
  the CPU (``oracle.edge_checks.family_error`` of the cases below):

      family              E (float32 CPU vs float64)    allowed = max(4 E, 8 eps32)
      Gaussian histogram  1.41e-07                      9.54e-07   (the floor)
      tanh_               3.00e-08                      9.54e-07   (the floor)

  The restatement of the histogram uses the kernel's float32 bin centres and widths (as float64 numbers).

gcmi_weave_pair_features picks the quad kernel when ``HT % 4 == 0, HT / 4 <= 256, fp <= 16, lduv % 4 == 0,
ldz % 4 == 0`` and u, v, z are 16-byte aligned (HT = H + H2), the per-column kernel otherwise; ``selects_quad``
restates that condition on the tensors each case passes and the case asserts the route it is meant for.
"""
import functools

import numpy as np
import pytest
import torch

from oracle.edge_checks import DEV, EPS32, allowed, assert_close, assert_outside_untouched, assert_sum_bound
from oracle.edge_checks import to_dev as _dev
from oracle.edge_checks import to_np as _np
from oracle.edge_checks import wide as _wide

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ pair_to_atom
def pair_to_atom_ref(pf, pair_src, n_atoms, w, b):
    """out[a, h] = sum over the pairs p of source atom a of relu(pf[p, :] . w[:, h] + b[h])."""
    v = np.asarray(pf, np.float64) @ np.asarray(w, np.float64) + (0.0 if b is None else np.asarray(b, np.float64))
    out = np.zeros((n_atoms, w.shape[1]))
    np.add.at(out, np.asarray(pair_src, np.int64), np.maximum(v, 0.0))
    return out


def seam_layout(n_pairs, layout):
    """Pairs per atom.  "seams": an atom over the 64-pair seam (60..69), one over the 256-pair seam (250..261), the
    rest in between; "long": one atom that owns the pairs of two whole workgroups (0..511).  Atoms without pairs come
    first, in the middle and last."""
    cuts = [0, 3, 60, 70, 250, 262, 300, n_pairs] if layout == "seams" else [0, 512, n_pairs]
    cuts = sorted({c for c in cuts if c <= n_pairs})
    counts = list(np.diff(cuts))
    return np.array([0] + counts[:2] + [0] + counts[2:] + [0], np.int64)


P2A_CASES = [(P, 50, 14, False, True, "seams") for P in (1, 63, 64, 65, 255, 256, 257, 513)]
P2A_CASES += [(513, 50, 14, False, True, "long"), (0, 50, 14, False, True, "seams")]
P2A_CASES += [(257, H, 14, False, True, "seams") for H in (1, 64, 65, 130)]
P2A_CASES += [(257, 50, fp, False, True, "seams") for fp in (1, 16, 17, 32)]  # <16> up to 16 features, <32> above
P2A_CASES += [(257, 50, 14, True, True, "seams"), (257, 50, 17, True, False, "seams"), (65, 65, 14, False, False, "seams")]


@pytest.mark.parametrize("P,H,fp,sliced,has_b,layout", P2A_CASES)
def test_pair_to_atom(P, H, fp, sliced, has_b, layout):
    """256 pairs per workgroup, 64 per wave: partial sums are flushed by atomics at those seams.  ``sliced``: ldp > fp;
    ``has_b`` False: b = None."""
    from deepchem_amd import ops
    rng = np.random.RandomState(P + 7 * H + 31 * fp)
    counts = seam_layout(P, layout)
    n_atoms = len(counts)
    pair_src = np.repeat(np.arange(n_atoms), counts).astype(np.int32)
    assert len(pair_src) == P
    pf = rng.standard_normal((P, fp)).astype(np.float32)
    w = rng.standard_normal((fp, H)).astype(np.float32)
    b = rng.standard_normal(H).astype(np.float32) if has_b else None
    pf_g = _wide(pf, 1, 2)[0] if sliced else _dev(pf)
    got = ops.weave_pair_to_atom(pf_g, _dev(pair_src), n_atoms, _dev(w), None if b is None else _dev(b))
    ref = pair_to_atom_ref(pf, pair_src, n_atoms, w, b)
    ref_abs = pair_to_atom_ref(np.abs(pf), pair_src, n_atoms, np.abs(w), None if b is None else np.abs(b))
    assert_sum_bound(got, ref, ref_abs, (fp + 1 + counts)[:, None], "pair_to_atom")
    assert not _np(got)[counts == 0].any(), "atoms without pairs must have zero rows"


def test_pair_to_atom_refuses_33_pair_features():
    from deepchem_amd import _lib, ops
    with pytest.raises(_lib.GcmiError):
        ops.weave_pair_to_atom(_dev(np.ones((2, 33), np.float32)), _dev(np.zeros(2, np.int32)), 1,
                               _dev(np.ones((33, 4), np.float32)), _dev(np.ones(4, np.float32)))


# ------------------------------------------------------------------------------------------------ pair_features
def pair_features_ref(u, v, b_ap, pf, w_pp, b_pp, a2p):
    """Z[p] = [relu(U[i] + V[j] + b_ap) + relu(U[j] + V[i] + b_ap) | relu(pf[p] . W_pp + b_pp)], (i, j) = a2p[p]."""
    u, v = np.asarray(u, np.float64), np.asarray(v, np.float64)
    i, j = a2p[:, 0], a2p[:, 1]
    b = 0.0 if b_ap is None else np.asarray(b_ap, np.float64)
    z = np.maximum(u[i] + v[j] + b, 0.0) + np.maximum(u[j] + v[i] + b, 0.0)
    if w_pp is None:
        return z
    t = np.asarray(pf, np.float64) @ np.asarray(w_pp, np.float64) + (0.0 if b_pp is None else np.asarray(b_pp, np.float64))
    return np.concatenate([z, np.maximum(t, 0.0)], 1)


def selects_quad(u, v, z, H, H2, fp):
    from deepchem_amd import ops
    HT = H + H2
    return (HT % 4 == 0 and HT // 4 <= 256 and fp <= 16 and ops._ld(u) % 4 == 0 and ops._ld(z) % 4 == 0 and
            u.data_ptr() % 16 == 0 and v.data_ptr() % 16 == 0 and z.data_ptr() % 16 == 0)


# (H, H2, fp, P, uv right padding, (z left, z right) padding, biases given, the route the case is meant for)
# quad kernel: Q = HT / 4 lanes per pair slot, slots = 256 / Q pair slots per workgroup, two pairs per slot and round
PF_CASES = {
    "quad_50_50": (50, 50, 14, 45, 2, (0, 0), True, True),                 # Q = 25, slots = 10 (lduv 52)
    "quad_26_50_straddling_quad": (26, 50, 14, 45, 2, (0, 0), True, True),  # columns 24..27: two of each group
    "quad_3_1_Q1": (3, 1, 14, 600, 1, (0, 0), True, True),                 # Q = 1, slots = 256: the quad straddles
    "quad_512_512_one_slot_grid_cap": (512, 512, 14, 4099, 0, (0, 0), True, True),  # slots = 1; 2050 > 2048 blocks
    "quad_8_0_no_pair_block": (8, 0, 14, 300, 0, (0, 0), True, True),     # w_pp = None
    "quad_50_50_pairs_19": (50, 50, 14, 19, 2, (0, 0), True, True),        # 2 * slots - 1
    "quad_50_50_pairs_20": (50, 50, 14, 20, 2, (0, 0), True, True),        # 2 * slots
    "quad_50_50_pairs_21": (50, 50, 14, 21, 2, (0, 0), True, True),        # 2 * slots + 1
    "quad_50_50_out_block": (50, 50, 16, 45, 2, (4, 4), True, True),       # aligned block of a wider matrix, ldz 108
    "quad_50_50_no_biases": (50, 50, 1, 45, 2, (0, 0), False, True),
    "column_5_2": (5, 2, 14, 45, 3, (0, 0), True, False),                  # HT % 4 != 0
    "column_5_2_pairs_1": (5, 2, 14, 1, 3, (0, 0), True, False),
    "column_5_2_pairs_3": (5, 2, 14, 3, 3, (0, 0), True, False),
    "column_5_2_pairs_4": (5, 2, 14, 4, 3, (0, 0), True, False),           # four pairs per wave and round
    "column_5_2_pairs_5": (5, 2, 14, 5, 3, (0, 0), True, False),
    "column_516_512": (516, 512, 14, 45, 0, (0, 0), True, False),          # HT / 4 = 257 > 256
    "column_7_0": (7, 0, 14, 45, 1, (0, 0), True, False),                  # w_pp = None, HT % 4 != 0
    "column_fp17": (50, 50, 17, 45, 2, (0, 0), True, False),               # fp > 16: pair_features_kernel<32>
    "column_fp32": (50, 50, 32, 45, 2, (0, 0), False, False),
    "column_out_ldz_103": (50, 50, 14, 45, 2, (0, 3), True, False),        # ldz % 4 != 0
    "column_out_from_column_1": (50, 50, 14, 45, 2, (1, 3), True, False),  # ldz 104, z 4 bytes off
    "column_lduv_50": (50, 50, 14, 45, 0, (0, 0), True, False),            # lduv % 4 != 0
}


@pytest.mark.parametrize("name", sorted(PF_CASES))
def test_pair_features(name):
    from deepchem_amd import ops
    H, H2, fp, P, uv_pad, (z_left, z_right), biases, quad = PF_CASES[name]
    rng = np.random.RandomState(H + 3 * H2 + 11 * fp + P)
    n_atoms = 9
    a2p = rng.randint(0, n_atoms, size=(P, 2)).astype(np.int32)
    a2p[::4, 1] = a2p[::4, 0]  # self pairs
    u, v = (rng.standard_normal((n_atoms, H)).astype(np.float32) for _ in range(2))
    pf = rng.standard_normal((P, fp)).astype(np.float32)
    w_pp = rng.standard_normal((fp, H2)).astype(np.float32) if H2 else None
    b_ap = rng.standard_normal(H).astype(np.float32) if biases else None
    b_pp = rng.standard_normal(H2).astype(np.float32) if biases and H2 else None
    u_g, v_g = (_wide(a, 0, uv_pad)[0] if uv_pad else _dev(a) for a in (u, v))
    HT = H + H2
    z_g, z_wide = _wide(np.zeros((P, HT), np.float32), z_left, z_right) if z_left + z_right else (None, None)
    dev = lambda a: None if a is None else _dev(a)
    probe = z_g if z_g is not None else torch.empty((P, HT), dtype=torch.float32, device=DEV)
    assert selects_quad(u_g, v_g, probe, H, H2, fp) == quad
    got = ops.weave_pair_features(u_g, v_g, dev(b_ap), _dev(pf), dev(w_pp), dev(b_pp), _dev(a2p), out=z_g)
    absq = lambda a: None if a is None else np.abs(a)
    ref = pair_features_ref(u, v, b_ap, pf, w_pp, b_pp, a2p)
    ref_abs = pair_features_ref(np.abs(u), np.abs(v), absq(b_ap), np.abs(pf), absq(w_pp), absq(b_pp), a2p)
    n_terms = np.concatenate([np.full(H, 6), np.full(H2, fp + 1)])[None, :]
    assert_sum_bound(got, ref, ref_abs, n_terms, name)
    if z_wide is not None:
        assert got.data_ptr() == z_g.data_ptr()
        assert_outside_untouched(z_wide, z_left, HT, name)


# ------------------------------------------------------------------------------------------------ weave_gather
GAUSS_MU = np.array([-1.645, -1.080, -0.739, -0.468, -0.228, 0., 0.228, 0.468, 0.739, 1.080, 1.645], np.float32)
GAUSS_SIGMA = np.array([0.283, 0.170, 0.134, 0.118, 0.114, 0.114, 0.114, 0.118, 0.134, 0.170, 0.283], np.float32)
GATHER_SIZES = (0, 1, 2, 3, 0, 3, 5, 0)  # 14 atoms: at one feature still the 11 centres, -4 and 4


def histogram_formula(x, mol_ptr, dtype):
    """out[m, f * 11 + k] = sum over the atoms a of m of g_k(x[a, f]) / sum_k' g_k'(x[a, f]),
    g_k(x) = exp(-(x - mu_k)^2 / (2 sigma_k^2)), in ``dtype`` with the float32 constants of the kernel."""
    x = torch.from_numpy(x).to(dtype)
    mu, sigma = torch.from_numpy(GAUSS_MU).to(dtype), torch.from_numpy(GAUSS_SIGMA).to(dtype)
    inv2var = 1.0 / (2.0 * sigma * sigma)
    dlt = x[:, :, None] - mu
    g = torch.exp(-(dlt * dlt) * inv2var)
    total = g.sum(-1, keepdim=True)
    hist = (g / total).reshape(x.shape[0], -1)
    rows = [hist[int(mol_ptr[m]):int(mol_ptr[m + 1])].sum(0) for m in range(len(mol_ptr) - 1)]
    return torch.stack(rows).double().numpy(), total.double().numpy()


class GatherCase:
    def __init__(self, F):
        rng = np.random.RandomState(F)
        self.F = F
        self.mol_ptr = np.concatenate([[0], np.cumsum(GATHER_SIZES)]).astype(np.int32)
        n = int(self.mol_ptr[-1])
        x = rng.uniform(-4.0, 4.0, size=(n, F)).astype(np.float32)
        flat = x.reshape(-1)
        k = min(flat.size, 11 + 2)
        flat[:k] = np.concatenate([GAUSS_MU, [-4.0, 4.0]])[:k]  # the bin centres and both ends of the range
        self.x = x

    def cpu(self, dtype):
        return [histogram_formula(self.x, self.mol_ptr, dtype)[0]]


GATHER_CASES = {F: GatherCase(F) for F in (1, 64, 65, 130)}
TANH_X = np.concatenate([np.random.RandomState(3).standard_normal(7 * 13 - 8) * 2,
                         [0.0, 1e-4, -1e-4, 30.0, -30.0, 100.0, -100.0, 9.0]]).astype(np.float32).reshape(7, 13)


class TanhCase:
    def cpu(self, dtype):
        return [torch.tanh(torch.from_numpy(TANH_X).to(dtype)).double().numpy()]


@functools.lru_cache(maxsize=None)
def _allowed(family):
    return allowed(list(GATHER_CASES.values()) if family == "gauss" else [TanhCase()])[0]


@pytest.mark.parametrize("F", sorted(GATHER_CASES))
def test_gather_gaussian_histogram(F):
    from deepchem_amd import ops
    case = GATHER_CASES[F]
    ref, total = histogram_formula(case.x, case.mol_ptr, torch.float64)
    # the reference itself is well inside the representable range (smallest bin total ~1e-15 at |x| = 4): the
    # underflow region, where the normalisation is 0 / 0, belongs to test_large_batch_against_oracle
    assert not np.isnan(ref).any() and float(total.min()) >= 1e-16
    got = ops.weave_gather(_wide(case.x, 1, 2)[0], _dev(case.mol_ptr), True)
    assert_close(got, ref, _allowed("gauss"), "weave_gather F=%d" % F)
    empty = np.diff(case.mol_ptr) == 0
    assert not _np(got)[empty].any()


@pytest.mark.parametrize("F", sorted(GATHER_CASES))
def test_gather_plain_sum(F):
    from deepchem_amd import ops
    case = GATHER_CASES[F]
    x64, ptr = case.x.astype(np.float64), case.mol_ptr
    seg = lambda a: np.stack([a[ptr[m]:ptr[m + 1]].sum(0) for m in range(len(ptr) - 1)])
    got = ops.weave_gather(_wide(case.x, 1, 2)[0], _dev(ptr), False)
    assert_sum_bound(got, seg(x64), seg(np.abs(x64)), np.diff(ptr).astype(np.int64)[:, None], "plain gather F=%d" % F)


# ------------------------------------------------------------------------------------------------ fold_affine, tanh_
@pytest.mark.parametrize("absent", [None, "b", "scale", "shift"])
@pytest.mark.parametrize("trans", [False, True])
@pytest.mark.parametrize("K,n", [(1, 1), (3, 257), (257, 3)])
def test_fold_affine(K, n, trans, absent):
    """(W diag(scale), b scale + shift); W is (K, n), or (n, K) when ``trans``."""
    from deepchem_amd import ops
    rng = np.random.RandomState(K + 5 * n)
    w = rng.standard_normal((n, K) if trans else (K, n)).astype(np.float32)
    vec = {k: (None if k == absent else rng.standard_normal(n).astype(np.float32)) for k in ("b", "scale", "shift")}
    dev = lambda a: None if a is None else _dev(a)
    w_out, b_out = ops.fold_affine(_dev(w), dev(vec["b"]), dev(vec["scale"]), dev(vec["shift"]), trans)

    def ref(w, b, scale, shift):
        s = np.ones(n) if scale is None else scale.astype(np.float64)
        bb = np.zeros(n) if b is None else b.astype(np.float64)
        sh = np.zeros(n) if shift is None else shift.astype(np.float64)
        return w.astype(np.float64) * (s[:, None] if trans else s[None, :]), bb * s + sh

    absq = lambda a: None if a is None else np.abs(a)
    (rw, rb), (aw, ab) = ref(w, **vec), ref(np.abs(w), **{k: absq(a) for k, a in vec.items()})
    assert_sum_bound(w_out, rw, aw, 2, "fold_affine w")
    assert_sum_bound(b_out, rb, ab, 2, "fold_affine b")


def test_tanh_on_a_column_slice():
    from deepchem_amd import ops
    x, wide = _wide(TANH_X, 2, 1)
    out = ops.tanh_(x)
    assert out.data_ptr() == x.data_ptr()
    assert_close(x, TanhCase().cpu(torch.float64)[0], _allowed("tanh"), "tanh_")
    assert_outside_untouched(wide, 2, TANH_X.shape[1], "tanh_")
