"""The MPNN kernels (csrc/mpnn.hip) and their autograd Functions (models/torch_models/mpnn.py) at the widths, pair
counts and dispatch edges where they take another path, every case against a FLOAT64 restatement written here from
the kernels' header comments; gradients from torch float64 autograd of that restatement.

Tolerances (none of them is tuned against a kernel's output):

* Sums and products (moments, edge_network_sum, EdgeNetwork, EdgeNetworkFn): per element
  ``|got - ref| <= (n_terms + 2) * eps32 * sum|terms|`` with ``sum|terms|`` from the float64 restatement run on the
  absolute values of its inputs and ``n_terms`` the length of the longest chain of additions behind the element
  (pairs of the atom for the moments, (K + 1) * pairs for edge_network_sum, d + (K + 1) * pairs through the layer,
  per output for the two chained EdgeNetworkFn rounds and their gradients, written out in that test).  eps32 = 2^-23.
  The matrix products of those cases run in the exact-fp32 GEMM mode, for which the bound holds.
* expf / tanhf kernels (GRU, LSTM, set2set): the same formula is run on the CPU in torch float32 on the test's own
  inputs; ``E`` is its largest error over ALL cases of the family, per output and relative to ``max(|ref|, 1)`` per
  element.  The kernel gets ``max(4 E, 8 eps32) * max(|ref|, 1)`` per element.  Measured on the CPU
  (``oracle.edge_checks.family_error`` of the case tables below; the largest output of each family):

      family, output             E (float32 CPU vs float64)    allowed = max(4 E, 8 eps32)
      GRU, all nine outputs      <= 2.21e-07                   9.54e-07   (the floor)
      LSTM, all four outputs     <= 2.09e-07                   9.54e-07   (the floor)
      set2set, logits ~1     q   6.53e-07                      2.61e-06
                             dx  1.00e-06                      4.02e-06
                             dh  5.81e-06                      2.33e-05
      set2set, logits ~+-200 q   1.92e-07                      9.54e-07   (the floor)
                             dx  3.58e-05                      1.43e-04
                             dh  4.71e-04                      1.88e-03

  The large-logit set2set inputs are a family of their own.  They are built from multiples of 1/4 times +-4 so that
  every logit is an integer computed exactly in float32 in any order; what float32 loses there is dh: de_a =
  w_a (dw_a - sum_b w_b dw_b) cancels two numbers of order 50 for the dominating atom and is multiplied by x ~ 50
  again (4.7e-4 in the F = 65 case, 1.3e-4 at F = 1, below 3e-5 elsewhere).  Results must also be finite.

The molecule-staged moments kernel is forced with GCMI_EDGE_MOMENTS_MOL=1, read once per process: its cases run in
ONE child process, the automatic switch-over (n_dst = 98 304) in a second one with the variable unset.
"""
import functools
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle.edge_checks import DEV, allowed, assert_close, assert_outside_untouched, assert_sum_bound, wide
from oracle.edge_checks import to_dev as _dev
from oracle.edge_checks import to_np as _np

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPECIALS = (30.0, -30.0, 100.0, -100.0)


# ------------------------------------------------------------------------------------------------ helpers
def _wide(a, left=2, right=3, grad=False):
    return wide(a, left, right, grad)


def _grads(outs, cots, leaves):
    """float64 numpy [outs..., d leaves...] of L = sum_k <out_k, cot_k> (a None cotangent: that output is unused)."""
    loss = sum((o * c).sum() for o, c in zip(outs, cots) if c is not None)
    gs = torch.autograd.grad(loss, leaves, allow_unused=True)
    return [_np(o) for o in outs] + [np.zeros(tuple(l.shape)) if g is None else _np(g) for l, g in zip(leaves, gs)]


def pair_list(rng, counts, n_src):
    counts = np.asarray(counts, np.int64)
    dst_ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    src = rng.randint(0, n_src, size=int(dst_ptr[-1])).astype(np.int32)
    return dst_ptr, src


# ------------------------------------------------------------------------------------------------ moments
def moments_ref(h, pf, dst_ptr, src):
    """T[i] = [sum_p pf[p, 0] h[src_p] | ... | sum_p pf[p, K-1] h[src_p] | sum_p h[src_p]] over the pairs of atom i."""
    h, pf = np.asarray(h, np.float64), np.asarray(pf, np.float64)
    n_dst, d, K = len(dst_ptr) - 1, h.shape[1], pf.shape[1]
    hs = h[np.asarray(src, np.int64)]
    contrib = np.concatenate([pf[:, :, None] * hs[:, None, :], hs[:, None, :]], axis=1).reshape(len(src), (K + 1) * d)
    T = np.zeros((n_dst, (K + 1) * d))
    np.add.at(T, np.repeat(np.arange(n_dst), np.diff(dst_ptr)), contrib)
    return T


def check_moments(got, h, pf, dst_ptr, src, what):
    counts = np.diff(dst_ptr).astype(np.int64)
    ref, ref_abs = moments_ref(h, pf, dst_ptr, src), moments_ref(np.abs(h), np.abs(pf), dst_ptr, src)
    assert_sum_bound(got, ref, ref_abs, counts[:, None], what)
    assert not _np(got)[counts == 0].any(), what + ": atoms without pairs must have zero rows"


# (0, 1, 2, 3 pairs: the two-per-round tail; a first, a middle and a trailing atom without pairs)
PER_ATOM_COUNTS = (0, 1, 2, 3, 0, 5, 4, 3, 0)


@pytest.mark.parametrize("sliced", [False, True])
@pytest.mark.parametrize("d,K", [(1, 1), (63, 7), (64, 8), (65, 9), (100, 8), (127, 15), (128, 16)])
def test_moments_per_atom_kernel(d, K, sliced):
    """edge_moments_kernel<16, 1> (d <= 64) and <16, 2>; ``sliced``: h and pair_feat are column slices (ld > cols)."""
    from deepchem_amd import ops
    rng = np.random.RandomState(1000 * d + K)
    n_src = 11
    dst_ptr, src = pair_list(rng, PER_ATOM_COUNTS, n_src)
    h = rng.standard_normal((n_src, d)).astype(np.float32)
    pf = rng.standard_normal((len(src), K)).astype(np.float32)
    h_g, pf_g = (_wide(h)[0], _wide(pf, 1, 2)[0]) if sliced else (_dev(h), _dev(pf))
    got = ops.edge_network_moments(h_g, pf_g, _dev(dst_ptr), _dev(src))
    check_moments(got, h, pf, dst_ptr, src, "moments d=%d K=%d" % (d, K))


def test_moments_refusals_and_empty_batch():
    from deepchem_amd import _lib, ops
    rng = np.random.RandomState(5)
    dst_ptr, src = pair_list(rng, (1, 2), 2)
    for d, K in ((129, 8), (8, 17)):
        with pytest.raises(_lib.GcmiError):
            ops.edge_network_moments(_dev(np.ones((2, d), np.float32)), _dev(np.ones((3, K), np.float32)), _dev(dst_ptr),
                                     _dev(src))
    t = ops.edge_network_moments(_dev(np.ones((2, 8), np.float32)), _dev(np.zeros((0, 3), np.float32)),
                                 _dev(np.zeros(1, np.int32)), _dev(np.zeros(0, np.int32)))
    assert tuple(t.shape) == (0, 32)


# ---- the molecule-staged kernel: the cases below run inside a child process (see _mol_child)
def _mol_batch(rng, sizes, per_atom_counts, d, K, leave_every=5):
    """Atoms grouped in molecules of ``sizes``; atom a gets per_atom_counts[a % len] pairs whose sources lie in its
    own molecule, except every ``leave_every``-th pair, whose source is any atom of the batch."""
    mol_ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    n = int(mol_ptr[-1])
    counts = np.array([per_atom_counts[a % len(per_atom_counts)] for a in range(n)], np.int64)
    dst_ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    mol_of = np.repeat(np.arange(len(sizes)), sizes)
    owner = np.repeat(np.arange(n), counts)
    lo, size = mol_ptr[:-1][mol_of[owner]], np.asarray(sizes)[mol_of[owner]]
    src = lo + (rng.randint(0, 1 << 30, size=len(owner)) % size)
    if leave_every:
        out = np.arange(len(owner)) % leave_every == leave_every - 1
        src[out] = rng.randint(0, n, size=int(out.sum()))
    h = rng.standard_normal((n, d)).astype(np.float32)
    pf = rng.standard_normal((len(src), K)).astype(np.float32)
    return mol_ptr, dst_ptr, src.astype(np.int32), h, pf


def _mol_run(ops, batch, max_mol_atoms, what, ld_pad=0):
    mol_ptr, dst_ptr, src, h, pf = batch
    h_g = _wide(h, 0, ld_pad)[0] if ld_pad else _dev(h)
    got = ops.edge_network_moments(h_g, _dev(pf), _dev(dst_ptr), _dev(src), _dev(mol_ptr), max_mol_atoms)
    check_moments(got, h, pf, dst_ptr, src, "%s max_mol_atoms=%d" % (what, max_mol_atoms))


def _mol_child(which):
    from deepchem_amd import _lib, ops
    rng = np.random.RandomState(7)
    n_cases = 0
    if which == "forced":
        assert os.environ.get("GCMI_EDGE_MOMENTS_MOL") == "1"
        # <8, 1>, <8, 2>, <16, 1>, <16, 2>; d = 75 (d % 4) and ldh = 101 (ldh % 4) read the rows from memory, unstaged
        for K, d, ld_pad in ((8, 64, 0), (8, 100, 0), (14, 64, 0), (9, 128, 0), (8, 75, 0), (8, 100, 1)):
            ppr = 8 if K <= 8 else 4  # pairs per round of the kernel: 64 / KP
            sizes = [0, 3, 12, 0, 1, 9, 0]  # empty molecules first, in the middle and last
            batch = _mol_batch(rng, sizes, (ppr - 1, ppr, ppr + 1, 0, 1, 2 * ppr + 1), d, K)
            # 0: the fixed 48 KB; 12: the true maximum; 5: understated, the 9- and 12-atom molecules go unstaged
            for mm in (0, 12, 5):
                _mol_run(ops, batch, mm, "mol K=%d d=%d ldh=%d" % (K, d, d + ld_pad), ld_pad)
                n_cases += 1
        # 97 atoms x 128 floats = 12 416 > 12 288: too large for LDS whatever the host says; a sparse pair list
        batch = _mol_batch(rng, [97, 3], (3, 2, 4, 0), 128, 3)
        for mm in (0, 97):
            _mol_run(ops, batch, mm, "mol 97 atoms d=128")
            n_cases += 1
        # 32 768 molecules > the 8 192-workgroup grid: the molecule loop strides (with its barrier) four times
        batch = _mol_batch(rng, [3] * 32768, (1, 2, 3), 8, 2, leave_every=0)
        _mol_run(ops, batch, 3, "mol 32768 molecules")
        n_cases += 1
        # a state matrix that is not 16-byte aligned with d % 4 == 0 and ldh % 4 == 0: refused before any launch
        mol_ptr, dst_ptr, src, h, pf = _mol_batch(rng, [3, 2], (1, 2), 64, 8)
        buf = torch.zeros(5 * 64 + 4, dtype=torch.float32, device=DEV)
        h_off = buf[1:1 + 5 * 64].view(5, 64)
        assert h_off.data_ptr() % 16 == 4
        try:
            ops.edge_network_moments(h_off, _dev(pf), _dev(dst_ptr), _dev(src), _dev(mol_ptr), 3)
        except _lib.GcmiError:
            n_cases += 1
        else:
            raise AssertionError("a misaligned state matrix was accepted")
    else:
        assert "GCMI_EDGE_MOMENTS_MOL" not in os.environ
        # n_dst = 98 301: the per-atom kernel; 98 304 = 96 * 1024: the automatic switch to the molecule kernel
        for n_mols in (32767, 32768):
            batch = _mol_batch(rng, [3] * n_mols, (1, 2, 3), 8, 2, leave_every=0)
            _mol_run(ops, batch, 3, "auto n_dst=%d" % (3 * n_mols))
            n_cases += 1
    torch.cuda.synchronize()
    print("ok %d" % n_cases)


def _run_child(which, env):
    code = "from tests.test_gpu_mpnn_edges import _mol_child; _mol_child(%r)" % which
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=240, cwd=ROOT)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    return out.stdout.strip().splitlines()[-1]


def test_moments_molecule_kernel_against_float64():
    assert "ok 22" == _run_child("forced", dict(os.environ, GCMI_EDGE_MOMENTS_MOL="1"))


def test_moments_automatic_switch_over_against_float64():
    env = {k: v for k, v in os.environ.items() if k != "GCMI_EDGE_MOMENTS_MOL"}
    assert "ok 2" == _run_child("auto", env)


# ------------------------------------------------------------------------------------------------ edge_network_sum
def edge_sum_ref(g, d, pf, dst_ptr, src):
    """out[i, r] = sum over the pairs p of i of (sum_k pf[p, k] G[src_p][k d + r] + G[src_p][K d + r])."""
    g, pf = np.asarray(g, np.float64), np.asarray(pf, np.float64)
    K, n_dst = pf.shape[1], len(dst_ptr) - 1
    G = g[np.asarray(src, np.int64)].reshape(len(src), K + 1, d)
    msg = (pf[:, :, None] * G[:, :K]).sum(1) + G[:, K]
    out = np.zeros((n_dst, d))
    np.add.at(out, np.repeat(np.arange(n_dst), np.diff(dst_ptr)), msg)
    return out


@pytest.mark.parametrize("d,K", [(129, 2), (8, 17), (8, 32)])
def test_edge_network_sum_kernel(d, K):
    from deepchem_amd import ops
    rng = np.random.RandomState(100 * d + K)
    n_src = 11
    dst_ptr, src = pair_list(rng, PER_ATOM_COUNTS, n_src)
    g = rng.standard_normal((n_src, (K + 1) * d)).astype(np.float32)
    pf = rng.standard_normal((len(src), K)).astype(np.float32)
    got = ops.edge_network_sum(_wide(g)[0], d, _wide(pf, 1, 2)[0], _dev(dst_ptr), _dev(src))
    counts = np.diff(dst_ptr).astype(np.int64)
    assert_sum_bound(got, edge_sum_ref(g, d, pf, dst_ptr, src), edge_sum_ref(np.abs(g), d, np.abs(pf), dst_ptr, src),
                     (counts * (K + 1))[:, None], "edge_network_sum d=%d K=%d" % (d, K))
    assert not _np(got)[counts == 0].any()


def test_edge_network_sum_refuses_33_pair_features():
    from deepchem_amd import _lib, ops
    dst_ptr, src = pair_list(np.random.RandomState(0), (1, 2), 2)
    with pytest.raises(_lib.GcmiError):
        ops.edge_network_sum(_dev(np.ones((2, 34 * 4), np.float32)), 4, _dev(np.ones((3, 33), np.float32)), _dev(dst_ptr),
                             _dev(src))


def edge_network_formula(h, W, b, pf, dst, src, n, d):
    """m_i = sum over the pairs (i, j) of reshape(pf_ij . W + b, (d, d)) h_j (any torch dtype, differentiable)."""
    A = (pf @ W + b).reshape(pf.shape[0], d, d)
    msg = torch.matmul(A, h[src].unsqueeze(2)).squeeze(2)
    return torch.zeros((n, d), dtype=h.dtype).index_add(0, dst, msg)


@pytest.mark.parametrize("d,K", [(130, 3), (8, 17)])
def test_edge_network_layer_takes_the_sum_route(d, K):
    """EdgeNetwork with d > 128 or K > 16: G = h . [W_k^T | B^T] by GEMM, then edge_network_sum."""
    import deepchem_amd as dc
    from deepchem_amd.models.torch_models.layers import EdgeNetwork
    rng = np.random.RandomState(10 * d + K)
    counts = np.array((0, 1, 2, 3, 0, 4, 1))  # (the layer returns rows up to the last atom that has a pair)
    n = len(counts)
    dst_ptr, src = pair_list(rng, counts, n)
    dst = np.repeat(np.arange(n), counts)
    h = rng.standard_normal((n, d)).astype(np.float32)
    pf = rng.standard_normal((len(src), K)).astype(np.float32)
    W = (rng.standard_normal((K, d * d)) / d).astype(np.float32)
    b = (rng.standard_normal(d * d) / d).astype(np.float32)
    layer = EdgeNetwork(K, d)
    layer.W, layer.b = torch.from_numpy(W), torch.from_numpy(b)
    dc.set_gemm_mode("exact")
    try:
        got = layer([pf, h, np.stack([dst, src], 1)])
    finally:
        dc.set_gemm_mode("fast")
    t64 = lambda a: torch.from_numpy(np.asarray(a, np.float64))
    idx = (torch.from_numpy(dst).long(), torch.from_numpy(src).long())
    ref = edge_network_formula(t64(h), t64(W), t64(b), t64(pf), idx[0], idx[1], n, d).numpy()
    ref_abs = edge_network_formula(t64(np.abs(h)), t64(np.abs(W)), t64(np.abs(b)), t64(np.abs(pf)), idx[0], idx[1], n,
                                   d).numpy()
    assert_sum_bound(got, ref, ref_abs, (d + (K + 1) * counts)[:, None], "EdgeNetwork d=%d K=%d" % (d, K))


# ------------------------------------------------------------------------------------------------ GRU, LSTM
def _with_specials(a):
    flat = a.reshape(-1)
    idx = np.arange(0, flat.size, 5)
    flat[idx] = np.resize(np.asarray(SPECIALS, np.float32), idx.size)
    return a


class GruCase:
    """GruGatesFn then GruOutFn as the model chains them: (zp, rp, h) -> z, r, hr; out = (1 - z) tanh(hpre) + z x,
    L = <out, g0> + <hr, g1> + <z, g2>.  (r reaches the loss through hr alone: the Function takes no gradient of r.)"""

    def __init__(self, n, special=None):
        rng = np.random.RandomState(n + (0 if special is None else int(special) % 97))
        self.n = n
        self.a = [(2 * rng.standard_normal((1, n))).astype(np.float32) for _ in range(5)]  # zp, rp, h, hpre, x
        self.cots = [rng.standard_normal((1, n)).astype(np.float32) for _ in range(3)]
        for k in (0, 1, 3):  # saturated gates, expf overflow
            if special is None:
                idx = np.arange(k, n, 5)
                self.a[k][0, idx] = np.resize(np.asarray(SPECIALS, np.float32), idx.size)
            else:
                self.a[k][:] = special if k != 1 else -special

    def _chain(self, gates, out_fn, leaves, cots):
        zp, rp, h, hpre, x = leaves
        z, r, hr = gates(zp, rp, h)
        out = out_fn(z, hpre, x)
        return _grads([z, r, hr, out], [cots[2], None, cots[1], cots[0]], leaves)

    def cpu(self, dtype):
        leaves = [torch.from_numpy(a).to(dtype).requires_grad_(True) for a in self.a]
        cots = [torch.from_numpy(c).to(dtype) for c in self.cots]

        def gates(zp, rp, h):
            z, r = torch.sigmoid(zp), torch.sigmoid(rp)
            return z, r, h * r
        return self._chain(gates, lambda z, hpre, x: (1 - z) * torch.tanh(hpre) + z * x, leaves, cots)

    def gpu(self):
        from deepchem_amd.models.torch_models.functions import GruGatesFn, GruOutFn
        leaves = [_dev(a, grad=True) for a in self.a]
        cots = [_dev(c) for c in self.cots]
        # (the gates work in place on their pre-activations: hand them copies, as the model hands them GEMM outputs)
        return self._chain(lambda zp, rp, h: GruGatesFn.apply(zp.clone(), rp.clone(), h), GruOutFn.apply, leaves, cots)


def lstm_formula(z, c, H):
    i, f, o = torch.sigmoid(z[:, :H]), torch.sigmoid(z[:, H:2 * H]), torch.sigmoid(z[:, 2 * H:3 * H])
    c2 = f * c + i * torch.tanh(z[:, 3 * H:4 * H])
    return o * torch.tanh(c2), c2


class LstmCase:
    """LstmCellFn: z (rows, 4H) = [i | f | o | g], c -> h', c'; L = <h', g0> + <c', g1>.
    layout "slice": z is a column block of a wider matrix (ldz > 4H); "tview": a (4H, 1).t() view, one row whose
    row stride is 1; "raw": gcmi_lstm_cell_bwd called directly with ldz > 4H and dc_next = NULL (L = <h', g0>)."""

    def __init__(self, H, rows, layout):
        rng = np.random.RandomState(100 * H + 10 * rows + len(layout))
        self.H, self.rows, self.layout = H, rows, layout
        self.z = _with_specials((2 * rng.standard_normal((rows, 4 * H))).astype(np.float32))
        self.c = rng.standard_normal((rows, H)).astype(np.float32)
        self.cots = [rng.standard_normal((rows, H)).astype(np.float32) for _ in range(2)]

    def cpu(self, dtype):
        z, c = (torch.from_numpy(a).to(dtype).requires_grad_(True) for a in (self.z, self.c))
        g0, g1 = (torch.from_numpy(a).to(dtype) for a in self.cots)
        return _grads(list(lstm_formula(z, c, self.H)), [g0, None if self.layout == "raw" else g1], [z, c])

    def gpu(self):
        from deepchem_amd import _lib, ops
        from deepchem_amd.models.torch_models.functions import LstmCellFn
        H, rows = self.H, self.rows
        g0, g1 = (_dev(a) for a in self.cots)
        c = _dev(self.c, grad=True)
        if self.layout == "tview":
            holder = _dev(self.z.reshape(4 * H, 1), grad=True)
            z = holder.t()
            assert z.stride(0) == 1  # the meaningless row stride of a one-row view
        else:
            z, holder = _wide(self.z, 1, 2, grad=self.layout != "raw")
        if self.layout != "raw":
            h2, c2 = LstmCellFn.apply(z, c)
            (h2 * g0).sum().add((c2 * g1).sum()).backward()
            dz = holder.grad.t() if self.layout == "tview" else holder.grad[:, 1:1 + 4 * H]
            if self.layout == "slice":  # (the gradient of the sentinel columns, which the loss never reads, is 0)
                assert_outside_untouched(holder.grad, 1, 4 * H, "lstm dz", value=0.0)
            return [_np(h2), _np(c2), _np(dz), _np(c.grad)]
        with torch.no_grad():
            c2 = c.detach().clone()
            h2 = ops.lstm_cell_(z, c2)
            dz = torch.empty((rows, 4 * H), dtype=torch.float32, device=DEV)
            dc = torch.empty((rows, H), dtype=torch.float32, device=DEV)
            _lib.call("gcmi_lstm_cell_bwd", ops._ptr(z), 4 * H + 3, H, rows, ops._ptr(c), ops._ptr(g0), None, ops._ptr(dz), ops._ptr(dc), ops._stream())
        return [_np(h2), _np(c2), _np(dz), _np(dc)]


GRU_CASES = {"n%d" % n: GruCase(n) for n in (255, 256, 257)}
GRU_CASES.update({"one_%+d" % s: GruCase(1, s) for s in SPECIALS})
LSTM_CASES = {"H%d_rows%d_%s" % (H, rows, lay): LstmCase(H, rows, lay)
              for H in (1, 3, 100) for rows in (1, 7) for lay in ("slice", "raw")}
LSTM_CASES.update({"H%d_rows1_tview" % H: LstmCase(H, 1, "tview") for H in (1, 3, 100)})


def _family(family):
    if family.startswith("set2set"):  # two families: logits of order 1 and of order +-200
        return [c for c in ATTEND_CASES.values() if c.big == (family == "set2set_big")]
    return list({"gru": GRU_CASES, "lstm": LSTM_CASES}[family].values())


@functools.lru_cache(maxsize=None)
def _allowed(family):
    return tuple(allowed(_family(family)))  # per output


def _run_case(family, cases, name, names):
    ref, got = cases[name].cpu(torch.float64), cases[name].gpu()
    assert len(ref) == len(got) == len(names)
    for r, g, nm, tol in zip(ref, got, names, _allowed(family)):
        assert_close(g, r, tol, "%s %s %s" % (family, name, nm))


@pytest.mark.parametrize("name", sorted(GRU_CASES))
def test_gru_kernels_forward_and_backward(name):
    _run_case("gru", GRU_CASES, name, ("z", "r", "hr", "out", "dzp", "drp", "dh", "dhpre", "dx"))


@pytest.mark.parametrize("name", sorted(LSTM_CASES))
def test_lstm_cell_forward_and_backward(name):
    _run_case("lstm", LSTM_CASES, name, ("h", "c", "dz", "dc"))


# ------------------------------------------------------------------------------------------------ set2set
ATTEND_SIZES = (0, 1, 40, 0, 3, 0)  # molecules without atoms first, in the middle and last


def attend_formula(x, h, mol_ptr):
    """q[m] = [h_m | sum_a softmax_a(<x_a, h_m>) x_a] over the atoms of molecule m; [h_m | 0] for an empty one."""
    rows = []
    for m in range(len(mol_ptr) - 1):
        xa = x[int(mol_ptr[m]):int(mol_ptr[m + 1])]
        rows.append(torch.softmax(xa @ h[m], 0) @ xa if xa.shape[0] else torch.zeros(x.shape[1], dtype=x.dtype))
    return torch.cat([h, torch.stack(rows)], 1)


class AttendCase:
    """mode "fn": AttendFn forward and backward on strided x and h; "raw0" / "raw1": the forward through ops, the
    backward through gcmi_set2set_attend_bwd with a strided dq and accumulate = 0 / 1 (dx then starts from ``pre``);
    "tview": one molecule, x and / or h as (d, 1).t() views."""

    def __init__(self, F, big, mode, sizes=ATTEND_SIZES, x_tview=False):
        rng = np.random.RandomState(10 * F + 3 * big + len(mode) + len(sizes))
        self.F, self.big, self.mode, self.sizes, self.x_tview = F, big, mode, sizes, x_tview
        self.mol_ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
        n, B = int(self.mol_ptr[-1]), len(sizes)
        if big:  # integer logits of order +-200, exact in float32 in any summation order
            self.h = (4.0 * rng.choice([-1.0, 1.0], size=(B, F))).astype(np.float32)
            self.x = (rng.randint(-4, 5, size=(n, F)) / 4.0).astype(np.float32)
            mol_of = np.repeat(np.arange(B), sizes)
            self.x[:, 0] += rng.choice([-200.0, 200.0, 199.0, 0.0], size=n) / 4.0 * np.sign(self.h[mol_of, 0])
        else:
            self.h = (2 * rng.standard_normal((B, F)) / np.sqrt(F)).astype(np.float32)
            self.x = rng.standard_normal((n, F)).astype(np.float32)
        self.cot = rng.standard_normal((B, 2 * F)).astype(np.float32)
        self.pre = rng.standard_normal((n, F)).astype(np.float32)

    def cpu(self, dtype):
        x, h = (torch.from_numpy(a).to(dtype).requires_grad_(True) for a in (self.x, self.h))
        q, dx, dh = _grads([attend_formula(x, h, self.mol_ptr)], [torch.from_numpy(self.cot).to(dtype)], [x, h])
        if self.mode == "raw1":  # (the kernel adds in float32)
            npt = np.float32 if dtype == torch.float32 else np.float64
            dx = (dx.astype(npt) + self.pre.astype(npt)).astype(np.float64)
        return [q, dx, dh]

    def gpu(self):
        from deepchem_amd import _lib, ops
        from deepchem_amd.models.torch_models.functions import AttendFn
        F, mol_ptr = self.F, _dev(self.mol_ptr)
        n, B = self.x.shape[0], self.h.shape[0]
        if self.mode == "tview":
            hh = _dev(self.h.reshape(F, 1), grad=True)
            xh = _dev(self.x.reshape(F, 1) if self.x_tview else self.x, grad=True)
            q = AttendFn.apply(xh.t() if self.x_tview else xh, hh.t(), mol_ptr)
            (q * _dev(self.cot)).sum().backward()
            return [_np(q), _np(xh.grad.t() if self.x_tview else xh.grad), _np(hh.grad.t())]
        x, xw = _wide(self.x, 2, 3, grad=self.mode == "fn")
        h, hw = _wide(self.h, 1, 2, grad=self.mode == "fn")
        if self.mode == "fn":
            q = AttendFn.apply(x, h, mol_ptr)
            (q * _dev(self.cot)).sum().backward()
            return [_np(q), _np(xw.grad[:, 2:2 + F]), _np(hw.grad[:, 1:1 + F])]
        q = ops.set2set_attend(x, _dev(self.mol_ptr), h)
        dq = _wide(self.cot, 3, 1)[0]
        dx, dxw = _wide(self.pre, 1, 1)
        dh, dhw = _wide(np.zeros((B, F), np.float32), 2, 1)
        _lib.call("gcmi_set2set_attend_bwd", ops._ptr(x), F + 5, F, ops._ptr(mol_ptr), B, ops._ptr(h), F + 3, ops._ptr(dq),
                  2 * F + 4, ops._ptr(dx), F + 2, 1 if self.mode == "raw1" else 0, ops._ptr(dh), F + 3, ops._stream())
        assert_outside_untouched(dxw, 1, F, "set2set dx")
        assert_outside_untouched(dhw, 2, F, "set2set dh")
        return [_np(q), _np(dx), _np(dh)]


ATTEND_CASES = {"F%d_%s_%s" % (F, "big" if big else "unit", mode): AttendCase(F, big, mode)
                for F in (1, 64, 65, 100, 511, 512) for big in (0, 1) for mode in ("fn", "raw0", "raw1")}
ATTEND_CASES["F100_one_molecule_h_tview"] = AttendCase(100, 0, "tview", sizes=(5,))
ATTEND_CASES["F100_one_atom_x_and_h_tview"] = AttendCase(100, 0, "tview", sizes=(1,), x_tview=True)


@pytest.mark.parametrize("name", sorted(ATTEND_CASES))
def test_set2set_attend_forward_and_backward(name):
    _run_case("set2set_big" if ATTEND_CASES[name].big else "set2set", ATTEND_CASES, name, ("q", "dx", "dh"))


def test_set2set_attend_refuses_513_features():
    from deepchem_amd import _lib, ops
    with pytest.raises(_lib.GcmiError):
        ops.set2set_attend(_dev(np.ones((2, 513), np.float32)), _dev(np.array([0, 2], np.int32)),
                           _dev(np.ones((1, 513), np.float32)))


def test_backward_wrappers_refuse_before_any_launch(monkeypatch):
    """gru_gates_bwd, gru_out_bwd, set2set_attend_bwd, lstm_cell_bwd: every float argument in turn as a CPU tensor, as
    float64, with twice the columns and without unit stride (where the C entry takes a leading dimension: without unit
    COLUMN stride) is refused on the host, and so are 513 attention features."""
    from deepchem_amd import _lib, ops
    ok = lambda *s: _dev(np.ones(s, np.float32))
    good = {"gru_gates_bwd": lambda: [ok(3, 4) for _ in range(5)],
            "gru_out_bwd": lambda: [ok(3, 4) for _ in range(4)],
            "set2set_attend_bwd": lambda: [ok(5, 4), _dev(np.array([0, 2, 5], np.int32)), ok(2, 4), ok(2, 8)],
            "lstm_cell_bwd": lambda: [ok(3, 8), ok(3, 2), ok(3, 2), ok(3, 2)]}
    spoil = {"cpu": lambda t: t.cpu(), "float64": lambda t: t.double(), "columns": lambda t: torch.cat([t, t], 1),
             "strided": lambda t: torch.cat([t, t], 1)[:, ::2]}
    for name, make in good.items():
        getattr(ops, name)(*make())  # (unspoiled, the arguments are accepted)
    launched = []
    monkeypatch.setattr(_lib, "call", lambda entry, *a: launched.append(entry))
    cases = [("set2set_attend_bwd", "513 features", [ok(5, 513), _dev(np.array([0, 5], np.int32)), ok(1, 513), ok(1, 1026)])]
    for name, make in good.items():
        for pos, how in itertools.product(range(len(make())), spoil):
            args = make()
            if args[pos].dtype == torch.float32:  # (mol_ptr goes through _i32vec, as in the forward)
                args[pos] = spoil[how](args[pos])
                cases.append((name, "%s argument %d" % (how, pos), args))
    for name, what, args in cases:
        with pytest.raises((ValueError, TypeError, _lib.GcmiError)):
            getattr(ops, name)(*args)
        assert launched == [], (name, what)


# ------------------------------------------------------------------------------------------------ EdgeNetworkFn
@pytest.mark.parametrize("variant", ["all", "h0_constant", "frozen", "no_pairs"])
@pytest.mark.parametrize("d,K", [(100, 8), (64, 16)])
def test_edge_network_fn_two_rounds_against_float64_autograd(d, K, variant):
    """m1 = EN(h0), h1 = m1 / 4 + hB, m2 = EN(h1) through EdgeMatsFn and two EdgeNetworkFn rounds that share one
    EdgeAccum; L = <m1, g1> + <m2, g2>.  Every product is multilinear, so the gradients of the same L on the absolute
    values of all inputs are the sums of the absolute terms behind each gradient element."""
    import deepchem_amd as dc
    from deepchem_amd.models.torch_models.mpnn import EdgeAccum, EdgeMatsFn, EdgeNetworkFn, PairPlan
    rng = np.random.RandomState(d + K)
    counts = np.array((0, 1, 2, 3, 4, 5, 2, 0, 3, 1, 2, 0)) * (0 if variant == "no_pairs" else 1)
    n = len(counts)
    dst_ptr, src = pair_list(rng, counts, n)
    dst = np.repeat(np.arange(n), counts)
    P = len(src)
    # chains of additions, D = (K + 1) d the product with M: a row of m1 is c_i pair terms then D; h1 = m1 / 4 + hB one
    # more; m2 the same on top of the deepest h1.  Backward, r_j pairs end in j: dhB_j = r_j + D (dm2 = g2 is exact);
    # dm1 = g1 + dh1 / 4; dh0_j = r_j + D on top of the deepest dm1.  dM (hence dW, db) sums n atoms per round of
    # products dm_i T_i, the deepest T being the second round's (c pairs of h1) and the deepest dm the first round's
    c, r = counts[:, None], np.bincount(src, minlength=n)[:, None]
    cmax, rmax, D = int(counts.max()), int(r.max()), (K + 1) * d
    n_w = 2 * n + max(2 * cmax + D + 1, rmax + D + 1 + cmax) + 2
    n_terms = {"m1": c + D, "m2": c + 2 * D + cmax + 1, "dhB": r + D, "dh0": r + 2 * D + rmax + 1, "dW": n_w, "db": n_w}
    arrs = dict(h0=0.5 * rng.standard_normal((n, d)), hB=0.5 * rng.standard_normal((n, d)),
                W=rng.standard_normal((K, d * d)) / d, b=rng.standard_normal(d * d) / d, pf=rng.rand(P, K),
                g1=rng.standard_normal((n, d)), g2=rng.standard_normal((n, d)))
    arrs = {k: v.astype(np.float32) for k, v in arrs.items()}
    wrt = {"all": ("h0", "hB", "W", "b"), "h0_constant": ("hB", "W", "b"), "frozen": ("h0", "hB"),
           "no_pairs": ("h0", "hB", "W", "b")}[variant]
    idx = (torch.from_numpy(dst).long(), torch.from_numpy(src).long())

    def reference(absolute):
        t = {k: torch.from_numpy(np.abs(v) if absolute else v).double().requires_grad_(k in wrt) for k, v in arrs.items()}
        m1 = edge_network_formula(t["h0"], t["W"], t["b"], t["pf"], idx[0], idx[1], n, d)
        m2 = edge_network_formula(0.25 * m1 + t["hB"], t["W"], t["b"], t["pf"], idx[0], idx[1], n, d)
        return _grads([m1, m2], [t["g1"], t["g2"]], [t[k] for k in wrt])

    ref, ref_abs = reference(False), reference(True)
    t = {k: _dev(v, grad=k in wrt) for k, v in arrs.items()}
    dc.set_gemm_mode("exact")
    try:
        M = EdgeMatsFn.apply(t["W"], t["b"], d)
        acc = EdgeAccum(M, K, d)
        plan = PairPlan(np.stack([dst, src], 1), t["pf"], n, torch.device(DEV))
        m1 = EdgeNetworkFn.apply(t["h0"], M, plan, acc)
        m2 = EdgeNetworkFn.apply(0.25 * m1 + t["hB"], M, plan, acc)
        got = _grads([m1, m2], [t["g1"], t["g2"]], [t[k] for k in wrt])
    finally:
        dc.set_gemm_mode("fast")
    assert acc.pending == 0 and acc.dM is None
    for nm, g, ra_ref, ra in zip(("m1", "m2") + tuple("d" + k for k in wrt), got, ref, ref_abs):
        assert_sum_bound(g, ra_ref, ra, n_terms[nm], "EdgeNetworkFn %s d=%d K=%d %s" % (variant, d, K, nm))
