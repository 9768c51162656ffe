"""The C-ABI shared library: loads, exports every symbol include/gcmi.h declares,
rejects bad arguments with an error string (no GPU needed: argument checks run
before any launch), and its host-side collation is bit-exact."""
import ctypes
import os
import re

import numpy as np
import pytest

from deepchem_amd import _lib
from deepchem_amd.feat.mol_graphs import collate_packed
from deepchem_amd.utils.synthetic import (concat_packed, single_atom_and_edge_cases,
                                          synthetic_molecules)
from oracle import mol_graphs_oracle as MO
from tests.util import load_golden, oracle_convmols, packed_from

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    text = open(os.path.join(ROOT, "include", "gcmi.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(gcmi_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_declared_symbol():
    lib = _lib.load()
    names = declared_symbols()
    assert len(names) >= 20
    for n in names:
        assert hasattr(lib, n), "libgcmi.so does not export %s" % n
    assert set(names) == set(_lib.EXPORTS), set(names) ^ set(_lib.EXPORTS)
    assert lib.gcmi_version() == 100


def test_bad_arguments_return_an_error_not_a_crash():
    lib = _lib.load()
    g = _lib.GcmiGraph()
    g.max_deg = 99
    rc = lib.gcmi_gather_sum_fwd(ctypes.byref(g), None, 0, 4, None, 0, 0, None)
    assert rc == -1 and b"max_deg" in lib.gcmi_last_error()
    g.max_deg = 10
    g.n_atoms = 5  # inconsistent with all-zero degree blocks
    rc = lib.gcmi_gather_sum_fwd(ctypes.byref(g), None, 0, 4, None, 0, 0, None)
    assert rc == -1
    with pytest.raises(_lib.GcmiError):
        _lib.call("gcmi_adam_step", None, None, None, None, 10, 1e-3, 0.9, 0.999, 1e-8, 0, None)
    _window_entries_reject_bad_arguments(lib)
    _block_entries_reject_bad_arguments(lib)
    _head_entry_rejects_bad_arguments(lib)


def _head_entry_rejects_bad_arguments(lib):
    """gcmi_head_backward: the argument checks are GCMI_ERR_ARG, and whatever head_bwd_fused refuses -- exact mode with
    more than 32 outputs, the one-pass kernels off, more than 256 outputs, a wide shape without its scratch or with
    ldfp % 4 != 0, sums without their inputs -- is GCMI_ERR_UNSUPPORTED with an error text: all before any launch.
    Device pointers are never followed here, and the route stays as it was."""
    A, OFF = 1 << 20, (1 << 20) + 4
    route = ctypes.c_int32(-7)

    def head(kind=1, logits=A, n_rows=10, n_tasks=4, n_classes=1, ldfp=256, n_mols=10, dw=A, ldg2=256, sums=None, runs=A,
             n_deg=11, arg=A, mean=A, dl=A, img=A, rt=route):
        return lib.gcmi_head_backward(kind, logits, A, None, n_rows, n_tasks, n_classes, A, ldfp, n_mols, A, dw, None, A,
                                      ldg2, A, sums, runs, n_deg, arg, A, mean, A, dl, img,
                                      None if rt is None else ctypes.byref(rt), None)

    def err():
        return lib.gcmi_last_error()

    assert head(kind=2) == -1 and b"kind" in err()
    assert head(logits=None) == -1 and b"NULL" in err()
    assert head(dw=None) == -1 and b"NULL" in err()
    assert head(rt=None) == -1 and b"NULL" in err()
    for n_rows in (0, -1, 11):
        assert head(n_rows=n_rows) == -1 and b"n_rows" in err(), n_rows
    assert head(n_mols=0, n_rows=0) == -1 and b"n_rows" in err()
    assert head(n_tasks=0) == -1 and b"n_tasks" in err()
    assert head(kind=0, n_classes=0) == -1 and b"n_classes" in err()
    assert head(ldfp=255) == -1 and b"ldfp" in err()
    assert head(ldg2=255) == -1 and b"ldg2" in err()
    for n_deg in (0, 12):
        assert head(sums=A, n_deg=n_deg) == -1 and b"n_deg" in err(), n_deg
    assert head(logits=OFF) == -1 and b"aligned" in err()
    assert head(sums=A, arg=OFF) == -1 and b"aligned" in err()

    unsupported = b"no other kernel stands behind this entry"
    assert head(n_tasks=257) == -3 and unsupported in err()
    assert head(kind=0, n_tasks=129, n_classes=2) == -3 and unsupported in err()
    assert head(kind=0, n_tasks=1 << 20, n_classes=1 << 20) == -3 and unsupported in err()  # (no 32-bit product)
    assert head(n_tasks=40, dl=None) == -3 and unsupported in err()
    assert head(n_tasks=40, img=None) == -3 and unsupported in err()
    assert head(n_tasks=40, ldfp=257) == -3 and unsupported in err()
    assert head(sums=A, runs=None) == -3 and unsupported in err()
    assert head(sums=A, mean=None) == -3 and unsupported in err()
    for option, value, n_tasks in ((_lib.GCMI_OPT_GEMM_EXACT, 1, 33), (_lib.GCMI_OPT_FUSED_BWD, 0, 4)):
        was = ctypes.c_int32(0)
        assert lib.gcmi_get_option(option, ctypes.byref(was)) == 0
        try:
            assert lib.gcmi_set_option(option, value) == 0
            assert head(n_tasks=n_tasks) == -3 and unsupported in err(), option
        finally:
            assert lib.gcmi_set_option(option, was.value) == 0
    assert route.value == -7


def _window_entries_reject_bad_arguments(lib):
    """The operation-level entries of the window kernels (gcmi_win_*): every check runs before any launch, and a
    batch without window plan is GCMI_ERR_UNSUPPORTED, not another kernel.  Pointers are never followed here."""
    A, OFF = 1 << 20, (1 << 20) + 4  # a 16-byte aligned address and one 4 bytes off
    F = 64

    def graph(max_deg=10, rev=True):  # two atoms bonded to each other
        g = _lib.GcmiGraph()
        g.max_deg, g.n_atoms, g.n_edges = max_deg, 2, 2
        for d in range(2, 12):
            g.deg_start[d], g.edge_start[d] = 2, 2
        g.d_col_idx = A
        g.d_rev_pos = A if rev else None
        return g

    # name -> arguments after the graph, as a function of (rows pointer, ld); stream last
    entries = {
        "gcmi_win_sum_h": lambda p, ld: (p, ld, F, p, ld, 0, None),
        "gcmi_win_sum_fh": lambda p, ld: (p, ld, F, A, A, 64, None),
        "gcmi_win_max_h": lambda p, ld: (p, ld, F, None, None, p, ld, A, None),
        "gcmi_win_max_bwd_h": lambda p, ld: (p, ld, F, A, p, ld, None, None, None),
        "gcmi_win_max_bwd_if_ill": lambda p, ld: (p, ld, F, A, p, ld, A, A, None),
        "gcmi_win_sumacc_max_bwd": lambda p, ld: (p, ld, F, p, ld, A, p, ld, None),
        "gcmi_win_sumacc_max_bwd_h": lambda p, ld: (p, ld, F, p, ld, A, p, ld, None),
    }
    backward = [n for n in entries if "bwd" in n]
    for name, args in entries.items():
        fn = getattr(lib, name)
        bf16 = name.endswith("_h")
        assert fn(ctypes.byref(graph(max_deg=99)), *args(A, F)) == -1 and b"max_deg" in lib.gcmi_last_error(), name
        assert fn(ctypes.byref(graph()), *args(None, F)) == -1 and b"NULL" in lib.gcmi_last_error(), name
        assert fn(ctypes.byref(graph()), *args(A, F - 4)) == -1 and b"ld" in lib.gcmi_last_error(), name
        assert fn(ctypes.byref(graph()), *args(OFF, F)) == -1 and b"aligned" in lib.gcmi_last_error(), name
        if bf16:  # 68 bf16 elements: rows of 136 bytes, no whole number of 16-byte pieces
            assert fn(ctypes.byref(graph()), *args(A, 68)) == -1 and b"ld % 8" in lib.gcmi_last_error(), name
        if name in backward:
            assert fn(ctypes.byref(graph(rev=False)), *args(A, F)) == -1 and b"reverse" in lib.gcmi_last_error(), name
        # all in order, but the graph carries no window plan: refused, nothing launched
        assert fn(ctypes.byref(graph()), *args(A, F)) == -3 and b"no window pass" in lib.gcmi_last_error(), name
    g = ctypes.byref(graph())
    assert lib.gcmi_win_max_h(g, A, F, F, A, None, A, F, A, None) == -1  # scale without shift
    assert lib.gcmi_win_max_h(g, A, F, F, None, None, A, F, A + 2, None) == -1  # arg rows 2 bytes off
    assert lib.gcmi_win_max_h(g, A, F, F, OFF, OFF, A, F, A, None) == -1  # scale / shift 4 bytes off
    assert lib.gcmi_win_max_bwd_h(g, A, F, F, A, A, F, A, None, None) == -1  # gamma without beta
    assert lib.gcmi_win_max_bwd_if_ill(g, A, F, F, A, A, F, None, None, None) == -1  # no gamma / beta
    assert lib.gcmi_win_sumacc_max_bwd(g, A, F, F, None, F, A, A, F, None) == -1  # dxs NULL
    assert lib.gcmi_win_sumacc_max_bwd_h(g, A, F, F, OFF, F, A, A, F, None) == -1  # dxs 4 bytes off


def _block_entries_reject_bad_arguments(lib):
    """The operation-level entries of the persistent block kernels (gcmi_fwd_fused_gemm, gcmi_fwd_fused_gemm_h,
    gcmi_fused_conv_bwd, gcmi_fused_dense_bwd): NULL pointers, ld < k, n_seg 0 and 17 and a bad segment are
    GCMI_ERR_ARG, a shape without persistent kernel is GCMI_ERR_UNSUPPORTED with an error text -- all before any
    launch.  Device pointers are never followed here; the segment and offset tables are host arrays."""
    A = 1 << 20  # a 16-byte aligned address
    i32, i64 = (lambda v: (ctypes.c_int32 * len(v))(*v)), (lambda v: (ctypes.c_int64 * len(v))(*v))

    def table(n_seg, rows=10, begin0=0):
        n = max(n_seg, 1)
        return n_seg, i32([begin0] + [rows] * (n - 1)), i32([rows] * n), i64([0] * n)

    def fwd(name, n_seg=1, a=A, ld=64, k=64, n_out=64, out=A, ldo=64, scratch=A, rows=10):
        ns, b, e, off = table(n_seg, rows)
        tail = (0, None, scratch, None) if name.endswith("_h") else (None, scratch, None)
        return getattr(lib, name)(ns, b, e, a, ld, k, A, off, a, ld, k, A, off, A, off, n_out, 0, 1, out, ldo, *tail)

    def conv(n_seg=1, gc=A, lds=64, k=64, rows=10, act_bf16=0):
        ns, b, e, off = table(n_seg, rows)
        return lib.gcmi_fused_conv_bwd(ns, b, e, off, off, off, A, 64, gc, 64, A, A, lds, A, max(lds, 64), k, A, A, A, None, 0,
                                       None, 0, None, act_bf16, 0, None)

    def dense(n_seg=1, membership=A, ldp=64, k=64, begin0=0, coef=A, ldg2=256):
        ns, b, e, off = table(n_seg, 10, begin0)
        return lib.gcmi_fused_dense_bwd(ns, b, e, off, off, membership, A, ldg2, A, 3, A, 128, coef, A, ldp, k, A, A, A,
                                        A, 64, None, 0, None)

    unsupported = b"no other kernel stands behind this entry"
    for name in ("gcmi_fwd_fused_gemm", "gcmi_fwd_fused_gemm_h"):
        assert fwd(name, out=None) == -1 and b"bad output" in lib.gcmi_last_error(), name
        assert fwd(name, a=None) == -1 and b"no operand" in lib.gcmi_last_error(), name
        assert fwd(name, ld=60) == -1 and b"operand" in lib.gcmi_last_error(), name
        assert fwd(name, ldo=60) == -1, name
        for n_seg in (0, 17):
            assert fwd(name, n_seg=n_seg) == -1 and b"n_seg" in lib.gcmi_last_error(), name
        assert fwd(name, rows=-1) == -1 and b"bad segment" in lib.gcmi_last_error(), name
        assert fwd(name, n_out=60, ldo=60) == -3 and unsupported in lib.gcmi_last_error(), name  # no 60-column kernel
        assert fwd(name, k=32) == -3 and unsupported in lib.gcmi_last_error(), name
    assert fwd("gcmi_fwd_fused_gemm_h", scratch=None) == -1 and b"scratch" in lib.gcmi_last_error()
    assert fwd("gcmi_fwd_fused_gemm_h", ld=68, k=64) == -3  # bf16 rows of 136 bytes
    assert fwd("gcmi_fwd_fused_gemm", ld=80, k=80, scratch=None) == -3  # the 80-column shape without its scratch

    assert conv(gc=None) == -1 and b"NULL" in lib.gcmi_last_error()
    assert conv(lds=60) == -1 and b"ld < k_in" in lib.gcmi_last_error()
    for n_seg in (0, 17):
        assert conv(n_seg=n_seg) == -1 and b"n_seg" in lib.gcmi_last_error()
    assert conv(rows=-1) == -1 and b"bad segment" in lib.gcmi_last_error()
    assert conv(act_bf16=3) == -1
    assert conv(k=32, lds=32) == -3 and unsupported in lib.gcmi_last_error()  # no kernel of one 32-column tile
    assert conv(k=97, lds=100) == -3

    assert dense(membership=None) == -1 and b"NULL" in lib.gcmi_last_error()
    assert dense(ldp=60) == -1 and b"ld < k_in" in lib.gcmi_last_error()
    assert dense(ldg2=255) == -1 and b"ldg2" in lib.gcmi_last_error()
    for n_seg in (0, 17):
        assert dense(n_seg=n_seg) == -1 and b"n_seg" in lib.gcmi_last_error()
    assert dense(begin0=4) == -3 and unsupported in lib.gcmi_last_error()  # the dense block starts at row 0
    assert dense(coef=None) == -3
    assert dense(k=32, ldp=32) == -3


def native_collate(packed, sel, out_ld=None, max_deg=10):
    lib = _lib.load()
    sel = np.ascontiguousarray(sel, np.int64)
    na, ne = ctypes.c_int64(), ctypes.c_int64()
    _lib.call("gcmi_collate_sizes", packed.atom_ptr.ctypes.data, packed.adj_ptr.ctypes.data,
              sel.ctypes.data, len(sel), ctypes.byref(na), ctypes.byref(ne))
    F = packed.n_feat
    out_ld = out_ld or F
    feats = np.full((na.value, out_ld), np.nan, np.float32)
    mem = np.empty(na.value, np.int32)
    col = np.empty(ne.value, np.int32)
    runs = np.empty(len(sel) * (max_deg + 1) * 2, np.int32)
    g = _lib.GcmiGraph()
    af = np.ascontiguousarray(packed.atom_features, np.float32)
    _lib.call("gcmi_collate", af.ctypes.data, F, packed.atom_ptr.ctypes.data, packed.adj_ptr.ctypes.data,
              packed.adj_idx.ctypes.data, sel.ctypes.data, len(sel), max_deg, feats.ctypes.data, out_ld,
              na.value, mem.ctypes.data, col.ctypes.data, ne.value, runs.ctypes.data, ctypes.byref(g))
    return feats, mem, col, runs.reshape(len(sel), max_deg + 1, 2), g


def check_against(multi_feats, deg_slice, membership, tables, feats, mem, col, runs, g, n_feat):
    assert g.n_atoms == multi_feats.shape[0]
    assert np.array_equal(feats[:, :n_feat], multi_feats.astype(np.float32))
    assert np.all(feats[:, n_feat:] == 0)
    assert np.array_equal(mem, membership)
    assert [g.deg_start[d + 1] - g.deg_start[d] for d in range(11)] == list(np.asarray(deg_slice)[:, 1])
    flat = np.concatenate([t.reshape(-1) for t in tables[1:]]) if g.n_edges else np.zeros(0, np.int32)
    assert np.array_equal(col, flat)
    # mol runs: the rows of molecule b inside every degree block
    for b in range(runs.shape[0]):
        rows = np.sort(np.concatenate([np.arange(r0, r1) for r0, r1 in runs[b]] + [np.zeros(0, int)]))
        assert np.array_equal(rows, np.nonzero(membership == b)[0])


@pytest.mark.parametrize("seed", [0, 1])
def test_native_collate_matches_reference_fixture(seed):
    gold = load_golden("collate_%d.npz" % seed)
    packed = packed_from(gold)
    feats, mem, col, runs, g = native_collate(packed, np.arange(packed.n_mols), out_ld=8)
    tables = [gold["deg_adj_%d" % d] for d in range(11)]
    check_against(gold["atom_features"], gold["deg_slice"], gold["membership"], tables, feats, mem, col,
                  runs, g, packed.n_feat)


def test_native_collate_threads_selection_and_padding():
    packed = concat_packed([synthetic_molecules(3000, seed=4, n_feat=9),
                            single_atom_and_edge_cases(9, 4)])
    rng = np.random.RandomState(0)
    sel = rng.randint(0, packed.n_mols, size=2600)  # > 256*k molecules: several threads, repeats
    feats, mem, col, runs, g = native_collate(packed, sel, out_ld=12)
    multi = collate_packed(packed, sel)
    check_against(multi.get_atom_features(), multi.deg_slice, multi.membership,
                  multi.get_deg_adjacency_lists(), feats, mem, col, runs, g, 9)
    # and the numpy collation equals the oracle on a small slice
    small = sel[:7]
    ref = MO.agglomerate([oracle_convmols(packed)[i] for i in small]) if False else None
    f2, m2, c2, r2, g2 = native_collate(packed, small)
    om = MO.agglomerate([MO.conv_mol(*packed.molecule(int(i))) for i in small])
    check_against(om["atom_features"], om["deg_slice"], om["membership"], om["deg_adj_lists"], f2, m2, c2,
                  r2, g2, 9)


def test_native_collate_errors():
    packed = synthetic_molecules(5, seed=1, n_feat=4)
    with pytest.raises(_lib.GcmiError):  # degree above max_deg
        native_collate(packed, np.arange(5), max_deg=1)
    lib = _lib.load()
    g = _lib.GcmiGraph()
    sel = np.arange(5, dtype=np.int64)
    rc = lib.gcmi_collate(packed.atom_features.ctypes.data, 4, packed.atom_ptr.ctypes.data,
                          packed.adj_ptr.ctypes.data, packed.adj_idx.ctypes.data, sel.ctypes.data, 5, 10,
                          None, 4, 0, None, None, 0, None, ctypes.byref(g))
    assert rc == -1 and b"capacity" in lib.gcmi_last_error()
