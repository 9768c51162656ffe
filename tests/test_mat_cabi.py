"""The C-ABI entries of csrc/mat.hip (gcmi_mat_bias, gcmi_mat_attention_fwd, gcmi_mat_attention_bwd) reject bad
arguments with the right status and an error text before any launch.  No GPU needed: device pointers are never
followed; the offset tables the entries validate are HOST arrays."""
import ctypes

from deepchem_amd import _lib

A, OFF = 1 << 20, (1 << 20) + 4  # a 16-byte aligned address and one 4 bytes off
ARG, UNSUPPORTED = -1, -3


def i32(v):
    return (ctypes.c_int32 * len(v))(*v)


def offsets(n_list):
    a, p = [0], [0]
    for n in n_list:
        a.append(a[-1] + n)
        p.append(p[-1] + n * n)
    return i32(a), i32(p)


def calls(lib):
    def bias(adj=A, dist=A, out=A, n_list=(3, 5), aoff=None, poff=None, d_aoff=A, d_poff=A, n_mols=None, kind=0):
        a, p = offsets(n_list)
        return lib.gcmi_mat_bias(adj, dist, a if aoff is None else aoff, p if poff is None else poff, d_aoff, d_poff,
                                 len(n_list) if n_mols is None else n_mols, kind, 0.33, 0.34, 1e-6, out, None)

    def common(q, k, v, ld, b, n_list, aoff, poff, d_aoff, d_poff, n_mols, h, dk):
        a, p = offsets(n_list)
        return (q, k, v, ld, b, a if aoff is None else aoff, p if poff is None else poff, d_aoff, d_poff,
                len(n_list) if n_mols is None else n_mols, h, dk, 0.33)

    def fwd(q=A, k=A, v=A, ld=32, b=A, n_list=(3, 5), aoff=None, poff=None, d_aoff=A, d_poff=A, n_mols=None, h=4, dk=8,
            o=A, ldo=32):
        return lib.gcmi_mat_attention_fwd(*common(q, k, v, ld, b, n_list, aoff, poff, d_aoff, d_poff, n_mols, h, dk), o, ldo,
                                          None)

    def bwd(q=A, k=A, v=A, ld=32, b=A, n_list=(3, 5), aoff=None, poff=None, d_aoff=A, d_poff=A, n_mols=None, h=4, dk=8,
            do=A, lddo=32, dq=A, dk_=A + 4096, dv=A + 8192, ldg=32, shared=0):
        return lib.gcmi_mat_attention_bwd(*common(q, k, v, ld, b, n_list, aoff, poff, d_aoff, d_poff, n_mols, h, dk), do,
                                          lddo, dq, dk_, dv, ldg, shared, None)
    return bias, fwd, bwd


def test_mat_entries_reject_bad_arguments_before_any_launch():
    lib = _lib.load()
    bias, fwd, bwd = calls(lib)

    def err():
        return lib.gcmi_last_error()

    for fn in (bias, fwd, bwd):
        assert fn(n_mols=0) == ARG and b"n_mols" in err()
        assert fn(n_mols=-2) == ARG and b"n_mols" in err()
        assert fn(aoff=ctypes.c_void_p(None)) == ARG and b"NULL" in err()
        assert fn(d_poff=None) == ARG and b"NULL" in err()
        assert fn(aoff=i32([0, 3, 3]), poff=i32([0, 9, 9])) == ARG and b"do not increase" in err()  # an empty molecule
        assert fn(aoff=i32([0, 5, 3]), poff=i32([0, 25, 34])) == ARG and b"do not increase" in err()
        assert fn(poff=i32([0, 9, 30])) == ARG and b"pair offsets" in err()  # not the sums of n^2
        assert fn(aoff=i32([1, 4, 9])) == ARG and b"start at 0" in err()
    assert bias(adj=None) == ARG and b"NULL" in err()
    assert bias(out=None) == ARG and b"NULL" in err()
    assert bias(kind=2) == ARG and b"dist_kernel" in err()
    for fn in (fwd, bwd):
        for name in ("q", "k", "v", "b"):
            assert fn(**{name: None}) == ARG and b"NULL" in err(), name
        assert fn(ld=28) == ARG and b"ld" in err()  # ld < h * d_k
        assert fn(ld=34) == ARG and b"16-byte" in err()  # rows of 136 bytes
        assert fn(q=OFF, k=OFF, v=OFF) == ARG and b"16-byte" in err()
        assert fn(h=0) == ARG
        # what no kernel covers: GCMI_ERR_UNSUPPORTED with a text
        assert fn(dk=6, ld=24) == UNSUPPORTED and b"multiple of 4" in err()
        assert fn(dk=68, ld=272) == UNSUPPORTED and b"multiple of 4" in err()
        assert fn(n_list=(3, 129)) == UNSUPPORTED and b"cap" in err()
    assert fwd(o=None) == ARG and b"output" in err()
    assert fwd(ldo=28) == ARG and b"output" in err()
    assert fwd(o=OFF) == ARG
    assert bwd(do=None) == ARG and b"dO" in err()
    assert bwd(lddo=30) == ARG and b"dO" in err()
    assert bwd(dq=None) == ARG and b"NULL" in err()
    assert bwd(dv=None) == ARG and b"NULL" in err()
    assert bwd(ldg=28) == ARG and b"gradient rows" in err()
    assert bwd(dk_=OFF) == ARG and b"gradient rows" in err()
    assert bwd(shared=1, k=A + 4096) == ARG and b"one tensor" in err()
    assert bwd(dk_=A) == ARG and b"distinct" in err()  # dK on dQ
    assert bwd(dv=A + 4096) == ARG and b"distinct" in err()  # dV on dK
    assert bwd(dv=A) == ARG and b"distinct" in err()
    assert _lib.GcmiError is not None and "gcmi_mat_bias" in _lib.EXPORTS
