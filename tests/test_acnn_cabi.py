"""The C-ABI entries of csrc/atomconv.hip reject bad arguments with GCMI_ERR_ARG and an error text before any launch.
No GPU needed: device pointers are never followed."""
import ctypes

from deepchem_amd import _lib, ops

A, OFF = 1 << 20, (1 << 20) + 2  # a 16-byte aligned address and one 2 bytes off
B_, C_, D_, E_ = A + (1 << 16), A + (2 << 16), A + (3 << 16), A + (4 << 16)
ARG = -1
PTRS = ("x", "nbrs", "z", "rc", "rs", "re")


def desc(types=(6.0, 7.0, -1.0), box=None, **change):
    """A description with made-up device addresses: 2 samples of 5 atoms with 4 neighbours, 3 filters."""
    d = _lib.GcmiAcInput()
    for i, k in enumerate(PTRS):
        setattr(d, k, A + 4096 * i)
    d.B, d.N, d.M, d.d, d.L, d.n_types = 2, 5, 4, 3, 3, len(types)
    for i, t in enumerate(types):
        d.types[i] = t
    d.has_box = int(box is not None)
    for i, v in enumerate(box or ()):
        d.box[i] = v
    for k, v in change.items():
        setattr(d, k, v)
    return d


def entries(lib):
    ref, f = ctypes.byref, ctypes.c_float

    def stats(**kw):
        k = dict(a=None, eps=1e-5, stats=C_, ws=E_, wsf=None)
        k.update(kw)
        a = k["a"] or desc()
        wsf = lib.gcmi_ac_workspace_floats(a.B, a.N, a.L) if k["wsf"] is None else k["wsf"]
        return lib.gcmi_ac_stats(ref(a), f(k["eps"]), k["stats"], k["ws"], wsf, None)

    def fwd(**kw):
        k = dict(a=None, stats=C_, out=D_)
        k.update(kw)
        return lib.gcmi_ac_fwd(ref(k["a"] or desc()), k["stats"], k["out"], None)

    def bwd(**kw):
        k = dict(a=None, stats=C_, dy=D_, grad=B_, ws=E_, wsf=None)
        k.update(kw)
        a = k["a"] or desc()
        wsf = lib.gcmi_ac_workspace_floats(a.B, a.N, a.L) if k["wsf"] is None else k["wsf"]
        return lib.gcmi_ac_bwd(ref(a), k["stats"], k["dy"], k["grad"], k["ws"], wsf, None)

    return dict(stats=stats, fwd=fwd, bwd=bwd)


def test_limits_agree_with_the_header():
    assert (ops.AC_MAX_NEIGHBORS, ops.AC_MAX_TYPES, ops.AC_MAX_CHANNELS) == (64, 32, 2048)
    assert len(_lib.GcmiAcInput().types) == ops.AC_MAX_TYPES
    assert ops.ac_width_ok(66, [6, 7., 8., 9., 11., 12., 15., 16., 17., 20., 25., 30., 35., 53., -1.])
    assert ops.ac_width_ok(2048) and not ops.ac_width_ok(2049) and not ops.ac_width_ok(0)
    assert ops.ac_width_ok(64, range(32)) and not ops.ac_width_ok(65, range(32)) and not ops.ac_width_ok(1, range(33))
    assert not ops.ac_width_ok(3, [6, 7, 6.0]) and not ops.ac_width_ok(3, [float("nan")])


def test_ac_entries_reject_bad_arguments_before_any_launch():
    lib = _lib.load()

    def err():
        return lib.gcmi_last_error()

    for name, call in entries(lib).items():
        assert call(a=desc(B=0)) == ARG and b"B 0" in err(), name
        assert call(a=desc(N=0)) == ARG and b"N 0" in err(), name
        assert call(a=desc(B=1 << 15, N=1 << 15)) == ARG and b"below 2^31" in err(), name
        for bad in (0, 65, -1):
            assert call(a=desc(M=bad)) == ARG and b"M %d" % bad in err(), (name, bad)
        for bad in (2, 4):
            assert call(a=desc(d=bad)) == ARG and b"3 coordinates" in err(), (name, bad)
        for bad in (-1, 33):
            assert call(a=desc(n_types=bad)) == ARG and b"atom types" in err(), (name, bad)
        for bad in (0, -3, 2049, 683):  # 683 filters x 3 types = 2049 channels
            assert call(a=desc(L=bad)) == ARG and b"channels" in err(), (name, bad)
        assert call(a=desc(types=(), L=2049)) == ARG and b"channels" in err(), name
        assert call(a=desc(types=(6.0, 7.0, 6.0))) == ARG and b"stands twice" in err(), name
        for p in PTRS:
            assert call(a=desc(**{p: None})) == ARG and b"NULL" in err(), (name, p)
            assert call(a=desc(**{p: OFF})) == ARG and b"4-byte aligned" in err(), (name, p)
        assert call(a=desc(has_box=2)) == ARG and b"has_box" in err(), name
        assert call(stats=None) == ARG and b"statistics" in err(), name
        assert call(stats=A + 4) == ARG and b"statistics" in err(), name
    fn = entries(lib)
    # the statistics need two values per slot
    assert fn["stats"](a=desc(types=(), B=1, L=1)) == ARG and b"at least 2 values" in err()
    assert fn["stats"](eps=-1.0) == ARG and b"eps" in err()
    assert fn["fwd"](out=None) == ARG and b"output" in err()
    assert fn["fwd"](out=OFF) == ARG and b"output" in err()
    assert fn["bwd"](dy=None) == ARG and b"dy" in err()
    assert fn["bwd"](grad=None) == ARG and b"gradient" in err()
    # the workspace: NULL, misaligned, too small
    for name in ("stats", "bwd"):
        need = lib.gcmi_ac_workspace_floats(2, 5, 3)
        assert need >= 2 * 2 * 2 * 5
        assert fn[name](ws=None) == ARG and b"workspace" in err(), name
        assert fn[name](ws=A + 8) == ARG and b"workspace" in err(), name
        assert fn[name](wsf=need - 1) == ARG and b"workspace" in err(), name
    assert lib.gcmi_ac_workspace_floats(0, 5, 3) == -1 and lib.gcmi_ac_workspace_floats(2, 5, 2049) == -1
    assert lib.gcmi_ac_workspace_floats(2, 5, 0) == -1
