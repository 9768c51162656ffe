"""The C-ABI entries of csrc/lcnn.hip reject bad arguments with GCMI_ERR_ARG and an error text before any launch.  No GPU
needed: device pointers are never followed."""
import ctypes

from deepchem_amd import _lib

A, OFF = 1 << 20, (1 << 20) + 2  # a 16-byte aligned address and one that is not 4-byte aligned
B, C, D, E_ = A + (1 << 16), A + (2 << 16), A + (3 << 16), A + (4 << 16)  # further aligned addresses, all distinct
ARG = -1
N, P, K, O = 5, 6, 19, 19
ENTRIES = ["gcmi_lc_site_fwd", "gcmi_lc_site_bwd", "gcmi_lc_rev_sum", "gcmi_lc_running"]


def desc(**change):
    d = dict(n_sites=N, P=P, K=K, O=O, nbr=A, rev_ptr=A + 4096, rev_row=A + 8192)
    d.update(change)
    return _lib.GcmiLcBatch(**d)


def entries(lib):
    """name -> a call with keyword overrides; every argument valid unless overridden."""
    ref, f = ctypes.byref, ctypes.c_float
    ws_floats = lib.gcmi_lc_workspace_floats(N, O)

    def site_fwd(**kw):
        k = dict(b=None, y=B, ldy=K * O, bias=C, gamma=C + 256, beta=C + 512, mean=None, var=None, eps=1e-5, mask=C + 1024,
                 out=D, ldo=O, x=E_)
        k.update(kw)
        return lib.gcmi_lc_site_fwd(ref(k["b"] or desc()), k["y"], k["ldy"], k["bias"], k["gamma"], k["beta"], k["mean"],
                                    k["var"], f(k["eps"]), k["mask"], k["out"], k["ldo"], k["x"], None)

    def site_bwd(**kw):
        k = dict(b=None, x=B, dout=D, lddo=O, mask=C + 1024, gamma=C + 256, mean=None, var=None, eps=1e-5, dx=E_, sums=C,
                 ws=E_ + (1 << 15), wsf=ws_floats)
        k.update(kw)
        return lib.gcmi_lc_site_bwd(ref(k["b"] or desc()), k["x"], k["dout"], k["lddo"], k["mask"], k["gamma"], k["mean"],
                                    k["var"], f(k["eps"]), k["dx"], k["sums"], k["ws"], k["wsf"], None)

    def rev_sum(**kw):
        k = dict(b=None, dx=B, dy=D, lddy=K * O)
        k.update(kw)
        return lib.gcmi_lc_rev_sum(ref(k["b"] or desc()), k["dx"], k["dy"], k["lddy"], None)

    def running(**kw):
        k = dict(b=None, x=B, momentum=0.1, rm=C, rv=C + 256, nbt=C + 512)
        k.update(kw)
        return lib.gcmi_lc_running(ref(k["b"] or desc()), k["x"], f(k["momentum"]), k["rm"], k["rv"], k["nbt"], None)

    return dict(site_fwd=site_fwd, site_bwd=site_bwd, rev_sum=rev_sum, running=running)


def test_lc_entries_reject_bad_arguments_before_any_launch():
    lib = _lib.load()
    fn = entries(lib)

    def err():
        return lib.gcmi_last_error()

    for name, call in fn.items():
        for bad in (0, -1, 65, 128):
            assert call(b=desc(O=bad)) == ARG and b"O %d" % bad in err(), (name, bad)
        for bad in (0, 1, 9, -2):
            assert call(b=desc(P=bad)) == ARG and b"P %d" % bad in err(), (name, bad)
        for bad in (0, 33, -1):
            assert call(b=desc(K=bad)) == ARG and b"K %d" % bad in err(), (name, bad)
        assert call(b=desc(n_sites=0)) == ARG and b"n_sites" in err(), name
        assert call(b=desc(n_sites=-3)) == ARG and b"n_sites" in err(), name
        assert call(b=desc(n_sites=2 ** 31 // (P * K * 64) + 1)) == ARG and b"below 2^31" in err(), name
        assert call(b=desc(nbr=None)) == ARG and b"neighbour table" in err(), name
        assert call(b=desc(nbr=OFF)) == ARG and b"neighbour table" in err(), name
    for lst in ("rev_ptr", "rev_row"):
        assert fn["rev_sum"](b=desc(**{lst: None})) == ARG and b"reverse lists" in err()
        assert fn["rev_sum"](b=desc(**{lst: OFF})) == ARG and b"reverse lists" in err()
    # forward
    fwd = fn["site_fwd"]
    for arg, text in (("y", b"bad Y"), ("out", b"bad output")):
        assert fwd(**{arg: None}) == ARG and text in err(), arg
        assert fwd(**{arg: OFF}) == ARG and text in err(), arg
    assert fwd(ldy=K * O - 1) == ARG and b"bad Y" in err()
    assert fwd(ldy=2 ** 31) == ARG and b"bad Y" in err()
    assert fwd(ldo=O - 1) == ARG and b"bad output" in err()
    assert fwd(out=B) == ARG and b"Y itself" in err()
    assert fwd(x=B) == ARG and fwd(x=D) == ARG and fwd(x=OFF) == ARG and b"bad X" in err()
    assert fwd(bias=OFF) == ARG and b"bias" in err()
    assert fwd(gamma=None) == ARG and fwd(gamma=OFF) == ARG and fwd(beta=OFF) == ARG and b"gamma / beta" in err()
    assert fwd(beta=None) == ARG and b"NULL beta" in err()
    assert fwd(mask=OFF) == ARG and b"mask" in err()
    for call in (fwd, fn["site_bwd"]):
        assert call(mean=C) == ARG and b"go together" in err()
        assert call(var=C) == ARG and b"go together" in err()
        assert call(mean=OFF, var=C) == ARG and b"mean / var" in err()
        assert call(eps=0.0) == ARG and call(eps=-1.0) == ARG and b"eps" in err()
    # backward
    bwd = fn["site_bwd"]
    assert bwd(x=None) == ARG and bwd(x=OFF) == ARG and b"X" in err()
    assert bwd(dout=None) == ARG and bwd(dout=OFF) == ARG and bwd(lddo=O - 1) == ARG and b"bad dOut" in err()
    assert bwd(mask=OFF) == ARG and b"mask" in err()
    assert bwd(gamma=None) == ARG and b"gamma" in err()
    assert bwd(dx=None) == ARG and bwd(dx=OFF) == ARG and bwd(dx=B) == ARG and bwd(dx=D) == ARG and b"bad dX" in err()
    assert bwd(sums=None) == ARG and bwd(sums=OFF) == ARG and b"sums" in err()
    assert bwd(ws=None) == ARG and bwd(ws=A + 4) == ARG and bwd(wsf=ws_floats_of(lib) - 1) == ARG and b"workspace" in err()
    rev = fn["rev_sum"]
    assert rev(dx=None) == ARG and rev(dx=OFF) == ARG and b"dX" in err()
    assert rev(dy=None) == ARG and rev(dy=OFF) == ARG and rev(dy=B) == ARG and rev(lddy=K * O - 1) == ARG and b"bad dY" in err()
    run = fn["running"]
    assert run(x=None) == ARG and run(x=OFF) == ARG and b"X" in err()
    assert run(momentum=0.05) == ARG and run(momentum=1.5) == ARG and b"momentum" in err()
    assert run(rm=None) == ARG and run(rv=OFF) == ARG and b"running_mean / running_var" in err()
    assert run(nbt=A + 4) == ARG and b"batches_tracked" in err()
    assert all(name in _lib.EXPORTS for name in ENTRIES + ["gcmi_lc_workspace_floats"])


def ws_floats_of(lib):
    return lib.gcmi_lc_workspace_floats(N, O)


def test_workspace_size():
    lib = _lib.load()
    # per workgroup 3 * O doubles; a workgroup takes floor(256 / O) sites, at most 1024 workgroups
    for n, o in ((5, 19), (1000, 44), (13, 19), (14, 19), (10 ** 6, 64), (1, 1), (0, 8)):
        parts = min(max(-(-n // (256 // o)), 1), 1024)
        assert lib.gcmi_lc_workspace_floats(n, o) == 2 * parts * 3 * o
    for bad in ((-1, 8), (1, 0), (1, 65)):
        assert lib.gcmi_lc_workspace_floats(*bad) == -1
