"""The C-ABI entries of csrc/cgcnn.hip reject bad arguments with GCMI_ERR_ARG and an error text before any launch.  No
GPU needed: device pointers are never followed."""
import ctypes

from deepchem_amd import _lib

A, OFF = 1 << 20, (1 << 20) + 4  # a 16-byte aligned address and one 4 bytes off
B, C, D, E_ = A + (1 << 16), A + (2 << 16), A + (3 << 16), A + (4 << 16)  # further aligned addresses, all distinct
ARG = -1
H = 8
ENTRIES = ["gcmi_cg_stats", "gcmi_cg_conv_fwd", "gcmi_cg_bwd_stats", "gcmi_cg_bwd_edges", "gcmi_cg_bwd_src"]
LISTS = ("src", "dst", "node_graph", "node_ptr", "edge_ptr", "inc_ptr", "inc_edge", "inc_other", "out_ptr", "out_edge",
         "out_other")


def desc(**change):
    """A directed description with made-up device addresses: 4 nodes, 3 edges, 2 graphs."""
    d = dict(n_nodes=4, n_edges=3, n_graphs=2, undirected=0, n_inc=3)
    d.update({k: A for k in LISTS})
    d.update(change)
    return _lib.GcmiGnGraph(**d)


def entries(lib):
    """name -> a call with keyword overrides; every argument valid unless overridden."""
    ref, f = ctypes.byref, ctypes.c_float
    ws_floats = lib.gcmi_cg_workspace_floats(4, 3, H)
    rows = dict(ps=A, pd=A + 64, ldp=4 * H, q=B, ldq=2 * H, H=H)
    norm = dict(mean=C, invstd=C + 64, gamma=C + 128, beta=C + 192)
    grad = dict(hnew=D, ldhn=H, dhnew=D + 4096, lddh=H)

    def head(k):
        return (ref(k["g"] or desc()), k["ps"], k["pd"], k["ldp"], k["q"], k["ldq"], k["H"])

    def stats(**kw):
        k = dict(g=None, **rows, mean=C, invstd=C + 64, rm=C + 128, rv=C + 192, nbt=C + 256, ws=E_, wsf=ws_floats, eps=1e-5,
                 momentum=0.1)
        k.update(kw)
        return lib.gcmi_cg_stats(*head(k), f(k["eps"]), f(k["momentum"]), k["mean"], k["invstd"], k["rm"], k["rv"], k["nbt"],
                                 k["ws"], k["wsf"], None)

    def conv_fwd(**kw):
        k = dict(g=None, **rows, **norm, h=D, ldh=H, out=E_, ldo=H)
        k.update(kw)
        return lib.gcmi_cg_conv_fwd(*head(k), k["mean"], k["invstd"], k["gamma"], k["beta"], k["h"], k["ldh"], k["out"], k["ldo"],
                                    None)

    def bwd_stats(**kw):
        k = dict(g=None, **rows, **norm, **grad, sums=E_, ws=E_ + 4096, wsf=ws_floats)
        k.update(kw)
        return lib.gcmi_cg_bwd_stats(*head(k), k["mean"], k["invstd"], k["gamma"], k["beta"], k["hnew"], k["ldhn"], k["dhnew"],
                                     k["lddh"], k["sums"], k["ws"], k["wsf"], None)

    def bwd_edges(**kw):
        k = dict(g=None, **rows, **norm, **grad, sums=E_, dq=E_ + 4096, lddq=2 * H, dpd=E_ + 8192, lddp=4 * H, dpre=E_ + 16384,
                 lddpre=H)
        k.update(kw)
        return lib.gcmi_cg_bwd_edges(*head(k), k["mean"], k["invstd"], k["gamma"], k["beta"], k["hnew"], k["ldhn"], k["dhnew"],
                                     k["lddh"], k["sums"], k["dq"], k["lddq"], k["dpd"], k["lddp"], k["dpre"], k["lddpre"], None)

    def bwd_src(**kw):
        k = dict(g=None, dq=B, lddq=2 * H, H=H, dps=E_, lddp=4 * H)
        k.update(kw)
        return lib.gcmi_cg_bwd_src(ref(k["g"] or desc()), k["dq"], k["lddq"], k["H"], k["dps"], k["lddp"], None)

    return dict(stats=stats, conv_fwd=conv_fwd, bwd_stats=bwd_stats, bwd_edges=bwd_edges, bwd_src=bwd_src)


def test_cg_entries_reject_bad_arguments_before_any_launch():
    lib = _lib.load()
    fn = entries(lib)

    def err():
        return lib.gcmi_last_error()

    for name, call in fn.items():
        # the description: sizes, NULL lists, and an UNDIRECTED one
        assert call(g=desc(n_nodes=0)) == ARG and b"n_nodes" in err(), name
        assert call(g=desc(n_graphs=0)) == ARG and b"n_graphs" in err(), name
        assert call(g=desc(n_graphs=5)) == ARG and b"every graph holds a node" in err(), name
        assert call(g=desc(n_edges=-1)) == ARG and b"n_edges" in err(), name
        assert call(g=desc(n_inc=6)) == ARG and b"n_inc" in err(), name
        assert call(g=desc(undirected=1, n_inc=6)) == ARG and b"must be directed" in err(), name
        assert call(g=desc(undirected=1)) == ARG and b"must be directed" in err(), name
        for lst in ("inc_ptr", "out_ptr", "src", "dst", "inc_edge", "inc_other", "out_edge", "out_other"):
            assert call(g=desc(**{lst: None})) == ARG and b"NULL" in err(), (name, lst)
        # H outside the range
        for bad in (0, 2, 6, 10, 132, 256, -4):
            assert call(H=bad) == ARG and b"multiple of 4" in err(), (name, bad)
    for name in ("stats", "conv_fwd", "bwd_stats", "bwd_edges"):
        call = fn[name]
        for arg, text in (("ps", b"Ps / Pd"), ("pd", b"Ps / Pd"), ("q", b"bad Q")):
            assert call(**{arg: None}) == ARG and text in err(), (name, arg)
            assert call(**{arg: OFF}) == ARG and b"16-byte" in err(), (name, arg)
        for ld, text in (("ldp", b"Ps / Pd"), ("ldq", b"bad Q")):
            assert call(**{ld: 2 * H - 4}) == ARG and text in err(), (name, ld)  # below the width
            assert call(**{ld: 2 * H + 2}) == ARG and text in err(), (name, ld)  # rows that are not 16-byte pieces
    for name in ("conv_fwd", "bwd_stats", "bwd_edges"):
        call = fn[name]
        for vec in ("mean", "invstd", "gamma", "beta"):
            assert call(**{vec: OFF}) == ARG and b"16-byte aligned" in err(), (name, vec)
        assert call(mean=None) == ARG and b"go together" in err(), name
        assert call(invstd=None) == ARG and b"go together" in err(), name
    # statistics
    stats = fn["stats"]
    assert stats(g=desc(n_edges=1, n_inc=1)) == ARG and b"at least 2 edges" in err()
    assert stats(g=desc(n_edges=0, n_inc=0)) == ARG and b"at least 2 edges" in err()
    assert stats(mean=None) == ARG and stats(invstd=OFF) == ARG and b"mean / invstd" in err()
    assert stats(rm=None) == ARG and b"go together" in err()
    assert stats(eps=0.0) == ARG and stats(momentum=1.5) == ARG and b"momentum" in err()
    for call in (stats, fn["bwd_stats"]):
        assert call(ws=None) == ARG and b"workspace" in err()
        assert call(ws=OFF) == ARG and b"workspace" in err()
        assert call(wsf=8) == ARG and b"workspace" in err()
    # forward
    fwd = fn["conv_fwd"]
    for arg, text in (("h", b"bad h"), ("out", b"bad output")):
        assert fwd(**{arg: None}) == ARG and text in err()
        assert fwd(**{arg: OFF}) == ARG and text in err()
    assert fwd(out=D) == ARG and b"h itself" in err()
    assert fwd(ldh=H - 4) == ARG and fwd(ldo=H + 1) == ARG and b"bad output" in err()
    # backward
    for name in ("bwd_stats", "bwd_edges"):
        call = fn[name]
        for arg, text in (("hnew", b"bad h'"), ("dhnew", b"bad dh'")):
            assert call(**{arg: None}) == ARG and text in err(), (name, arg)
            assert call(**{arg: OFF}) == ARG and text in err(), (name, arg)
        assert call(ldhn=H - 4) == ARG and b"bad h'" in err() and call(lddh=H + 2) == ARG and b"bad dh'" in err()
    assert fn["bwd_stats"](sums=None) == ARG and fn["bwd_stats"](sums=OFF) == ARG and b"sums" in err()
    assert fn["bwd_stats"](g=desc(n_edges=0, n_inc=0)) == ARG and b"no edges" in err()
    edges = fn["bwd_edges"]
    assert edges(sums=OFF) == ARG and b"sums" in err()
    assert edges(g=desc(n_edges=0, n_inc=0)) == ARG and b"sums without edges" in err()
    for arg, ld, text in (("dq", "lddq", b"bad dQ"), ("dpd", "lddp", b"bad dPd"), ("dpre", "lddpre", b"bad dpre")):
        assert edges(**{arg: None}) == ARG and text in err(), arg
        assert edges(**{arg: OFF}) == ARG and text in err(), arg
        assert edges(**{ld: 4}) == ARG and text in err(), ld
    assert edges(dq=B) == ARG and b"Q itself" in err()
    assert edges(dpre=D) == ARG and b"one of the inputs" in err()
    src = fn["bwd_src"]
    for arg, ld, text in (("dq", "lddq", b"bad dQ"), ("dps", "lddp", b"bad dPs")):
        assert src(**{arg: None}) == ARG and text in err(), arg
        assert src(**{arg: OFF}) == ARG and text in err(), arg
        assert src(**{ld: 2 * H - 4}) == ARG and text in err(), ld
    assert all(name in _lib.EXPORTS for name in ENTRIES + ["gcmi_cg_workspace_floats"])


def test_workspace_size():
    lib = _lib.load()
    # one row of 8H + 4 floats (a count, 4H doubles) per workgroup of the larger of the two launches (at most 1024); a workgroup takes floor(256 / (H / 4)) rows
    for n_nodes, n_edges, h in ((4, 3, 8), (1000, 12000, 64), (300, 100, 60), (5, 0, 4), (10**6, 12 * 10**6, 128)):
        rows_per_wg = 256 // (h // 4)
        parts = min(max(-(-max(n_nodes, n_edges) // rows_per_wg), 1), 1024)
        assert lib.gcmi_cg_workspace_floats(n_nodes, n_edges, h) == parts * (8 * h + 4)
    for bad in ((-1, 0, 8), (1, -1, 8), (1, 1, 6), (1, 1, 0), (1, 1, 132)):
        assert lib.gcmi_cg_workspace_floats(*bad) == -1
