"""The C-ABI entries of csrc/megnet.hip reject bad arguments with GCMI_ERR_ARG and an error text before any launch.  No
GPU needed: device pointers are never followed; ``gcmi_gn_graph_check`` follows HOST arrays only."""
import ctypes

import numpy as np

from deepchem_amd import _lib

A, OFF = 1 << 20, (1 << 20) + 4  # a 16-byte aligned address and one 4 bytes off
ARG = -1
ENTRIES = ["gcmi_gn_graph_check", "gcmi_gn_edge_fwd", "gcmi_gn_node_fwd", "gcmi_gn_edge_bwd", "gcmi_gn_node_bwd",
           "gcmi_gn_seg_reduce", "gcmi_gn_seg_spread"]
LISTS = ("src", "dst", "node_graph", "node_ptr", "edge_ptr", "inc_ptr", "inc_edge", "inc_other", "out_ptr", "out_edge",
         "out_other")


def desc(undirected=1, **change):
    """A description with made-up device addresses: 4 nodes, 3 edges, 2 graphs."""
    d = dict(n_nodes=4, n_edges=3, n_graphs=2, undirected=undirected, n_inc=6 if undirected else 3)
    d.update({k: A for k in LISTS})
    if undirected:
        d.update(out_ptr=None, out_edge=None, out_other=None)
    d.update(change)
    return _lib.GcmiGnGraph(**d)


def host_graph(undirected, **change):
    """The same graph with real host arrays: edges 0 -> 1, 1 -> 0 in graph 0, 2 -> 3 in graph 1."""
    src, dst = [0, 1, 2], [1, 0, 3]
    a = dict(src=src, dst=dst, node_graph=[0, 0, 1, 1], node_ptr=[0, 2, 4], edge_ptr=[0, 2, 3])
    if undirected:
        a.update(inc_ptr=[0, 2, 4, 5, 6], inc_edge=[1, 0, 0, 1, 2, 2], inc_other=[1, 1, 0, 0, 3, 2])
    else:
        a.update(inc_ptr=[0, 1, 2, 2, 3], inc_edge=[1, 0, 2], inc_other=[1, 0, 2],
                 out_ptr=[0, 1, 2, 3, 3], out_edge=[0, 1, 2], out_other=[1, 0, 3])
    a.update(change)
    arrays = {k: np.asarray(v, np.int32) for k, v in a.items()}
    d = _lib.GcmiGnGraph(n_nodes=4, n_edges=3, n_graphs=2, undirected=undirected, n_inc=6 if undirected else 3,
                         **{k: v.ctypes.data for k, v in arrays.items()})
    return d, arrays


def test_gn_entries_reject_bad_arguments_before_any_launch():
    lib = _lib.load()
    ref = ctypes.byref

    def err():
        return lib.gcmi_last_error()

    def edge_fwd(g=None, ps=A, pd=A + 128, ldp=64, q=A, ldq=32, r=A, ldr=32, out=A, ldo=32, fn=lib.gcmi_gn_edge_fwd):
        return fn(ref(g or desc()), ps, pd, ldp, q, ldq, r, ldr, out, ldo, None)

    def node_fwd(**kw):
        return edge_fwd(fn=lib.gcmi_gn_node_fwd, **kw)

    def edge_bwd(g=None, dhs=A, ldh=32, dps=A, dpd=A + 128, ldp=64, dr=A, ldr=32):
        return lib.gcmi_gn_edge_bwd(ref(g or desc()), dhs, ldh, dps, dpd, ldp, dr, ldr, None)

    def node_bwd(g=None, dmh=A, ldm=32, dq=A, ldq=32, dps=A, dpd=A + 128, ldp=64, dr=A, ldr=32):
        return lib.gcmi_gn_node_bwd(ref(g or desc()), dmh, ldm, dq, ldq, dps, dpd, ldp, dr, ldr, None)

    for fn in (edge_fwd, node_fwd, edge_bwd, node_bwd):
        assert fn(g=desc(n_nodes=0)) == ARG and b"n_nodes" in err()
        assert fn(g=desc(n_graphs=0)) == ARG and b"n_graphs" in err()
        assert fn(g=desc(n_graphs=5)) == ARG and b"every graph holds a node" in err()
        assert fn(g=desc(n_edges=-1)) == ARG and b"n_edges" in err()
        assert fn(g=desc(undirected=2)) == ARG and b"undirected" in err()
        assert fn(g=desc(n_inc=3)) == ARG and b"n_inc" in err()
        assert fn(g=desc(undirected=0, n_inc=6)) == ARG and b"n_inc" in err()
        for name in ("node_graph", "node_ptr", "edge_ptr", "inc_ptr", "src", "dst", "inc_edge", "inc_other"):
            assert fn(g=desc(**{name: None})) == ARG and b"NULL" in err(), name
        assert fn(g=desc(undirected=0, out_ptr=None)) == ARG and b"sorted by source" in err()
        assert fn(g=desc(undirected=0, out_other=None)) == ARG and b"sorted by source" in err()
    for fn in (edge_fwd, node_fwd):
        for name, text in (("ps", b"Ps / Pd"), ("pd", b"Ps / Pd"), ("q", b"bad Q"), ("r", b"bad R"), ("out", b"output")):
            assert fn(**{name: None}) == ARG and text in err(), name
            assert fn(**{name: OFF}) == ARG and b"16-byte" in err(), name
        for name in ("ldp", "ldq", "ldr", "ldo"):
            assert fn(**{name: 28}) == ARG, name  # below the width
            assert fn(**{name: 34}) == ARG, name  # rows of 136 bytes
    for fn, rows in ((edge_bwd, "dhs"), (node_bwd, "dmh"), (node_bwd, "dq")):
        assert fn(**{rows: None}) == ARG and b"NULL" in err()
        assert fn(**{rows: OFF}) == ARG
    for fn in (edge_bwd, node_bwd):
        assert fn(dps=None) == ARG and b"dPs / dPd" in err()
        assert fn(dpd=A) == ARG and b"one buffer" in err()
        assert fn(ldp=34) == ARG and b"dPs / dPd" in err()
        assert fn(dr=None) == ARG and b"bad dR" in err()
        assert fn(ldr=16) == ARG and b"bad dR" in err()
    for fn in (lib.gcmi_gn_seg_reduce, lib.gcmi_gn_seg_spread):
        def seg(ptr=A, n_seg=2, n_rows=5, width=7, mean=1, x=A, ldx=7, out=A, ldo=7):
            return fn(ptr, n_seg, n_rows, width, mean, x, ldx, out, ldo, None)
        assert seg(ptr=None) == ARG and b"NULL ptr" in err()
        assert seg(n_seg=0) == ARG and seg(n_rows=-1) == ARG and seg(width=0) == ARG
        assert seg(x=None) == ARG and b"NULL rows" in err()
        assert seg(out=None) == ARG and seg(ldx=6) == ARG and seg(ldo=6) == ARG and b"leading dimension" in err()
        assert seg(mean=2) == ARG and b"mean" in err()
    assert all(name in _lib.EXPORTS for name in ENTRIES)


def test_gn_graph_check_follows_the_host_lists():
    lib = _lib.load()
    for undirected in (1, 0):
        d, keep = host_graph(undirected)
        assert lib.gcmi_gn_graph_check(ctypes.byref(d)) == 0, lib.gcmi_last_error()
        # one edge listed twice in a place where it belongs, another one missing
        twice = dict(inc_edge=[0, 0, 0, 1, 2, 2]) if undirected else \
            dict(src=[0, 0, 2], dst=[1, 1, 3], inc_ptr=[0, 0, 2, 2, 3], inc_edge=[0, 0, 2], inc_other=[0, 0, 2],
                 out_ptr=[0, 2, 2, 3, 3], out_other=[1, 1, 3])
        bad = [(dict(node_ptr=[0, 2, 3]), b"node_ptr"), (dict(node_ptr=[0, 0, 4]), b"no node"),
               (dict(node_ptr=[0, 9, 4]), b"past the end"),
               (dict(edge_ptr=[0, 3, 2]), b"edge_ptr"), (dict(node_graph=[0, 1, 1, 1]), b"node_graph"),
               (dict(src=[0, 1, 4]), b"leaves the"), (dict(dst=[1, 0, -1]), b"leaves the"),
               (dict(src=[0, 2, 2], dst=[1, 0, 3]), b"not inside graph"),
               (dict(inc_ptr=[0, 2, 4, 5, 7] if undirected else [0, 1, 2, 2, 4]), b"inc_ptr"),
               (dict(inc_ptr=[0, 2, 1, 5, 6] if undirected else [0, 1, 0, 2, 3]), b"decreases"),
               (dict(inc_ptr=[0, 2, 9, 5, 6] if undirected else [0, 1, 9, 2, 3]), b"past the end"),
               (dict(inc_edge=[1, 0, 0, 1, 2, 3] if undirected else [1, 0, 3]), b"out of range"),
               (dict(inc_other=[1, 1, 0, 0, 3, 4] if undirected else [1, 0, 4]), b"out of range"),
               (dict(inc_other=[1, 1, 0, 0, 2, 2] if undirected else [1, 0, 3]), b"is not edge"),
               (twice, b"time")]
        if not undirected:
            bad += [(dict(out_other=[1, 1, 3]), b"is not edge"), (dict(out_ptr=[0, 1, 2, 3, 4]), b"out_ptr")]
        for change, text in bad:
            d, keep = host_graph(undirected, **change)
            rc = lib.gcmi_gn_graph_check(ctypes.byref(d))
            assert rc == ARG and text in lib.gcmi_last_error(), (change, lib.gcmi_last_error())
    assert lib.gcmi_gn_graph_check(None) == ARG and b"NULL graph" in lib.gcmi_last_error()
