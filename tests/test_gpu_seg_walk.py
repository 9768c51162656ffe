"""The walk over a segment table (csrc/common.h: SegTable, seg_of_tile, pick_n, the `rev` sweep), pinned through
``ops.seg_gemm`` on tables with every kind of awkward segment.

Which kernel a case reaches, from the dispatch in csrc/gemm.hip (``seg_gemm``) and csrc/gemm_split.hip
(``launch_seg_gemm4``).  ``ops.seg_gemm`` is ``gcmi_seg_gemm``; with more than one segment it goes

  * fast mode: to ``seg_gemm4_kernel`` whenever the output rows are 16-byte addressable and n_out % 4 == 0 -- ALL four
    shapes below, those that ``fwd_shape`` accepts included: the persistent kernels (``fwd_fused_kernel``,
    ``fwd_reg_kernel``) are entered from ``seg_gemm_stats`` only, i.e. from the whole-model forward, and no Python
    entry reaches them with a table of one's own.  128-row tiles, one workgroup per tile, the grid reversed on alternate
    launches (``next_sweep_direction``); the 75- and 64-column shapes take its 16-byte operand loads, the 50-column
    shape (rows of 50 floats) its scalar ones;
  * exact mode: to ``seg_gemm2_kernel`` (128-row tiles) for the three shapes with 16-byte addressable operand rows, and
    to ``seg_gemm_kernel`` (64-row tiles) for the 50-column shape.

So this file pins the table, its fill, the tile -> segment search and the reversed sweep; the cursor of the persistent
kernels (``SegCursor``, ``tile_range``) is walked by tests/test_gpu_fused_edges.py, which reaches ``fwd_fused_kernel``,
``fwd_reg_kernel``, ``fwd_hd_kernel`` and ``fused_bwd_kernel`` through entries of their own (``ops.fwd_fused_gemm``,
``ops.fused_conv_bwd``, ``ops.fused_dense_bwd``) on SMALL, on a 16-segment table and on tables of more tiles than three
times the largest grid.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TOL = 1e-4  # of tests/test_gpu_kernels.py::test_seg_gemm, both modes
SENTINEL = -12345.5

# 11 segments, like degrees 0..10: empty first, one row, exactly one 64-row tile, empty middle, exactly 128 rows, two
# adjacent empty ones, three ragged ones (the middle one followed by rows that belong to no segment), empty last
SMALL = (0, 1, 64, 0, 128, 0, 0, 200, 37, 270, 0)               # 700 rows, 9 tiles of 128 / 14 of 64
LARGE = (0, 1, 64, 0, 128, 0, 0, 30000, 5037, 30100, 0)         # 65 330 rows, 514 tiles of 128: more than any grid
GAP_AFTER, GAP_ROWS, TAIL_ROWS = 8, 5, 3

# name: (k1, ld1, k2, n_out, trans_w, relu)
SHAPES = {
    "conv75": (75, 76, 75, 64, False, True),    # two operands, 75 -> 64 (rows of 76 floats, as the model keeps them)
    "conv64": (64, 64, 64, 64, False, True),    # two operands, 64 -> 64
    "dense": (64, 64, 0, 128, True, True),      # one operand, 64 -> 128, nn.Linear layout, ReLU
    "odd50": (50, 50, 50, 24, False, False),    # fwd_shape refuses it (50 columns, 24 outputs); rows not 16-byte addressable
}


def _bounds(sizes):
    begin, end, row = [], [], 0
    for s, n in enumerate(sizes):
        begin.append(row)
        end.append(row + n)
        row += n
        if s == GAP_AFTER:
            row += GAP_ROWS
    return begin, end, row + TAIL_ROWS


def _case(size, shape):
    """Inputs on the GPU and the float64 product of one (size, shape): both modes use them, nothing is kept after."""
    k1, ld1, k2, n_out, trans, relu = SHAPES[shape]
    begin, end, n = _bounds(SMALL if size == "small" else LARGE)
    n_seg = len(begin)
    rng = np.random.default_rng(len(shape) * 1000 + n)
    a1 = rng.standard_normal((n, ld1)).astype(np.float32)
    a2 = rng.standard_normal((n, ld1)).astype(np.float32) if k2 else None
    wshape = (n_seg, n_out, k1) if trans else (n_seg, k1, n_out)
    w1 = rng.standard_normal(wshape).astype(np.float32)
    w2 = rng.standard_normal(wshape).astype(np.float32) if k2 else None
    bias = rng.standard_normal((n_seg, n_out)).astype(np.float32)
    skip1 = 1 if k2 else -1  # the one-row segment has no first term (degree-0 rows have no neighbour sum)
    ref = np.full((n, n_out), SENTINEL, dtype=np.float64)
    for s in range(n_seg):
        r = slice(begin[s], end[s])
        acc = np.broadcast_to(bias[s].astype(np.float64), (end[s] - begin[s], n_out)).copy()
        for a, w, on in ((a1, w1, s != skip1), (a2, w2, bool(k2))):
            if on:
                ws = w[s].astype(np.float64)
                acc += a[r, :k1].astype(np.float64) @ (ws.T if trans else ws)
        ref[r] = np.maximum(acc, 0.0) if relu else acc
    covered = np.zeros(n, dtype=bool)
    for s in range(n_seg):
        covered[begin[s]:end[s]] = True
    dev = torch.device("cuda:0")
    args = dict(
        begin=begin, end=end, n=n, k1=k1, k2=k2, n_out=n_out, trans=trans, relu=relu,
        a1=torch.from_numpy(a1).to(dev)[:, :k1], a2=torch.from_numpy(a2).to(dev)[:, :k1] if k2 else None,
        w1=torch.from_numpy(w1).to(dev).reshape(-1), w2=torch.from_numpy(w2).to(dev).reshape(-1) if k2 else None,
        bias=torch.from_numpy(bias).to(dev).reshape(-1),
        w1_off=[(-1 if s == skip1 else s * k1 * n_out) for s in range(n_seg)],
        w2_off=[s * k1 * n_out for s in range(n_seg)] if k2 else None,
        bias_off=[s * n_out for s in range(n_seg)])
    return args, ref, covered


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("size", ["small", "large"])
def test_seg_walk(size, shape):
    c, ref, covered = _case(size, shape)
    for mode in ("fast", "exact"):
        _check(c, ref, covered, "%s %s %s" % (size, shape, mode), mode)


def _check(c, ref, covered, what, mode):
    import deepchem_amd as dc
    from deepchem_amd import ops
    outs = []
    dc.set_gemm_mode(mode)
    try:
        for _ in range(4):  # the sweep direction alternates per launch: both directions, twice
            out = torch.full((c["n"], c["n_out"]), SENTINEL, dtype=torch.float32, device="cuda:0")
            ops.seg_gemm(c["begin"], c["end"], c["a1"], c["w1"], c["w1_off"], c["a2"], c["w2"], c["w2_off"], c["bias"],
                         c["bias_off"], c["n_out"], c["trans"], c["relu"], c["n"], c["k1"], c["k2"], out=out)
            outs.append(out.cpu().numpy())
    finally:
        dc.set_gemm_mode("fast")
    for i in range(1, 4):  # no atomics in these products: the same bits whichever way the tiles are walked
        assert np.array_equal(outs[0], outs[i]), "%s: launch %d differs from launch 0" % (what, i)
    got = outs[0].astype(np.float64)
    assert np.all(got[~covered] == SENTINEL), what + ": rows outside every segment were written"
    err = np.abs(got[covered] - ref[covered]).max() / max(np.abs(ref[covered]).max(), 1e-30)
    print("seg_walk %s: rel err %.3g" % (what, err))
    assert err < TOL, what
