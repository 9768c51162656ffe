"""Float64 restatements of the small primitive kernels (csrc/bn.hip, csrc/readout.hip, csrc/loss.hip), written from
the formulas of the layers they replace and used by tests/test_gpu_bn_edges.py, tests/test_gpu_readout_edges.py and
tests/test_gpu_loss_edges.py.  Plain numpy on the CPU: no kernel of this project and no float32 library routine.
tests/test_edge_refs_host.py checks them without a device (against torch in float64 and the oracle) together with
the exactness conditions the GPU tests lean on.

The last section restates the operations of the molecule-window kernels (csrc/gather_lds.hip) for
tests/test_gpu_win_ops.py -- in the kernels' own arithmetic (float32 adds in neighbour-table order), so that those
comparisons are bit for bit; tests/test_win_refs_host.py checks them against the oracle and autograd.

The section after it restates the segmented products (csrc/gemm.hip, csrc/gemm_split.hip) for
tests/test_gpu_product_edges.py: the two contracts in float64, the float32 arithmetic each product mode claims, and the
operands that tell a lost piece product; tests/test_product_refs_host.py checks them.

The last section restates the per-molecule head backward (csrc/head_bwd.hip) for tests/test_gpu_head_bwd.py;
tests/test_head_refs_host.py checks it against torch autograd and the row-level definition of the BatchNorm sums.
"""
import numpy as np

TOL = 1e-4  # tests/test_gpu_kernels.py, BASELINE.json north star
BN_EPS = float(np.float32(1e-3))  # the value the kernel receives: eps travels as a float
BN_MOMENTUM = 0.99


def f64(a):
    return np.asarray(a, np.float64)


# ------------------------------------------------------------------------------------------------ BatchNorm
def bn_ref(x, gamma, beta, dy, eps=BN_EPS):
    """Training-mode BatchNorm1d over the rows of x and its backward for the incoming gradient dy, in float64.
    ``unbiased``: what goes into running_var (the variance itself for one row, as bn_finalize_kernel does; torch
    refuses one row in training mode)."""
    x, gamma, beta, dy = f64(x), f64(gamma), f64(beta), f64(dy)
    n = x.shape[0]
    mean = x.mean(0)
    var = ((x - mean) ** 2).mean(0)  # biased
    invstd = 1.0 / np.sqrt(var + eps)
    unbiased = var * n / (n - 1.0) if n > 1 else var
    scale = gamma * invstd
    shift = beta - mean * scale
    y = x * scale + shift
    xhat = (x - mean) * invstd
    dbeta = dy.sum(0)
    dgamma = (dy * xhat).sum(0)
    dx = gamma * invstd * (dy - dbeta / n - xhat * dgamma / n)
    return dict(mean=mean, var=var, unbiased=unbiased, invstd=invstd, scale=scale, shift=shift, y=y, dgamma=dgamma,
                dbeta=dbeta, dx=dx, dx_relu=np.where(x > 0, dx, 0.0))


def bn_running_ref(start, stat, times, momentum=BN_MOMENTUM):
    """``times`` momentum updates r <- (1 - momentum) r + momentum stat (momentum weighs the NEW value, as
    nn.BatchNorm1d counts it)."""
    r = f64(start).copy()
    for _ in range(times):
        r = (1.0 - momentum) * r + momentum * f64(stat)
    return r


def bn_fold_eval_ref(gamma, beta, running_mean, running_var, eps=BN_EPS):
    scale = f64(gamma) / np.sqrt(f64(running_var) + eps)
    return scale, f64(beta) - f64(running_mean) * scale


def bn_ref_f32(x, gamma, beta, dy, eps=BN_EPS):
    """The same formulas with everything that is stored or multiplied per element in FLOAT32 and the column sums in
    float64, as any float32 BatchNorm with exact reductions has them: mean, invstd, scale, shift and the backward's
    three coefficient vectors are float32 numbers, y = x * scale + shift and dx = A dy + (B x + C) are float32
    products and sums (two roundings each where a kernel may fuse them into one).  What this loses against
    ``bn_ref`` is what the number format loses, not what a particular kernel loses."""
    f32 = np.float32
    x, gamma, beta, dy = (np.asarray(a, f32) for a in (x, gamma, beta, dy))
    n = x.shape[0]
    xd = x.astype(np.float64)
    m = xd.sum(0) / n
    var = np.maximum((xd * xd).sum(0) / n - m * m, 0.0)
    mean = m.astype(f32)
    invstd = (1.0 / np.sqrt(var + eps)).astype(f32)
    unbiased = var * n / (n - 1.0) if n > 1 else var
    scale = gamma * invstd
    shift = beta - mean * scale
    y = x * scale + shift
    xhat = (x - mean) * invstd
    dyd = dy.astype(np.float64)
    dbeta = dyd.sum(0)
    dgamma = (dyd * xhat.astype(np.float64)).sum(0)
    isd = invstd.astype(np.float64)
    A = gamma.astype(np.float64) * isd
    B = -A * isd * dgamma / n
    C = -A * dbeta / n - B * mean.astype(np.float64)
    A, B, C = A.astype(f32), B.astype(f32), C.astype(f32)
    dx = A * dy + (B * x + C)
    assert y.dtype == f32 and dx.dtype == f32 and xhat.dtype == f32
    return dict(mean=mean, var=var, unbiased=unbiased.astype(f32), invstd=invstd, scale=scale, shift=shift, y=y,
                dgamma=dgamma.astype(f32), dbeta=dbeta.astype(f32), dx=dx, dx_relu=np.where(x > 0, dx, f32(0)))


# ------------------------------------------------------------------------------------------------ readout
def hand_batch(counts):
    """counts[m][d] = atoms of molecule m in degree block d -> (deg_counts, membership): the rows of a collated
    batch are sorted by degree first and by molecule inside a degree block."""
    counts = np.asarray(counts, np.int64)
    deg_counts = counts.sum(0)
    membership = np.concatenate([np.repeat(np.arange(counts.shape[0]), counts[:, d]) for d in range(counts.shape[1])])
    return [int(c) for c in deg_counts], membership.astype(np.int32)


def readout_batch(n_deg, n_fill, seed):
    """The molecules tests/test_gpu_readout_edges.py asks for, as a counts[m][d] table: empty molecules at the
    front, in the middle and at the end; 1, 3, 4, 5, 8, 9, 12, 13 and 25 atoms (the four-row rounds and the three
    rounds in flight on and off their boundaries); all rows in one degree block; one row in every block; rows in
    the first and the last block only; 64 atoms; ``n_fill`` random molecules of at most 64 atoms."""
    rng = np.random.RandomState(seed)

    def spread(n_atoms):
        return np.bincount(rng.randint(0, n_deg, size=n_atoms), minlength=n_deg)

    def one_block(d, n_atoms):
        c = np.zeros(n_deg, np.int64)
        c[d] = n_atoms
        return c

    empty = np.zeros(n_deg, np.int64)
    first_last = one_block(0, 3) + one_block(n_deg - 1, 2)
    mols = [empty, empty] + [spread(k) for k in (1, 3, 4, 5)] + [one_block(min(3, n_deg - 1), 7), empty]
    mols += [spread(k) for k in (8, 9, 12, 13, 25)] + [np.ones(n_deg, np.int64), first_last, spread(64)]
    mols += [one_block(n_deg - 1, 1), one_block(0, 4), one_block(1, 13)]
    mols += [spread(int(k)) for k in rng.randint(1, 41, size=n_fill)]
    mols += [empty]
    counts = np.stack(mols)
    assert counts.sum(1).max() <= 64
    return counts


def readout_ref(x, membership, n_mols, scale=None, shift=None, tanh=False):
    """GraphGather in float64: per molecule [sum | max] over its rows of a = x * scale + shift, then tanh.
    Returns (out (n_mols, 2F), arg (n_mols, F)): arg is the LOWEST row index attaining the maximum of a, -1 for a
    molecule without atoms (whose sum is 0 and whose max is -inf)."""
    a = f64(x)
    if scale is not None:
        a = a * f64(scale) + f64(shift)
    membership = np.asarray(membership, np.int64)
    F = a.shape[1]
    out = np.zeros((n_mols, 2 * F))
    out[:, F:] = -np.inf
    arg = np.full((n_mols, F), -1, np.int64)
    for m in range(n_mols):
        rows = np.nonzero(membership == m)[0]  # ascending
        if rows.size == 0:
            continue
        am = a[rows]
        out[m, :F] = am.sum(0)
        out[m, F:] = am.max(0)
        arg[m] = rows[am.argmax(0)]  # numpy: the first occurrence of the maximum
    if tanh:
        out = np.tanh(out)
    return out, arg


def readout_bwd_ref(dout, out, arg, membership, tanh):
    """d loss / d a for loss = <out, dout>: every row gets its molecule's sum gradient, the arg-max row the max
    gradient on top; with tanh both carry 1 - out^2 of the (saved) output."""
    dout, out = f64(dout), f64(out)
    membership = np.asarray(membership, np.int64)
    F = arg.shape[1]
    g = dout * (1.0 - out * out) if tanh else dout
    rows = np.arange(membership.shape[0])[:, None]
    return g[membership, :F] + np.where(np.asarray(arg)[membership] == rows, g[membership, F:], 0.0)


# ------------------------------------------------------------------------------------------------ loss
def log_softmax_ref(x):
    x = f64(x)
    z = x - x.max(-1, keepdims=True)
    return z - np.log(np.exp(z).sum(-1, keepdims=True))


def softmax_ref(x):
    return np.exp(log_softmax_ref(x))


def ce_loss_ref(logits, labels, weights):
    """(loss, dlogits, probs): loss = mean over (rows, tasks) of w * (-sum_c y_c logp_c) and
    dlogits = w (p sum_c y_c - y) / count.  ``weights`` None: all ones."""
    x, y = f64(logits), f64(labels)
    logp = log_softmax_ref(x)
    p = np.exp(logp)
    w = np.ones(x.shape[:-1]) if weights is None else f64(weights).reshape(x.shape[:-1])
    count = w.size
    loss = float((w * -(y * logp).sum(-1)).sum() / count)
    dlogits = w[..., None] * (p * y.sum(-1, keepdims=True) - y) / count
    return loss, dlogits, p


def l2_loss_ref(outputs, labels, weights):
    """(loss, doutputs): loss = mean of w (x - y)^2, gradient 2 w (x - y) / count."""
    x, y = f64(outputs), f64(labels)
    w = np.ones(x.shape) if weights is None else f64(weights).reshape(x.shape)
    return float((w * (x - y) ** 2).sum() / x.size), 2.0 * w * (x - y) / x.size


# ------------------------------------------------------------------------------------------------ dispatch
# What the host code of the kernels decides from a shape, restated so that every test case can carry the branch it
# reaches in its id (launch_col_sums / bn_bwd_impl in csrc/bn.hip, readout_fwd_impl in csrc/readout.hip).
def bn_branch(n_rows, n_feat, vec4, min_rows=512):
    """``vec4``: every operand of the launch is 16-byte aligned with ld % 4 == 0.  ``min_rows``: 512 for the column
    sums, 256 for the dx kernel."""
    V = 4 if (vec4 and n_feat % 4 == 0) else 1
    lpr = n_feat // V
    lx = min(lpr, 256)
    ry = 256 // lx
    round_rows = 4 * ry
    rpb = max(-(-n_rows // 2048), min_rows)
    rpb = -(-rpb // round_rows) * round_rows
    blocks = -(-n_rows // rpb)
    return dict(V=V, lpr=lpr, lx=lx, ry=ry, idle=256 - lx * ry, col_passes=-(-lpr // lx), round_rows=round_rows, rpb=rpb,
                blocks=blocks, last_rows=n_rows - (blocks - 1) * rpb)


def bn_case_id(n_rows, n_feat, layout, vec4_sums, vec4_dx):
    s, d = bn_branch(n_rows, n_feat, vec4_sums, 512), bn_branch(n_rows, n_feat, vec4_dx, 256)
    return "n%d-f%d-%s-sumsV%d-dxV%d-lx%d-ry%d-idle%d-colpasses%d-wg%d+%d-lastrows%d+%d" % (
        n_rows, n_feat, layout, s["V"], d["V"], s["lx"], s["ry"], s["idle"], s["col_passes"], s["blocks"], d["blocks"],
        s["last_rows"], d["last_rows"])


def readout_branch(n_feat, n_deg, vec4=True):
    V = 4 if (vec4 and n_feat % 4 == 0) else 1
    lpr = n_feat // V
    gl = min(lpr, 256)
    mpb = 256 // gl
    pipelined = V == 4 and gl == lpr and n_deg <= gl <= 64 and (gl & (gl - 1)) == 0
    return dict(V=V, lpr=lpr, gl=gl, mpb=mpb, idle=256 - gl * mpb, col_passes=-(-lpr // gl), pipelined=pipelined)


def readout_case_id(n_feat, n_deg, n_mols, layout="c", vec4=True):
    b = readout_branch(n_feat, n_deg, vec4)
    return "f%d-%s-ndeg%d-mols%d-V%d-gl%d-mpb%d-idle%d-colpasses%d-%s-lastwg%d" % (
        n_feat, layout, n_deg, n_mols, b["V"], b["gl"], b["mpb"], b["idle"], b["col_passes"],
        "pipelined" if b["pipelined"] else "plain", n_mols - (-(-n_mols // b["mpb"]) - 1) * b["mpb"])


# ------------------------------------------------------------------------------------------------ window gather ops
# GraphConv.sum_neigh, GraphPool and its backward over the degree blocks of a collated batch, vectorised per degree
# block.  Every function works in the dtype of its input: float32 rows give the kernels' arithmetic (one float32 add
# per neighbour, in neighbour-table order, starting from 0), float64 rows the value the oracle and autograd give.
class HostGraph:
    """deg_counts[d] atoms of degree d, rows sorted by degree; col_idx: the neighbour tables of the degrees 1, 2, ...
    back to back, (n_d, d) global rows each.  ``rev[d][r, j]``: the position of row r of block d in the neighbour
    list of its j-th neighbour, the n-th bond between two atoms paired with the n-th one seen from the other end --
    found here from the tables alone."""

    def __init__(self, deg_counts, col_idx):
        self.deg_counts = [int(c) for c in deg_counts]
        col_idx = np.asarray(col_idx, np.int64)
        self.n_atoms = sum(self.deg_counts)
        self.row0, self.nb = [], []
        r = e = 0
        for d, c in enumerate(self.deg_counts):
            self.row0.append(r)
            self.nb.append(col_idx[e:e + c * d].reshape(c, d))
            r += c
            e += c * d
        assert e == col_idx.shape[0]
        self.max_present = max([d for d, c in enumerate(self.deg_counts) if c] + [0])
        width = max(self.max_present, 1)
        table = np.full((self.n_atoms, width), -1, np.int64)
        for d, c in enumerate(self.deg_counts):
            if c:
                table[self.row0[d]:self.row0[d] + c, :d] = self.nb[d]
        self.rev = []
        for d, c in enumerate(self.deg_counts):
            rev = np.zeros((c, d), np.int64)
            k = self.rows(d)
            for j in range(d):
                i = self.nb[d][:, j]
                nth = (self.nb[d][:, :j] == i[:, None]).sum(1)
                hit = table[i] == k[:, None]
                want = hit & (np.cumsum(hit, 1) == (nth + 1)[:, None])
                assert want.any(1).all(), "a bond is not listed from both ends"
                rev[:, j] = want.argmax(1)
            self.rev.append(rev)

    def rows(self, d):
        return np.arange(self.row0[d], self.row0[d] + self.deg_counts[d])

    def degree_blocks(self):
        return [(d, self.rows(d), self.nb[d], self.rev[d]) for d, c in enumerate(self.deg_counts) if c]


def bf16_round(x):
    """float32 values rounded to the nearest bf16 (ties to even, as torch's .to(torch.bfloat16)), kept as float32."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    r = (u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)
    return r.view(np.float32)


def neigh_sum(hg, x, old=None):
    """s[i] = sum_j x[nb(i, j)], accumulated from 0 in neighbour order; ``old`` (accumulate) is added LAST."""
    out = np.zeros_like(x)
    for d, rows, nb, _ in hg.degree_blocks():
        acc = np.zeros((rows.shape[0], x.shape[1]), x.dtype)
        for j in range(d):
            acc = acc + x[nb[:, j]]
        out[rows] = acc
    if old is not None:
        out = out + old
    assert out.dtype == x.dtype
    return out


def pool_max(hg, y):
    """(values, arg bytes): the maximum over the atom's own row and its neighbours' -- self first, then the neighbours
    in order, a later candidate wins only if strictly greater; arg 0 = self, j + 1 = neighbour j."""
    best = y.copy()
    arg = np.zeros(y.shape, np.uint8)
    for d, rows, nb, _ in hg.degree_blocks():
        b, a = y[rows], np.zeros((rows.shape[0], y.shape[1]), np.uint8)
        for j in range(d):
            v = y[nb[:, j]]
            m = v > b
            b = np.where(m, v, b)
            a = np.where(m, np.uint8(j + 1), a)
        best[rows], arg[rows] = b, a
    return best, arg


def pool_bwd(hg, g, arg):
    """dx[k] = g[k] where arg[k] == 0, then += g[i_j] per neighbour j in order where arg[i_j] names k (reverse
    position + 1)."""
    out = np.zeros_like(g)
    zero = g.dtype.type(0)
    for d, rows, nb, rev in hg.degree_blocks():
        acc = np.where(arg[rows] == 0, g[rows], zero)
        for j in range(d):
            i = nb[:, j]
            acc = acc + np.where(arg[i] == (rev[:, j] + 1)[:, None], g[i], zero)
        out[rows] = acc
    assert out.dtype == g.dtype
    return out


def two_stage_bwd(hg, ds, dxs, arg, bf16=False):
    """(dX, dy): dX = neigh_sum(dS) + dXs, dy = pool_bwd(dX, arg); ``bf16``: dX and dy each rounded once."""
    dx = neigh_sum(hg, ds, old=dxs)
    if bf16:
        dx = bf16_round(dx)
    dy = pool_bwd(hg, dx, arg)
    return dx, (bf16_round(dy) if bf16 else dy)


def exact_rows(rng, n, width):
    """Rows k / 4, k in [-3, 3]: ties everywhere; sums of <= 11 of them are < 2^8 quarter-units (exact in bf16)."""
    return (rng.randint(-3, 4, size=(n, width)) / 4.0).astype(np.float32)


def plant_winners(hg, x):
    """Around the first atom of the highest degree D present, make candidate c % (D + 1) the only maximum of column
    c (0: a tie of all, which the atom itself wins): every arg byte 0..D then occurs.  x is changed in place."""
    d = hg.max_present
    k, nb = hg.row0[d], hg.nb[d][0]
    lo, hi = x.dtype.type(-0.75), x.dtype.type(0.75)
    x[k] = lo
    x[nb] = lo
    for c in range(x.shape[1]):
        if c % (d + 1):
            x[nb[c % (d + 1) - 1], c] = hi
    return x


def exact_bn(rng, width):
    """(scale, shift): scales from {+-0.5, +-1, +-1.5, +-2}, shifts m / 4 with |m| <= 8, both signs present.  With
    ``exact_rows`` every x * scale + shift is a multiple of 1/8 of magnitude <= 3.5: six significant bits, exact in
    float32 and in bf16 whether the product is rounded before the sum (numpy) or not (fmaf)."""
    scale = (rng.choice([0.5, 1.0, 1.5, 2.0], size=width) * rng.choice([-1.0, 1.0], size=width)).astype(np.float32)
    shift = (rng.randint(-8, 9, size=width) / 4.0).astype(np.float32)
    scale[:2] = [-1.5, 0.5]
    shift[:2] = [0.75, -2.0]
    return scale, shift


def ulp(v, bf16=False):
    """The spacing of float32 (bf16) numbers at |v|: one unit in the last of 24 (8) significant bits."""
    a = np.maximum(np.abs(np.asarray(v, np.float64)), 2.0 ** -126)
    return 2.0 ** (np.floor(np.log2(a)) - (7 if bf16 else 23))


def window_rows(meta_row):
    """The global rows of one window descriptor (include/gcmi.h, d_win_meta): slot s of degree d is row base[d] + s."""
    m = [int(v) for v in meta_row]
    base, start = m[:11], [0] + m[11:22]
    return np.concatenate([np.arange(start[d], start[d + 1]) + base[d] for d in range(11)] + [np.zeros(0, np.int64)])


def candidate_value(hg, y, arg):
    """y of the candidate each arg byte names (0: the atom's own row, j + 1: its neighbour j); a byte above the
    atom's degree names nothing and fails."""
    out = np.empty_like(y)
    cols = np.arange(y.shape[1])[None, :]
    for d, rows, nb, _ in hg.degree_blocks():
        a = arg[rows].astype(np.int64)
        assert a.max(initial=0) <= d, "arg byte above the degree"
        src = np.concatenate([rows[:, None], nb], 1)  # (n_d, d + 1) candidate rows
        out[rows] = y[np.take_along_axis(src, a, 1), cols]
    return out


# What make_plan / launch_lpr (csrc/gather_lds.hip) decide from a batch's window sizes, restated so that a test knows
# which launches run over windows and which two-stage forms must refuse.  c: the gcmi_graph of the batch.
WIN_LDS_BYTES = 160 * 1024
WIN_HEAD_BYTES = 320 + 2048  # the ring of three window descriptors and 512 floats of per-op constants


def win_plan_bytes(c, row_bytes, aux, third_tiles=0):
    """Dynamic LDS of one workgroup: two window buffers [rows | arg bytes | neighbour entries] and ``third_tiles``
    more row tiles.  aux: 0 none, 4 / 8 = arg bytes per 16-byte piece (float / bf16 rows).  The two buffers of the
    ordinary windows together also hold one oversized window: they grow by 8 atoms until they do."""
    def buf(alloc, ecap):
        tile = alloc * row_bytes
        a = 0 if not aux else (-(-(tile // 4) // 16) * 16 if aux == 4 else -(-(alloc * (row_bytes // 16)) // 64) * 512)
        return tile + a + max(ecap, 8) * 2
    alloc = max(c.win_alloc, 1)
    if c.n_win_big > 0:
        while 2 * buf(alloc, c.win_ecap) < buf(c.win_alloc_big, c.win_ecap_big):
            alloc += 8
    return 2 * buf(alloc, c.win_ecap) + WIN_HEAD_BYTES + third_tiles * alloc * row_bytes, alloc


def win_fits(c, row_bytes, aux, third_tiles=0):
    return c.n_win > 0 and win_plan_bytes(c, row_bytes, aux, third_tiles)[0] <= WIN_LDS_BYTES


# ------------------------------------------------------------------------------------------------ segmented products
# The two product entry points of csrc/gemm.hip restated in float64 from that file's header comment, the two float32
# arithmetics the product modes claim (exact: a k-ordered float32 chain; fast: the three-way bf16 split of
# csrc/split_bf16.h with six piece products), and operands built so that one missing piece product changes the result.
# tests/test_gpu_product_edges.py compares the kernels with these; tests/test_product_refs_host.py checks them here.
U24 = 2.0 ** -24  # one float32 rounding of a value in [1, 2): the unit of every accuracy figure
SIX_TERMS = ((0, 2), (2, 0), (1, 1), (1, 0), (0, 1), (0, 0))  # (piece of a, piece of w) the kernels multiply


def seg_product_ref(begin, end, operands, bias, bias_off, n_out, trans, act, out0):
    """gcmi_seg_gemm: out[rows_s] = act(a1[rows_s] . w1[s] + a2[rows_s] . w2[s] + bias[s]) in float64.
    operands: up to two (a, w_flat, w_off, k) or None; a is (rows, >= k), the block of segment s starts at
    w_flat[w_off[s]] and is k x n_out (trans: n_out x k, nn.Linear's layout); an offset of -1 means the term is absent.
    bias: flat or None, bias_off[s] = -1: none.  act 0: none, 1: ReLU, 2: out0 + result.  Rows outside every segment
    keep out0.  Returns (out, S): S is the same sum of absolute values (and |out0| under act 2), 0 on untouched rows."""
    out, S = f64(out0).copy(), np.zeros(np.shape(out0), np.float64)
    operands = [None if op is None or op[0] is None else (f64(op[0]), f64(op[1]), op[2], op[3]) for op in operands]
    for s in range(len(begin)):
        r = slice(begin[s], end[s])
        acc = np.zeros((end[s] - begin[s], n_out), np.float64)
        mag = np.zeros_like(acc)
        for op in operands:
            if op is None or op[2][s] < 0:
                continue
            a, w, off, k = op
            blk = w[off[s]:off[s] + k * n_out]
            ws = blk.reshape(n_out, k).T if trans else blk.reshape(k, n_out)
            acc += a[r, :k] @ ws
            mag += np.abs(a[r, :k]) @ np.abs(ws)
        if bias is not None and bias_off[s] >= 0:
            b = f64(bias)[bias_off[s]:bias_off[s] + n_out]
            acc += b
            mag += np.abs(b)
        if act == 1:
            acc = np.maximum(acc, 0.0)
        elif act == 2:
            acc += f64(out0)[r]
            mag += np.abs(f64(out0)[r])
        out[r], S[r] = acc, mag
    return out, S


def seg_wgrad_ref(begin, end, a, g, k, n, dw0, dw_off, dbias0, dbias_off, trans):
    """gcmi_seg_gemm_wgrad: dw[s] += a[rows_s]^T . g[rows_s] (k x n; trans: n x k), dbias[s] += colsum g[rows_s], in
    float64, onto the flat dw0 / dbias0 (dbias0 None: no bias gradient); an offset of -1: not written.  Segments may
    share a block.  Returns (dw, dbias, S_dw, S_dbias): S the same sums of absolute values, starting values included."""
    dw, S = f64(dw0).copy(), np.abs(f64(dw0))
    db = None if dbias0 is None else f64(dbias0).copy()
    Sb = None if dbias0 is None else np.abs(f64(dbias0))
    for s in range(len(begin)):
        ar, gr = f64(a[begin[s]:end[s], :k]), f64(g[begin[s]:end[s], :n])
        if dw_off[s] >= 0:
            p, m = ar.T @ gr, np.abs(ar).T @ np.abs(gr)
            sl = slice(dw_off[s], dw_off[s] + k * n)
            dw[sl] += (p.T if trans else p).reshape(-1)
            S[sl] += (m.T if trans else m).reshape(-1)
        if db is not None and dbias_off[s] >= 0:
            sl = slice(dbias_off[s], dbias_off[s] + n)
            db[sl] += gr.sum(0)
            Sb[sl] += np.abs(gr).sum(0)
    return dw, db, S, Sb


def any_order_exact(S, lsb):
    """The any-order exactness condition: when every term is a multiple of lsb (a power of two) and the sum of their
    absolute values stays below 2^24 lsb, every partial sum in any order is a float32 number -- atomics included."""
    return float(np.max(S, initial=0.0)) < 2.0 ** 24 * lsb


def is_multiple(x, lsb):
    q = f64(x)[np.isfinite(f64(x))] / lsb
    return bool(np.all(q == np.round(q)))


def seq32_product(a, w, acc=None):
    """a . w in float32, accumulated sequentially in contraction order with two roundings per term (the product, then
    the sum), as a loop of numpy float32 operations: deterministic on any host.  acc: continue this sum."""
    a, w = np.asarray(a, np.float32), np.asarray(w, np.float32)
    acc = np.zeros((a.shape[0], w.shape[1]), np.float32) if acc is None else np.asarray(acc, np.float32).copy()
    for kk in range(a.shape[1]):
        acc = (acc + (a[:, kk, None] * w[None, kk, :]).astype(np.float32)).astype(np.float32)
    return acc


def bf16_round(x):
    """float32 -> the nearest bf16 value (ties to even), as a float32 (finite inputs)."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return r.astype(np.uint32).view(np.float32).reshape(np.shape(x))


def split3_np(x):
    """split3_pair of csrc/split_bf16.h: three bf16 pieces by round to nearest even with exact residuals."""
    x = np.asarray(x, np.float32)
    p1 = bf16_round(x)
    r1 = (x - p1).astype(np.float32)
    p2 = bf16_round(r1)
    r2 = (r1 - p2).astype(np.float32)
    return p1, p2, bf16_round(r2)


def split_product_np(a, w, terms=SIX_TERMS, acc=None, group=16):
    """a . w assembled from the piece products ``terms`` (pairs (i, j): piece i of a times piece j of w), one float32
    accumulation per term and 16-wide contraction step, in the order given -- the kernels' loop with each
    32x32x16 product formed exactly and rounded once.  acc: continue this sum.
    group = 8: the 16 products of a step enter the accumulator as two exact sums of 8 with a rounding after each,
    which is what v_mfma_f32_32x32x16_bf16 does on gfx950 (measured through head_bwd_wide_kernel, DESIGN 39: 86 % of
    76 000 outputs bit for bit and 1.2 ulp apart on average, against 15 % and 53 ulp for one rounding per step)."""
    A, W = split3_np(a), split3_np(w)
    acc = np.zeros((np.shape(a)[0], np.shape(w)[1]), np.float32) if acc is None else np.asarray(acc, np.float32).copy()
    for k0 in range(0, np.shape(a)[1], 16):
        for i, j in terms:
            if group == 16:
                blk = A[i][:, k0:k0 + 16].astype(np.float64) @ W[j][k0:k0 + 16].astype(np.float64)
                acc = (acc + blk.astype(np.float32)).astype(np.float32)
                continue
            for g0 in range(k0, k0 + 16, group):
                blk = A[i][:, g0:g0 + group].astype(np.float64) @ W[j][g0:g0 + group].astype(np.float64)
                acc = (acc.astype(np.float64) + blk).astype(np.float32)
    return acc


# Piece probes: entries +-(1 + p 2^-9 + q 2^-17) with random bits p, q split into the pieces (1, p 2^-9, q 2^-17) when
# p = 1 (and (1, q 2^-17, 0) when p = 0), so every product of pieces is a multiple of 2^-17 (2^-18 for two-piece times
# two-piece) and a sum over at most 96 (48) of them meets the any-order condition.  name: (pieces of a, pieces of w,
# longest contraction, lsb, the terms the pair is built to see).  No term outside SIX_TERMS is ever non-zero.
PROBES = {
    "a3w1": (3, 1, 96, 2.0 ** -17, ((0, 0), (1, 0), (2, 0))),
    "a1w3": (1, 3, 96, 2.0 ** -17, ((0, 0), (0, 1), (0, 2))),
    "a2w2": (2, 2, 48, 2.0 ** -18, ((0, 0), (0, 1), (1, 0), (1, 1))),
}


def probe_values(rng, shape, pieces):
    sign = rng.choice(np.array([-1.0, 1.0]), shape)
    p = rng.integers(0, 2, shape) if pieces >= 2 else 0
    q = rng.integers(0, 2, shape) if pieces >= 3 else 0
    return (sign * (1.0 + p * 2.0 ** -9 + q * 2.0 ** -17)).astype(np.float32)


def probe_operands(name, rows, k, n_out, seed, nnz=None):
    """(a (rows, k), w (k, n_out)) of one probe.  nnz: only that many columns of every row of a are non-zero (the
    head's 256-column rows keep the contraction at the probe's length that way)."""
    pa, pw = (PROBES[name] if name in PROBES else BLOCK_PROBES[name])[:2]
    rng = np.random.default_rng(seed)
    a, w = probe_values(rng, (rows, k), pa), probe_values(rng, (k, n_out), pw)
    if nnz is not None and nnz < k:
        keep = np.argsort(rng.random((rows, k)), axis=1)[:, :nnz]
        mask = np.zeros((rows, k), bool)
        np.put_along_axis(mask, keep, True, 1)
        a = np.where(mask, a, np.float32(0.0))
    return a, w


# ------------------------------------------------------------------------------------------------ persistent block kernels
# The forward products of csrc/fwd_fused.hip / csrc/fwd_bf16.hip keep gcmi_seg_gemm's contract (seg_product_ref above) and
# add the column sums of what they store; the one-pass backward of csrc/bwd_fused.hip is restated here from that file's
# header.  tests/test_gpu_fused_edges.py compares the kernels with these; tests/test_fused_refs_host.py checks them here.
BN_REPLICAS = 32  # kBnReplicas: the sums are added into 32 replicas behind 2F unused doubles
# (piece of a, piece of w) each form multiplies, in the kernels' order (small terms first); a = the left operand of the
# product AS WRITTEN HERE: dW = In^T . G (a = In^T, w = G), dIn = G . W^T (a = G, w = W^T), out = a . W
HD_TERMS = ((0, 2), (0, 1), (0, 0))       # fwd_hd_kernel: the stored operand is its own piece x three weight pieces
HB_DW_TERMS = ((0, 1), (0, 0))            # HB: In one piece x the two leading pieces of G
HB_DIN_TERMS = ((1, 0), (0, 1), (0, 0))   # HB: g1 w1 + g1 w2 + g2 w1 (pieces counted from 0 here)
IB_DW_TERMS = ((0, 2), (0, 1), (0, 0))    # IB: In one piece x all three pieces of G
# two-piece against one-piece probes, by the rule of PROBES: products are multiples of 2^-9.  (A table of their own: the
# product tests run every entry of PROBES.)
BLOCK_PROBES = {
    "a2w1": (2, 1, 96, 2.0 ** -9, ((0, 0), (1, 0))),
    "a1w2": (1, 2, 96, 2.0 ** -9, ((0, 0), (0, 1))),
}


def probe_spec(name):
    return PROBES[name] if name in PROBES else BLOCK_PROBES[name]


def readout_dy_ref(g2, arg, membership, n_feat):
    """dy[r, f] = g2[mol(r), f] + (arg[mol(r), f] == r) * g2[mol(r), F + f] in float64; also its magnitude."""
    g2, m = f64(g2), np.asarray(membership, np.int64)
    rows = np.arange(m.shape[0])[:, None]
    hit = np.asarray(arg)[m][:, :n_feat] == rows
    dy = g2[m, :n_feat] + np.where(hit, g2[m, n_feat:2 * n_feat], 0.0)
    return dy, np.abs(g2[m, :n_feat]) + np.where(hit, np.abs(g2[m, n_feat:2 * n_feat]), 0.0)


def block_bwd_ref(begin, end, w_off, b_off, dy, gc, coef, ins, k_in, w, dw0, db0, width, dense, dy_mag=None):
    """The header of csrc/bwd_fused.hip in float64.  G = (gc > 0) (A dy + B gc + C) with coef = [A | B | C] (None:
    (gc > 0) dy); per segment s and operand o (w_off[o][s] >= 0): dW[s][o] += In_o^T G (k_in x width; dense: G^T In,
    width x k_in), dIn_o = G W_o[s]^T; db[s] += colsum G (b_off[s] >= 0; db0 None: no bias gradient).  An absent term
    adds nothing to dW and leaves ZEROS in its rows of dIn_o (the kernel writes the tile it owns); rows outside every
    segment are NaN in dIn.  Returns a dict: G, dw, db, din (list) and the same sums over absolute values S_dw, S_db,
    S_din, where |G| counts |A dy| + |B gc| + |C| (dy_mag: the magnitude of a recomputed dy)."""
    dy, gc = f64(dy), f64(gc)
    n = gc.shape[0]
    dmag = np.abs(dy) if dy_mag is None else f64(dy_mag)
    if coef is None:
        G, Gm = dy.copy(), dmag.copy()
    else:
        A, B, C = (f64(coef)[i * width:(i + 1) * width] for i in range(3))
        G, Gm = A * dy + B * gc + C, np.abs(A) * dmag + np.abs(B * gc) + np.abs(C)
    G, Gm = np.where(gc > 0, G, 0.0), np.where(gc > 0, Gm, 0.0)
    dw, S_dw = f64(dw0).copy(), np.abs(f64(dw0))
    db = None if db0 is None else f64(db0).copy()
    S_db = None if db0 is None else np.abs(f64(db0))
    din = [np.full((n, k_in), np.nan) for _ in ins]
    S_din = [np.zeros((n, k_in)) for _ in ins]
    wf = f64(w)
    for s in range(len(begin)):
        r = slice(begin[s], end[s])
        if end[s] == begin[s]:
            continue
        for o, a in enumerate(ins):
            din[o][r] = 0.0
            off = w_off[o][s]
            if off < 0:
                continue
            ar = f64(a)[r, :k_in]
            p, m = ar.T @ G[r], np.abs(ar).T @ Gm[r]
            sl = slice(off, off + k_in * width)
            dw[sl] += (p.T if dense else p).reshape(-1)
            S_dw[sl] += (m.T if dense else m).reshape(-1)
            ws = wf[sl].reshape(width, k_in).T if dense else wf[sl].reshape(k_in, width)
            din[o][r] = G[r] @ ws.T
            S_din[o][r] = Gm[r] @ np.abs(ws).T
        if db is not None and b_off[s] >= 0:
            db[b_off[s]:b_off[s] + width] += G[r].sum(0)
            S_db[b_off[s]:b_off[s] + width] += Gm[r].sum(0)
    return dict(G=G, Gmag=Gm, dw=dw, db=db, din=din, S_dw=S_dw, S_db=S_db, S_din=S_din)


def g_float32(dy, gc, coef, width):
    """G formed in float32 numpy: (gc > 0) (A dy + (B gc + C)), two roundings where the kernel's fmaf has one."""
    f32 = np.float32
    dy, gc = np.asarray(dy, f32), np.asarray(gc, f32)
    if coef is None:
        G = dy.copy()
    else:
        A, B, C = (np.asarray(coef, f32)[i * width:(i + 1) * width] for i in range(3))
        G = (A * dy + (B * gc + C)).astype(f32)
    return np.where(gc > 0, G, f32(0))


def block_bwd_f32(begin, end, w_off, dy, gc, coef, ins, k_in, w, n_w, width, dense, dw_product, din_product):
    """The same contract with G formed in float32 numpy (two roundings where the kernel fuses) and the products by
    ``dw_product(In^T, G)`` / ``din_product(G, W^T)`` (seq32_product, or split_product_np with a term subset): dW from
    zero (no shared blocks) and the dIn list."""
    f32 = np.float32
    G = g_float32(dy, gc, coef, width)
    dw = np.zeros(n_w, f32)
    din = [np.zeros((G.shape[0], k_in), f32) for _ in ins]
    for s in range(len(begin)):
        r = slice(begin[s], end[s])
        if end[s] == begin[s]:
            continue
        for o, a in enumerate(ins):
            off = w_off[o][s]
            if off < 0:
                continue
            ar = np.asarray(a, f32)[r, :k_in]
            p = dw_product(np.ascontiguousarray(ar.T), G[r])
            sl = slice(off, off + k_in * width)
            dw[sl] += (p.T if dense else p).reshape(-1)
            ws = np.asarray(w, f32)[sl]
            ws = ws.reshape(width, k_in).T if dense else ws.reshape(k_in, width)
            din[o][r] = din_product(G[r], np.ascontiguousarray(ws.T))
    return dw, din


def psums_ref(begin, end, din, ins, k_in, conv):
    """(2, k_in) float64: conv -- sum over the rows of (s dS + dXs) and of (dS S + dXs X), s = the row's SEGMENT INDEX
    (the degree); dense -- sum dP and sum dP P.  din: the input gradients AS STORED (rounded under GB)."""
    out = np.zeros((2, k_in))
    for s in range(len(begin)):
        r = slice(begin[s], end[s])
        for o, (d, a) in enumerate(zip(din, ins)):
            wgt = float(s) if (conv and o == 0) else 1.0
            out[0] += wgt * f64(d)[r, :k_in].sum(0)
            out[1] += (f64(d)[r, :k_in] * f64(a)[r, :k_in]).sum(0)
    return out


def psums_mag(begin, end, din, ins, k_in, conv):
    out = np.zeros((2, k_in))
    for s in range(len(begin)):
        r = slice(begin[s], end[s])
        for o, (d, a) in enumerate(zip(din, ins)):
            wgt = float(s) if (conv and o == 0) else 1.0
            out[0] += wgt * np.abs(f64(d)[r, :k_in]).sum(0)
            out[1] += np.abs(f64(d)[r, :k_in] * f64(a)[r, :k_in]).sum(0)
    return out


def bn_sums_ref(out_stored, covered):
    """(2, F) float64: column sums of out and out^2 over the covered rows, of the values as stored."""
    v = f64(out_stored)[np.asarray(covered, bool)]
    return np.stack([v.sum(0), (v * v).sum(0)])


def read_acc(acc, n_feat, sentinel):
    """An accumulator in the layout [2F unused][BN_REPLICAS][F | F] that started as: sentinel in the first 2F doubles,
    zeros in the replicas, sentinel in everything behind them.  Returns the (2, F) sum of the replicas after asserting
    that both sentinel regions are untouched."""
    acc = f64(acc).reshape(-1)
    F2 = 2 * n_feat
    assert np.all(acc[:F2] == sentinel), "the first 2F doubles of an accumulator were written"
    assert np.all(acc[F2 * (1 + BN_REPLICAS):] == sentinel), "doubles past the last replica were written"
    return acc[F2:F2 * (1 + BN_REPLICAS)].reshape(BN_REPLICAS, 2, n_feat).sum(0)


def fresh_acc(n_feat, sentinel, pad=64):
    acc = np.full(2 * n_feat * (1 + BN_REPLICAS) + pad, sentinel, np.float64)
    acc[2 * n_feat:2 * n_feat * (1 + BN_REPLICAS)] = 0.0
    return acc


def seq32_colsum(values, chunk, weights=None, other=None):
    """Column sums as a float32 chain over ``chunk`` rows at a time (one rounding per add; with ``other`` the terms are
    values * other, with ``weights`` weights * values, each rounded once as a fused multiply-add does), the chunks added
    in float64: the arithmetic of the kernels' periodic flush with one thread per column."""
    v = np.asarray(values, np.float32).astype(np.float64)
    if other is not None:
        v = v * np.asarray(other, np.float32).astype(np.float64)
    if weights is not None:
        v = v * np.asarray(weights, np.float64)[:, None]
    total = np.zeros(v.shape[1])
    for c0 in range(0, v.shape[0], chunk):
        acc = np.zeros(v.shape[1], np.float32)
        for row in v[c0:c0 + chunk]:
            acc = (acc.astype(np.float64) + row).astype(np.float32)
        total += acc
    return total


def cancelling_probe(rng, rows, k, n_out, piece):
    """(a (rows, k), w (k, n_out)) for a kernel that rounds its output to bf16, where a plain probe's sum of up to 96
    terms would not survive the rounding: a = +-1 in equal adjacent pairs, w in adjacent pairs of opposite sign, so
    that the leading parts cancel and the result is a small multiple of one power of two, exact in bf16.
    piece 1: w = +-(1 + p 2^-9), the result is n 2^-9 and sees (0, 1); piece 2: w = +-(1 + 2^-9 + q 2^-17), the result
    is m 2^-17 and sees (0, 2).  |n|, |m| <= k / 2 <= 48.  Returns (a, w, lsb)."""
    assert k % 2 == 0 and k <= 96
    a = np.repeat(rng.choice(np.array([-1.0, 1.0]), (rows, k // 2)), 2, axis=1)
    s = np.repeat(rng.choice(np.array([-1.0, 1.0]), (k // 2, n_out)), 2, axis=0)
    s[1::2] *= -1.0
    bit = rng.integers(0, 2, (k, n_out))
    if piece == 1:
        return a.astype(np.float32), (s * (1.0 + bit * 2.0 ** -9)).astype(np.float32), 2.0 ** -9
    return a.astype(np.float32), (s * (1.0 + 2.0 ** -9 + bit * 2.0 ** -17)).astype(np.float32), 2.0 ** -17


# ------------------------------------------------------------------------------------------------ per-molecule head backward
# csrc/head_bwd.hip (head_bwd_kernel; head_prep_kernel + head_bwd_wide_kernel + head_wgrad_wide_kernel) restated from the
# formulas of the layers it replaces: the loss of models/losses.py on logits = tanh(pre) . W^T + b, the gradients w.r.t.
# W, b and pre, and the column sums of the dense BatchNorm's backward taken from per-molecule data.
# tests/test_gpu_head_bwd.py compares the kernels with these; tests/test_head_refs_host.py checks them on the host.
LOSS_REPLICAS = 16  # kLossRep: the loss is added into any of 16 doubles
HEAD_K = 256        # fingerprint columns: [sum half | max half] of the 128-column dense layer
MFMA_GROUP = 8      # contraction columns per rounding inside one 32x32x16 bf16 product (split_product_np)
TINY32 = 2.0 ** -102  # a magnitude below it cannot be resolved to 2^-24 of itself inside float32's normal range (2^-126)


def head_bwd_ref(kind, logits, labels, weights, n_rows, fp, w, sums_inputs=None):
    """kind 0: logits / labels (>= n_rows, n_tasks, n_classes), softmax cross-entropy over the classes; kind 1: (>= n_rows,
    n_tasks), L2; weights (>= n_rows, n_tasks) or None.  The first n_rows of the fp.shape[0] molecules carry a loss;
    fp (n_mols, 256) = tanh(pre), w (outputs, 256).  Float64 throughout.  Returns a dict:
      loss  the SUM of w l over rows and tasks (the mean loss times n_rows n_tasks, which is what the kernels add into
            their accumulator), dl (n_mols, outputs) = d mean loss / d logits, zero rows for the padding molecules,
      g2 = (dl W) (1 - fp^2) = d / d pre, dw = dl^T fp, db = column sums of dl,
      sums  (2, 128), with sums_inputs = dict(runs, arg, rawsum, mean, invstd): head_sums_ref of this g2,
    and for every output the sum of the absolute values of its terms as S_loss, S_dl, S_g2, S_dw, S_db, S_sums."""
    x, y = f64(logits)[:n_rows], f64(labels)[:n_rows]
    wt = None if weights is None else f64(weights)[:n_rows]
    n_mols = fp.shape[0]
    count = x.shape[0] * x.shape[1]
    wa = np.ones(x.shape[:2]) if wt is None else np.abs(wt)
    if kind == 0:
        _, dl_rows, p = ce_loss_ref(x, y, wt)
        terms = (wa if wt is None else wt) * -(y * log_softmax_ref(x)).sum(-1)
        S_loss = float((wa * np.abs(y * log_softmax_ref(x)).sum(-1)).sum())
        S_rows = wa[..., None] * (p * np.abs(y.sum(-1, keepdims=True)) + np.abs(y)) / count
    else:
        _, dl_rows = l2_loss_ref(x, y, wt)
        terms = (wa if wt is None else wt) * (x - y) ** 2
        S_loss = float((wa * (x - y) ** 2).sum())
        S_rows = 2.0 * wa * (np.abs(x) + np.abs(y)) / count
    tc = dl_rows[0].size
    dl, S_dl = np.zeros((n_mols, tc)), np.zeros((n_mols, tc))
    dl[:n_rows], S_dl[:n_rows] = dl_rows.reshape(n_rows, tc), S_rows.reshape(n_rows, tc)
    fp, w = f64(fp), f64(w)
    out = dict(loss=float(terms.sum()), S_loss=S_loss, dl=dl, S_dl=S_dl)  # (the sum itself: no division to undo)
    out.update(head_linear_ref(dl, S_dl, fp, w))
    if sums_inputs is not None:
        out["sums"], out["S_sums"] = head_sums_ref(out["g2"], sums_inputs)
    return out


def head_linear_ref(dl, S_dl, fp, w):
    """The outputs that are linear in d logits, from ANY d logits (the reference's, or the ones a kernel returned): g2,
    dw, db and their magnitudes in float64."""
    dl, S_dl, fp, w = f64(dl), f64(S_dl), f64(fp), f64(w)
    return dict(g2=(dl @ w) * (1.0 - fp * fp), S_g2=(S_dl @ np.abs(w)) * (1.0 + fp * fp),
                dw=dl.T @ fp, S_dw=S_dl.T @ np.abs(fp), db=dl.sum(0), S_db=S_dl.sum(0))


def _head_sums_terms(g2, si, dtype):
    """Per molecule and column the four terms of the two sums: (n g_sum, [arg >= 0] g_max, g_sum xhat_sum, [arg >= 0] g_max
    xhat_max) with xhat_sum = (rawsum - n mean) invstd, xhat_max = (rawmax - mean) invstd, and the magnitudes of the last
    two.  rawsum's max half is not looked at where arg < 0."""
    g = np.asarray(g2, dtype)
    runs = np.asarray(si["runs"], np.int64)
    n = (runs[:, :, 1] - runs[:, :, 0]).sum(1).astype(dtype)[:, None]
    rs, mu, ist = np.asarray(si["rawsum"], dtype), np.asarray(si["mean"], dtype), np.asarray(si["invstd"], dtype)
    has = np.asarray(si["arg"]) >= 0
    F = HEAD_K // 2
    rmax = np.where(has, rs[:, F:], dtype(0))
    gs, gm = g[:, :F], np.where(has, g[:, F:], dtype(0))
    terms = (n * gs, gm, gs * ((rs[:, :F] - n * mu) * ist), gm * ((rmax - mu) * ist))
    mags = (np.abs(gs) * (np.abs(rs[:, :F]) + n * np.abs(mu)) * np.abs(ist), np.abs(gm) * (np.abs(rmax) + np.abs(mu)) * np.abs(ist))
    return terms, mags


def head_sums_ref(g2, si):
    """(2, 128): sum over the atom rows of dy and of dy * xhat from per-molecule data, formed and added pairwise in the
    host's extended precision (64-bit significand: a sum of 25 000 terms is good to a hundredth of 2^-53 of S), returned
    in that precision; and S (float64)."""
    assert np.finfo(np.longdouble).nmant >= 63, "no extended precision on this host"
    (a1, b1, a2, b2), (ma, mb) = _head_sums_terms(g2, si, np.longdouble)
    sums = np.stack([a1.sum(0) + b1.sum(0), a2.sum(0) + b2.sum(0)])
    S = np.stack([np.abs(a1).sum(0) + np.abs(b1).sum(0), ma.sum(0) + mb.sum(0)]).astype(np.float64)
    return sums, S


def head_sums_seq64(g2, si, reverse=True):
    """The same sums as two sequential float64 chains per column (the sum half, the max half; one rounding per
    operation), over the molecules in reversed order, added at the end: the e_ref of the kernels' fp64 sums."""
    (a1, b1, a2, b2), _ = _head_sums_terms(g2, si, np.float64)
    order = range(a1.shape[0] - 1, -1, -1) if reverse else range(a1.shape[0])
    t = np.zeros((4, HEAD_K // 2))
    for m in order:
        t[0] += a1[m]
        t[1] += b1[m]
        t[2] += a2[m]
        t[3] += b2[m]
    return np.stack([t[0] + t[1], t[2] + t[3]])


def _fma32(a, b, c):
    """fmaf: a * b is exact in float64, the sum is rounded to float64 and then to float32 (a double rounding is rare)."""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def head_dl_f32(kind, logits, labels, weights, n_rows, two_class_fast):
    """Loss and d logits in float32 numpy, one rounding per operation, in the order of head_bwd_kernel's phase 1;
    two_class_fast: the one-exponential form of head_bwd_wide_kernel for two classes.  Returns (sum of the float32
    terms w l in float64, dl_rows (n_rows, outputs) float32)."""
    f32 = np.float32
    x, y = np.asarray(logits, f32)[:n_rows], np.asarray(labels, f32)[:n_rows]
    w = np.ones(x.shape[:2], f32) if weights is None else np.asarray(weights, f32)[:n_rows]
    inv = f32(1.0) / f32(x.shape[0] * x.shape[1])
    if kind == 1:
        dlt = x - y
        loss = float(((w * dlt) * dlt).astype(np.float64).sum())
        return loss, (((f32(2.0) * dlt) * w) * inv).reshape(n_rows, -1)
    C = x.shape[2]
    if two_class_fast and C == 2:
        x0, x1, y0, y1 = x[..., 0], x[..., 1], y[..., 0], y[..., 1]
        first = x0 >= x1
        dd = np.where(first, x1 - x0, x0 - x1)
        e = np.exp(dd)
        se = f32(1.0) + e
        lse = np.log(se)
        invs = f32(1.0) / se
        lp_max, lp_oth, p_max, p_oth = -lse, dd - lse, invs, e * invs
        lp = np.stack([np.where(first, lp_max, lp_oth), np.where(first, lp_oth, lp_max)], -1)
        p = np.stack([np.where(first, p_max, p_oth), np.where(first, p_oth, p_max)], -1)
        ysum = y0 + y1
        l = -(y0 * lp[..., 0]) - y1 * lp[..., 1]
    else:
        mx = x.max(-1)
        se, ysum = np.zeros(mx.shape, f32), np.zeros(mx.shape, f32)
        for c in range(C):
            se = se + np.exp(x[..., c] - mx)
            ysum = ysum + y[..., c]
        lse = np.log(se)
        lp = (x - mx[..., None]) - lse[..., None]
        p = np.exp(lp)
        l = np.zeros(mx.shape, f32)
        for c in range(C):
            l = l - y[..., c] * lp[..., c]
    assert lp.dtype == f32 and p.dtype == f32 and l.dtype == f32
    dl = (w[..., None] * (p * ysum[..., None] - y)) * inv
    return float((w * l).astype(np.float64).sum()), dl.reshape(n_rows, -1)


def head_bwd_f32(kind, logits, labels, weights, n_rows, fp, w, wide):
    """head_bwd_ref's chain in sequential float32 (numpy's float32 exp / log, one rounding per operation): the e_ref of
    the accuracy bounds.  wide False: the order of head_bwd_kernel -- dfp a fused-multiply-add chain over the outputs,
    dw such a chain over the molecules, db a chain of adds.  wide True: the two products by split_product_np with the six
    piece terms and the instruction's two roundings per step (dl . W over the outputs, dl^T . fp over the molecules),
    the two-class loss in its one-exponential form.  Returns dict(loss, dl, g2, dw, db)."""
    f32 = np.float32
    fp, w = np.asarray(fp, f32), np.asarray(w, f32)
    n_mols = fp.shape[0]
    loss, dl_rows = head_dl_f32(kind, logits, labels, weights, n_rows, wide)
    dl = np.zeros((n_mols, dl_rows.shape[1]), f32)
    dl[:n_rows] = dl_rows
    return dict(loss=loss, dl=dl, **head_linear_f32(dl, fp, w, wide))


def head_linear_f32(dl, fp, w, wide):
    """g2, dw, db from given float32 d logits in the float32 arithmetic head_bwd_f32 describes."""
    f32 = np.float32
    dl, fp, w = np.asarray(dl, f32), np.asarray(fp, f32), np.asarray(w, f32)
    n_mols, tc = dl.shape
    if wide:
        dfp = split_product_np(dl, w, group=MFMA_GROUP)
        dw = split_product_np(np.ascontiguousarray(dl.T), fp, group=MFMA_GROUP)
    else:
        dfp = np.zeros((n_mols, HEAD_K), f32)
        for t in range(tc):
            dfp = _fma32(dl[:, t, None], w[None, t, :], dfp)
        dw = np.zeros((tc, HEAD_K), f32)
        for m in range(n_mols):
            dw = _fma32(dl[m, :, None], fp[None, m, :], dw)
    db = np.zeros(tc, f32)
    for m in range(n_mols):
        db = db + dl[m]
    g2 = dfp * (f32(1.0) - fp * fp)
    assert g2.dtype == f32 and db.dtype == f32
    return dict(g2=g2, dw=dw, db=db)


def head_err_units(got, ref, S, unit=U24):
    """max |got - ref| / max(S, TINY32) over the elements with S > 0, in units of ``unit``; the others must be zero."""
    got, S = np.asarray(got), f64(S)
    m = S > 0
    assert np.all(got[~m] == 0), "an output without any term is not zero"
    if not m.any():
        return 0.0
    diff = np.abs(np.asarray(got[m], np.longdouble) - np.asarray(ref, np.longdouble)[m]).astype(np.float64)
    return float((diff / np.maximum(S[m], TINY32)).max() / unit)


# ------------------------------------------------------------------------------------------------ direct gather kernels
# csrc/gather.hip: the kernels behind gcmi_gather_sum_fwd, gcmi_scatter_add, gcmi_gather_max_fwd, gcmi_gather_max_bwd and
# gcmi_build_rev_pos wherever no window pass runs.  neigh_sum, pool_max, pool_bwd and candidate_value above are their
# restatements too (the direct kernels add in float32 in neighbour-table order); below: the two scatter forms, which need
# no reverse table, the launch geometry, the vector-width rule, and the named batches of tests/test_gpu_direct_ops.py.
# tests/test_direct_refs_host.py checks all of it without a device.
DIRECT_SLOTS = 256 * 4  # kBlock * kUnroll lane slots per workgroup; one row takes lpr = n_feat / V of them


def direct_tiles(deg_counts, lpr, skip_deg0):
    """make_tiles: per degree (first workgroup, workgroups, slots in the last workgroup); a block without rows (or the
    skipped degree-0 block of the accumulate and scatter forms) has no workgroup and shares its start with the next."""
    out, first = [], 0
    for d, c in enumerate(deg_counts):
        slots = 0 if (skip_deg0 and d == 0) else int(c) * lpr
        n = -(-slots // DIRECT_SLOTS)
        out.append((first, n, slots - (n - 1) * DIRECT_SLOTS if n else 0))
        first += n
    return out


def direct_vec(ptr, ld, n_feat):
    """vec_width: four floats per lane only for a 16-byte aligned pointer, ld % 4 == 0 and n_feat % 4 == 0."""
    return 4 if (ptr % 16 == 0 and ld % 4 == 0 and n_feat % 4 == 0) else 1


class NeighbourTables:
    """HostGraph without the reverse positions: only ``nb``, so a bond may be listed from one end.  neigh_sum, pool_max,
    candidate_value, plant_winners, scatter_ref and pool_bwd_scatter take either."""

    def __init__(self, deg_counts, col_idx):
        self.deg_counts = [int(c) for c in deg_counts]
        col_idx = np.asarray(col_idx, np.int64)
        self.n_atoms = sum(self.deg_counts)
        self.row0, self.nb = [], []
        r = e = 0
        for d, c in enumerate(self.deg_counts):
            self.row0.append(r)
            self.nb.append(col_idx[e:e + c * d].reshape(c, d))
            r += c
            e += c * d
        assert e == col_idx.shape[0]
        self.max_present = max([d for d, c in enumerate(self.deg_counts) if c] + [0])

    def rows(self, d):
        return np.arange(self.row0[d], self.row0[d] + self.deg_counts[d])

    def degree_blocks(self):
        return [(d, self.rows(d), self.nb[d], None) for d, c in enumerate(self.deg_counts) if c]


def scatter_ref(hg, ds, dx0=None):
    """dx[nb(i, j)] += ds[i] for every neighbour entry, onto dx0 (zeros), in the dtype of ds: the transpose of neigh_sum
    whatever the adjacency.  (The order of the additions is numpy's; compare bit for bit only where any order is exact.)"""
    dx = np.zeros_like(ds) if dx0 is None else np.array(dx0, ds.dtype)
    for d, rows, nb, _ in hg.degree_blocks():
        for j in range(d):
            np.add.at(dx, nb[:, j], ds[rows])
    assert dx.dtype == ds.dtype
    return dx


def pool_bwd_scatter(hg, g, arg):
    """The GraphPool backward as a scatter: g[i, f] goes to row i where arg[i, f] == 0 and to neighbour arg[i, f] - 1 of
    i otherwise, in the dtype of g.  No reverse table."""
    dx = np.zeros_like(g)
    cols = np.broadcast_to(np.arange(g.shape[1])[None, :], (1, g.shape[1]))
    for d, rows, nb, _ in hg.degree_blocks():
        a = arg[rows].astype(np.int64)
        assert a.max(initial=0) <= d, "arg byte above the degree"
        src = np.concatenate([rows[:, None], nb], 1)
        target = np.take_along_axis(src, a, 1)
        np.add.at(dx, (target, np.broadcast_to(cols, target.shape)), g[rows])
    assert dx.dtype == g.dtype
    return dx


def collate_adjs(adjs, max_deg=10):
    """Per-molecule adjacency lists (molecule-local ids) -> (deg_counts, col_idx, membership) in the collated layout:
    rows sorted by degree, then by molecule, then by the atom's place in its molecule -- one stable sort by degree."""
    sizes = np.array([len(a) for a in adjs], np.int64)
    off = np.concatenate([[0], np.cumsum(sizes)])
    lists = [[int(off[m]) + int(j) for j in nb] for m, a in enumerate(adjs) for nb in a]
    deg = np.array([len(l) for l in lists], np.int64)
    assert deg.max(initial=0) <= max_deg
    order = np.argsort(deg, kind="stable")
    new = np.empty(deg.shape[0], np.int64)
    new[order] = np.arange(deg.shape[0])
    col = np.array([new[j] for k in order for j in lists[k]], np.int32)
    membership = np.repeat(np.arange(len(adjs)), sizes)[order].astype(np.int32)
    return [int(c) for c in np.bincount(deg, minlength=max_deg + 1)], col, membership


def packed_from_adjs(adjs, n_feat=4):
    """The same molecules as a PackedMols (zero features), for the project's own host collations."""
    from deepchem_amd.utils.synthetic import PackedMols
    sizes = np.array([len(a) for a in adjs], np.int64)
    atom_ptr = np.zeros(len(adjs) + 1, np.int64)
    np.cumsum(sizes, out=atom_ptr[1:])
    deg = np.array([len(nb) for a in adjs for nb in a], np.int64)
    adj_ptr = np.zeros(deg.shape[0] + 1, np.int64)
    np.cumsum(deg, out=adj_ptr[1:])
    adj_idx = np.array([j for a in adjs for nb in a for j in nb], np.int32)
    return PackedMols(np.zeros((int(atom_ptr[-1]), n_feat), np.float32), atom_ptr, adj_ptr, adj_idx)


def adjs_of_packed(packed):
    return [packed.molecule(m)[1] for m in range(packed.n_mols)]


def chain_adj(n):
    return [[j for j in (i - 1, i + 1) if 0 <= j < n] for i in range(n)]


def star_adj(arms):
    return [list(range(1, arms + 1))] + [[0] for _ in range(arms)]


LONE_ADJ = [[]]
DOUBLE_BOND_ADJ = [[1, 1, 2], [0, 0], [0]]  # a lists b twice and b lists a twice; c hangs on a


def null_adj(max_deg=10):
    """The reference's null molecule: one atom per degree, bonded to itself that many times."""
    return [d * [d] for d in range(max_deg + 1)]


TILE_ROWS = {"tile_exact": 64, "tile_plus": 65, "tile_minus": 63}  # rows in the degree-0, -1 and -2 blocks


def _tile_adjs(k):
    """Lone atoms, two-atom molecules, two chains and stars of three such that the blocks of degree 0, 1 and 2 hold
    exactly k rows each: 2 stars for an even k and 1 for an odd one (3 degree-1 rows each), two chains (4), the rest of
    the degree-1 rows in pairs; the chains carry the k degree-2 rows.  Shuffled by a fixed seed."""
    stars = 2 - k % 2
    pairs = (k - 4 - 3 * stars) // 2
    mols = [LONE_ADJ] * k + [star_adj(3)] * stars + [chain_adj(2)] * pairs + [chain_adj(2 + k // 2), chain_adj(2 + k - k // 2)]
    order = np.random.RandomState(k).permutation(len(mols))
    return [mols[i] for i in order]


def direct_batch_adjs(name):
    """(adjacency lists, max_deg) of the named batches of tests/test_gpu_direct_ops.py."""
    from deepchem_amd.utils.synthetic import concat_packed, single_atom_and_edge_cases, synthetic_molecules
    if name == "mixed":
        return adjs_of_packed(concat_packed([synthetic_molecules(40, seed=3, max_atoms=40),
                                             single_atom_and_edge_cases(75, 1)])), 10
    if name in TILE_ROWS:
        return _tile_adjs(TILE_ROWS[name]), 10
    if name == "gappy":
        return ([LONE_ADJ] * 3 + [star_adj(4)] * 4) * 5, 10
    if name == "high_only":
        return [star_adj(10)] * 7, 10
    if name == "lone":
        return [LONE_ADJ] * 300, 10
    if name == "shallow2":
        return [chain_adj(n) for n in (2, 3, 5, 8, 13, 21, 2, 40, 7)], 2
    if name == "shallow0":
        return [LONE_ADJ] * 37, 0
    ordinary = [chain_adj(5), star_adj(3), chain_adj(2), LONE_ADJ, star_adj(10), chain_adj(9)]
    if name == "multi":
        return ordinary[:3] + [null_adj(), DOUBLE_BOND_ADJ] + ordinary[3:] + [null_adj(), DOUBLE_BOND_ADJ, chain_adj(4)], 10
    if name == "one_sided":
        return ordinary + [[[1], []]] + adjs_of_packed(synthetic_molecules(12, seed=5, max_atoms=30)), 10
    raise KeyError(name)


DIRECT_BATCHES = ("mixed", "tile_exact", "tile_plus", "tile_minus", "gappy", "high_only", "lone", "shallow2", "shallow0",
                  "multi", "one_sided")
DIRECT_LPR = (1, 16, 17, 19, 64, 2, 7, 75)  # the widths 4, 64, 68, 76, 256 in fours and 1, 2, 7, 75 (and 64) singly


def direct_batch_check(name, deg_counts, col_idx):
    """What the named batch is there for, asserted from its degree counts, direct_tiles and the neighbour tables."""
    counts = [int(c) for c in deg_counts]
    present = [d for d, c in enumerate(counts) if c]
    n_edges = sum(d * c for d, c in enumerate(counts))
    assert n_edges == len(col_idx)
    t16, t16s = direct_tiles(counts, 16, False), direct_tiles(counts, 16, True)
    if name == "mixed":
        assert present == [0, 1, 2, 3, 4, 6, 10]
        assert direct_tiles(counts, 64, False)[2][1] > 1  # a degree block of several workgroups at 256 columns
    elif name in TILE_ROWS:
        k = TILE_ROWS[name]
        assert counts[:3] == [k, k, k]
        # lpr 16: 64 rows are 1024 slots -- one full workgroup; one slot-row more or fewer
        last = {64: (1, DIRECT_SLOTS), 65: (2, 16), 63: (1, DIRECT_SLOTS - 16)}[k]
        assert [t[1:] for t in t16[:3]] == [last] * 3
        assert t16[1][0] == last[0] and t16s[1][0] == 0 and t16s[0][1:] == (0, 0)
        for lpr in (17, 19, 75):  # a row straddles two unroll steps (256 slots) and, at these counts, two workgroups
            assert 256 % lpr and DIRECT_SLOTS % lpr and k * lpr > DIRECT_SLOTS
            assert direct_tiles(counts, lpr, False)[1][1] == -(-k * lpr // DIRECT_SLOTS) >= 2
        assert direct_tiles(counts, 1, False)[1][1:] == (1, k)
    elif name == "gappy":
        assert present == [0, 1, 4]
    elif name == "high_only":
        assert present == [1, 10] and counts[0] == 0
        assert t16s[0][1] == 0 and t16[0][1] == 0  # an empty degree-0 block, skipped or not
        assert all(t16[d][1] == 0 and t16[d][0] == t16[10][0] for d in range(2, 10))  # block_degree jumps 2..9
    elif name == "lone":
        assert present == [0] and len(counts) == 11 and n_edges == 0
        assert sum(t[1] for t in t16s) == 0 and t16[0][1] > 1  # the accumulate form launches nothing
    elif name == "shallow2":
        assert len(counts) == 3 and present == [1, 2]
    elif name == "shallow0":
        assert len(counts) == 1 and present == [0] and n_edges == 0
    elif name == "multi":
        nt = NeighbourTables(counts, col_idx)
        assert present == list(range(11))
        loops = [int((nt.nb[d] == nt.rows(d)[:, None]).all(1).sum()) for d in range(11)]
        assert loops[1:] == [2] * 10  # two null molecules: per degree d two atoms listing themselves d times
        twice = sum(int(((nb[:, :, None] == nb[:, None, :]).sum((1, 2)) > nb.shape[1]).sum()) for nb in nt.nb[2:])
        assert twice >= 2 * 2 + 2 * 9  # rows with a repeated neighbour: both ends of both double bonds, and the loops
    elif name == "one_sided":
        nt = NeighbourTables(counts, col_idx)
        src = np.concatenate([np.repeat(nt.rows(d), d) for d in range(len(counts))])
        dst = np.concatenate([nb.reshape(-1) for nb in nt.nb])
        fwd, bwd = np.sort(src * nt.n_atoms + dst), np.sort(dst * nt.n_atoms + src)
        assert len(np.setdiff1d(fwd, bwd)) == 1 and counts[0] > 0 and counts[10] > 0  # exactly one bond without its mate
    else:
        raise KeyError(name)
    return True
