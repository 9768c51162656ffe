"""Float64 restatements of the small primitive kernels (csrc/bn.hip, csrc/readout.hip, csrc/loss.hip), written from
the formulas of the layers they replace and used by tests/test_gpu_bn_edges.py, tests/test_gpu_readout_edges.py and
tests/test_gpu_loss_edges.py.  Plain numpy on the CPU: no kernel of this project and no float32 library routine.
tests/test_edge_refs_host.py checks them without a device (against torch in float64 and the oracle) together with
the exactness conditions the GPU tests lean on.
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
