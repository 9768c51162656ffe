"""The kernels of synchronised BatchNorm on their own (csrc/bn.hip: bn_collapse_kernel, bn_finalize_sync_kernel,
bn_bwd_coef_sync_kernel, through the gcmi_bn_sync_* entry points): the sums of one batch taken in two parts, as two
ranks would take them, summed as the exchange would sum them, give what the existing kernels give on the whole batch.
Both sides finalise fp64 sums once, so the bound is 1e-6 relative."""
import ctypes

import pytest
import torch

from deepchem_amd import _lib
from deepchem_amd.graph import _stream

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS, MOM = 1e-3, 0.99


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _acc(F):
    return torch.full((66 * F,), 3.0, dtype=torch.float64, device=DEV)  # (dirty: the entry points clear it themselves)


def _close(a, b, what):
    a, b = a.double(), b.double()
    scale = max(float(b.abs().max()), 1e-30)
    assert float((a - b).abs().max()) <= 1e-6 * scale, (what, float((a - b).abs().max()), scale)


def _data(N, F, seed):
    gen = torch.Generator().manual_seed(seed)
    x = (torch.randn((N, F), generator=gen) * 1.5 + 0.7).relu().to(DEV)
    dy = torch.randn((N, F), generator=gen).to(DEV)
    gamma = (torch.rand(F, generator=gen) + 0.5).to(DEV)
    beta = (torch.randn(F, generator=gen) * 0.1).to(DEV)
    return x.contiguous(), dy.contiguous(), gamma, beta


def _whole_forward(x, gamma, beta):
    N, F = x.shape
    out = {k: torch.zeros(F, device=DEV) for k in ("mean", "invstd", "scale", "shift")}
    out["rm"] = torch.full((F,), 0.25, device=DEV)
    out["rv"] = torch.full((F,), 2.0, device=DEV)
    _lib.call("gcmi_bn_stats", _p(x), F, N, F, _p(gamma), _p(beta), EPS, MOM, _p(out["rm"]), _p(out["rv"]), _p(out["mean"]),
              _p(out["invstd"]), _p(out["scale"]), _p(out["shift"]), _p(_acc(F)), _stream())
    return out


@pytest.mark.parametrize("N,F,cut", [(1000, 64, 600), (4099, 128, 1), (700, 64, 0)])
def test_split_sums_finalise_to_the_whole_batch_statistics(N, F, cut):
    """cut = 0: one part has no rows at all (a rank without atoms) and contributes zero sums and count 0."""
    x, _, gamma, beta = _data(N, F, 3)
    whole = _whole_forward(x, gamma, beta)
    bufs = []
    for part in (x[:cut], x[cut:]):
        part = part.contiguous()
        acc, xb = _acc(F), torch.full((2 * F + 1,), -1.0, dtype=torch.float64, device=DEV)
        _lib.call("gcmi_bn_sync_sums", _p(part) if part.shape[0] else None, F, part.shape[0], F, _p(acc), _p(xb), _stream())
        assert float(acc[2 * F:].abs().max()) == 0.0, "the replicas must be clean afterwards"
        assert float(xb[2 * F]) == part.shape[0]
        if part.shape[0] == 0:
            assert float(xb.abs().max()) == 0.0
        bufs.append(xb)
    summed = bufs[0] + bufs[1]
    assert float(summed[2 * F]) == N
    got = {k: torch.zeros(F, device=DEV) for k in ("mean", "invstd", "scale", "shift")}
    got["rm"] = torch.full((F,), 0.25, device=DEV)
    got["rv"] = torch.full((F,), 2.0, device=DEV)
    tracked = torch.full((), 4, dtype=torch.int64, device=DEV)
    _lib.call("gcmi_bn_sync_finalize", _p(summed), F, _p(gamma), _p(beta), EPS, MOM, _p(got["rm"]), _p(got["rv"]),
              _p(got["mean"]), _p(got["invstd"]), _p(got["scale"]), _p(got["shift"]), _p(tracked), _stream())
    torch.cuda.synchronize()
    assert int(tracked) == 5
    for k in whole:
        _close(got[k], whole[k], k)
    # and against the definition (torch, float64): unbiased variance with the GLOBAL count into running_var
    xd = x.double()
    _close(got["mean"], xd.mean(0), "mean vs torch")
    _close(got["rv"], 0.01 * 2.0 + 0.99 * xd.var(0, unbiased=True), "running_var vs torch")


def test_zero_and_one_global_rows_do_not_divide_by_zero():
    F = 64
    _, _, gamma, beta = _data(4, F, 5)
    for n in (0.0, 1.0):
        xb = torch.zeros(2 * F + 1, dtype=torch.float64, device=DEV)
        xb[:F] = 0.5 * n
        xb[F:2 * F] = 0.25 * n
        xb[2 * F] = n
        rm, rv = torch.full((F,), 0.25, device=DEV), torch.full((F,), 2.0, device=DEV)
        outs = [torch.full((F,), 7.0, device=DEV) for _ in range(4)]
        tracked = torch.zeros((), dtype=torch.int64, device=DEV)
        _lib.call("gcmi_bn_sync_finalize", _p(xb), F, _p(gamma), _p(beta), EPS, MOM, _p(rm), _p(rv), _p(outs[0]), _p(outs[1]),
                  _p(outs[2]), _p(outs[3]), _p(tracked), _stream())
        coef = torch.full((3 * F,), 7.0, device=DEV)
        mean, invstd = torch.full((F,), 0.5, device=DEV), torch.ones(F, device=DEV)
        _lib.call("gcmi_bn_sync_bwd_coef", _p(xb), F, _p(gamma), _p(mean), _p(invstd), _p(coef), _stream())
        torch.cuda.synchronize()
        assert int(tracked) == 1
        assert bool(torch.isfinite(rm).all()) and bool(torch.isfinite(rv).all()) and bool(torch.isfinite(coef).all())
        if n == 0.0:  # as a batch without atoms: nothing but the counter moves
            assert bool((rm == 0.25).all()) and bool((rv == 2.0).all()) and all(bool((o == 7.0).all()) for o in outs)
        else:  # one row: variance 0, and it goes into running_var as it is
            assert torch.allclose(rv, torch.full((F,), 0.01 * 2.0, device=DEV))


@pytest.mark.parametrize("N,F,cut", [(1000, 64, 600), (4099, 128, 7)])
def test_split_backward_sums_give_the_whole_batch_gradients_and_coefficients(N, F, cut):
    x, dy, gamma, beta = _data(N, F, 9)
    st = _whole_forward(x, gamma, beta)
    # the existing backward on the whole batch: dgamma, dbeta, and [A | B | C] at the head of its scratch
    dgamma, dbeta = torch.zeros(F, device=DEV), torch.zeros(F, device=DEV)
    acc = _acc(F)
    _lib.call("gcmi_bn_bwd", _p(dy), F, _p(x), F, N, F, _p(gamma), _p(st["mean"]), _p(st["invstd"]), _p(dgamma), _p(dbeta),
              None, F, 0, _p(acc), _stream())
    torch.cuda.synchronize()
    coef_whole = acc[:2 * F].view(torch.float32)[:3 * F].clone()
    parts = []
    for sl in (slice(0, cut), slice(cut, N)):
        xp, dyp = x[sl].contiguous(), dy[sl].contiguous()
        dg, db = torch.zeros(F, device=DEV), torch.zeros(F, device=DEV)
        a, xb = _acc(F), torch.full((2 * F + 1,), -1.0, dtype=torch.float64, device=DEV)
        _lib.call("gcmi_bn_sync_bwd_sums", _p(dyp), F, _p(xp), F, xp.shape[0], F, _p(gamma), _p(st["mean"]), _p(st["invstd"]),
                  _p(dg), _p(db), _p(a), _p(xb), _stream())
        torch.cuda.synchronize()
        assert float(a[2 * F:].abs().max()) == 0.0, "the replicas must be clean afterwards"
        assert float(xb[2 * F]) == xp.shape[0]
        # the parameter gradients are the LOCAL sums: exactly what went into the buffer, rounded to float
        assert torch.equal(db, xb[:F].float()) and torch.equal(dg, xb[F:2 * F].float())
        parts.append((dg, db, xb))
    _close(parts[0][0].double() + parts[1][0].double(), dgamma, "dgamma")
    _close(parts[0][1].double() + parts[1][1].double(), dbeta, "dbeta")
    summed = parts[0][2] + parts[1][2]
    coef = torch.zeros(3 * F, device=DEV)
    _lib.call("gcmi_bn_sync_bwd_coef", _p(summed), F, _p(gamma), _p(st["mean"]), _p(st["invstd"]), _p(coef), _stream())
    torch.cuda.synchronize()
    for i, name in enumerate("ABC"):
        _close(coef[i * F:(i + 1) * F], coef_whole[i * F:(i + 1) * F], "coefficient " + name)


@pytest.mark.parametrize("ill", [False, True])
def test_collapse_of_pooled_sums_recovers_the_direct_sums(ill):
    """The accumulators as a one-pass block backward leaves them (gcmi_bn_sync_bwd_pool): the pooled sums, sum dP and
    sum dP * P with P = gamma * xhat + beta, spread over the 32 replicas, give dbeta = sum dP and dgamma =
    (sum dP * P - beta * sum dP) / gamma = sum dy * xhat -- what gcmi_bn_sync_bwd_sums takes from the rows.  With a
    column of |beta| > 64 |gamma| the pooled form is ill-conditioned and the direct sums are taken instead (here
    the pooled accumulator holds rubbish then, to show which one was read).  Both accumulators are clean afterwards."""
    N, F = 1500, 64
    x, dy, gamma, beta = _data(N, F, 13)
    if ill:
        beta[5] = 100.0 * float(gamma[5])
    st = _whole_forward(x, gamma, beta)
    want_dg, want_db = torch.zeros(F, device=DEV), torch.zeros(F, device=DEV)
    want = torch.zeros(2 * F + 1, dtype=torch.float64, device=DEV)
    _lib.call("gcmi_bn_sync_bwd_sums", _p(dy), F, _p(x), F, N, F, _p(gamma), _p(st["mean"]), _p(st["invstd"]), _p(want_dg),
              _p(want_db), _p(_acc(F)), _p(want), _stream())
    # the two accumulators, filled by hand in fp64: 32 replicas of [sum a | sum b] behind 2 F coefficient doubles
    xhat = (x.double() - st["mean"].double()) * st["invstd"].double()
    P = gamma.double() * xhat + beta.double()
    rep = torch.arange(N, device=DEV) % 32
    psums = torch.zeros((33, 2 * F), dtype=torch.float64, device=DEV)
    acc = torch.zeros((33, 2 * F), dtype=torch.float64, device=DEV)
    for r in range(32):
        sel = rep == r
        d = dy[sel].double()
        psums[1 + r, :F], psums[1 + r, F:] = d.sum(0), (d * P[sel]).sum(0)
        if ill:
            acc[1 + r, :F], acc[1 + r, F:] = d.sum(0), (d * xhat[sel]).sum(0)
    if ill:
        psums[1:] = 12345.0
    dg, db = torch.zeros(F, device=DEV), torch.zeros(F, device=DEV)
    xb = torch.full((2 * F + 1,), -1.0, dtype=torch.float64, device=DEV)
    _lib.call("gcmi_bn_sync_bwd_pool", _p(psums), _p(acc), N, F, _p(gamma), _p(beta), _p(dg), _p(db), _p(xb), _stream())
    torch.cuda.synchronize()
    assert float(psums[1:].abs().max()) == 0.0 and float(acc[1:].abs().max()) == 0.0, "both accumulators clean afterwards"
    assert float(xb[2 * F]) == N
    _close(xb[:F], want[:F], "sum dy")
    _close(xb[F:2 * F], want[F:2 * F], "sum dy xhat")
    _close(db, want_db, "dbeta")
    _close(dg, want_dg, "dgamma")
