"""``DenseFn`` on the CPU: which primitives it calls, in which order, with which flags, sizes and buffers -- and that the
algebra around them is right.

``ops.seg_gemm``, ``ops.seg_gemm_wgrad`` and ``ops.relu_bwd_`` are replaced by stand-ins that record their arguments and
compute in float64 with torch, so no kernel runs and the comparison with float64 autograd (1e-12 relative) checks the
glue alone.  All data are small integers held in float32: ``ops.grad_target`` hands out float32 ``p.grad`` only, and on
integers float32 products and sums are exact, so the 1e-12 bound holds for the tensors the Function really sees.

Where ``TABLE`` comes from.  It was taken from the three Functions that ``DenseFn`` replaced (``ops.LinearFn``,
``mpnn.MatmulFn``, ``dmpnn_layers.Linear2Fn``) by recording them once with these same stand-ins, over the same cases:
``LinearFn`` gave "single" / "out_in" (ReLU, grad_masked), ``MatmulFn`` "single" and "dual" / "in_out", ``Linear2Fn``
"one_weight" / "out_in" (ReLU).  The other layout of each form is the same rows with the layout flag flipped.  One order
was chosen where the originals disagreed and no result depends on it: ``MatmulFn`` ran input gradient, weight gradient
per operand; ``DenseFn`` runs all weight gradients, then all input gradients, as the other two did.  ``MatmulFn``'s
recording matches its rows as a set, the other two in order.
"""
import itertools

import pytest
import torch

N, K, K2, O = 5, 3, 2, 4
SIZES = {"n": N, "k": K, "k2": K2, "o": O}

# phase, when it runs, entry, layout flag (same / other than the Function's), ReLU / accumulate / bias-buffer flag,
# rows, inner size(s), output size, buffer(s) written.  "when": x, W, b, x2, W2 = that input needs a gradient.
TABLE = {
    "single": [
        ("fwd", "always", "seg_gemm", "same", "relu", "n", ("k", 0), "o", "new"),
        ("bwd", "unmasked relu", "relu_bwd_", None, None, "n", None, "o", "copy"),
        ("bwd", "W|b", "seg_gemm_wgrad", "same", "bias", "n", "k", "o", ("W", "b")),
        ("bwd", "x", "seg_gemm", "other", False, "n", ("o", 0), "k", "new"),
    ],
    "dual": [
        ("fwd", "always", "seg_gemm", "same", "relu", "n", ("k", "k2"), "o", "new"),
        ("bwd", "unmasked relu", "relu_bwd_", None, None, "n", None, "o", "copy"),
        ("bwd", "W|b", "seg_gemm_wgrad", "same", "bias", "n", "k", "o", ("W", "b")),
        ("bwd", "W2", "seg_gemm_wgrad", "same", False, "n", "k2", "o", ("W2", None)),
        ("bwd", "x", "seg_gemm", "other", False, "n", ("o", 0), "k", "new"),
        ("bwd", "x2", "seg_gemm", "other", False, "n", ("o", 0), "k2", "new"),
    ],
    "one_weight": [
        ("fwd", "always", "seg_gemm", "same", "relu", "n", ("k", "k2"), "o", "new"),
        ("bwd", "unmasked relu", "relu_bwd_", None, None, "n", None, "o", "copy"),
        ("bwd", "W|b", "seg_gemm_wgrad", "same", "bias", "n", "k", "o", ("fresh", "fresh")),
        ("bwd", "W|b", "seg_gemm_wgrad", "same", False, "n", "k2", "o", ("fresh", None)),
        ("bwd", "x", "seg_gemm", "other", False, "n", ("o", 0), "k", "new"),
        ("bwd", "x2", "seg_gemm", "other", False, "n", ("o", 0), "k2", "new"),
    ],
}


def expected_calls(form, layout, relu, masked, bias, needs, grads_of):
    """The rows of TABLE that run for this case, with sizes and buffer names filled in."""
    size = lambda s: SIZES.get(s, s)
    calls = []
    for phase, when, entry, lay, flag, rows, inner, outs, wrote in TABLE[form]:
        if when == "unmasked relu":
            if not (relu and not masked):
                continue
        elif when != "always" and not any(needs.get(nm, False) for nm in when.split("|")):
            continue
        trans = None if lay is None else (layout == "out_in") == (lay == "same")
        flag = {"relu": relu, "bias": bias}.get(flag, flag)
        if isinstance(wrote, tuple):
            dw, db = wrote
            wrote = (grads_of.get(dw, "fresh"), grads_of.get(db, "fresh") if flag else None)
        inner = tuple(size(s) for s in inner) if isinstance(inner, tuple) else size(inner)
        calls.append((phase, entry, trans, flag, size(rows), inner, size(outs), wrote))
    return calls


class Recorder:
    """The three stand-ins.  ``names``: data_ptr -> name of the buffers a call may write (the ``p.grad`` tensors)."""

    def __init__(self):
        self.calls, self.names, self.phase, self.cot = [], {}, "fwd", None

    def _blocks(self, flat, off, k, n_out, trans_w):
        blk = flat.reshape(-1)[off:off + k * n_out]
        return blk.reshape(n_out, k).t() if trans_w else blk.reshape(k, n_out)

    def seg_gemm(self, seg_begin, seg_end, a1, w1, w1_off, a2, w2, w2_off, bias, bias_off, n_out, trans_w, relu, n_rows,
                 k1=0, k2=0, out=None, accumulate=False):
        assert list(seg_begin) == [0] and list(seg_end) == [n_rows] and a1.shape == (n_rows, k1)
        y = a1.double() @ self._blocks(w1, w1_off[0], k1, n_out, trans_w).double()
        if a2 is not None:
            assert a2.shape == (n_rows, k2)
            y = y + a2.double() @ self._blocks(w2, w2_off[0], k2, n_out, trans_w).double()
        if bias is not None:
            y = y + bias.double()[bias_off[0]:bias_off[0] + n_out]
        if relu:
            y = torch.relu(y)
        self.calls.append((self.phase, "seg_gemm", bool(trans_w), bool(accumulate or relu), n_rows,
                           (k1, k2 if a2 is not None else 0), n_out, "new" if out is None else "out"))
        if out is None:
            return y.to(a1.dtype)
        return out.add_(y.to(out.dtype)) if accumulate else out.copy_(y)

    def seg_gemm_wgrad(self, seg_begin, seg_end, a, g, dw, dw_off, dbias, dbias_off, trans_w):
        n, k, n_out = a.shape[0], a.shape[1], g.shape[1]
        assert list(seg_begin) == [0] and list(seg_end) == [n] and g.shape[0] == n and dw.is_contiguous()
        wrote = []
        for buf in (dw, dbias):
            name = None if buf is None else self.names.get(buf.data_ptr(), "fresh")
            if name == "fresh":
                assert not buf.any(), "a fresh gradient buffer must arrive zeroed"
            wrote.append(name)
        prod = g.double().t() @ a.double() if trans_w else a.double().t() @ g.double()
        dw.view(-1)[dw_off[0]:dw_off[0] + k * n_out].add_(prod.reshape(-1).to(dw.dtype))
        if dbias is not None:
            dbias.view(-1)[dbias_off[0]:dbias_off[0] + n_out].add_(g.double().sum(0).to(dbias.dtype))
        self.calls.append((self.phase, "seg_gemm_wgrad", bool(trans_w), dbias is not None, n, k, n_out, tuple(wrote)))

    def relu_bwd_(self, g, y):
        assert g.shape == y.shape
        self.calls.append((self.phase, "relu_bwd_", None, None, g.shape[0], None, g.shape[1],
                           "copy" if g.data_ptr() != self.cot.data_ptr() else "the incoming gradient"))
        return g.mul_(y > 0)


@pytest.fixture
def recorder(monkeypatch):
    from deepchem_amd import ops
    rec = Recorder()
    for name in ("seg_gemm", "seg_gemm_wgrad", "relu_bwd_"):
        monkeypatch.setattr(ops, name, getattr(rec, name))
    return rec


def ints(gen, *shape):
    return torch.randint(-3, 4, shape, generator=gen).float()


def dense_fn(x, W, b, x2, W2, layout, relu, masked):
    from deepchem_amd.models.torch_models.functions import DenseFn
    return DenseFn.apply(x, W, b, x2, W2, layout, relu, masked)


def close(got, ref):
    return float((got.detach().double() - ref).abs().max()) <= 1e-12 * float(ref.abs().max())


def check_case(rec, apply, form, layout, relu, masked, bias, direct, needs, seed=0, ordered=True):
    """One forward and backward of ``apply`` (DenseFn's signature) against the table and float64 autograd."""
    from deepchem_amd import ops
    gen = torch.Generator().manual_seed(seed)
    kw = K + K2 if form == "one_weight" else K
    shape = (lambda k: (O, k)) if layout == "out_in" else (lambda k: (k, O))
    t = {"x": ints(gen, N, K), "W": torch.nn.Parameter(ints(gen, *shape(kw))),
         "b": torch.nn.Parameter(ints(gen, O)) if bias else None,
         "x2": ints(gen, N, K2) if form != "single" else None,
         "W2": torch.nn.Parameter(ints(gen, *shape(K2))) if form == "dual" else None}
    cot = ints(gen, N, O)
    start = {}
    for nm, v in t.items():
        if v is not None:
            v.requires_grad_(bool(needs.get(nm, False)))
            if v.requires_grad and isinstance(v, torch.nn.Parameter):
                v.grad = start[nm] = ints(gen, *v.shape)
                start[nm] = start[nm].clone()
    # float64 autograd on copies
    r = {nm: None if v is None else v.detach().double().requires_grad_(v.requires_grad) for nm, v in t.items()}
    mat = (lambda w: w.t()) if layout == "out_in" else (lambda w: w)
    if form == "one_weight":
        z = torch.cat([r["x"], r["x2"]], 1) @ mat(r["W"])
    else:
        z = r["x"] @ mat(r["W"]) + (r["x2"] @ mat(r["W2"]) if form == "dual" else 0)
    z = z + (r["b"] if bias else 0)
    ref_out = torch.relu(z) if relu else z
    # (grad_masked: the incoming gradient counts as masked already, so it passes the ReLU unchanged)
    ((z if masked else ref_out) * cot.double()).sum().backward()

    rec.calls.clear()
    rec.phase, rec.cot = "fwd", cot
    grads_of = {}
    if direct and form != "one_weight":
        grads_of = {nm: nm + ".grad" for nm in start}
    rec.names = {t[nm].grad.data_ptr(): nm + ".grad" for nm in start}
    with ops.direct_param_grads(direct):
        out = apply(t["x"], t["W"], t["b"], t["x2"], t["W2"], layout, relu, masked)
        assert close(out, ref_out.detach())
        rec.phase = "bwd"
        out.backward(cot)
    want = expected_calls(form, layout, relu, masked, bias, needs, grads_of)
    assert (rec.calls == want) if ordered else (rec.calls[0] == want[0] and sorted(map(repr, rec.calls)) == sorted(map(repr, want))), \
        "%s\n  ran  %s\n  want %s" % ((form, layout, relu, masked, bias, direct, needs), rec.calls, want)
    for nm, v in t.items():
        if v is not None and v.requires_grad:
            assert close(v.grad, r[nm].grad + (start[nm].double() if nm in start else 0)), (nm, form, layout, needs)
            if nm in grads_of:
                assert rec.names[v.grad.data_ptr()] == nm + ".grad"  # still the tensor the kernels added into


def cases(form):
    inputs = {"single": ("x", "W", "b"), "dual": ("x", "W", "b", "x2", "W2"), "one_weight": ("x", "W", "b", "x2")}[form]
    for relu, masked in ((False, False), (True, False), (True, True)):
        for bias in (True, False):
            names = [nm for nm in inputs if bias or nm != "b"]
            for r in range(1, len(names) + 1):
                for subset in itertools.combinations(names, r):
                    yield relu, masked, bias, {nm: True for nm in subset}


@pytest.mark.parametrize("direct", [False, True])
@pytest.mark.parametrize("layout", ["out_in", "in_out"])
@pytest.mark.parametrize("form", ["single", "dual", "one_weight"])
def test_dense_fn_calls_and_gradients(recorder, form, layout, direct):
    for seed, (relu, masked, bias, needs) in enumerate(cases(form)):
        check_case(recorder, dense_fn, form, layout, relu, masked, bias, direct, needs, seed)


def test_weight_used_twice_accumulates_in_place(recorder):
    """y = relu(relu(x W^T + b) W^T + b) under direct_param_grads: both weight-gradient calls add into W.grad and b.grad,
    autograd gets None for the parameters, and the buffers end with the sum of both contributions."""
    from deepchem_amd import ops
    gen = torch.Generator().manual_seed(7)
    x, cot = ints(gen, N, O), ints(gen, N, O)
    W, b = torch.nn.Parameter(ints(gen, O, O)), torch.nn.Parameter(ints(gen, O))
    W.grad, b.grad = torch.zeros_like(W), torch.zeros_like(b)
    recorder.names = {W.grad.data_ptr(): "W.grad", b.grad.data_ptr(): "b.grad"}
    recorder.cot = cot
    Wd, bd = W.detach().double().requires_grad_(), b.detach().double().requires_grad_()
    ref = torch.relu(torch.relu(x.double() @ Wd.t() + bd) @ Wd.t() + bd)
    (ref * cot.double()).sum().backward()
    with ops.direct_param_grads(True):
        y = dense_fn(dense_fn(x, W, b, None, None, "out_in", True, False), W, b, None, None, "out_in", True, False)
        assert close(y, ref.detach())
        recorder.phase = "bwd"
        returned = torch.autograd.grad(y, [W, b], cot, allow_unused=True)
    assert returned == (None, None)
    wgrads = [c for c in recorder.calls if c[1] == "seg_gemm_wgrad"]
    assert [c[-1] for c in wgrads] == [("W.grad", "b.grad")] * 2
    assert close(W.grad, Wd.grad) and close(b.grad, bd.grad)


def test_grad_buffer():
    from deepchem_amd import ops
    p = torch.nn.Parameter(torch.ones(2, 3))
    like = torch.ones(2, 3)
    for direct, has_grad in itertools.product((False, True), repeat=2):
        p.grad = torch.full((2, 3), 5.0) if has_grad else None
        with ops.direct_param_grads(direct):
            buf, ret = ops.grad_buffer(p, like)
        if direct and has_grad:
            assert buf is p.grad and ret is None
        else:
            assert ret is buf and buf.shape == like.shape and not buf.any()
    buf, ret = ops.grad_buffer(None, like)
    assert ret is buf and not buf.any()


def test_dense_refuses_mismatched_operands(recorder):
    from deepchem_amd import ops
    x, w = torch.ones(N, K), torch.ones(O, K)
    with pytest.raises(TypeError):
        ops.dense(x, w)  # the layout has no default
    for bad in (dict(layout="rows"), dict(layout="in_out"), dict(layout="out_in", x2=torch.ones(N, K2)),
                dict(layout="out_in", x2=torch.ones(N, K2), w2=torch.ones(O, K)), dict(layout="out_in", b=torch.ones(O + 1))):
        with pytest.raises(ValueError):
            ops.dense(x, w, **bad)
    assert recorder.calls == []
    ops.dense_wgrad(torch.ones(0, K), torch.ones(0, O), torch.zeros(O, K), layout="out_in")  # zero rows: nothing runs
    assert recorder.calls == []
