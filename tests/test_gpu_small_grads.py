"""The small-batch engine (csrc/smallstep.hip) step by step: the RAW gradient of every step, captured through the
data-parallel hook (``grad_sync.reduce_flat`` sees the trained range of the gradient arena between the backward launches
and the optimizer launch), against the float64 oracle on batches qualified on the CPU (tests/small_refs.py, DESIGN
section 43).  The optimizer is plain gradient descent at rate 0, so the parameters stay where they are over a call of
any length and every step of it has one reference; a constant factor in a gradient, which Adam's normalised step hides
from tests/test_gpu_small.py, is a distance of that factor here."""
import numpy as np
import pytest
import torch

from oracle import graphconv_oracle as O
from tests import small_refs as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MOMENTUM = 0.99  # nn.BatchNorm1d(momentum=0.99) of the model (oracle: _batch_norm)


class _Capture:
    """The grad_sync object of SmallBatchEngine.fit: keeps a copy of what every step hands to the all-reduce."""

    def __init__(self):
        self.grads = []

    def reduce_flat(self, bucket):
        self.grads.append(bucket.clone())


def _model(model_id, grad_mode, state, lr, batch_size=48):
    import deepchem_amd as dc
    m = R.MODELS[model_id]
    model = dc.models.torch_models.GraphConvModel(m.T, number_input_features=[75] + list(m.widths[:-1]),
                                                  graph_conv_layers=list(m.widths), dense_layer_size=m.dense, mode=m.mode,
                                                  batch_size=batch_size, batch_normalize=m.bn, grad_mode=grad_mode,
                                                  device=torch.device(DEV),
                                                  optimizer=dc.models.optimizers.GradientDescent(lr))
    model.model.load_state_dict({k: v.clone() for k, v in state.items()})
    model._ensure_built()
    assert type(model._pytorch_optimizer).__name__ == "GcmiSGD"
    native = model.model._native_net()
    assert native is not None
    return model, native


def _device_batch(packed, y, w, cfg, n_real):
    """The whole of ``packed`` as one device batch, the way tests/test_gpu_small.py::_device_batches forms a batch: rows
    from n_real on (repeats of the first rows) carry weight 0."""
    from deepchem_amd.data.collate import collate_to_device
    from deepchem_amd.metrics import to_one_hot
    n = packed.n_mols
    batch = collate_to_device(packed, np.arange(n), torch.device(DEV), n_samples=n)
    batch.graph.ensure_rev_pos()
    y_b = y
    if cfg.mode == "classification":
        y_b = to_one_hot(y.flatten(), cfg.n_classes).reshape(-1, cfg.n_tasks, cfg.n_classes)
    w_b = w.copy()
    w_b[n_real:] = 0
    return (batch, torch.as_tensor(y_b.astype(np.float32), device=DEV),
            torch.as_tensor(w_b.astype(np.float32), device=DEV))


def _named_slices(model, native):
    return list(zip([k for k, _ in model.model.named_parameters()], native._slices))


def _trained_range(native):
    d, L = native.desc, native.n_layers
    if d.grad_mode == 1:
        return 0, int(d.n_params)
    return int(d.off_bn_gamma[L - 1] if d.batch_norm else d.off_dense_w), int(d.n_params)


def _check_gradient(what, captured, lo, hi, slices, r64, r32):
    """One captured gradient range against the float64 oracle step.  Returns (worst GPU distance, worst float32-oracle
    distance), both in units of the bound, after asserting the bound, the exact zeros and the coverage count."""
    got = captured.cpu().numpy().astype(np.float64)
    assert got.shape[0] == hi - lo and np.isfinite(got).all(), what
    compared, worst, worst32, bad = 0, (0.0, None), 0.0, []
    for name, (off, cnt) in slices:
        want = r64.grads[name]
        inside = lo <= off and off + cnt <= hi
        if want is None:
            assert not inside, (what, name, "inside the trained range without a reference gradient")
            continue
        assert inside, (what, name, "has a reference gradient but lies outside the trained range")
        want = want.reshape(-1)
        g = got[off - lo:off - lo + cnt]
        bound = R.BOUND * max(np.abs(want).max(), 1e-6) + 1e-7
        err = np.abs(g - want).max()
        if not want.any():
            assert not g.any(), (what, name, "exactly zero in float64, not on the device")
        if err > bound:
            bad.append((name, float(err / bound), int((np.abs(g - want) > bound).sum()), cnt))
        if err / bound >= worst[0]:
            worst = (float(err / bound), name)
        worst32 = max(worst32, float(np.abs(r32.grads[name].reshape(-1) - want).max() / bound))
        compared += 1
    print("%s: %d gradient tensors, worst GPU %.3f of the bound (%s), float32 oracle %.3f" %
          (what, compared, worst[0], worst[1], worst32))
    assert not bad, (what, bad)
    assert compared == sum(g is not None for g in r64.grads.values()), what
    return worst[0], worst32


def _check_loss(what, got, r64):
    assert abs(got - r64.loss) <= 1e-4 * max(abs(r64.loss), 1.0), (what, got, r64.loss)


def _check_buffer(key, got, want):
    """Running statistics: the 2e-4 * scale of tests/test_gpu_small.py::_same_after_adam for buffers."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    scale = max(np.abs(want).max(), 1e-3)
    assert np.abs(got - want).max() <= 2e-4 * scale, (key, float(np.abs(got - want).max()), scale)


def _batch_statistics(r64, start):
    """What one training-mode forward contributes to every running statistic, from the float64 oracle's state after one
    step from ``start``: running = (1 - m) start + m batch."""
    return {k: (v.double().numpy() - (1 - MOMENTUM) * start[k].double().numpy()) / MOMENTUM
            for k, v in r64.state.items() if k.endswith("running_mean") or k.endswith("running_var")}


ONE_STEP = [(c, g) for c in R.ONE_STEP for g in c.modes]


@pytest.mark.parametrize("case,grad_mode", ONE_STEP, ids=[R.case_id(c, g) for c, g in ONE_STEP])
def test_one_step_gradient_against_the_float64_oracle(case, grad_mode):
    from deepchem_amd.small import SmallBatchEngine
    what = R.case_id(case, grad_mode)
    packed, y, w, cfg, state, n_real = R.case_inputs(case.model, case.kind, case.seed)
    r64, r32 = R.references(case.model, case.kind, case.seed, grad_mode)
    model, native = _model(case.model, grad_mode, state, 0.0, packed.n_mols)
    model.model.train()
    engine = SmallBatchEngine(native)
    batch, labels, weights = _device_batch(packed, y, w, cfg, n_real)
    before = {k: v.detach().clone() for k, v in model.model.state_dict().items()}
    capture = _Capture()
    losses = engine.fit([engine.describe(batch, labels, weights, packed.n_mols)], model._pytorch_optimizer,
                        batch.n_atoms, packed.n_mols, grad_sync=capture)
    torch.cuda.synchronize()
    lo, hi = _trained_range(native)
    L = native.n_layers
    assert lo == (0 if grad_mode == "full" else
                  native.offsets["batch_norms.%d.weight" % (L - 1) if cfg.batch_normalize else "dense.weight"])
    assert native.grad_range == (lo, hi) and len(capture.grads) == 1
    _check_gradient(what, capture.grads[0], lo, hi, _named_slices(model, native), r64, r32)
    _check_loss(what, float(losses[0]), r64)
    after = model.model.state_dict()
    for k, v in before.items():
        if O.is_parameter(k):
            assert torch.equal(after[k].view(torch.int32), v.view(torch.int32)), (what, k)
        elif k.endswith("num_batches_tracked"):
            assert int(after[k]) == 1, (what, k)
        else:
            _check_buffer(k, after[k].cpu().numpy(), r64.state[k].numpy())


@pytest.mark.parametrize("grad_mode", R.GRAD_MODES)
@pytest.mark.parametrize("model_id", sorted(R.SEQUENCE))
def test_eighteen_steps_in_one_call(model_id, grad_mode):
    """[ordinary, shaped, padded] x 6 from one state at rate 0: eighteen steps pass the 16 conv-output slots (set 0 is
    reused behind ev_free; in reference mode the conv stacks run ahead on the side stream), a 126-atom batch follows a
    500-atom one in the same workspace, and every step needs the zeroing the step before left behind."""
    from deepchem_amd.small import SmallBatchEngine
    seed = R.SEQUENCE[model_id]
    cases = [R.case_inputs(model_id, kind, seed) for kind in R.SEQUENCE_KINDS]
    refs = [R.references(model_id, kind, seed, grad_mode) for kind in R.SEQUENCE_KINDS]
    state = cases[0][4]
    for c in cases[1:]:
        assert all(torch.equal(state[k], c[4][k]) for k in state)  # one state for the three batches
    model, native = _model(model_id, grad_mode, state, 0.0)
    model.model.train()
    engine = SmallBatchEngine(native)
    dev = [_device_batch(packed, y, w, cfg, n_real) for packed, y, w, cfg, _, n_real in cases]
    assert dev[0][0].n_atoms > 3 * dev[1][0].n_atoms
    one_round = [engine.describe(b, l, ww, c[0].n_mols) for (b, l, ww), c in zip(dev, cases)]
    descs = one_round * 6
    before = {k: v.detach().clone() for k, v in model.model.state_dict().items()}
    capture = _Capture()
    losses = engine.fit(descs, model._pytorch_optimizer, max(b.n_atoms for b, _, _ in dev),
                        max(c[0].n_mols for c in cases), grad_sync=capture)
    torch.cuda.synchronize()
    losses = losses.cpu().tolist()
    lo, hi = _trained_range(native)
    assert len(capture.grads) == 18 and len(losses) == 18
    slices = _named_slices(model, native)
    for i in range(18):
        what = "%s-%s step %d (%s)" % (model_id, grad_mode, i, R.SEQUENCE_KINDS[i % 3])
        _check_gradient(what, capture.grads[i], lo, hi, slices, *refs[i % 3])
        _check_loss(what, losses[i], refs[i % 3][0])
    after = model.model.state_dict()
    stats = [_batch_statistics(r64, state) for r64, _ in refs]
    for k, v in before.items():
        if O.is_parameter(k):
            assert torch.equal(after[k].view(torch.int32), v.view(torch.int32)), k
        elif k.endswith("num_batches_tracked"):
            assert int(after[k]) == 18, k
        else:
            run = state[k].double().numpy()
            for i in range(18):
                run = (1 - MOMENTUM) * run + MOMENTUM * stats[i % 3][k]
            _check_buffer(k, after[k].cpu().numpy(), run)


@pytest.mark.parametrize("grad_mode", R.GRAD_MODES)
def test_the_optimizer_consumes_what_the_hook_saw(grad_mode):
    """Gradient descent at rate 1: inside the trained range p_new is float32(p_old) - float32(g) bit for bit (the product
    by 1 is exact, and a fused or an unfused subtract rounds once either way); below it nothing moves."""
    from deepchem_amd.small import SmallBatchEngine
    case = R.ONE_STEP[0]
    assert (case.model, case.kind) == ("A", "shaped")
    packed, y, w, cfg, state, n_real = R.case_inputs(case.model, case.kind, case.seed)
    model, native = _model(case.model, grad_mode, state, 1.0, packed.n_mols)
    model.model.train()
    engine = SmallBatchEngine(native)
    batch, labels, weights = _device_batch(packed, y, w, cfg, n_real)
    p_old = native.flat.detach().clone()
    capture = _Capture()
    engine.fit([engine.describe(batch, labels, weights, packed.n_mols)], model._pytorch_optimizer, batch.n_atoms,
               packed.n_mols, grad_sync=capture)
    torch.cuda.synchronize()
    lo, hi = _trained_range(native)
    g = capture.grads[0].cpu()
    p_old, p_new = p_old.cpu(), native.flat.detach().cpu()
    assert float(g.abs().max()) > 1e-3  # something was subtracted
    want = p_old[lo:hi] - g
    assert torch.equal(p_new[lo:hi].view(torch.int32), want.view(torch.int32))
    if grad_mode == "reference":
        assert lo > 0 and torch.equal(p_new[:lo].view(torch.int32), p_old[:lo].view(torch.int32))
    else:
        assert lo == 0


@pytest.mark.parametrize("model_id", ["B", "C", "E", "F"])
def test_eval_forward_at_the_widths_no_other_test_reaches(model_id):
    """engine.predict against the float64 oracle's predict at the bounds of
    tests/test_gpu_small.py::test_small_engine_prediction_matches_the_oracle, running statistics away from (0, 1).
    The forward is continuous in its inputs: no qualification is needed."""
    from deepchem_amd.small import SmallBatchEngine
    case = next(c for c in R.ONE_STEP if (c.model, c.kind) == (model_id, "shaped"))
    m = R.MODELS[model_id]
    packed, y, w, cfg, state, n_real = R.case_inputs(case.model, case.kind, case.seed)
    state = {k: v.clone() for k, v in state.items()}
    rng = np.random.RandomState(1)
    if m.bn:
        for i in range(len(m.widths) + 1):
            n = state["batch_norms.%d.running_mean" % i].numel()
            state["batch_norms.%d.running_mean" % i] = torch.from_numpy(rng.rand(n).astype(np.float32))
            state["batch_norms.%d.running_var" % i] = torch.from_numpy((0.5 + rng.rand(n)).astype(np.float32))
    model, native = _model(model_id, "reference", state, 0.0, packed.n_mols)
    model.model.eval()
    engine = SmallBatchEngine(native)
    batch, _, _ = _device_batch(packed, y, w, cfg, n_real)
    B, T = packed.n_mols, m.T
    TC = T * (2 if m.mode == "classification" else 1)
    d = engine.describe(batch)
    lo = torch.empty((B, TC), device=DEV)
    pr = torch.empty((B, TC), device=DEV)
    fp = torch.empty((B, 2 * m.dense), device=DEV)
    d.d_logits, d.d_probs, d.d_fingerprint = lo.data_ptr(), pr.data_ptr(), fp.data_ptr()
    engine.predict([d], batch.n_atoms, B)
    torch.cuda.synchronize()
    ref = R.oracle_predict64(packed, cfg, state)
    lo, pr, fp = (t.cpu().numpy().astype(np.float64) for t in (lo, pr, fp))
    if m.mode == "classification":
        e_pr = np.abs(pr.reshape(B, T, 2) - ref[0].numpy()).max()
        e_lo = np.abs(lo.reshape(B, T, 2) - ref[1].numpy()).max() / max(1.0, float(ref[1].abs().max()))
        e_fp = np.abs(fp - ref[2].numpy()).max()
    else:
        e_pr = 0.0
        e_lo = np.abs(lo - ref[0].numpy()).max() / max(1.0, float(ref[0].abs().max()))
        e_fp = np.abs(fp - ref[1].numpy()).max()
    print("%s eval forward: logits %.2e probabilities %.2e fingerprint %.2e (bound 1e-4)" % (model_id, e_lo, e_pr, e_fp))
    assert e_pr < 1e-4 and e_lo < 1e-4 and e_fp < 1e-4
