"""The small-batch engine (csrc/smallstep.hip, deepchem_amd/small.py) against the oracle and against the
per-batch native path: same losses, parameters, Adam moments, BatchNorm running statistics, predictions."""
import numpy as np
import pytest
import torch

from oracle import graphconv_oracle as O
from tests.util import oracle_batch, oracle_convmols, oracle_predict

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _setup(mode, T, B, n, bn, grad_mode, seed, widths=(64, 64), dense=128):
    import deepchem_amd as dc
    from deepchem_amd.utils.synthetic import concat_packed, single_atom_and_edge_cases, synthetic_labels, synthetic_molecules
    packed = concat_packed([synthetic_molecules(n - 8, seed=seed, max_atoms=40), single_atom_and_edge_cases(75, seed)])
    n = packed.n_mols
    y, w = synthetic_labels(n, T, mode, seed, pos_rate=0.4)
    cfg = O.ModelConfig(T, graph_conv_layers=widths, number_input_features=(75,) + tuple(widths[:-1]),
                        dense_layer_size=dense, mode=mode, batch_normalize=bn, batch_size=B)
    if tuple(widths) == (64, 64):
        state = O.init_state(cfg, seed)
    else:
        state = None
    torch.manual_seed(seed)  # other widths start from the model's own initialisation: the same one in any test order
    model = dc.models.torch_models.GraphConvModel(T, number_input_features=[75] + list(widths[:-1]),
                                                  graph_conv_layers=list(widths), dense_layer_size=dense, mode=mode,
                                                  batch_size=B, batch_normalize=bn, grad_mode=grad_mode,
                                                  device=torch.device(DEV), learning_rate=1e-3)
    if state is not None:
        model.model.load_state_dict({k: v.clone() for k, v in state.items()})
    else:
        state = {k: v.detach().cpu().clone() for k, v in model.model.state_dict().items()}
    return packed, y, w, cfg, state, model


def _device_batches(model, packed, y, w, cfg, B):
    from deepchem_amd.data.collate import collate_to_device
    from deepchem_amd.metrics import to_one_hot
    out = []
    n = packed.n_mols
    for s in range(0, n, B):
        idx = np.arange(s, min(n, s + B))
        n_real = len(idx)
        if n_real < B:
            idx = idx[np.arange(B) % n_real]
        batch = collate_to_device(packed, idx, torch.device(DEV), n_samples=B)
        batch.graph.ensure_rev_pos()
        y_b = y[idx]
        if cfg.mode == "classification":
            y_b = to_one_hot(y_b.flatten(), cfg.n_classes).reshape(-1, cfg.n_tasks, cfg.n_classes)
        w_b = w[idx].copy()
        w_b[n_real:] = 0
        out.append((batch, torch.as_tensor(y_b.astype(np.float32), device=DEV),
                    torch.as_tensor(w_b.astype(np.float32), device=DEV), idx, n_real))
    return out


def _same_after_adam(key, got, want, n_steps, is_param, lr=1e-3):
    """Parameters after a few Adam steps.  Adam moves every entry by about lr per step in the direction of
    g / (|g| + eps): an entry whose gradient is at rounding-noise level can go either way, so single entries may
    differ by up to 2 lr per step whatever the implementation; a systematic error shows in the typical entry.
    Buffers (running statistics) are plain averages and must agree tightly."""
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    scale = max(np.abs(want).max(), 1e-3)
    if not is_param:
        assert err.max() <= 2e-4 * scale, (key, float(err.max()), scale)
        return
    assert err.max() <= 2.2 * lr * n_steps, (key, float(err.max()))
    assert np.median(err) <= 2e-4 * scale and np.mean(err) <= 1e-3 * scale, (key, float(np.median(err)), float(np.mean(err)))


CASES = [
    ("classification", 12, 10, 48, True, "reference"),
    ("classification", 12, 10, 48, True, "full"),
    ("classification", 3, 16, 40, False, "reference"),
    ("classification", 3, 16, 40, False, "full"),
    ("regression", 2, 12, 44, True, "full"),
    ("regression", 1, 12, 44, True, "reference"),
]


@pytest.mark.parametrize("mode,T,B,n,bn,grad_mode", CASES)
def test_small_engine_training_matches_the_oracle(mode, T, B, n, bn, grad_mode):
    from deepchem_amd.small import SmallBatchEngine
    packed, y, w, cfg, state, model = _setup(mode, T, B, n, bn, grad_mode, seed=7)
    model._ensure_built()
    model.model.train()
    native = model.model._native_net()
    assert native is not None
    engine = SmallBatchEngine(native)
    batches = _device_batches(model, packed, y, w, cfg, B)
    descs = [engine.describe(b, l, ww, B) for b, l, ww, _, _ in batches]
    max_atoms = max(b.n_atoms for b, *_ in batches)
    losses = []
    for _ in range(2):  # two epochs, one C call each
        losses += engine.fit(descs, model._pytorch_optimizer, max_atoms, B).cpu().tolist()
    torch.cuda.synchronize()
    tr = O.OracleTrainer(cfg, state, grad_mode=grad_mode, faithful=False)
    mols = oracle_convmols(packed)
    ref = []
    for _ in range(2):
        for _, _, _, idx, n_real in batches:
            inputs, labels, weights = oracle_batch(cfg, mols, y, w, idx, n_real, True)
            ref.append(tr.train_step(inputs, labels, weights))
    assert np.allclose(losses, ref, rtol=2e-4, atol=1e-6), (losses, ref)
    sd = model.model.state_dict()
    n_steps = 2 * len(batches)
    for k, v in tr.state.items():
        got = sd[k].detach().float().cpu().numpy()
        want = v.detach().float().numpy()
        _same_after_adam(k, got, want, n_steps, O.is_parameter(k))
    # untrained parameters did not move in reference mode
    if grad_mode == "reference":
        for k in state:
            if k.startswith("graph_convs") or k.startswith("batch_norms.0.w") or k.startswith("batch_norms.0.b"):
                assert torch.equal(sd[k].cpu(), state[k]), k
    # Adam state: torch layout, one step count for the trained range
    steps = {float(st["step"]) for st in model._pytorch_optimizer.state.values() if "step" in st}
    assert steps == {float(2 * len(batches))}


@pytest.mark.parametrize("mode,T,B,n,bn", [("classification", 12, 10, 48, True), ("regression", 2, 16, 40, False)])
def test_small_engine_prediction_matches_the_oracle(mode, T, B, n, bn):
    from deepchem_amd.small import SmallBatchEngine
    packed, y, w, cfg, state, model = _setup(mode, T, B, n, bn, "reference", seed=9)
    # running statistics that are not the identity
    rng = np.random.RandomState(1)
    if bn:
        sd = model.model.state_dict()
        for i in range(3):
            sd["batch_norms.%d.running_mean" % i].copy_(torch.from_numpy(rng.rand(sd["batch_norms.%d.running_mean" % i].numel()).astype(np.float32)))
            sd["batch_norms.%d.running_var" % i].copy_(torch.from_numpy((0.5 + rng.rand(sd["batch_norms.%d.running_var" % i].numel())).astype(np.float32)))
        state = {k: v.detach().cpu().clone() for k, v in model.model.state_dict().items()}
    model._ensure_built()
    model.model.eval()
    native = model.model._native_net()
    engine = SmallBatchEngine(native)
    batches = _device_batches(model, packed, y, w, cfg, B)
    TC = T * (2 if mode == "classification" else 1)
    outs = []
    descs = []
    for b, _, _, _, _ in batches:
        d = engine.describe(b)
        lo = torch.empty((B, TC), device=DEV)
        pr = torch.empty((B, TC), device=DEV)
        fp = torch.empty((B, 256), device=DEV)
        d.d_logits, d.d_probs, d.d_fingerprint = lo.data_ptr(), pr.data_ptr(), fp.data_ptr()
        outs.append((lo, pr, fp))
        descs.append(d)
    engine.predict(descs, max(b.n_atoms for b, *_ in batches), B)
    torch.cuda.synchronize()
    tr = O.OracleTrainer(cfg, state, grad_mode="reference", faithful=False)
    mols = oracle_convmols(packed)
    for (lo, pr, fp), (_, _, _, idx, n_real) in zip(outs, batches):
        inputs, _, _ = oracle_batch(cfg, mols, None, None, idx, n_real, True, predict=True)
        ref = tr.predict(inputs)
        if mode == "classification":
            assert np.abs(pr.cpu().numpy().reshape(B, T, 2) - ref[0].numpy()).max() < 1e-4
            assert np.abs(lo.cpu().numpy().reshape(B, T, 2) - ref[1].numpy()).max() < 1e-4 * max(1.0, float(ref[1].abs().max()))
            assert np.abs(fp.cpu().numpy() - ref[2].numpy()).max() < 1e-4
        else:
            assert np.abs(lo.cpu().numpy() - ref[0].numpy()).max() < 1e-4 * max(1.0, float(ref[0].abs().max()))
            assert np.abs(fp.cpu().numpy() - ref[1].numpy()).max() < 1e-4


# (192, 256) / 64 and (256, 192) / 128 would reach the three- and four-tile forms of the product kernels and the 64-wide
# readout, but the per-batch path this test compares against does not hold the after-Adam bounds below at those widths
# (DESIGN section 33 has the figures), so they are not cases here.  Those forms are held to the float64 oracle step by
# step, gradient by gradient, in tests/test_gpu_small_grads.py (cases B and C).
OTHER_WIDTHS = [((128, 128), 256)]


@pytest.mark.parametrize("widths,dense", OTHER_WIDTHS)
def test_small_engine_other_widths(widths, dense):
    """GraphConv and dense widths other than the default 64/64/128: [128, 128] with a 256-wide dense layer is MolNet's
    regression preset (molnet/preset_hyper_parameters.py:128-135).  Training against the per-batch path from the same
    state, then the eval-mode forward of one batch against the per-batch forward."""
    from deepchem_amd.small import SmallBatchEngine
    packed, y, w, cfg, state, model = _setup("regression", 1, 12, 44, True, "full", seed=11, widths=widths, dense=dense)
    model._ensure_built()
    model.model.train()
    native = model.model._native_net()
    engine = SmallBatchEngine(native)
    batches = _device_batches(model, packed, y, w, cfg, 12)
    descs = [engine.describe(b, l, ww, 12) for b, l, ww, _, _ in batches]
    losses = engine.fit(descs, model._pytorch_optimizer, max(b.n_atoms for b, *_ in batches), 12).cpu().tolist()
    # this test is about the two native paths agreeing: compare with the per-batch native path of this repository, from
    # the same state.  (The oracle could run these widths too: O.init_state sizes BatchNorm and the dense layer from
    # graph_conv_layers, and tests/test_gpu_scale.py and tests/test_gpu_small_grads.py run it at them; it is the
    # reference's TORCH model that hard-codes 64, graphconvmodel.py:151.)
    import deepchem_amd as dc
    dc.set_gemm_mode("exact")
    try:
        ref_model = dc.models.torch_models.GraphConvModel(1, number_input_features=[75, widths[0]],
                                                          graph_conv_layers=list(widths), dense_layer_size=dense,
                                                          mode="regression", batch_size=12, grad_mode="full",
                                                          device=torch.device(DEV), learning_rate=1e-3)
        ref_model.model.load_state_dict({k: v.clone() for k, v in state.items()})
        ref_model._ensure_built()
        ref_model.model.train()
        ref = []
        for b, l, ww, _, _ in batches:
            ref.append(float(ref_model._train_step(b, [l], [ww], ref_model._loss_fn, ref_model._pytorch_optimizer)))
        # the first step has no history: tight.  From the second on Adam has moved entries whose gradient is at rounding
        # level by lr * sign(noise), in any arithmetic (the per-batch path's own two product modes drift by 2e-4 here)
        assert abs(losses[0] - ref[0]) <= 1e-5 * abs(ref[0]), (losses, ref)
        assert np.allclose(losses, ref, rtol=2e-3, atol=1e-6), (losses, ref)
        sd, rsd = model.model.state_dict(), ref_model.model.state_dict()
        for k in sd:
            a, b = sd[k].float().cpu().numpy(), rsd[k].float().cpu().numpy()
            _same_after_adam(k, a, b, len(batches), "running" not in k and "num_batches" not in k)
        # the forward of one batch in eval mode: the engine against the per-batch path, both from the reference state
        # (the engine reads the parameters of `model`: give it the reference model's)
        model.model.load_state_dict({k: v.clone() for k, v in rsd.items()})
        model.model.eval()
        ref_model.model.eval()
        batch = batches[0][0]
        d = engine.describe(batch)
        lo = torch.empty((12, 1), device=DEV)
        fp = torch.empty((12, 2 * dense), device=DEV)
        d.d_logits, d.d_fingerprint = lo.data_ptr(), fp.data_ptr()
        engine.predict([d], batch.n_atoms, 12)
        torch.cuda.synchronize()
        with torch.no_grad():
            want = ref_model.model(batch)
    finally:
        dc.set_gemm_mode("fast")
    want_lo, want_fp = want[0].detach().float().cpu().numpy(), want[-1].detach().float().cpu().numpy()
    assert np.abs(lo.cpu().numpy().reshape(want_lo.shape) - want_lo).max() < 1e-4 * max(1.0, float(np.abs(want_lo).max()))
    assert np.abs(fp.cpu().numpy() - want_fp).max() < 1e-4


# ------------------------------------------------------------------ bf16 activation storage (opt-in)
def _bf16(x):
    """Round an fp32 array to bfloat16 (nearest even) and back."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return r.astype(np.uint32).view(np.float32)


@pytest.mark.parametrize("grad_mode", ["reference", "full"])
def test_bf16_storage_follows_fp32_within_bf16_resolution(grad_mode):
    """``activation_storage="bf16"``: the same two epochs as the fp32 engine from the same state.  Stored activations
    carry 8 significant bits (relative rounding 2^-9 per stored matrix, three to five of them between input and
    loss), so first-epoch losses agree to ~1 %, far outside the fp32 mode's bound and far inside an error: a
    wrong stride or a missing conversion is off by O(1)."""
    import deepchem_amd as dc
    from deepchem_amd.small import SmallBatchEngine
    results = {}
    for storage in ("fp32", "bf16"):
        packed, y, w, cfg, state, _ = _setup("classification", 12, 10, 48, True, grad_mode, seed=7)
        model = dc.models.torch_models.GraphConvModel(12, number_input_features=[75, 64], batch_size=10,
                                                      grad_mode=grad_mode, device=torch.device(DEV), learning_rate=1e-3,
                                                      activation_storage=storage)
        model.model.load_state_dict({k: v.clone() for k, v in state.items()})
        model._ensure_built()
        model.model.train()
        engine = SmallBatchEngine(model.model._native_net())
        assert engine.native.desc.storage == (1 if storage == "bf16" else 0)
        batches = _device_batches(model, packed, y, w, cfg, 10)
        descs = [engine.describe(b, l, ww, 10) for b, l, ww, _, _ in batches]
        losses = []
        for _ in range(2):
            losses += engine.fit(descs, model._pytorch_optimizer, max(b.n_atoms for b, *_ in batches), 10).cpu().tolist()
        outs = []
        model.model.eval()
        for b, *_ in batches:
            d = engine.describe(b)
            lo, pr, fp = (torch.empty((10, 24), device=DEV), torch.empty((10, 24), device=DEV),
                          torch.empty((10, 256), device=DEV))
            d.d_logits, d.d_probs, d.d_fingerprint = lo.data_ptr(), pr.data_ptr(), fp.data_ptr()
            engine.predict([d], b.n_atoms, 10)
            outs.append(pr.cpu().numpy())
        results[storage] = (np.array(losses), np.concatenate(outs))
    l32, p32 = results["fp32"]
    l16, p16 = results["bf16"]
    assert not np.array_equal(l32, l16)                       # the mode is really on
    # ten-molecule batches (BatchNorm over ~200 rows) and ten optimizer steps: the two runs drift by a few percent
    assert np.allclose(l16, l32, rtol=8e-2), (l16, l32)
    assert np.allclose(l16[:5], l32[:5], rtol=2e-2), (l16, l32)  # first epoch: rounding only, no drift yet
    # (a training run is chaotic in ANY arithmetic, DESIGN section 19, and bf16 rounding (2^-9) is noise far above the
    # level at which Adam's sign-like first steps flip: ten steps later the probabilities differ by 0.06 max / <0.01
    # mean in reference mode and, with the GraphConv weights training too, 0.30 max / 0.04 mean in full mode -- measured;
    # a wrong stride or a missing conversion gives uncorrelated outputs, mean ~0.3)
    assert np.abs(p16 - p32).max() < 0.6 and np.abs(p16 - p32).mean() < 0.1, (np.abs(p16 - p32).max(), np.abs(p16 - p32).mean())


def test_bf16_storage_is_refused_only_where_no_kernel_has_it():
    """bf16 storage runs on the library's own steps: the small-batch engine, and (round 3) the streaming kernels of
    the per-batch path (gcmi_model_* with storage = 1).  What is left without a bf16 form -- the layer-by-layer
    autograd path a custom loss needs, shapes the streaming kernels do not cover -- refuses instead of computing in
    some other way."""
    import deepchem_amd as dc
    from deepchem_amd._lib import GcmiError
    from deepchem_amd.utils.synthetic import synthetic_labels, synthetic_molecules
    packed = synthetic_molecules(16, seed=1, max_atoms=20)
    y, w = synthetic_labels(16, 2, "classification", 1)
    model = dc.models.torch_models.GraphConvModel(2, number_input_features=[75, 64], batch_size=8,
                                                  device=torch.device(DEV), activation_storage="bf16")
    ds = dc.data.PackedDataset(packed, y, w)
    model.fit(ds, nb_epoch=1, checkpoint_interval=0)           # small batches: the engine
    assert model.predict(ds).shape == (16, 2, 2)
    seen = []
    model.fit(ds, nb_epoch=1, checkpoint_interval=0, callbacks=[lambda m, s: seen.append(s)])   # per-batch path: streaming kernels
    assert len(seen) == 2
    with pytest.raises(NotImplementedError, match="library's own step"):
        model.fit(ds, nb_epoch=1, checkpoint_interval=0, loss=lambda o, l, w_: (o[0] * 0).sum())   # autograd path
    wide = dc.models.torch_models.GraphConvModel(2, number_input_features=[75, 128], graph_conv_layers=[128, 128],
                                                 dense_layer_size=256, batch_size=8, device=torch.device(DEV),
                                                 activation_storage="bf16")
    wide.small_batch_engine = False
    with pytest.raises(GcmiError, match="bf16 activation storage covers"):
        wide.fit(ds, nb_epoch=1, checkpoint_interval=0)
    with pytest.raises(ValueError):
        dc.models.torch_models.GraphConvModel(2, number_input_features=[75, 64], activation_storage="fp8")
