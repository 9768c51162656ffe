"""MPNNModel (BASELINE.json config 4) on the GPU against ``oracle.mpnn_oracle.MPNNOracle`` -- a torch-CPU autograd
restatement of the Keras MPNNModel (deepchem/models/graph_models.py:1045-1247, models/layers.py:3648-3887).
MODEL-LEVEL PARITY IS UNPINNED: the reference's Keras model needs TensorFlow and its torch MPNNModel is dgllife's
(neither is available); the sub-layers composed here are pinned by the reference's own assets in
tests/test_gpu_mpnn.py / tests/test_oracle_mpnn.py.  Tolerance 1e-4 relative (north_star)."""
import numpy as np
import pytest
import torch

from oracle.mpnn_oracle import MPNNOracle

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


class Mol:
    """The three accessors MPNNModel.default_generator uses (a WeaveMol with all n x n pairs)."""

    def __init__(self, nodes, pairs):
        self.nodes, self.pairs = nodes, pairs

    def get_num_atoms(self):
        return self.nodes.shape[0]

    def get_atom_features(self):
        return self.nodes

    def get_pair_features(self):
        return self.pairs


def qm9_like(n_mols, n_atom_feat, n_pair_feat, seed, max_atoms=12):
    rng = np.random.RandomState(seed)
    mols = np.empty(n_mols, dtype=object)
    for i in range(n_mols):
        n = int(rng.randint(1, max_atoms + 1))
        nodes = (rng.rand(n, n_atom_feat) < 0.15).astype(np.float64)
        pairs = (rng.rand(n, n, n_pair_feat) < 0.3).astype(np.float64) * rng.rand(n, n, n_pair_feat)
        mols[i] = Mol(nodes, pairs)
    return mols


def build(mode, T, M, d, B, n_tasks, seed, n_pair_feat=6):
    import deepchem_amd as dc
    from deepchem_amd.models.torch_models.mpnn import MPNNModel
    torch.manual_seed(seed)
    model = MPNNModel(n_tasks, n_atom_feat=20, n_pair_feat=n_pair_feat, n_hidden=d, T=T, M=M, mode=mode, batch_size=B,
                      device=torch.device(DEV), learning_rate=1e-3)
    # biases away from zero so that their gradients are exercised too
    with torch.no_grad():
        for name, p in model.model.named_parameters():
            if name.endswith("bias") or "_b" in name:
                p.add_(0.05 * torch.randn_like(p))
    return model


# (B, d, T, M, n_pair_feat, max_atoms); the second shape is the model's default width: edge_moments_kernel<16, 2> and
# the second 64-lane feature chunk of the set2set kernels, in both directions
SMALL, DEFAULT_WIDTH = (6, 32, 3, 4, 6, 12), (4, 100, 2, 2, 8, 10)


@pytest.mark.parametrize("mode,n_tasks,shape", [
    pytest.param("regression", 3, SMALL, id="regression-3"),
    pytest.param("classification", 2, SMALL, id="classification-2"),
    pytest.param("regression", 3, DEFAULT_WIDTH, id="regression-3-default-width")])
def test_mpnn_forward_and_gradients_match_the_oracle(mode, n_tasks, shape):
    import deepchem_amd as dc
    dc.set_gemm_mode("exact")
    try:
        B, d, T, M, K, max_atoms = shape
        model = build(mode, T, M, d, B, n_tasks, seed=1, n_pair_feat=K)
        mols = qm9_like(B, 20, K, seed=2, max_atoms=max_atoms)
        rng = np.random.RandomState(3)
        y = rng.randn(B, n_tasks) if mode == "regression" else (rng.rand(B, n_tasks) < 0.5).astype(float)
        w = (rng.rand(B, n_tasks) < 0.8).astype(float)
        ds = dc.data.NumpyDataset(mols, y, w)
        (inputs, labels, weights), = list(model.default_generator(ds, pad_batches=True))
        state = {k: v.detach().cpu() for k, v in model.model.state_dict().items()}
        oracle = MPNNOracle(state, 20, d, T, M, B, mode, n_tasks)
        ref_out = oracle.forward(*inputs)
        ref_loss = oracle.loss(ref_out, labels[0], weights[0])
        ref_loss.backward()
        model._ensure_built()
        model.model.train()
        prepared, lab, wts = model._prepare_batch((inputs, labels, weights))
        outs = model.model(prepared)
        for a, b in zip(outs, ref_out):
            assert np.abs(a.detach().cpu().numpy() - b.detach().numpy()).max() <= 1e-4 * max(1.0, float(b.abs().max()))
        loss = model._loss_fn([outs[i] for i in model._loss_outputs], lab, wts)
        assert abs(float(loss) - float(ref_loss)) <= 1e-4 * max(1.0, abs(float(ref_loss)))
        loss.backward()
        for name, p in model.model.named_parameters():
            g = p.grad.detach().cpu().numpy()
            r = oracle.p[name].grad.numpy()
            scale = max(np.abs(r).max(), 1e-6)
            assert np.abs(g - r).max() <= 1e-4 * scale, (name, float(np.abs(g - r).max()), scale)
    finally:
        dc.set_gemm_mode("fast")


def test_mpnn_fit_loss_trajectory_and_predict():
    """Three optimizer steps through ``fit`` against the oracle stepped by torch.optim.Adam on the same batches; then
    ``predict`` of a set whose size is not a multiple of the batch size."""
    import deepchem_amd as dc
    dc.set_gemm_mode("exact")
    try:
        B, d, T, M, n_tasks = 5, 32, 2, 3, 2
        model = build("regression", T, M, d, B, n_tasks, seed=4)
        mols = qm9_like(13, 20, 6, seed=5)
        rng = np.random.RandomState(6)
        y, w = rng.randn(13, n_tasks), np.ones((13, n_tasks))
        ds = dc.data.NumpyDataset(mols, y, w)
        state = {k: v.detach().cpu().clone() for k, v in model.model.state_dict().items()}
        oracle = MPNNOracle(state, 20, d, T, M, B, "regression", n_tasks)
        opt = torch.optim.Adam(list(oracle.p.values()), lr=1e-3)
        ref_losses = []
        for inputs, labels, weights in model.default_generator(ds, deterministic=True, pad_batches=True):
            opt.zero_grad()
            l = oracle.loss(oracle.forward(*inputs), labels[0], weights[0])
            l.backward()
            opt.step()
            ref_losses.append(float(l))
        losses = []
        model.fit(ds, nb_epoch=1, deterministic=True, checkpoint_interval=0,
                  callbacks=[lambda m, s, iteration_loss=None: losses.append(float(iteration_loss))])
        assert len(losses) == 3 and np.allclose(losses, ref_losses, rtol=2e-4), (losses, ref_losses)
        pred = model.predict(ds)
        assert pred.shape == (13, n_tasks)
        with torch.no_grad():
            ref = np.concatenate([oracle.forward(*inp)[0].numpy()
                                  for inp, _, _ in model.default_generator(ds, mode='predict', pad_batches=False)])
        assert np.abs(pred - ref).max() <= 5e-3 * max(1.0, np.abs(ref).max())  # three Adam steps apart
    finally:
        dc.set_gemm_mode("fast")


# ------------------------------------------------------------------ the reference's own MPNN tests (overfit bars)
def _real_weave_dataset(mode, n_tasks=2, n=20, seed=0):
    """get_dataset of the reference's test file (models/tests/test_graph_models.py:24-46): 20 real molecules
    (here: the committed Delaney sample through the native WeaveFeaturizer), random labels."""
    import deepchem_amd as dc
    import pandas as pd
    import os
    from tests.util import GOLDEN
    smiles = pd.read_csv(os.path.join(GOLDEN, "delaney_sample.csv"))["smiles"].tolist()[:n]
    X = dc.feat.WeaveFeaturizer().featurize(smiles)
    rng = np.random.RandomState(seed)
    if mode == "classification":
        y = rng.randint(0, 2, size=(n, n_tasks)).astype(float)
    else:
        y = rng.normal(size=(n, n_tasks))
    mols = np.empty(n, dtype=object)
    for i, m in enumerate(X):
        k = m.get_num_atoms()
        mols[i] = Mol(np.asarray(m.get_atom_features(), np.float32), np.asarray(m.get_pair_features(), np.float32).reshape(k, k, -1))
    return dc.data.NumpyDataset(mols, y, np.ones((n, n_tasks)))


def test_mpnn_model_overfits_classification():
    """models/tests/test_graph_models.py:253-271: n_hidden 75, T 1, M 1, lr 5e-4, 150 epochs, mean ROC-AUC >= 0.9."""
    from deepchem_amd.metrics import roc_auc_per_task
    from deepchem_amd.models.torch_models.mpnn import MPNNModel
    torch.manual_seed(0)
    ds = _real_weave_dataset("classification")
    model = MPNNModel(2, mode='classification', n_hidden=75, n_atom_feat=75, n_pair_feat=14, T=1, M=1,
                      learning_rate=0.0005, batch_size=100, device=torch.device(DEV))
    model.fit(ds, nb_epoch=150, checkpoint_interval=0)
    auc = roc_auc_per_task(ds.y, model.predict(ds), ds.w)
    assert np.mean(auc) >= 0.9, auc


def test_mpnn_model_overfits_regression():
    """:274-291: batch 10, 60 epochs, mean absolute error < 0.1 -- marked @flaky(max_runs=3, min_passes=1) in the
    reference (random labels, random initialisation): the same rule here, with the three runs seeded."""
    from deepchem_amd.models.torch_models.mpnn import MPNNModel
    ds = _real_weave_dataset("regression")
    errors = []
    for seed in range(3):
        torch.manual_seed(seed)
        np.random.seed(seed)
        model = MPNNModel(2, mode='regression', n_hidden=75, n_atom_feat=75, n_pair_feat=14, T=1, M=1, batch_size=10,
                          device=torch.device(DEV))
        model.fit(ds, nb_epoch=60, checkpoint_interval=0)
        errors.append(float(np.abs(model.predict(ds) - ds.y).mean()))
        if errors[-1] < 0.1:
            break
    assert min(errors) < 0.1, errors


def test_mpnn_regression_uncertainty():
    """:294-320: the uncertainty head; error and predicted deviation in the reference's relations (random labels and
    initialisation: up to three seeded runs, like the reference's flaky regression test next to it)."""
    from deepchem_amd.models.torch_models.mpnn import MPNNModel
    ds = _real_weave_dataset("regression")
    seen = []
    for seed in range(3):
        torch.manual_seed(seed)
        np.random.seed(seed)
        model = MPNNModel(2, mode='regression', n_hidden=75, n_atom_feat=75, n_pair_feat=14, T=1, M=1, dropout=0.1,
                          batch_size=10, uncertainty=True, device=torch.device(DEV))
        model.fit(ds, nb_epoch=40, checkpoint_interval=0)
        pred, std = model.predict_uncertainty(ds, masks=3)
        mean_error = np.mean(np.abs(ds.y - pred))
        mean_value = np.mean(np.abs(ds.y))
        mean_std = np.mean(std)
        seen.append((float(mean_error), float(mean_std), float(mean_value)))
        if mean_error < 0.5 * mean_value and mean_std > 0.5 * mean_error and mean_std < mean_value:
            break
    else:
        raise AssertionError(seen)
    with pytest.raises(ValueError, match="Dropout must be included"):
        MPNNModel(1, uncertainty=True)
    with pytest.raises(ValueError, match="only supported in regression"):
        MPNNModel(1, mode="classification", uncertainty=True, dropout=0.1)


def test_flat_step_equals_the_per_tensor_step():
    """The flat step (parameters / gradients / Adam moments in three flat buffers, weight gradients accumulated in place
    by the kernels, one Adam launch: TorchModel._ensure_built, ops.direct_param_grads) against the per-tensor path
    (autograd accumulates, one Adam launch per tensor): same losses and parameters after three steps, up to the order
    in which a shared weight's T per-round gradients are added."""
    import deepchem_amd as dc
    B, d, T, M, n_tasks = 5, 32, 3, 3, 2
    mols = qm9_like(15, 20, 6, seed=8)
    rng = np.random.RandomState(9)
    ds = dc.data.NumpyDataset(mols, rng.randn(15, n_tasks), np.ones((15, n_tasks)))
    out = []
    for flat in (True, False):
        model = build("regression", T, M, d, B, n_tasks, seed=7)
        model._flat_step = flat
        losses = []
        model.fit(ds, nb_epoch=1, deterministic=True, checkpoint_interval=0,
                  callbacks=[lambda m, s, iteration_loss=None: losses.append(float(iteration_loss))])
        assert (getattr(model, "_grad_arena", None) is not None) == flat
        if flat:
            assert model._grad_arena.params_homed() and model._pytorch_optimizer._flat is not None
            steps = {float(st["step"]) for st in model._pytorch_optimizer.state.values() if "step" in st}
            assert steps == {3.0}
        out.append((losses, {k: v.detach().cpu().clone() for k, v in model.model.state_dict().items()}))
    assert np.allclose(out[0][0], out[1][0], rtol=1e-5), (out[0][0], out[1][0])
    for k in out[0][1]:
        a, b = out[0][1][k].double(), out[1][1][k].double()
        # (three Adam steps of lr 1e-3: an entry whose gradient is at rounding level may step the other way)
        assert float((a - b).abs().max()) <= 2.2e-3 * 3 and float((a - b).abs().median()) <= 1e-5 * max(1.0, float(b.abs().max())), k
