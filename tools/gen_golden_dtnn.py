"""Generate tests/golden/dtnn_*.npz by running the reference's DTNN on the CPU (plain numeric arrays, no pickles).

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_dtnn.py

The reference is imported through ``oracle.gen_golden.import_reference`` (its rdkit import stub).  One stand-in:
``torch_geometric.utils.scatter`` is not installed, so ``scatter`` is bound IN MEMORY in the reference's ``layers``
module to a sum by index (``index_add_`` along dimension 0 with ``max(index) + 1`` rows unless ``dim_size`` is given:
the function's documented meaning).

* ``dtnn_data.npz``       X and T of the reference's example_DTNN.mat (30 QM7 molecules): data.
* ``dtnn_generator.npz``  ``batch_coulomb_matrix_features`` of a 6-molecule batch.
* ``dtnn_layers.npz``     inputs, parameters and outputs of DTNNEmbedding, DTNNStep and DTNNGather.
* ``dtnn_model.npz``      DTNN(2) on the 30 molecules at batch_size 16 (second batch padded): parameters, first-batch
  outputs, loss and the 17 gradients, the per-step losses of a deterministic 2-epoch fit, the trained parameters and
  ``predict``; and ``e_ref[k] = |loss32 - loss64| / |loss64|`` of the restatement (tests/dtnn_refs.py) per step.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle.gen_golden import REF, import_reference  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")


def scatter_sum(src, index, dim=0, dim_size=None, reduce="sum"):
    import torch
    assert dim == 0 and reduce == "sum"
    rows = int(index.max()) + 1 if dim_size is None else dim_size
    return torch.zeros((rows,) + tuple(src.shape[1:]), dtype=src.dtype).index_add_(0, index, src)


def main():
    import scipy.io
    import torch
    dc = import_reference()
    from deepchem.models.torch_models import layers as ref_layers
    from deepchem.models.torch_models.dtnn import DTNNModel
    from deepchem.utils.batch_utils import batch_coulomb_matrix_features
    import dtnn_refs
    ref_layers.scatter = scatter_sum

    mat = scipy.io.loadmat(os.path.join(REF, "deepchem/models/tests/assets/example_DTNN.mat"))
    X, T = np.asarray(mat["X"], np.float64), np.asarray(mat["T"], np.float64)
    np.savez_compressed(os.path.join(OUT, "dtnn_data.npz"), X=X, T=T)

    # ---- generator: the 6 smallest molecules (the Gaussian matrix is 800 bytes per pair)
    n_atoms = X.astype(bool)[:, :, 0].sum(1)
    six = np.sort(np.argsort(n_atoms, kind="stable")[:6])
    feats = batch_coulomb_matrix_features(X[six], 18, -1, 100)
    np.savez_compressed(os.path.join(OUT, "dtnn_generator.npz"), mols=six, atom_number=feats[0], gaussian=feats[1],
                        atom_membership=feats[2], mem_i=feats[3], mem_j=feats[4])

    # ---- layers
    torch.manual_seed(7)
    rng = np.random.RandomState(7)
    emb = ref_layers.DTNNEmbedding(30, 30)
    z = torch.as_tensor(feats[0], dtype=torch.int64)
    step = ref_layers.DTNNStep(30, 100, 60)
    gath = ref_layers.DTNNGather(30, 5, [40])
    with torch.no_grad():
        for b in (step.b_cf, step.b_df, gath.b_list[0], gath.b_list[1]):
            b.copy_(torch.as_tensor(rng.normal(0, 0.3, b.shape).astype(np.float32)))
    atom_features = torch.as_tensor(rng.normal(0, 1, (len(feats[0]), 30)).astype(np.float32))
    gauss32 = torch.as_tensor(feats[1].astype(np.float32))
    mem = [torch.as_tensor(a) for a in feats[2:]]
    with torch.no_grad():
        out = {"emb_table": emb.embedding_list.numpy(), "emb_in": feats[0], "emb_out": emb(z).numpy(),
               "step_in": atom_features.numpy(), "step_gaussian": gauss32.numpy(), "step_mem_i": feats[3],
               "step_mem_j": feats[4], "step_out": step([atom_features, gauss32, mem[1], mem[2]]).numpy(),
               "gather_in": atom_features.numpy(), "gather_membership": feats[2],
               "gather_out": gath([atom_features, mem[0]]).numpy()}
    for k, v in step.state_dict().items():
        out["step_p_" + k] = v.numpy()
    for k, v in gath.state_dict().items():
        out["gather_p_" + k] = v.numpy()
    np.savez_compressed(os.path.join(OUT, "dtnn_layers.npz"), **out)

    # ---- model
    Tn = (T - T.mean()) / T.std()
    y = np.concatenate([Tn, 0.5 * Tn * Tn - 0.3], axis=1)
    w = np.ones_like(y)
    ds = dc.data.NumpyDataset(X, y, w, ids=None)
    torch.manual_seed(11)
    model = DTNNModel(2, batch_size=16, learning_rate=0.001, log_frequency=1, device=torch.device("cpu"))
    batches = list(model.default_generator(ds, epochs=1, deterministic=True, pad_batches=True))
    first = batches[0]
    inputs, labels, weights = model._prepare_batch(first)
    model.model(inputs)  # materialises the LazyLinear
    rng = np.random.RandomState(11)
    with torch.no_grad():
        for k, p in model.model.named_parameters():
            if p.dim() == 1:
                p.copy_(torch.as_tensor(rng.normal(0, 0.2, p.shape).astype(np.float32)))
    state0 = {k: v.detach().clone().numpy() for k, v in model.model.state_dict().items()}
    out = {"y": y, "w": w}
    for k, v in state0.items():
        out["param0_" + k] = v
    model.model.zero_grad()
    o = model.model(inputs)
    loss = model._loss_fn([o], labels, weights)
    loss.backward()
    out["out0"], out["loss0"] = o.detach().numpy(), np.float64(loss.item())
    for k, p in model.model.named_parameters():
        out["grad_" + k] = p.grad.detach().numpy().copy()
    model.model.zero_grad()
    losses = []
    model.fit(ds, nb_epoch=2, deterministic=True, checkpoint_interval=0, all_losses=losses)
    out["fit_losses"] = np.asarray(losses, np.float64)
    for k, v in model.model.state_dict().items():
        out["final_" + k] = v.detach().numpy()
    out["predict"] = np.asarray(model.predict(ds))

    # the restatement in both precisions over the same four steps
    two_epochs = [(b[0], b[1][0], b[2][0]) for b in batches] * 2
    traj = {}
    for dtype in (torch.float32, torch.float64):
        ref = dtnn_refs.DTNNRef(state0, dtype)
        traj[dtype] = np.asarray(dtnn_refs.fit(ref, two_epochs, 0.001))
    out["e_ref"] = np.abs(traj[torch.float32] - traj[torch.float64]) / np.abs(traj[torch.float64])
    out["fit_losses64"] = traj[torch.float64]
    np.savez_compressed(os.path.join(OUT, "dtnn_model.npz"), **out)
    print("fit losses", out["fit_losses"], "restated32", traj[torch.float32], "e_ref", out["e_ref"])
    for name in ("dtnn_data", "dtnn_generator", "dtnn_layers", "dtnn_model"):
        print(name, os.path.getsize(os.path.join(OUT, name + ".npz")), "bytes")


if __name__ == "__main__":
    main()
