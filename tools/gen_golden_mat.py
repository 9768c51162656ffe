"""Generate tests/golden/mat_layers.npz and mat_model.npz by running the reference's MAT on the CPU (plain numeric
arrays, no pickles).

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_mat.py

The reference is imported through ``oracle.gen_golden.import_reference`` (its rdkit import stub).  The molecules are
synthetic (tests/mat_refs.py: ``fixture_molecules``, random trees laid out as the featurizer lays a molecule out,
regenerated from a seed by the tests; no all-zero feature row, checked here).

* ``mat_layers.npz``  inputs, parameters and outputs of MATEmbedding, MultiHeadedMATAttention, SublayerConnection,
  MATEncoderLayer and MATGenerator (width 32, 4 heads) on a padded batch of 3 molecules, both ``dist_kernel``s.
* ``mat_model.npz``   MATModel(n_encoders=2, h=4, width 32) at batch_size 8 on 20 molecules of 1..30 atoms (second and
  third batch padded): the state-dict key list, parameters, the first batch's padded arrays, outputs, loss and all
  gradients, the per-step losses of a deterministic 2-epoch fit, the trained parameters, ``predict``, and
  ``e_ref[k] = |loss32 - loss64| / |loss64|`` of the restatement (tests/mat_refs.py) per step.  Every reference run
  is on a batch of two or more molecules.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle.gen_golden import import_reference  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
WIDTH = dict(sa_hsize=32, d_input=32, d_hidden=32, d_output=32, encoder_hsize=32)


def main():
    import torch
    dc = import_reference()
    from deepchem.models.torch_models import layers as ref_layers
    from deepchem.models.torch_models.mat import MATModel
    import mat_refs

    # ---- layers
    rng = np.random.RandomState(5)
    mols = [mat_refs.synthetic_molecule(n, rng) for n in (2, 6, 4)]
    helper = MATModel(n_encoders=1, h=4, device=torch.device("cpu"), **WIDTH)
    node = helper.pad_sequence([torch.tensor(m.node_features).float() for m in mols]).astype(np.float32)
    adj = helper.pad_sequence([torch.tensor(m.adjacency_matrix).float() for m in mols]).astype(np.float32)
    dist = helper.pad_sequence([torch.tensor(m.distance_matrix).float() for m in mols]).astype(np.float32)
    mask = torch.sum(torch.abs(torch.as_tensor(node)), dim=-1) != 0
    x = (torch.as_tensor(rng.normal(0, 1, node.shape[:2] + (32,)).astype(np.float32)) * mask.unsqueeze(-1)).contiguous()
    y = torch.as_tensor(rng.normal(0, 1, x.shape).astype(np.float32))
    out = {"node": node, "adj": adj, "dist": dist, "x": x.numpy(), "y": y.numpy(), "n_atoms": np.asarray([3, 7, 5])}

    def save_params(prefix, module):
        for k, v in module.state_dict().items():
            out[prefix + "_p_" + k] = v.numpy().copy()

    def randomise_vectors(module, seed):
        r = np.random.RandomState(seed)
        with torch.no_grad():
            for p in module.parameters():
                if p.dim() == 1:
                    p.copy_(torch.as_tensor(r.normal(0, 0.3, p.shape).astype(np.float32)) + (1.0 if p.mean() > 0.5 else 0.0))

    torch.manual_seed(3)
    with torch.no_grad():
        emb = ref_layers.MATEmbedding(36, 32, 0.0)
        randomise_vectors(emb, 1)
        save_params("emb", emb)
        out["emb_out"] = emb(torch.as_tensor(node)).numpy()
        sub = ref_layers.SublayerConnection(32, 0.0)
        randomise_vectors(sub, 2)
        save_params("sub", sub)
        out["sub_out"] = sub(x, y).numpy()
        for kind in ("softmax", "exp"):
            att = ref_layers.MultiHeadedMATAttention(kind, 0.33, 0.33, 4, 32)
            randomise_vectors(att, 3)
            save_params("att_" + kind, att)
            out["att_%s_out" % kind] = att(x, x, x, mask, torch.as_tensor(adj), torch.as_tensor(dist)).numpy()
            enc = ref_layers.MATEncoderLayer(dist_kernel=kind, h=4, **WIDTH)
            randomise_vectors(enc, 4)
            save_params("enc_" + kind, enc)
            out["enc_%s_out" % kind] = enc(x, mask, torch.as_tensor(adj), torch.as_tensor(dist)).numpy()
        for agg in ("mean", "grover"):
            gen = ref_layers.MATGenerator(32, agg, 2, 1, 0.0, 16, 4)
            randomise_vectors(gen, 5)
            save_params("gen_" + agg, gen)
            out["gen_%s_out" % agg] = gen(x, mask).numpy()
    np.savez_compressed(os.path.join(OUT, "mat_layers.npz"), **out)

    # ---- model
    mols = mat_refs.fixture_molecules()
    assert all(np.abs(m.node_features).sum(1).min() > 0 for m in mols), "a fixture molecule has an all-zero feature row"
    X = np.empty(len(mols), dtype=object)
    X[:] = mols
    rng = np.random.RandomState(11)
    yv = rng.normal(0, 1, (len(mols), 1))
    w = np.ones_like(yv)
    out = {"y": yv, "w": w, "n_atoms": np.asarray([m.node_features.shape[0] for m in mols])}
    for kind in ("softmax", "exp"):
        pre = "" if kind == "softmax" else "exp_"
        ds = dc.data.NumpyDataset(X, yv, w, ids=None)
        torch.manual_seed(11)
        model = MATModel(dist_kernel=kind, n_encoders=2, h=4, batch_size=8, learning_rate=0.001, log_frequency=1,
                         device=torch.device("cpu"), **WIDTH)
        randomise_vectors(model.model, 12)
        state0 = {k: v.detach().clone().numpy() for k, v in model.model.state_dict().items()}
        if kind == "softmax":
            out["keys"] = np.asarray(list(state0))
            for k, v in state0.items():
                out["param0_" + k] = v
        else:
            assert all(np.array_equal(out["param0_" + k], v) for k, v in state0.items())
        batches = list(model.default_generator(ds, epochs=1, deterministic=True, pad_batches=True))
        inputs, labels, weights = model._prepare_batch(batches[0])
        if kind == "softmax":
            out["gen_node"], out["gen_adj"], out["gen_dist"] = [np.asarray(a, np.float32) for a in batches[0][0]]
        model.model.zero_grad()
        o = model.model(inputs)
        loss = model._loss_fn([o], labels, weights)
        loss.backward()
        out[pre + "out0"], out[pre + "loss0"] = o.detach().numpy(), np.float64(loss.item())
        for k, p in model.model.named_parameters():
            out[pre + "grad_" + k] = p.grad.detach().numpy().copy()
        model.model.zero_grad()
        losses = []
        model.fit(ds, nb_epoch=2, deterministic=True, checkpoint_interval=0, all_losses=losses)
        out[pre + "fit_losses"] = np.asarray(losses, np.float64)
        if kind == "softmax":
            for k, v in model.model.state_dict().items():
                out["final_" + k] = v.detach().numpy()
        out[pre + "predict"] = np.asarray(model.predict(ds))

        # the restatement in both precisions over the same six steps
        steps = [(mat_refs.pack(list(X_b)), y_b, w_b)
                 for X_b, y_b, w_b, _ in ds.iterbatches(batch_size=8, deterministic=True, pad_batches=True)] * 2
        traj = {}
        for dtype in (torch.float32, torch.float64):
            ref = mat_refs.MATRef(state0, dtype, dist_kernel=kind, h=4)
            traj[dtype] = np.asarray(mat_refs.fit(ref, steps, 0.001))
        out[pre + "e_ref"] = np.abs(traj[torch.float32] - traj[torch.float64]) / np.abs(traj[torch.float64])
        print(kind, "fit losses", out[pre + "fit_losses"], "restated32", traj[torch.float32], "e_ref", out[pre + "e_ref"])
    np.savez_compressed(os.path.join(OUT, "mat_model.npz"), **out)
    for name in ("mat_layers", "mat_model"):
        print(name, os.path.getsize(os.path.join(OUT, name + ".npz")), "bytes")


if __name__ == "__main__":
    main()
