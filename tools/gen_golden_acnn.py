"""Generate tests/golden/acnn_layer.npz and acnn_model.npz by running the reference's AtomicConvolution, AtomicConv
and AtomConvModel on the CPU (plain numeric arrays, no pickles).

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_acnn.py

The reference is imported through ``oracle.gen_golden.import_reference``; the model is pure torch and needs no stand-in.

* ``acnn_layer.npz``  cases ``c{k}_``: inputs (X, Nbrs, Nbrs_Z), the (rc, rs, re) triples, the type list (``types``, empty:
  none), the box (``box``, empty: none), the output, a cotangent and the gradients of sum(out * cot) for rc, rs, re.
  Cases 0-2 are the inputs of the reference's own test of the layer (models/tests/test_layers.py:895-945: 4 samples of 5
  atoms with 2 neighbours, three filters; no types, types [1, 2, 8], and a zero box whose output is all NaN) drawn from
  a seeded RandomState; case 3 has the model's 66 default filters and 15 default types with Z = 0 padding and a box;
  case 4 float64 coordinates and integer types (what ``default_generator`` hands over before the model casts).
* ``acnn_model.npz``  a model with frag sizes (3, 5, 7), 4 neighbours, batch_size 3, one dense layer of 8, dropout 0,
  types [6, 7, 8, -1] and 6 filters on 7 dataset rows (last batch padded): the rows (coordinates, z, neighbour lists as
  padded arrays with counts and a has-entry mask), the 12 arrays of every batch of the reference's generator loop, the
  state-dict keys, shapes and values, the first batch's output, loss and gradients, ``predict`` before and after a
  2-epoch fit, the six losses, the float64 restatement's (``fit_losses64``) and ``e_ref`` = the float32 restatement's
  relative distance from them per step.
"""
import copy
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.gen_golden import import_reference  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
SIZES, MAX_NBRS, BATCH, N_ITEMS = (3, 5, 7), 4, 3, 7
MODEL_TYPES = [6, 7., 8., -1.]
MODEL_RADIAL = [[1.5, 3.0, 6.0], [0.0, 2.0], [0.4]]


def rows_to_arrays(rows):
    """Dataset rows as numeric arrays: per fragment k ``f{k}_coords`` (n, N, 3), ``f{k}_z`` (n, N), ``f{k}_nbrs``
    (n, N, MAX_NBRS) padded with -1, ``f{k}_has`` (n, N): whether the dict has the atom."""
    out = {}
    for k, n_atoms in enumerate(SIZES):
        nb = -np.ones((len(rows), n_atoms, MAX_NBRS), np.int64)
        has = np.zeros((len(rows), n_atoms), bool)
        for i, row in enumerate(rows):
            for a, lst in row[3 * k + 1].items():
                has[i, a] = True
                nb[i, a, :len(lst)] = lst
        out.update({"f%d_coords" % k: np.stack([r[3 * k] for r in rows]), "f%d_z" % k: np.stack([r[3 * k + 2] for r in rows]),
                    "f%d_nbrs" % k: nb, "f%d_has" % k: has})
    return out


def main():
    import torch
    dc = import_reference()
    from deepchem.models.torch_models.layers import AtomicConvolution
    from deepchem.models.torch_models.acnn import AtomConvModel
    from tests import acnn_refs as R

    # ---- the layer
    out = {}
    rng = np.random.RandomState(3)
    test_params = [[5.0, 2.0, 0.5], [10.0, 2.0, 0.5], [5.0, 1.0, 0.2]]
    x = rng.rand(4, 5, 3).astype(np.float32)
    nb = rng.randint(5, size=(4, 5, 2))
    z = rng.randint(1, 10, size=(4, 5, 2))
    cases = [(x, nb, z, test_params, None, None), (x, nb, z, test_params, [1, 2, 8], None),
             (x, nb, z, test_params, None, [0.0, 0.0, 0.0])]
    X3, nb3, Z3 = R.random_case(rng, 3, 7, 12, scale=6.0)
    box3 = [5.0, 6.5, 4.0]
    X3 = R.settle_box(rng, X3, nb3, box3, 6.0)
    Z3 = rng.choice(np.asarray([0, 1, 6, 7, 8, 16, 53, -1], np.float32), Z3.shape)
    cases.append((X3, nb3, Z3, R.radial_params(), R.DEFAULT_TYPES, box3))
    X4, nb4, Z4 = R.random_case(rng, 2, 6, 3, scale=4.0)
    cases.append((X4.astype(np.float64) + 1e-9, nb4.astype(np.int64), Z4.astype(np.int64), R.radial_params()[:5], [6, 7, -1], None))
    for k, (X, nbrs, Z, params, types, box) in enumerate(cases):
        layer = AtomicConvolution(atom_types=types, radial_params=params if k else torch.tensor(params), box_size=box)
        o = layer([X, nbrs, Z])
        cot = torch.as_tensor(rng.normal(0, 1, o.shape), dtype=o.dtype)
        (o * cot).sum().backward()
        pre = "c%d_" % k
        out.update({pre + "X": X, pre + "nbrs": nbrs, pre + "Z": Z, pre + "params": np.asarray(params, np.float64),
                    pre + "types": np.asarray(types or [], np.float64), pre + "box": np.asarray(box or [], np.float64),
                    pre + "out": o.detach().numpy(), pre + "cot": cot.numpy(),
                    pre + "grad_rc": layer.rc.grad.numpy().reshape(-1), pre + "grad_rs": layer.rs.grad.numpy().reshape(-1),
                    pre + "grad_re": layer.re.grad.numpy().reshape(-1)})
    out["n_cases"] = np.asarray(len(cases))
    np.savez_compressed(os.path.join(OUT, "acnn_layer.npz"), **out)

    # ---- the model
    rng = np.random.RandomState(5)
    rows = R.fixture_dataset_rows(rng, N_ITEMS, SIZES, MAX_NBRS)
    out = rows_to_arrays(rows)
    y, w = rng.normal(0, 1, (N_ITEMS, 1)), np.ones((N_ITEMS, 1))
    out["y"], out["w"] = y, w
    ds = dc.data.NumpyDataset(copy.deepcopy(rows), y, w, ids=None)  # (the reference's generator writes into the z arrays)
    torch.manual_seed(5)
    model = AtomConvModel(n_tasks=1, frag1_num_atoms=SIZES[0], frag2_num_atoms=SIZES[1], complex_num_atoms=SIZES[2],
                          max_num_neighbors=MAX_NBRS, batch_size=BATCH, atom_types=MODEL_TYPES, radial=MODEL_RADIAL,
                          layer_sizes=[8], dropouts=0.0, log_frequency=1, device=torch.device("cpu"))
    state0 = {k: v.detach().clone().numpy() for k, v in model.model.state_dict().items()}
    out["keys"] = np.asarray(list(state0))
    out["shapes"] = np.asarray([list(v.shape) + [0] * (2 - v.ndim) for v in state0.values()])
    for k, v in state0.items():
        out["param0_" + k] = v
    batches = list(model.default_generator(ds, epochs=1, deterministic=True, pad_batches=True))
    out["n_batches"] = np.asarray(len(batches))
    for b, (inputs, labels, weights) in enumerate(batches):
        for j, a in enumerate(inputs):
            out["gen%d_%d" % (b, j)] = np.asarray(a)
        out["gen%d_y" % b], out["gen%d_w" % b] = np.asarray(labels[0]), np.asarray(weights[0])
    out["predict0"] = np.asarray(model.predict(ds))
    inputs, labels, weights = model._prepare_batch(batches[0])
    model.model.train()
    model.model.zero_grad()
    o = model.model(inputs)
    loss = model._loss_fn(o, labels, weights)
    loss.backward()
    out["out0"], out["loss0"] = o[0].detach().numpy(), np.float64(loss.item())
    for k, p in model.model.named_parameters():
        out["grad_" + k] = p.grad.detach().numpy().copy()
    model.model.zero_grad()
    losses = []
    model.fit(ds, nb_epoch=2, deterministic=True, checkpoint_interval=0, all_losses=losses)
    out["fit_losses"] = np.asarray(losses, np.float64)
    out["predict"] = np.asarray(model.predict(ds))

    steps = [(inputs, labels[0], weights[0]) for inputs, labels, weights in batches] * 2
    traj = {}
    for dtype in (torch.float32, torch.float64):
        traj[dtype] = np.asarray(R.fit(R.ACNNRef(state0, dtype, MODEL_TYPES, MODEL_RADIAL), steps, 0.001))
    out["fit_losses64"] = traj[torch.float64]
    out["e_ref"] = np.abs(traj[torch.float32] - traj[torch.float64]) / np.abs(traj[torch.float64])
    print("fit losses", out["fit_losses"], "restated32", traj[torch.float32], "e_ref", out["e_ref"])
    np.savez_compressed(os.path.join(OUT, "acnn_model.npz"), **out)
    for name in ("acnn_layer", "acnn_model"):
        print(name, os.path.getsize(os.path.join(OUT, name + ".npz")), "bytes")


if __name__ == "__main__":
    main()
