"""Generate tests/golden/megnet_layers.npz and megnet_model.npz by running the reference's GraphNetwork and MEGNetModel
on the CPU (plain numeric arrays, no pickles).

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_megnet.py

The reference is imported through ``oracle.gen_golden.import_reference``.  Its MEGNet needs torch_geometric, which is
not installed where this runs; three stand-ins are placed in ``sys.modules`` for the run, each written from
torch_geometric's published behaviour:

* ``torch_geometric.utils.scatter``  sum and mean along dimension 0 into ``index.max() + 1`` rows (the sizing rule that
  makes the reference raise when the last node has no arriving edge or the last graph no edge; a row in the middle
  with nothing to average is zero).  The GraphNetwork numbers below are the reference's own code on this function.
* ``torch_geometric.data.Data`` / ``Batch``  ``Batch.from_data_list`` concatenates ``x``, ``edge_attr`` and
  ``global_features`` along dimension 0, ``edge_index`` along dimension 1 with node offsets, and carries ``batch``.
* ``torch_geometric.nn.Set2Set``  an ``nn.LSTM`` submodule ``lstm`` and the forward of ``tests/megnet_refs.set2set``.  So
  the Set2Set numbers (and the state-dict key names ``set2set_*.lstm.*``) are a RESTATEMENT of torch_geometric's
  published source, not its output.

Graphs: built by hand from a seeded RandomState (tests/megnet_refs.py: ``random_graph``, ``fixture_graphs``), about 10
nodes at average degree 4, Fn = 5, Fe = 3, Fg = 4, every node with an arriving edge, duplicate edges and self-loops
included.

* ``megnet_layers.npz``  GraphNetwork: inputs, parameters, outputs and all gradients (of sum(out * cotangent)) for
  undirected / directed x residual on / off x (one graph with batch=None, a 4-graph batch).
* ``megnet_model.npz``   a regression model (n_tasks=2) and a classification model (n_classes=5, prefix ``cls_``), both
  n_blocks=3, on 20 graphs at batch_size 8 (last batch short): the state-dict key list and shapes, parameters, the
  first batch's outputs, loss and every gradient, ``predict`` before and after a deterministic 2-epoch fit, the
  per-step losses, and ``e_ref[k] = |loss32 - loss64| / |loss64|`` of the restatement per step.
"""
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle.gen_golden import import_reference  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
SIZES = dict(n_node_features=5, n_edge_features=3, n_global_features=4)


def install_scatter():
    import torch

    def scatter(src, index, dim=0, dim_size=None, reduce="sum"):
        assert dim in (0, -2) and reduce in ("sum", "add", "mean")
        n = int(index.max()) + 1 if dim_size is None else dim_size
        # (scatter_add_, as torch_geometric does: index_add_ keeps its source for the backward, which the reference's
        # in-place residual then invalidates)
        out = src.new_zeros((n,) + tuple(src.shape[1:])).scatter_add_(0, index.view(-1, 1).expand_as(src), src)
        if reduce == "mean":
            count = src.new_zeros(n).index_add_(0, index, src.new_ones(index.shape[0])).clamp(min=1)
            out = out / count.view((n,) + (1,) * (src.dim() - 1))
        return out
    pkg = types.ModuleType("torch_geometric")
    pkg.__path__ = []  # a package without further submodules: the reference's other torch_geometric imports stay absent
    utils = types.ModuleType("torch_geometric.utils")
    utils.scatter = scatter
    pkg.utils = utils
    sys.modules["torch_geometric"], sys.modules["torch_geometric.utils"] = pkg, utils


def install_data_and_set2set():
    import torch
    import megnet_refs

    class Data:
        def __init__(self, **kwargs):
            self.items = {k: v for k, v in kwargs.items() if v is not None}

        def __getitem__(self, key):
            return self.items[key]

    class Batch(Data):
        @classmethod
        def from_data_list(cls, data_list):
            at, idx, batch = 0, [], []
            for k, d in enumerate(data_list):
                idx.append(d["edge_index"] + at)
                batch.append(torch.full((d["x"].shape[0],), k, dtype=torch.int64))
                at += d["x"].shape[0]
            return cls(x=torch.cat([d["x"] for d in data_list]), edge_index=torch.cat(idx, dim=1),
                       edge_attr=torch.cat([d["edge_attr"] for d in data_list]),
                       global_features=torch.cat([d["global_features"] for d in data_list]), batch=torch.cat(batch))

    class Set2Set(torch.nn.Module):
        def __init__(self, in_channels, processing_steps, **kwargs):
            super().__init__()
            self.in_channels, self.out_channels, self.processing_steps = in_channels, 2 * in_channels, processing_steps
            self.lstm = torch.nn.LSTM(self.out_channels, in_channels, **kwargs)

        def forward(self, x, index):
            m = self.lstm
            return megnet_refs.set2set(m.weight_ih_l0, m.weight_hh_l0, m.bias_ih_l0, m.bias_hh_l0, x, index,
                                       int(index.max()) + 1, self.processing_steps)

    data, nn_ = types.ModuleType("torch_geometric.data"), types.ModuleType("torch_geometric.nn")
    data.Data, data.Batch, nn_.Set2Set = Data, Batch, Set2Set
    sys.modules["torch_geometric.data"], sys.modules["torch_geometric.nn"] = data, nn_
    sys.modules["torch_geometric"].data, sys.modules["torch_geometric"].nn = data, nn_


def main():
    import torch
    install_scatter()
    dc = import_reference()
    from deepchem.models.torch_models.layers import GraphNetwork
    install_data_and_set2set()
    from deepchem.models.torch_models.megnet import MEGNetModel
    import megnet_refs as R

    # ---- layers
    out = {}
    rng = np.random.RandomState(7)
    single = [R.random_graph(rng, 10, 28)]
    four = [R.random_graph(rng, n, 3 * n - 2) for n in (9, 1, 12, 10)]  # (a 1-node graph: its cycle is a self-loop)
    case = 0
    for undirected in (True, False):
        for residual in (True, False):
            for graphs, with_batch in ((single, False), (four, True)):
                x, ei, e, u, batch = R.pack(graphs)
                torch.manual_seed(20 + case)
                gn = GraphNetwork(is_undirected=undirected, residual_connection=residual, **SIZES)
                tx, te, tu = (torch.tensor(a, dtype=torch.float32, requires_grad=True) for a in (x, e, u))
                # (clones: the reference adds its residual in place, which a leaf that needs a gradient does not allow)
                o = gn(tx.clone(), torch.as_tensor(ei), te.clone(), tu.clone(), torch.as_tensor(batch) if with_batch else None)
                cots = [torch.as_tensor(rng.normal(0, 1, t.shape).astype(np.float32)) for t in o]
                sum((t * c).sum() for t, c in zip(o, cots)).backward()
                pre = "c%d_" % case
                out.update({pre + "undirected": np.asarray(undirected), pre + "residual": np.asarray(residual),
                            pre + "with_batch": np.asarray(with_batch), pre + "x": x, pre + "ei": ei, pre + "e": e, pre + "u": u,
                            pre + "batch": batch})
                for name, t, c, leaf in zip("xeu", o, cots, (tx, te, tu)):
                    out[pre + "out_" + name], out[pre + "cot_" + name] = t.detach().numpy(), c.numpy()
                    out[pre + "grad_" + name] = leaf.grad.numpy().copy()
                for k, v in gn.named_parameters():
                    out[pre + "p_" + k], out[pre + "gradp_" + k] = v.detach().numpy().copy(), v.grad.numpy().copy()
                case += 1
    out["n_cases"] = np.asarray(case)
    np.savez_compressed(os.path.join(OUT, "megnet_layers.npz"), **out)

    # ---- models
    graphs = R.fixture_graphs()
    X = np.empty(len(graphs), dtype=object)
    X[:] = [dc.feat.GraphData(g.node_features, g.edge_index, g.edge_features, global_features=g.global_features)
            for g in graphs]
    rng = np.random.RandomState(11)
    out = {"n_nodes": np.asarray([g.num_nodes for g in graphs]), "n_edges": np.asarray([g.num_edges for g in graphs])}
    for mode in ("regression", "classification"):
        pre = "" if mode == "regression" else "cls_"
        kw = dict(n_tasks=2) if mode == "regression" else dict(n_classes=5)
        yv = rng.normal(0, 1, (len(graphs), 2)) if mode == "regression" else \
            rng.randint(0, 5, (len(graphs), 1)).astype(np.float64)
        w = np.ones((len(graphs), yv.shape[1]))
        out[pre + "y"], out[pre + "w"] = yv, w
        ds = dc.data.NumpyDataset(X, yv, w, ids=None)
        torch.manual_seed(11)
        model = MEGNetModel(n_blocks=3, mode=mode, batch_size=8, learning_rate=0.001, log_frequency=1,
                            device=torch.device("cpu"), **SIZES, **kw)
        state0 = {k: v.detach().clone().numpy() for k, v in model.model.state_dict().items()}
        out[pre + "keys"] = np.asarray(list(state0))
        out[pre + "shapes"] = np.asarray([list(v.shape) + [0] * (2 - v.ndim) for v in state0.values()])
        for k, v in state0.items():
            out[pre + "param0_" + k] = v
        out[pre + "predict0"] = np.asarray(model.predict(ds))
        batches = list(model.default_generator(ds, epochs=1, deterministic=True, pad_batches=True))
        inputs, labels, weights = model._prepare_batch(batches[0])
        model.model.train()
        model.model.zero_grad()
        o = model.model(inputs)
        loss = model._loss_fn([o[1]] if mode == "classification" else [o], labels, weights)
        loss.backward()
        o = o if mode == "regression" else o[0]
        out[pre + "out0"], out[pre + "loss0"] = o.detach().numpy(), np.float64(loss.item())
        for k, p in model.model.named_parameters():
            out[pre + "grad_" + k] = p.grad.detach().numpy().copy()
        model.model.zero_grad()
        losses = []
        model.fit(ds, nb_epoch=2, deterministic=True, checkpoint_interval=0, all_losses=losses)
        out[pre + "fit_losses"] = np.asarray(losses, np.float64)
        out[pre + "predict"] = np.asarray(model.predict(ds))

        # the restatement in both precisions over the same six steps
        steps = [(R.pack(list(X_b)), y_b, w_b)
                 for X_b, y_b, w_b, _ in ds.iterbatches(batch_size=8, deterministic=True, pad_batches=True)] * 2
        traj = {}
        for dtype in (torch.float32, torch.float64):
            ref = R.MEGNetRef(state0, dtype, 3, mode=mode, n_tasks=kw.get("n_tasks", 1), n_classes=kw.get("n_classes", 2))
            traj[dtype] = np.asarray(R.fit(ref, steps, 0.001))
        out[pre + "e_ref"] = np.abs(traj[torch.float32] - traj[torch.float64]) / np.abs(traj[torch.float64])
        print(mode, "fit losses", out[pre + "fit_losses"], "restated32", traj[torch.float32], "e_ref", out[pre + "e_ref"])
    np.savez_compressed(os.path.join(OUT, "megnet_model.npz"), **out)
    for name in ("megnet_layers", "megnet_model"):
        print(name, os.path.getsize(os.path.join(OUT, name + ".npz")), "bytes")


if __name__ == "__main__":
    main()
