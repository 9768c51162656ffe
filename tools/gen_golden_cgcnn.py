"""Generate tests/golden/cgcnn_layers.npz and cgcnn_model.npz by running the reference's CGCNNLayer, CGCNN and
CGCNNModel on the CPU (plain numeric arrays, no pickles).

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_cgcnn.py

The reference is imported through ``oracle.gen_golden.import_reference``.  Its CGCNN needs DGL, which is not installed
where this runs; an in-memory stand-in is placed in ``sys.modules`` for the run, written from DGL's published
behaviour.  The reference uses DGL only for generic message passing and the readout, so the arithmetic of the layer is
the reference's own code running on:

* ``dgl.graph((src, dst), num_nodes=n)``  a graph with ``ndata`` / ``edata`` dictionaries and ``to(device)``.
* ``dgl.batch(graphs)``  nodes and edges concatenated in order, edge ends shifted by the node offsets, the features
  of ``ndata`` / ``edata`` concatenated, the node count of every graph kept.
* ``graph.update_all(message_func, reduce_func)``  ``message_func`` once over all edges (``edges.src``, ``edges.dst``,
  ``edges.data``); then the nodes are bucketed by in-degree and ``reduce_func`` is called once per bucket of positive
  degree with ``nodes.mailbox[key]`` of shape (nodes of the bucket, degree, width), a node's messages in edge order,
  and ``nodes.data``; nodes of in-degree ZERO are not passed to ``reduce_func`` and their new feature is filled with
  zeros (DGL's documented rule; taken from the documentation, not from a run).
* ``dgl.mean_nodes(graph, key)``  the mean of ``ndata[key]`` over the nodes of each graph of the batch.

Graphs: built by hand from a seeded RandomState (tests/cgcnn_refs.py: ``random_graph``, ``fixture_graphs``), about 10
nodes with 4 arriving edges each, Fn = 5, Fe = 3, duplicate edges and self-loops included; one fixture graph and one
layer case hold a node nothing arrives at.

* ``cgcnn_layers.npz``  CGCNNLayer (H = 8): inputs, parameters, running statistics before and after, outputs and all
  gradients (of sum(out * cotangent)) for batch_norm on / off x training / eval x (one graph, a 4-graph batch).
* ``cgcnn_model.npz``   a regression model (n_tasks = 2) and a one-task classification model (n_classes = 5, prefix
  ``cls_``), both hidden 8, num_conv 3, predictor 16, on 20 graphs at batch_size 8 (last batch short): the state-dict
  key list and shapes, the state, the first batch's outputs, loss and every gradient, ``predict`` before and after a
  deterministic 2-epoch fit, the per-step losses, the float64 restatement's losses of the same steps (``fit_losses64``) and
  ``e_ref[k] = |loss32 - loss64| / |loss64|`` of the restatement per step.  Only there is the reference's ``softmax`` without ``dim`` the softmax over the classes.
"""
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.gen_golden import import_reference  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
H, FN, FE = 8, 5, 3


def install_dgl():
    import torch

    class Frame(dict):
        pass

    class View:
        def __init__(self, **kw):
            self.__dict__.update(kw)

    class DGLGraph:
        def __init__(self, src, dst, num_nodes, sizes=None):
            self.src, self.dst, self.n = src.long(), dst.long(), int(num_nodes)
            self.ndata, self.edata = Frame(), Frame()
            self.sizes = [self.n] if sizes is None else list(sizes)

        def to(self, device):
            return self

        def edges(self):
            return self.src, self.dst

        def update_all(self, message_func, reduce_func):
            edges = View(src={k: v[self.src] for k, v in self.ndata.items()},
                         dst={k: v[self.dst] for k, v in self.ndata.items()}, data=dict(self.edata))
            messages = message_func(edges)
            degree = torch.bincount(self.dst, minlength=self.n)
            order = torch.argsort(self.dst, stable=True)  # a node's messages in edge order
            start = torch.cumsum(degree, 0) - degree
            new = {}
            for deg in sorted(set(degree.tolist())):
                if deg == 0:
                    continue
                nodes = torch.nonzero(degree == deg).reshape(-1)
                take = order[(start[nodes].unsqueeze(1) + torch.arange(deg).unsqueeze(0)).reshape(-1)]
                mailbox = {k: v[take].reshape(nodes.numel(), deg, *v.shape[1:]) for k, v in messages.items()}
                got = reduce_func(View(mailbox=mailbox, data={k: v[nodes] for k, v in self.ndata.items()}))
                for k, v in got.items():
                    if k not in new:
                        new[k] = v.new_zeros((self.n,) + tuple(v.shape[1:]))  # in-degree zero: zeros
                    new[k] = new[k].index_copy(0, nodes, v)
            for k, v in new.items():
                self.ndata[k] = v

    def graph(ends, num_nodes=None):
        return DGLGraph(ends[0], ends[1], num_nodes)

    def batch(graphs):
        at, src, dst = 0, [], []
        for g in graphs:
            src.append(g.src + at), dst.append(g.dst + at)
            at += g.n
        out = DGLGraph(torch.cat(src), torch.cat(dst), at, [g.n for g in graphs])
        for k in graphs[0].ndata:
            out.ndata[k] = torch.cat([g.ndata[k] for g in graphs])
        for k in graphs[0].edata:
            out.edata[k] = torch.cat([g.edata[k] for g in graphs])
        return out

    def mean_nodes(g, key):
        return torch.stack([rows.mean(0) for rows in torch.split(g.ndata[key], g.sizes)])

    dgl = types.ModuleType("dgl")
    dgl.graph, dgl.batch, dgl.mean_nodes, dgl.DGLGraph = graph, batch, mean_nodes, DGLGraph
    sys.modules["dgl"] = dgl
    return dgl


def main():
    import torch
    dgl = install_dgl()
    dc = import_reference()
    from deepchem.models.torch_models.cgcnn import CGCNNLayer, CGCNNModel
    from tests import cgcnn_refs as R

    def to_dgl(graphs):
        gs = []
        for g in graphs:
            d = dgl.graph((torch.as_tensor(g.edge_index[0]), torch.as_tensor(g.edge_index[1])), num_nodes=g.num_nodes)
            gs.append(d)
        return dgl.batch(gs)

    # ---- layers
    out = {}
    rng = np.random.RandomState(7)
    single = [R.random_graph(rng, 10, 28, H, FE)]
    four = [R.random_graph(rng, n, 3 * n - 2, H, FE) for n in (9, 1, 12, 10)]
    bare = four[2]  # one more node, nothing arrives at it
    four[2] = R.Graph(np.concatenate([bare.node_features, rng.normal(0, 1, (1, H))]), bare.edge_index, bare.edge_features)
    case = 0
    for with_bn in (True, False):
        for training in (True, False):
            for graphs in (single, four):
                x, ei, e, batch = R.pack(graphs)
                torch.manual_seed(40 + case)
                layer = CGCNNLayer(hidden_node_dim=H, edge_dim=FE, batch_norm=with_bn)
                pre = "c%d_" % case
                if with_bn:
                    with torch.no_grad():  # statistics and an affine map that are not the initial ones
                        layer.batch_norm.running_mean.copy_(torch.as_tensor(rng.normal(0, 0.3, 2 * H), dtype=torch.float32))
                        layer.batch_norm.running_var.copy_(torch.as_tensor(rng.uniform(0.5, 2, 2 * H), dtype=torch.float32))
                        layer.batch_norm.weight.copy_(torch.as_tensor(rng.uniform(0.5, 1.5, 2 * H), dtype=torch.float32))
                        layer.batch_norm.bias.copy_(torch.as_tensor(rng.normal(0, 0.3, 2 * H), dtype=torch.float32))
                    out[pre + "rm0"] = layer.batch_norm.running_mean.numpy().copy()
                    out[pre + "rv0"] = layer.batch_norm.running_var.numpy().copy()
                layer.train(training)
                for k, v in layer.named_parameters():
                    out[pre + "p_" + k] = v.detach().numpy().copy()
                th, te = (torch.tensor(a, dtype=torch.float32, requires_grad=True) for a in (x, e))
                o = layer(to_dgl(graphs), th, te)
                cot = torch.as_tensor(rng.normal(0, 1, o.shape).astype(np.float32))
                (o * cot).sum().backward()
                out.update({pre + "with_bn": np.asarray(with_bn), pre + "training": np.asarray(training), pre + "h": x, pre + "ei": ei,
                            pre + "e": e, pre + "out": o.detach().numpy(), pre + "cot": cot.numpy(),
                            pre + "grad_h": th.grad.numpy().copy(), pre + "grad_e": te.grad.numpy().copy()})
                for k, v in layer.named_parameters():
                    out[pre + "gradp_" + k] = v.grad.numpy().copy()
                if with_bn:
                    out[pre + "rm1"] = layer.batch_norm.running_mean.numpy().copy()
                    out[pre + "rv1"] = layer.batch_norm.running_var.numpy().copy()
                    out[pre + "tracked"] = np.asarray(int(layer.batch_norm.num_batches_tracked))
                case += 1
    out["n_cases"] = np.asarray(case)
    np.savez_compressed(os.path.join(OUT, "cgcnn_layers.npz"), **out)

    # ---- models
    graphs = R.fixture_graphs(FN, FE)
    X = np.empty(len(graphs), dtype=object)
    X[:] = [dc.feat.GraphData(g.node_features, g.edge_index, g.edge_features) for g in graphs]
    rng = np.random.RandomState(11)
    out = {"n_nodes": np.asarray([g.num_nodes for g in graphs]), "n_edges": np.asarray([g.num_edges for g in graphs])}
    sizes = dict(in_node_dim=FN, hidden_node_dim=H, in_edge_dim=FE, num_conv=3, predictor_hidden_feats=16)
    for mode in ("regression", "classification"):
        pre = "" if mode == "regression" else "cls_"
        kw = dict(n_tasks=2) if mode == "regression" else dict(n_classes=5)
        yv = rng.normal(0, 1, (len(graphs), 2)) if mode == "regression" else \
            rng.randint(0, 5, (len(graphs), 1)).astype(np.float64)
        w = np.ones((len(graphs), yv.shape[1]))
        out[pre + "y"], out[pre + "w"] = yv, w
        ds = dc.data.NumpyDataset(X, yv, w, ids=None)
        torch.manual_seed(11)
        model = CGCNNModel(mode=mode, batch_size=8, learning_rate=0.001, log_frequency=1, device=torch.device("cpu"),
                           **sizes, **kw)
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
        # (that forward moved the running statistics: the trajectory below starts from the initial state again)
        model.model.load_state_dict({k: torch.as_tensor(v) for k, v in state0.items()})
        losses = []
        model.fit(ds, nb_epoch=2, deterministic=True, checkpoint_interval=0, all_losses=losses)
        out[pre + "fit_losses"] = np.asarray(losses, np.float64)
        out[pre + "predict"] = np.asarray(model.predict(ds))
        for k, v in model.model.state_dict().items():
            if "running_" in k or "tracked" in k:
                out[pre + "after_" + k] = v.detach().numpy().copy()

        # the restatement in both precisions over the same six steps
        steps = [(R.pack(list(X_b)), y_b, w_b)
                 for X_b, y_b, w_b, _ in ds.iterbatches(batch_size=8, deterministic=True, pad_batches=True)] * 2
        traj = {}
        for dtype in (torch.float32, torch.float64):
            ref = R.CGCNNRef(state0, dtype, 3, mode=mode, n_tasks=kw.get("n_tasks", 1), n_classes=kw.get("n_classes", 2))
            traj[dtype] = np.asarray(R.fit(ref, steps, 0.001))
        out[pre + "fit_losses64"] = traj[torch.float64]
        out[pre + "e_ref"] = np.abs(traj[torch.float32] - traj[torch.float64]) / np.abs(traj[torch.float64])
        print(mode, "fit losses", out[pre + "fit_losses"], "restated32", traj[torch.float32], "e_ref", out[pre + "e_ref"])
    np.savez_compressed(os.path.join(OUT, "cgcnn_model.npz"), **out)
    for name in ("cgcnn_layers", "cgcnn_model"):
        print(name, os.path.getsize(os.path.join(OUT, name + ".npz")), "bytes")


if __name__ == "__main__":
    main()
