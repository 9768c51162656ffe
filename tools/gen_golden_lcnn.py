"""Generate tests/golden/lcnn_layers.npz and lcnn_model.npz by running the reference's LCNNBlock, LCNN and LCNNModel on
the CPU (plain numeric arrays, no pickles).

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_lcnn.py

The reference is imported through ``oracle.gen_golden.import_reference``.  Its LCNN needs DGL, which is not installed
where this runs; the in-memory stand-in of tools/gen_golden_cgcnn.py is placed in ``sys.modules`` for the run, with what
LCNN needs in addition, written from DGL's published behaviour:

* ``dgl.function.copy_u(u, out)``  a message function: the feature ``u`` of every edge's source under the key ``out``.
* ``graph.local_var()``  a graph with the same structure whose ``ndata`` / ``edata`` are shallow copies: writing to them
  does not reach the caller's graph.
* ``graph.ndata.pop(key)``  the dictionary's.

The reference uses DGL only for that message passing and the readout, so the arithmetic of the block is the reference's
own code.  The dropout masks the reference draws are RECORDED by wrapping the ``forward`` of its ``nn.Dropout`` modules for
the run (one call of P values per site in a block, stacked to (N, P); one (N, S) call in the atom-wise convolution), so
the tests can inject them.

Graphs: periodic triangular lattices of at most 12 sites (tests/lcnn_refs.py: ``torus``, ``fixture_graphs``), K = 19
neighbour slots, P = 6 permutations.

* ``lcnn_layers.npz``  LCNNBlock(19 * 3, 8): inputs, parameters, masks, running statistics before and after, outputs and
  all gradients (of sum(out * cotangent)) for training / eval x (one graph, a 4-graph batch).
The fit runs on plain gradient descent (rate 0.01), not on the model's default Adam.  In training mode the gradient of a
block's convolution bias is zero but for rounding (a site's centred rows sum to zero), and Adam divides a gradient by its
own running magnitude: it turns that rounding into steps of the full learning rate in directions no two runs share,
which eval mode then sees (the bias no longer cancels against the running mean).  Gradient descent leaves it where it is.
The graphs of the model fixture leave out tori of width 1, on which all permutations of a site coincide.

* ``lcnn_model.npz``   LCNNModel(n_features 8, sitewise_n_feature 10) on 20 graphs at batch_size 8: the state-dict key
  list and shapes, the state, the first batch's outputs, loss, masks and every gradient, ``predict`` before and after a
  deterministic 2-epoch fit, the masks of its six steps, the per-step losses, the float64 restatement's losses of the same
  steps with the same masks (``fit_losses64``), ``e_ref[k] = |loss32 - loss64| / |loss64|`` of the restatement, and how far
  the float32 restatement ends from the float64 one (``e_ref_after``: ``predict``, then the running statistics).
"""
import copy
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from oracle.gen_golden import import_reference  # noqa: E402
from gen_golden_cgcnn import install_dgl  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
O, F_IN, K, P, S = 8, 3, 19, 6, 10
FIT_LR = 0.01  # plain gradient descent: see the docstring


def install_dgl_for_lcnn():
    dgl = install_dgl()

    def local_var(self):
        g = copy.copy(self)
        g.ndata, g.edata = type(self.ndata)(self.ndata), type(self.edata)(self.edata)
        return g

    dgl.DGLGraph.local_var = local_var
    fn = types.ModuleType("dgl.function")
    fn.copy_u = lambda u, out: (lambda edges: {out: edges.src[u]})
    dgl.function = fn
    sys.modules["dgl.function"] = fn
    return dgl


class Recorder:
    """Wraps the forward of nn.Dropout modules; ``taken[name]`` holds the masks of the training-mode calls, read off the
    outputs."""

    def __init__(self):
        self.taken = {}

    def wrap(self, name, module):
        plain = module.forward

        def forward(x):
            y = plain(x)
            if module.training:  # the mask itself: kept entries scaled by 1 / (1 - p) (a zero input stays zero under any mask)
                self.taken.setdefault(name, []).append((y.detach() != 0).to(y.dtype) / (1.0 - module.p))
            return y
        module.forward = forward

    def pop(self):
        import torch
        got = {k: (torch.stack(v) if v[0].dim() == 1 else v[0]).numpy().copy() for k, v in self.taken.items()}
        assert all(len(v) == 1 or v[0].dim() == 1 for v in self.taken.values())
        self.taken = {}
        return got


def main():
    import torch
    dgl = install_dgl_for_lcnn()
    dc = import_reference()
    from deepchem.models.torch_models.lcnn import LCNNBlock, LCNNModel
    from tests import lcnn_refs as R

    def to_dgl(graphs):
        return dgl.batch([dgl.graph((torch.as_tensor(g.edge_index[0]), torch.as_tensor(g.edge_index[1])), num_nodes=g.num_nodes)
                          for g in graphs])

    normal = lambda rng, n, f: rng.normal(0, 1, (n, f))  # noqa: E731
    # ---- layers
    out = {}
    rng = np.random.RandomState(7)
    single = [R.torus(rng, 3, 3, F_IN, P, K, normal)]
    four = [R.torus(rng, a, b, F_IN, P, K, normal) for a, b in ((3, 3), (1, 1), (3, 4), (2, 2))]
    case = 0
    for training in (True, False):
        for graphs in (single, four):
            x, nbr, ptr = R.pack(graphs, P, K)
            torch.manual_seed(40 + case)
            layer = LCNNBlock(K * F_IN, O, P)
            rec = Recorder()
            rec.wrap("mask", layer.dropout.dropout)
            pre = "c%d_" % case
            bn = layer.batch_norm
            with torch.no_grad():  # statistics and an affine map that are not the initial ones
                bn.running_mean.copy_(torch.as_tensor(rng.normal(0, 0.3, O), dtype=torch.float32))
                bn.running_var.copy_(torch.as_tensor(rng.uniform(0.5, 2, O), dtype=torch.float32))
                bn.weight.copy_(torch.as_tensor(rng.uniform(0.5, 1.5, O), dtype=torch.float32))
                bn.bias.copy_(torch.as_tensor(rng.normal(0, 0.3, O), dtype=torch.float32))
            out[pre + "rm0"], out[pre + "rv0"] = bn.running_mean.numpy().copy(), bn.running_var.numpy().copy()
            layer.train(training)
            for k, v in layer.named_parameters():
                out[pre + "p_" + k] = v.detach().numpy().copy()
            tx = torch.tensor(x, dtype=torch.float32, requires_grad=True)
            o = layer(to_dgl(graphs), tx)
            cot = torch.as_tensor(rng.normal(0, 1, o.shape).astype(np.float32))
            (o * cot).sum().backward()
            out.update({pre + "training": np.asarray(training), pre + "x": x, pre + "nbr": nbr, pre + "ptr": ptr,
                        pre + "ei": np.concatenate([g.edge_index + at for g, at in zip(graphs, ptr)], axis=1),
                        pre + "out": o.detach().numpy(), pre + "cot": cot.numpy(), pre + "grad_x": tx.grad.numpy().copy(),
                        pre + "mask": rec.pop()["mask"] if training else np.ones((x.shape[0], P), np.float32)})
            for k, v in layer.named_parameters():
                if v.grad is not None:
                    out[pre + "gradp_" + k] = v.grad.numpy().copy()
            out[pre + "rm1"], out[pre + "rv1"] = bn.running_mean.numpy().copy(), bn.running_var.numpy().copy()
            out[pre + "tracked"] = np.asarray(int(bn.num_batches_tracked))
            case += 1
    out["n_cases"] = np.asarray(case)
    np.savez_compressed(os.path.join(OUT, "lcnn_layers.npz"), **out)

    # ---- model
    graphs = R.fixture_graphs(F_IN, K)
    X = np.empty(len(graphs), dtype=object)
    X[:] = [dc.feat.GraphData(g.node_features, g.edge_index) for g in graphs]
    rng = np.random.RandomState(11)
    out = {"n_nodes": np.asarray([g.num_nodes for g in graphs])}
    yv = rng.normal(0, 1, (len(graphs), 1))
    w = np.ones((len(graphs), 1))
    out["y"], out["w"] = yv, w
    ds = dc.data.NumpyDataset(X, yv, w, ids=None)
    torch.manual_seed(11)
    model = LCNNModel(n_occupancy=F_IN, n_neighbor_sites_list=K, n_permutation_list=P, n_features=O, sitewise_n_feature=S,
                      batch_size=8, optimizer=dc.models.optimizers.GradientDescent(learning_rate=FIT_LR), log_frequency=1,
                      device=torch.device("cpu"))
    rec = Recorder()
    names = ["b%d" % i for i in range(len(model.model.LCNN_blocks))] + ["atom"]
    for name, m in zip(names, [b.dropout.dropout for b in model.model.LCNN_blocks] + [model.model.Atom_wise_Conv.dropout]):
        rec.wrap(name, m)
    steps_masks = []
    plain_forward = model.model.forward

    def forward(G):
        o = plain_forward(G)
        if model.model.training:
            steps_masks.append(rec.pop())
        return o
    model.model.forward = forward

    state0 = {k: v.detach().clone().numpy() for k, v in model.model.state_dict().items()}
    out["keys"] = np.asarray(list(state0))
    out["shapes"] = np.asarray([(list(v.shape) + [0, 0])[:2] for v in state0.values()])
    for k, v in state0.items():
        out["param0_" + k] = v
    out["predict0"] = np.asarray(model.predict(ds))
    batches = list(model.default_generator(ds, epochs=1, deterministic=True, pad_batches=True))
    inputs, labels, weights = model._prepare_batch(batches[0])
    model.model.train()
    model.model.zero_grad()
    o = model.model(inputs)
    loss = model._loss_fn([o], labels, weights)
    loss.backward()
    out["out0"], out["loss0"] = o.detach().numpy(), np.float64(loss.item())
    for k, p in model.model.named_parameters():
        if p.grad is not None:
            out["grad_" + k] = p.grad.detach().numpy().copy()
    for k, v in steps_masks.pop().items():
        out["masks0_" + k] = v
    model.model.zero_grad()
    # (that forward moved the running statistics: the trajectory below starts from the initial state again)
    model.model.load_state_dict({k: torch.as_tensor(v) for k, v in state0.items()})
    losses = []
    model.fit(ds, nb_epoch=2, deterministic=True, checkpoint_interval=0, all_losses=losses)
    out["fit_losses"] = np.asarray(losses, np.float64)
    out["predict"] = np.asarray(model.predict(ds))
    for k, v in model.model.state_dict().items():
        if "running_" in k or "tracked" in k:
            out["after_" + k] = v.detach().numpy().copy()
    assert len(steps_masks) == len(losses) == 6
    for s, masks in enumerate(steps_masks):
        for k, v in masks.items():
            out["fit%d_%s" % (s, k)] = v

    # the restatement in both precisions over the same six steps with the same masks
    rows = [(R.pack(list(X_b), P, K), y_b, w_b)
            for X_b, y_b, w_b, _ in ds.iterbatches(batch_size=8, deterministic=True, pad_batches=True)] * 2
    steps = [(packed + (([m["b0"], m["b1"]], m["atom"]),), y_b, w_b) for (packed, y_b, w_b), m in zip(rows, steps_masks)]
    traj, after = {}, {}
    for dtype in (torch.float32, torch.float64):
        ref = R.LCNNRef(state0, dtype)
        traj[dtype] = np.asarray(R.fit(ref, steps, FIT_LR))
        with torch.no_grad():
            after[dtype] = [ref.eval()(R.pack(graphs, P, K) + (None,)).numpy().astype(np.float64)] + \
                [t.numpy().astype(np.float64) for bn in ref.bn for t in (bn.mean, bn.var)]
    # how far the float32 restatement ends from the float64 one after the six steps: the prediction, then the running
    # statistics (mean, var per block), each relative to the tensor's largest entry
    out["predict64"] = after[torch.float64][0]
    out["e_ref_after"] = np.asarray([R.rel_err(a, b) for a, b in zip(after[torch.float32], after[torch.float64])])
    print("e_ref_after (predict, then running mean / var per block)", out["e_ref_after"])
    out["fit_losses64"] = traj[torch.float64]
    out["e_ref"] = np.abs(traj[torch.float32] - traj[torch.float64]) / np.abs(traj[torch.float64])
    print("fit losses", out["fit_losses"], "restated32", traj[torch.float32], "e_ref", out["e_ref"])
    np.savez_compressed(os.path.join(OUT, "lcnn_model.npz"), **out)
    for name in ("lcnn_layers", "lcnn_model"):
        print(name, os.path.getsize(os.path.join(OUT, name + ".npz")), "bytes")


if __name__ == "__main__":
    main()
