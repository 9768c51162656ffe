"""CGCNN without a GPU: the split algebra of csrc/cgcnn.hip against the reference's order in float64, the restatements
of tests/cgcnn_refs.py against the fixtures recorded from the reference, the state-dict keys and a checkpoint round
trip, the classification shapes, the error for fewer than two edges, and the torch route of the layer and of
``CGCNNModel`` on the CPU."""
import os

import numpy as np
import pytest
import torch

import deepchem_amd as dc
from deepchem_amd.feat import GraphData
from deepchem_amd.models import CGCNN, CGCNNModel
from deepchem_amd.models.torch_models import CgcnnBatch, CGCNNLayer
from tests import cgcnn_refs as R

TOL = 1e-4
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LAYERS = np.load(os.path.join(GOLDEN, "cgcnn_layers.npz"))
MODEL = np.load(os.path.join(GOLDEN, "cgcnn_model.npz"))
H, FN, FE = 8, 5, 3
SIZES = dict(in_node_dim=FN, hidden_node_dim=H, in_edge_dim=FE, num_conv=3, predictor_hidden_feats=16)
CPU = torch.device("cpu")
MODES = {"regression": ("", dict(n_tasks=2)), "classification": ("cls_", dict(n_classes=5))}
# What eval mode sees after a fit is ill-conditioned in the reference itself: the gradient of every conv layer's
# ``linear.bias`` is zero in exact arithmetic (the batch statistics remove the bias), what arrives is rounding noise,
# and Adam normalises noise to steps of the full learning rate.  After k steps a bias has moved by up to k * lr in a
# direction the last bits decide; training losses and the running variances do not see it, the running means (and so
# ``predict``) do.  Six steps at lr = 0.001, two runs that may drift apart: 1.2e-2 of a column's spread, which is of
# order one.  The running means are therefore not compared after a fit, and ``predict`` at this bound.
AFTER_FIT_TOL = 2 * 6 * 0.001
PARAMS = ("linear.weight", "linear.bias", "batch_norm.weight", "batch_norm.bias")


def close(got, want, name, tol=TOL):
    err = R.rel_err(got, want)
    assert err <= tol, (name, err)


def close_param_grads(got, want, tol=TOL, bias_cancels=True):
    """``got`` / ``want``: gradients by parameter name.  ``bias_cancels``: a BatchNorm on batch statistics follows every
    ``linear`` of a conv layer, which removes the bias -- its gradient is zero and what the reference recorded is
    rounding at the scale of the terms that cancel, so it is compared at the scale of the weight's gradient."""
    for name, w in want.items():
        if bias_cancels and name.endswith("linear.bias") and name[:-4] + "weight" in want:
            scale = float(np.max(np.abs(want[name[:-4] + "weight"])))
            err = float(np.max(np.abs(np.asarray(got[name], np.float64) - np.asarray(w, np.float64)))) / scale
            assert err <= tol, (name, err)
        else:
            close(got[name], w, name, tol)


def layer_case(k):
    pre = "c%d_" % k
    c = {n: LAYERS[pre + n] for n in ("h", "ei", "e", "out", "cot", "grad_h", "grad_e")}
    c["with_bn"], c["training"] = bool(LAYERS[pre + "with_bn"]), bool(LAYERS[pre + "training"])
    c["params"] = {n[len(pre) + 2:]: LAYERS[n] for n in LAYERS.files if n.startswith(pre + "p_")}
    c["gradp"] = {n[len(pre) + 6:]: LAYERS[n] for n in LAYERS.files if n.startswith(pre + "gradp_")}
    if c["with_bn"]:
        c.update({n: LAYERS[pre + n] for n in ("rm0", "rv0", "rm1", "rv1")}, tracked=int(LAYERS[pre + "tracked"]))
    return c


def run_layer(form, c, dtype):
    """outputs, gradients (inputs, parameters) and the BatchNorm state of a restated layer on a layer case."""
    p = {k: torch.tensor(v, dtype=dtype, requires_grad=True) for k, v in c["params"].items()}
    h, e = (torch.tensor(c[n], dtype=dtype, requires_grad=True) for n in "he")
    state = R.BNState(p["linear.bias"].numel(), dtype, c.get("rm0"), c.get("rv0"))
    out = form(p["linear.weight"], p["linear.bias"], p.get("batch_norm.weight"), p.get("batch_norm.bias"), h,
               torch.as_tensor(c["ei"]), e, state, c["training"])
    (out * torch.tensor(c["cot"], dtype=dtype)).sum().backward()
    res = {"out": out.detach().numpy(), "grad_h": h.grad.numpy(), "grad_e": e.grad.numpy(), "rm": state.mean.numpy(),
           "rv": state.var.numpy(), "tracked": state.tracked}
    res.update({"gradp_" + k: v.grad.numpy() for k, v in p.items()})
    return res


def case_batch(name, with_bn, training, hidden=H, fe=FE, seed=3):
    """A named graph batch (``cgcnn_refs.case_graphs``) as a layer case with random parameters and statistics."""
    x, ei, e, _ = R.pack(R.case_graphs(name, hidden, fe))
    torch.manual_seed(seed)
    layer = CGCNNLayer(hidden, fe, batch_norm=with_bn)
    rng = np.random.RandomState(seed)
    c = dict(h=x, ei=ei, e=e, with_bn=with_bn, training=training, cot=rng.normal(0, 1, x.shape),
             params={k: v.detach().numpy() for k, v in layer.named_parameters()})
    if with_bn:
        c["params"]["batch_norm.weight"] = rng.uniform(0.5, 1.5, 2 * hidden)
        c["params"]["batch_norm.bias"] = rng.normal(0, 0.3, 2 * hidden)
        c.update(rm0=rng.normal(0, 0.3, 2 * hidden), rv0=rng.uniform(0.5, 2, 2 * hidden))
    return c


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("with_bn", [True, False])
def test_split_form_equals_concatenated_form_in_float64(with_bn, training):
    cases = [layer_case(k) for k in range(int(LAYERS["n_cases"]))]
    cases = [c for c in cases if c["with_bn"] == with_bn and c["training"] == training]
    cases += [case_batch(name, with_bn, training) for name in ("edge", "g1", "below", "above")]
    assert len(cases) == 6
    for c in cases:
        a, b = run_layer(R.layer_direct, c, torch.float64), run_layer(R.layer_split, c, torch.float64)
        assert set(a) == set(b) and a["tracked"] == b["tracked"] == (1 if with_bn and training else 0)
        for name in a:
            if name == "gradp_linear.bias" and with_bn and training:
                # batch statistics remove the bias: its gradient is zero, and what is left is rounding at the scale of
                # the terms that cancel
                scale = float(np.max(np.abs(a["gradp_linear.weight"])))
                assert max(np.max(np.abs(a[name])), np.max(np.abs(b[name]))) <= 1e-12 * scale, name
                continue
            err = R.rel_err(b[name], a[name])
            assert err <= 1e-12, (name, err)


def test_edge_case_batch_holds_what_it_promises():
    graphs = R.case_graphs("edge")
    x, ei, _, batch = R.pack(graphs)
    N, E, G = batch.size, ei.shape[1], len(graphs)
    arriving, leaving = np.bincount(ei[1], minlength=N), np.bincount(ei[0], minlength=N)
    firsts = np.concatenate([[0], np.cumsum([g.num_nodes for g in graphs])[:-1]])
    assert [g.num_edges for g in (graphs[0], graphs[-1])] == [0, 0] and graphs[0].num_nodes == graphs[-1].num_nodes == 1
    assert any(g.num_nodes == 1 and g.num_edges == 0 for g in graphs[1:-1])
    assert sorted(set(arriving[firsts]) & set(R.STAR_ARMS)) == sorted(R.STAR_ARMS)
    assert sorted(set(leaving[firsts]) & set(R.STAR_ARMS)) == sorted(R.STAR_ARMS)
    assert arriving[firsts[1] + 3] == 0 and np.sum((ei[0] == ei[1])) >= 1  # the bare node, the self-loop
    assert np.sum((ei[0] == firsts[1] + 1) & (ei[1] == firsts[1])) == 3  # the triple edge
    assert any(g.num_nodes == 300 for g in graphs) and G > 1
    for name, (n, e) in (("below", (127, 191)), ("above", (129, 193))):
        (g,) = R.case_graphs(name)
        assert (g.num_nodes, g.num_edges) == (n, e)
    assert len(R.case_graphs("g1")) == 1 and E > 2


@pytest.mark.parametrize("k", range(int(LAYERS["n_cases"])))
def test_restatement_reproduces_the_layer_fixtures(k):
    c = layer_case(k)
    got = run_layer(R.layer_direct, c, torch.float64)
    for n in ("out", "grad_h", "grad_e"):
        close(got[n], c[n], n, 1e-5)
    close_param_grads({k[6:]: v for k, v in got.items() if k.startswith("gradp_")}, c["gradp"], 1e-5,
                      c["with_bn"] and c["training"])
    if c["with_bn"]:
        close(got["rm"], c["rm1"], "running_mean", 1e-5)
        close(got["rv"], c["rv1"], "running_var", 1e-5)
        assert got["tracked"] == c["tracked"] == (1 if c["training"] else 0)


def load_layer(c, device):
    layer = CGCNNLayer(H, FE, batch_norm=c["with_bn"]).to(device)
    layer.load_state_dict({n: torch.as_tensor(v) for n, v in c["params"].items()}, strict=False)
    if c["with_bn"]:
        layer.batch_norm.running_mean.copy_(torch.as_tensor(c["rm0"]))
        layer.batch_norm.running_var.copy_(torch.as_tensor(c["rv0"]))
    return layer.train(c["training"])


def check_layer(layer, c, device, route, graph=None):
    h, e = (torch.tensor(c[n], dtype=torch.float32, device=device, requires_grad=True) for n in "he")
    out = layer(torch.as_tensor(c["ei"], device=device) if graph is None else graph, h, e)
    assert layer.last_route == route
    (out * torch.as_tensor(c["cot"], device=device)).sum().backward()
    close(out.detach().cpu().numpy(), c["out"], "out")
    close(h.grad.cpu().numpy(), c["grad_h"], "grad_h")
    close(e.grad.cpu().numpy(), c["grad_e"], "grad_e")
    close_param_grads({k: p.grad.cpu().numpy() for k, p in layer.named_parameters()}, c["gradp"], TOL,
                      c["with_bn"] and c["training"])
    if c["with_bn"]:
        close(layer.batch_norm.running_mean.cpu().numpy(), c["rm1"], "running_mean")
        close(layer.batch_norm.running_var.cpu().numpy(), c["rv1"], "running_var")
        assert int(layer.batch_norm.num_batches_tracked) == c["tracked"]
    return out


@pytest.mark.parametrize("k", range(int(LAYERS["n_cases"])))
def test_torch_route_layer_on_the_cpu(k):
    c = layer_case(k)
    check_layer(load_layer(c, CPU), c, CPU, "torch")


def test_state_dict_keys_are_the_reference_ones_and_a_checkpoint_round_trips(tmp_path):
    for mode, (pre, kw) in MODES.items():
        model = CGCNN(mode=mode, **SIZES, **kw)
        state = model.state_dict()
        assert list(state) == [str(k) for k in MODEL[pre + "keys"]]
        for (k, v), shape in zip(state.items(), MODEL[pre + "shapes"]):
            assert list(v.shape) == [int(s) for s in shape[:v.dim()]], k
        model.load_state_dict({str(k): torch.as_tensor(MODEL[pre + "param0_" + str(k)]) for k in MODEL[pre + "keys"]})
    want = ["embedding.weight", "embedding.bias"]
    for i in range(3):
        want += ["conv_layers.%d.linear.%s" % (i, n) for n in ("weight", "bias")]
        want += ["conv_layers.%d.batch_norm.%s" % (i, n)
                 for n in ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")]
    assert list(CGCNN(**SIZES).state_dict()) == want + ["fc.weight", "fc.bias", "out.weight", "out.bias"]
    assert list(CGCNNLayer(H, FE, batch_norm=False).state_dict()) == ["linear.weight", "linear.bias"]
    # defaults of the reference
    d = CGCNN()
    assert d.embedding.weight.shape == (64, 92) and d.conv_layers[0].linear.weight.shape == (128, 169) and \
        len(d.conv_layers) == 3 and d.fc.weight.shape == (128, 64) and d.out.weight.shape == (1, 128)
    ds = fixture_dataset("")
    m = fixture_model("regression", CPU, model_dir=str(tmp_path))
    m.fit(ds, nb_epoch=1, deterministic=True, checkpoint_interval=0)
    before = m.predict(ds)
    m.save_checkpoint()
    m2 = CGCNNModel(mode="regression", n_tasks=2, batch_size=8, model_dir=str(tmp_path), device=CPU, **SIZES)
    m2.restore()
    assert np.array_equal(m2.predict(ds), before)
    assert int(m2.model.conv_layers[0].batch_norm.num_batches_tracked) == 3


def graph_data(g):
    return GraphData(g.node_features, g.edge_index, g.edge_features)


def test_classification_shapes_and_class_axis_softmax():
    graphs = [graph_data(g) for g in R.fixture_graphs(FN, FE)]
    for n_tasks, n_graphs, shape in ((1, 1, (1, 4)), (3, 1, (1, 3, 4)), (3, 5, (5, 3, 4)), (1, 5, (5, 4))):
        model = CGCNN(mode="classification", n_tasks=n_tasks, n_classes=4, **SIZES).eval()
        proba, logits = model(CgcnnBatch(graphs[:n_graphs], CPU))
        assert tuple(proba.shape) == tuple(logits.shape) == shape
        assert torch.allclose(proba.sum(-1), torch.ones(shape[:-1]), atol=1e-6)
        assert torch.allclose(proba, torch.softmax(logits, -1))
    out = CGCNN(n_tasks=3, **SIZES).eval()(CgcnnBatch(graphs[:1], CPU))
    assert tuple(out.shape) == (1, 3)


def test_fewer_than_two_edges_raise_in_training_and_run_in_eval():
    rng = np.random.RandomState(0)
    for n_edges in (0, 1):
        g = GraphData(rng.normal(size=(3, FN)), np.asarray([[0], [1]])[:, :n_edges], rng.normal(size=(n_edges, FE)))
        model = CGCNN(**SIZES)
        with pytest.raises(ValueError, match="more than 1 value per channel"):
            model.train()(CgcnnBatch([g, g][:max(n_edges, 1)], CPU))
        assert int(model.conv_layers[0].batch_norm.num_batches_tracked) == 0
        out = model.eval()(CgcnnBatch([g], CPU))
        assert tuple(out.shape) == (1, 1) and bool(torch.isfinite(out).all())
        layer = CGCNNLayer(H, FE)
        with pytest.raises(ValueError, match="more than 1 value per channel"):
            layer(np.asarray([[0], [1]])[:, :n_edges], torch.zeros(3, H), torch.zeros(n_edges, FE))
        # without a BatchNorm nothing needs two rows
        assert CGCNNLayer(H, FE, batch_norm=False)(np.zeros((2, 0), np.int64), torch.zeros(3, H), torch.zeros(0, FE)).abs().sum() == 0


def test_constructor_and_batch_errors():
    with pytest.raises(ValueError, match="mode must be"):
        CGCNN(mode="ranking")
    with pytest.raises(ValueError, match="route"):
        CGCNNModel(route="fast", device=CPU)
    rng = np.random.RandomState(0)
    ei = np.asarray([[0, 1], [1, 0]])
    good = GraphData(rng.normal(size=(2, FN)), ei, rng.normal(size=(2, FE)))
    assert CgcnnBatch([good], CPU)["edge_index"].shape == (2, 2)
    with pytest.raises(ValueError, match="no edge_features"):
        CgcnnBatch([good, GraphData(rng.normal(size=(2, FN)), ei)], CPU)
    with pytest.raises(ValueError, match="one width"):
        CgcnnBatch([good, GraphData(rng.normal(size=(2, FN + 1)), ei, rng.normal(size=(2, FE)))], CPU)
    with pytest.raises(ValueError, match="no graphs"):
        CgcnnBatch([], CPU)
    with pytest.raises(ValueError, match="the model was built for"):
        CGCNN(in_node_dim=FN + 1, in_edge_dim=FE).eval()(CgcnnBatch([good], CPU))
    with pytest.raises(ValueError, match="CgcnnBatch"):
        CGCNN(**SIZES)(good)


# ------------------------------------------------------------------------------------------------ the models
def fixture_dataset(pre):
    graphs = R.fixture_graphs(FN, FE)
    X = np.empty(len(graphs), dtype=object)
    X[:] = [graph_data(g) for g in graphs]
    return dc.data.NumpyDataset(X, MODEL[pre + "y"], MODEL[pre + "w"])


def initial_state(pre):
    return {str(k): torch.as_tensor(MODEL[pre + "param0_" + str(k)]) for k in MODEL[pre + "keys"]}


def fixture_model(mode, device, **extra):
    pre, kw = MODES[mode]
    model = CGCNNModel(mode=mode, batch_size=8, learning_rate=0.001, log_frequency=1, device=device, **SIZES, **kw, **extra)
    model.model.load_state_dict(initial_state(pre))
    return model


def check_first_batch(model, mode, ds, tol=TOL):
    pre = MODES[mode][0]
    batch = next(iter(model.default_generator(ds, epochs=1, deterministic=True, pad_batches=True)))
    inputs, labels, weights = model._prepare_batch(batch)
    model.model.train()
    model.model.zero_grad()
    o = model.model(inputs)
    loss = model._loss_fn([o[1]] if mode == "classification" else [o], labels, weights)
    loss.backward()
    close((o if mode == "regression" else o[0]).detach().cpu().numpy(), MODEL[pre + "out0"], "out0", tol)
    assert abs(float(loss.detach()) - float(MODEL[pre + "loss0"])) <= tol * abs(float(MODEL[pre + "loss0"]))
    names = [k for k, _ in model.model.named_parameters()]
    close_param_grads({k: p.grad.cpu().numpy() for k, p in model.model.named_parameters()},
                      {k: MODEL[pre + "grad_" + k] for k in names}, tol)
    model.model.zero_grad()
    model.model.load_state_dict(initial_state(pre))  # (the forward moved the running statistics)


def check_fit(model, mode, ds, tol=TOL, bar64=False):
    """The 2-epoch fit against the reference's six losses at the project's relative bar ``tol``.  ``bar64``: also the
    accuracy bar against the float64 restatement's losses of the same steps -- the distance to them is at most 4 times
    the float32 restatement's own (the largest ``e_ref`` of the trajectory: one step's is a single rounding sample), with
    a floor of one float32 ulp of the loss.  Returns the largest (distance to the reference, distance to float64)."""
    pre = MODES[mode][0]
    close(np.asarray(model.predict(ds)), MODEL[pre + "predict0"], "predict0", tol)
    losses = []
    model.fit(ds, nb_epoch=2, deterministic=True, checkpoint_interval=0, all_losses=losses)
    want, want64 = MODEL[pre + "fit_losses"], MODEL[pre + "fit_losses64"]
    e_ref = float(np.max(MODEL[pre + "e_ref"]))
    worst, worst64 = 0.0, 0.0
    for k, (a, b, b64) in enumerate(zip(losses, want, want64)):
        d, d64 = abs(a - b) / abs(b), abs(a - b64) / abs(b64)
        bound64 = max(4 * e_ref, float(np.spacing(np.float32(b64))) / abs(b64))
        worst, worst64 = max(worst, d), max(worst64, d64)
        print("step %d loss %.9f reference %.9f rel %.3g | float64 %.12f rel %.3g, restatement32 %.3g, bound %.3g" %
              (k, a, b, d, b64, d64, float(MODEL[pre + "e_ref"][k]), bound64))
        assert d <= tol, (k, a, b)
        assert not bar64 or d64 <= bound64, (k, a, b64, d64, bound64)
    assert len(losses) == len(want) == 6
    close(np.asarray(model.predict(ds)), MODEL[pre + "predict"], "predict", AFTER_FIT_TOL)
    for k, v in model.model.state_dict().items():
        if "running_var" in k:  # (a shift of the bias does not reach the variance)
            close(v.cpu().numpy(), MODEL[pre + "after_" + k], k, tol)
        elif "tracked" in k:
            assert int(v) == int(MODEL[pre + "after_" + k]) == 6
    return worst, worst64


@pytest.mark.parametrize("mode", list(MODES))
def test_torch_route_model_on_the_cpu(mode):
    ds = fixture_dataset(MODES[mode][0])
    model = fixture_model(mode, CPU)
    check_first_batch(model, mode, ds)
    assert model.last_route == "torch" and all(c.last_route == "torch" for c in model.model.conv_layers)
    check_fit(model, mode, ds)
    assert model.model.mode == mode and model.last_route == "torch"
