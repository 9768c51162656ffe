"""LCNN without a GPU: the restatements of tests/lcnn_refs.py against the reference's fixtures, the split form against the
concatenated one, the closed form of the running statistics against the recurrence, and the torch route of the layers and
the model (CPU tensors) against the fixtures, the fit trajectory with the recorded masks injected included.

Tolerances: 1e-4 of each tensor's largest entry against the reference's float32 fixtures (the gradient of the
convolution bias in training mode is exactly zero in exact arithmetic, so it is held to 1e-4 of the weight gradient's
largest entry instead: both are sums of the same rows -- the one exception); 1e-12 between the float64 forms.  The fit
(plain gradient descent on tori without a width of 1: tools/gen_golden_lcnn.py says why) holds 1e-4 on every loss, on
``predict`` after it and on the running statistics.
"""
import copy
import os

import numpy as np
import pytest
import torch

from deepchem_amd import ops
from deepchem_amd.data import NumpyDataset
from deepchem_amd.feat.graph_data import GraphData
from deepchem_amd.models import LCNNModel
from deepchem_amd.models.optimizers import GradientDescent
from deepchem_amd.models.torch_models import LCNN, LCNNBlock, LcnnBatch
from tests import lcnn_refs as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LAYERS = np.load(os.path.join(GOLDEN, "lcnn_layers.npz"))
MODEL = np.load(os.path.join(GOLDEN, "lcnn_model.npz"))
TOL, P, K, F_IN, O, S = 1e-4, 6, 19, 3, 8, 10
CPU = torch.device("cpu")
PARAMS = ("conv_weights.weight", "conv_weights.bias", "batch_norm.weight", "batch_norm.bias")


def close(got, want, name, tol=TOL):
    err = R.rel_err(got, want)
    print("%s: %.3g" % (name, err))
    assert err <= tol, (name, err)


def layer_case(c):
    pre = "c%d_" % c
    return {k[len(pre):]: LAYERS[k] for k in LAYERS.files if k.startswith(pre)}


def restated(c, dtype, order):
    """(out, grads by name, BNState) of a restatement on a layer case; order 'loop': the literal per-site loop."""
    x = torch.tensor(c["x"], dtype=dtype, requires_grad=True)
    p = [torch.tensor(c["p_" + k], dtype=dtype, requires_grad=True) for k in PARAMS]
    state = R.BNState(0, dtype, c["rm0"], c["rv0"])
    args = (x, c["nbr"], *p, c["mask"], state, bool(c["training"]))
    out = R.block_loop(*args) if order == "loop" else R.block(*args, order)
    grads = torch.autograd.grad((out * torch.tensor(c["cot"], dtype=dtype)).sum(), [x] + p, allow_unused=True)
    names = ["x"] + list(PARAMS)
    return out.detach(), {n: (torch.zeros_like(t) if g is None else g) for n, g, t in zip(names, grads, [x] + p)}, state


def check_against_fixture(c, out, grads, rm, rv, tracked, name):
    close(out, c["out"], name + " out")
    close(grads["x"], c["grad_x"], name + " grad_x")
    for k in PARAMS:
        if k == "conv_weights.bias" and bool(c["training"]):
            # exactly zero in exact arithmetic (the centred rows of a site sum to zero): the reference's entries are
            # rounding alone, so the scale is that of the other sums of the same dX rows, the weight gradient's
            scale = float(np.max(np.abs(c["gradp_conv_weights.weight"])))
            err = float(np.max(np.abs(np.asarray(grads[k].detach().cpu(), np.float64) - c["gradp_" + k]))) / scale
            print("%s grad %s: %.3g of the weight gradient's largest entry" % (name, k, err))
            assert err <= TOL, (name, k, err)
            continue
        close(grads[k], c["gradp_" + k], name + " grad " + k)
    close(rm, c["rm1"], name + " running_mean")
    close(rv, c["rv1"], name + " running_var")
    assert int(tracked) == int(c["tracked"])


@pytest.mark.parametrize("case", range(int(LAYERS["n_cases"])))
@pytest.mark.parametrize("order", ["concat", "split", "split_rev", "loop"])
def test_restatements_match_the_reference(case, order):
    c = layer_case(case)
    out, grads, st = restated(c, torch.float64, order)
    check_against_fixture(c, out, grads, st.mean, st.var, st.tracked, "case %d %s" % (case, order))


@pytest.mark.parametrize("case", range(int(LAYERS["n_cases"])))
def test_split_and_concatenated_forms_agree_in_float64(case):
    c = layer_case(case)
    want = restated(c, torch.float64, "concat")
    for order in ("split", "split_rev"):
        got = restated(c, torch.float64, order)
        close(got[0], want[0], "out", 1e-12)
        for k in want[1]:
            if k == "conv_weights.bias" and bool(c["training"]):  # zero but for rounding: at the weight gradient's scale
                scale = float(want[1]["conv_weights.weight"].abs().max())
                assert float((got[1][k] - want[1][k]).abs().max()) <= 1e-12 * scale
            elif float(want[1][k].abs().max()) > 0:
                close(got[1][k], want[1][k], "grad " + k, 1e-12)
        close(got[2].mean, want[2].mean, "running_mean", 1e-12)
        close(got[2].var, want[2].var, "running_var", 1e-12)


def make_block(c=None, o=O, p=P, width=K * F_IN, training=True, seed=0):
    torch.manual_seed(seed)
    layer = LCNNBlock(width, o, p)
    if c is not None:
        with torch.no_grad():
            for k in PARAMS:
                dict(layer.named_parameters())[k].copy_(torch.as_tensor(c["p_" + k]))
            layer.batch_norm.running_mean.copy_(torch.as_tensor(c["rm0"]))
            layer.batch_norm.running_var.copy_(torch.as_tensor(c["rv0"]))
    return layer.train(training)


def sites_of(c, device=CPU):
    ptr = c["ptr"]
    graphs = [R.Graph(c["x"][a:b], R.edges_of(c["nbr"][a:b] - a)) for a, b in zip(ptr[:-1], ptr[1:])]
    return LcnnBatch(graphs, device, P, K)


@pytest.mark.parametrize("N", [1, 2, 7, 1025, 3000])
def test_closed_form_running_statistics_match_the_recurrence(N):
    """The torch route's closed form on N sites against the sequential recurrence in float64, within the project's
    accuracy bar: at most 4 times the error of the float32 recurrence, with a floor of one float32 ulp."""
    rng = np.random.RandomState(N)
    p, k, f, o = 3, 2, 2, 4
    g = R.random_sites(rng, N, p, k, f)
    b = LcnnBatch([g], CPU, p, k)
    layer = make_block(None, o, p, k * f, seed=N)
    r0m, r0v = rng.normal(0, 1, o).astype(np.float32), rng.uniform(0.5, 2, o).astype(np.float32)
    with torch.no_grad():
        layer.batch_norm.running_mean.copy_(torch.as_tensor(r0m))
        layer.batch_norm.running_var.copy_(torch.as_tensor(r0v))
        layer(b.sites, b.x, torch.ones(N, p))
        X = layer.conv_weights(b.x[b.sites.nbr.long()].view(N, p, -1))
    stats = {"mean": (X.mean(1), r0m, layer.batch_norm.running_mean), "var": (X.var(1, unbiased=True), r0v, layer.batch_norm.running_var)}
    for name, (s, r0, got) in stats.items():
        want = R.running_loop(s.double(), r0).numpy()
        e32 = np.max(np.abs(R.running_loop(s, r0).numpy() - want))
        e = np.max(np.abs(got.numpy() - want))
        floor = float(np.spacing(np.float32(np.max(np.abs(want)))))
        print("N %d %s: error %.3g, float32 recurrence %.3g, floor %.3g" % (N, name, e, e32, floor))
        assert e <= max(4 * e32, floor)
        close(R.running_closed(s, r0), want, "refs closed form", 1e-6)
    assert int(layer.batch_norm.num_batches_tracked) == N


@pytest.mark.parametrize("case", range(int(LAYERS["n_cases"])))
def test_torch_route_layer_on_the_cpu(case):
    c = layer_case(case)
    layer = make_block(c, training=bool(c["training"]))
    b = sites_of(c)
    x = torch.tensor(c["x"], dtype=torch.float32, requires_grad=True)
    out = layer(b.sites, x, torch.as_tensor(c["mask"]))
    assert layer.last_route == "torch" and layer.last_reason == "not on the GPU"
    (out * torch.as_tensor(c["cot"])).sum().backward()
    grads = {"x": x.grad}
    grads.update({k: v.grad for k, v in layer.named_parameters() if k in PARAMS})
    bn = layer.batch_norm
    check_against_fixture(c, out.detach(), grads, bn.running_mean, bn.running_var, bn.num_batches_tracked, "torch route %d" % case)


# ------------------------------------------------------------------------------------------------ the model
def fixture_dataset():
    graphs = R.fixture_graphs(F_IN, K)
    X = np.empty(len(graphs), dtype=object)
    X[:] = [GraphData(g.node_features, g.edge_index) for g in graphs]
    return NumpyDataset(X, MODEL["y"], MODEL["w"])


def fixture_model(device, route="auto"):
    model = LCNNModel(n_occupancy=F_IN, n_neighbor_sites_list=K, n_permutation_list=P, n_features=O, sitewise_n_feature=S,
                      batch_size=8, optimizer=GradientDescent(learning_rate=0.01), log_frequency=1, device=device, route=route)
    model.model.load_state_dict({k: torch.as_tensor(MODEL["param0_" + k]) for k in MODEL["keys"]})
    return model


def inject(model, steps):
    """Makes ``draw_masks`` hand out the recorded masks of ``steps`` (prefixes of the fixture), one step per call."""
    queue = list(steps)

    def draw_masks(n_sites):
        pre = queue.pop(0)
        dev = model.model.fc.weight.device
        masks = [torch.as_tensor(MODEL[pre + "b%d" % i], device=dev) for i in range(len(model.model.LCNN_blocks))]
        assert masks[0].shape[0] == n_sites
        return masks, torch.as_tensor(MODEL[pre + "atom"], device=dev)
    model.model.draw_masks = draw_masks


def check_first_batch(model, ds, tol=TOL):
    batch = next(iter(model.default_generator(ds, epochs=1, deterministic=True, pad_batches=True)))
    inputs, labels, weights = model._prepare_batch(batch)
    inject(model, ["masks0_"])
    model.model.train()
    model.model.zero_grad()
    out = model.model(inputs)
    loss = model._loss_fn([out], labels, weights)
    loss.backward()
    close(out.detach().cpu(), MODEL["out0"], "out0", tol)
    assert abs(float(loss.detach()) - float(MODEL["loss0"])) <= tol * abs(float(MODEL["loss0"]))
    for k, p in model.model.named_parameters():
        if p.requires_grad and k.endswith("conv_weights.bias") and k.startswith("LCNN_blocks"):  # zero but for rounding
            scale = float(np.max(np.abs(MODEL["grad_" + k.replace(".bias", ".weight")])))
            assert float(np.max(np.abs(p.grad.cpu().numpy() - MODEL["grad_" + k]))) <= tol * scale, k
        elif p.requires_grad:
            close(p.grad.cpu(), MODEL["grad_" + k], "grad " + k, tol)
    model.model.load_state_dict({k: torch.as_tensor(MODEL["param0_" + k]) for k in MODEL["keys"]})


def check_fit(model, ds, bar64=False):
    """The 2-epoch fit with the recorded masks against the reference's six losses, ``predict`` and running statistics
    after it, all at 1e-4.  ``bar64``: also
    the accuracy bar against the float64 restatement's losses of the same steps: at most 4 times the float32
    restatement's own distance (the largest ``e_ref`` of the trajectory), floor one float32 ulp of the loss."""
    close(np.asarray(model.predict(ds)), MODEL["predict0"], "predict0")
    inject(model, ["fit%d_" % s for s in range(6)])
    losses = []
    model.fit(ds, nb_epoch=2, deterministic=True, checkpoint_interval=0, all_losses=losses)
    e_ref, tol = float(np.max(MODEL["e_ref"])), TOL
    worst64 = 0.0
    for k, (a, b, b64) in enumerate(zip(losses, MODEL["fit_losses"], MODEL["fit_losses64"])):
        d, d64 = abs(a - b) / abs(b), abs(a - b64) / abs(b64)
        bound64 = max(4 * e_ref, float(np.spacing(np.float32(b64))) / abs(b64))
        worst64 = max(worst64, d64 / bound64)
        print("step %d loss %.9f reference %.9f rel %.3g | float64 %.12f rel %.3g bound %.3g" % (k, a, b, d, b64, d64, bound64))
        assert d <= tol, (k, a, b)
        assert not bar64 or d64 <= bound64, (k, a, b64)
    assert len(losses) == 6
    close(np.asarray(model.predict(ds)), MODEL["predict"], "predict after the fit", tol)
    for k, v in model.model.state_dict().items():
        if "tracked" in k:
            assert int(v) == int(MODEL["after_" + k])
        elif "running_" in k:
            close(v.cpu(), MODEL["after_" + k], k, tol)
    return worst64


def test_torch_route_model_on_the_cpu():
    ds, model = fixture_dataset(), fixture_model(CPU)
    check_first_batch(model, ds)
    assert model.last_route == "torch"
    check_fit(model, ds)


def test_restated_model_matches_the_reference():
    state0 = {k: MODEL["param0_" + k] for k in MODEL["keys"]}
    graphs = R.fixture_graphs(F_IN, K)
    masks = ([MODEL["masks0_b0"], MODEL["masks0_b1"]], MODEL["masks0_atom"])
    for order in ("concat", "split"):
        ref = R.LCNNRef(state0, torch.float64, order=order).train()
        close(ref(R.pack(graphs[:8], P, K) + (masks,)).detach(), MODEL["out0"], "out0 " + order)
        ref = R.LCNNRef(state0, torch.float64, order=order).eval()
        close(ref(R.pack(graphs, P, K) + (None,)).detach(), MODEL["predict0"], "predict0 " + order)


def test_reference_state_dict_round_trips():
    model = LCNN(F_IN, K, P, 1, 0.2, 2, O, S)
    state = model.state_dict()
    assert list(state) == [str(k) for k in MODEL["keys"]]
    for k, shape in zip(MODEL["keys"], MODEL["shapes"]):
        assert list(state[str(k)].shape) == [int(s) for s in shape[:state[str(k)].dim()]], k
    loaded = {k: torch.as_tensor(MODEL["param0_" + k]) for k in MODEL["keys"]}
    model.load_state_dict(loaded)
    for k, v in model.state_dict().items():
        assert torch.equal(v, loaded[k]), k
    assert not model.activation.shift.requires_grad and not model.LCNN_blocks[0].dropout.ones.requires_grad
    assert float(model.activation.shift) == pytest.approx(0.69310)
    assert isinstance(model.Atom_wise_Conv.batch_norm, torch.nn.LayerNorm)
    # the reference's defaults and quirks
    full = LCNNModel(device=CPU)
    assert full.model.LCNN_blocks[1].conv_weights.weight.shape == (44, 19 * 44) and full.model.LCNN_blocks[0].permutation == 6
    assert LCNN().LCNN_blocks[0].conv_weights.weight.shape == (19, 57)
    assert all(b.dropout.dropout.p == 0.2 for b in LCNNModel(dropout_rate=0.7, device=CPU).model.LCNN_blocks)


def test_checks_raise():
    rng = np.random.RandomState(0)
    g = R.torus(rng, 2, 2, F_IN)
    u, v = g.edge_index
    short = R.Graph(g.node_features, np.stack([u[:-1], v[:-1]]))  # the last site lacks one arriving edge
    with pytest.raises(ValueError, match=r"graph 1, node 3 has in-degree 113"):
        LcnnBatch([g, short], CPU, P, K)
    model = LCNNModel(n_occupancy=F_IN, n_features=O, device=CPU, batch_size=2)
    X = np.empty(2, dtype=object)
    X[:] = [GraphData(g.node_features, g.edge_index), GraphData(short.node_features, short.edge_index)]
    with pytest.raises(ValueError, match=r"graph 1, node 3"):
        model.predict(NumpyDataset(X, np.zeros((2, 1)), np.ones((2, 1))))
    with pytest.raises(ValueError, match="n_permutation must be 6"):
        LCNN(n_permutation=4)
    with pytest.raises(ValueError, match="n_permutation must be 6"):
        LCNNModel(n_permutation_list=8, device=CPU)
    one = R.random_sites(rng, 5, 1, 2, 3)
    b = LcnnBatch([one], CPU, 1, 2)
    layer = LCNNBlock(2 * 3, 4, 1)
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        layer(b.sites, b.x)
    assert layer.eval()(b.sites, b.x).shape == (5, 4) and layer.last_route == "torch"
    with pytest.raises(ValueError, match="route"):
        LCNNModel(route="native", device=CPU)


def test_cached_tables_equal_fresh_ones_and_leave_the_dataset_alone():
    rng = np.random.RandomState(3)
    graphs = [R.torus(rng, 2, 3, F_IN), R.torus(rng, 1, 1, F_IN), R.torus(rng, 3, 3, F_IN)]
    # the edges of the last graph interleaved across destinations, each destination's own order kept: the stable
    # sort by destination has work to do
    t = np.sort(rng.rand(graphs[2].num_nodes, P * K), axis=1).reshape(-1)
    interleaved = graphs[2].edge_index[:, np.argsort(t, kind="stable")]
    assert np.any(np.diff(interleaved[1]) < 0)
    X = np.empty(3, dtype=object)
    X[:] = [GraphData(g.node_features, g.edge_index) for g in graphs]
    before = [(g.node_features.copy(), g.edge_index.copy()) for g in X]
    model = LCNNModel(n_occupancy=F_IN, n_features=O, device=CPU, batch_size=3)
    ds = NumpyDataset(X, np.zeros((3, 1)), np.ones((3, 1)))
    first = np.asarray(model.predict(ds))
    cached = [copy.deepcopy(model.graph_tables(g)) for g in X]
    assert all(model.graph_tables(g) is g._lcnn_tables[2] for g in X) and not hasattr(model, "_tables")
    other = GraphData(X[0].node_features, X[0].edge_index.copy())  # another item: its own tables, nothing kept by the model
    assert model.graph_tables(other) is not model.graph_tables(X[0])
    again = np.asarray(model.predict(ds))
    assert np.array_equal(first, again)
    for g, got, (x0, e0) in zip(X, cached, before):
        fresh = ops.lc_graph_tables(g.edge_index, g.num_nodes, P, K)
        assert all(np.array_equal(a, b) for a, b in zip(got, fresh))
        assert np.array_equal(g.node_features, x0) and np.array_equal(g.edge_index, e0)
        nbr = fresh[0].reshape(g.num_nodes, P, K)
        assert np.array_equal(nbr, R.table_of(g, P, K))
        # the reverse lists invert the table: list (u, j) holds exactly the rows v * P + p with nbr[v, p, j] = u, ascending
        ptr = np.concatenate([[0], np.cumsum(fresh[1])])
        for u in range(g.num_nodes):
            for j in (0, 5, K - 1):
                want = np.nonzero(nbr[:, :, j].reshape(-1) == u)[0]
                assert np.array_equal(fresh[2][ptr[u * K + j]:ptr[u * K + j + 1]], want)
    # a batch is the concatenation plus offsets
    b = LcnnBatch(list(X), CPU, P, K, cached)
    x, nbr, ptr = R.pack(graphs, P, K)
    assert np.array_equal(b.sites.nbr.numpy().reshape(-1, P, K), nbr) and np.array_equal(b.sites.node_ptr.numpy(), ptr)
    assert np.array_equal(b.x.numpy(), x.astype(np.float32))
    N = nbr.shape[0]
    rp, rr = b.sites.rev_ptr.numpy(), b.sites.rev_row.numpy()
    for u in (0, 6, 7, N - 1):
        for j in (0, K - 1):
            assert np.array_equal(rr[rp[u * K + j]:rp[u * K + j + 1]], np.nonzero(nbr[:, :, j].reshape(-1) == u)[0])
    # edges that do not arrive grouped by destination give the same table
    fresh = ops.lc_graph_tables(graphs[2].edge_index, 9, P, K)
    assert all(np.array_equal(a, b) for a, b in zip(ops.lc_graph_tables(interleaved, 9, P, K), fresh))
