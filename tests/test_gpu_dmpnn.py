"""D-MPNN on the GPU: the message kernel (csrc/dmpnn.hip) in both directions against the float64 restatement of
tests/dmpnn_refs.py under a DERIVED bound, the bond update (the fused kernel and its decomposed form) and the encoder's
gradients on the native path against float64 (autograd of the restatement), the layers and ``DMPNNModel`` against the reference's fixtures
(tests/golden/dmpnn_*.npz), and a short fit on SMILES end to end.

The message bound: every output element is a sum of n rows' elements in float32, so
``|error| <= (n + 1) * 2^-24 * sum |terms|`` (dmpnn_refs.message returns ``(n + 1) * sum |terms|`` beside the value).
Everything else: 1e-4 of each tensor's largest entry, the project's bar.  Errors are printed per tensor.
"""
import os

import numpy as np
import pytest
import torch

import deepchem_amd as dc
from deepchem_amd import _lib, ops
from deepchem_amd.feat import GraphData
from deepchem_amd.models.torch_models import DMPNN, DMPNNModel, layers
from deepchem_amd.models.torch_models.dmpnn import DmpnnBatch
from deepchem_amd.models.torch_models.dmpnn_layers import MessageUpdateFn
from tests import dmpnn_refs as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-4
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LAYERS = np.load(os.path.join(GOLDEN, "dmpnn_layers.npz"))
MODEL = np.load(os.path.join(GOLDEN, "dmpnn_model.npz"))
E2E = np.load(os.path.join(GOLDEN, "dmpnn_e2e.npz"))
AGG, ACTS = ["mean", "sum", "norm"], ["relu", "tanh"]


def bonds_only(bond_lists):
    """A batch of graphs given as (undirected bond list, atoms), one feature each: only the plan matters."""
    rng = np.random.RandomState(1)
    return DmpnnBatch.from_graphs([R.graph(rng, b, n, 1, 1, 0) for b, n in bond_lists])


MIXED = [([], 1), (R.chain(2), 2), (R.chain(3), 3), (R.ring(6), 6), (R.star(4), 5), (R.star(6), 7), ([], 2),
         (R.chain(130), 130)]
BATCHES = {"one_atom": [([], 1)], "mixed": MIXED}
# chains alone totalling 2, 30, 34, 62, 66, 126, 130 and 258 bond rows
BATCHES.update({"chain%d" % (2 * (n - 1)): [(R.chain(n), n)] for n in (2, 16, 18, 32, 34, 64, 66, 130)})
# a degree-6 atom whose run of bond rows would straddle row 32, 64 and 128 of the batch
BATCHES.update({"straddle%d" % r: [(R.chain((r - 2) // 2 + 1), (r - 2) // 2 + 1), (R.star(6), 7)] for r in (32, 64, 128)})


def within(name, got, want, tol=TOL):
    e = R.rel_err(got, want)
    print(name, e)
    assert np.asarray(got).shape == np.asarray(want).shape, name
    assert e <= tol, (name, e)


def inside(name, got, want, bound):
    """|got - want| <= 2^-24 * bound per element; prints the worst ratio."""
    err = np.abs(got.astype(np.float64) - want)
    ratio = float(np.max(err / np.maximum(R.U * bound, 1e-300))) if err.size else 0.0
    print(name, "worst |error| / bound", ratio)
    assert got.shape == want.shape and np.all(err <= R.U * bound), (name, ratio)


# ------------------------------------------------------------------------------------------------ the message op
@pytest.mark.parametrize("d", [300, 64, 20, 1])
@pytest.mark.parametrize("name", sorted(BATCHES))
def test_message_both_directions_and_the_atom_sum(name, d):
    batch = bonds_only(BATCHES[name]).to(DEV)
    plan, h = batch.plan, batch.host
    A, B = batch.n_atoms, batch.n_bonds
    rng = np.random.RandomState(d)
    x, g, dS = (rng.normal(0, 1, s).astype(np.float32) for s in ((B, d), (B, d), (A, d)))
    rev64 = torch.as_tensor(h["rev"], dtype=torch.int64)
    t64 = lambda a: torch.as_tensor(a.astype(np.float64))  # noqa: E731
    q64, S64, bq, bS = R.message(t64(x), h["out_ptr"], rev64, bounds=True)
    dx64, bdx = R.message_t(t64(g), t64(dS), h["out_ptr"], rev64, bounds=True)

    xd, gd, dSd = (torch.tensor(a, device=DEV) for a in (x, g, dS))
    S, q = ops.dmpnn_message(xd, plan.out_ptr, plan.rev, want_s=True)
    S_alone, none = ops.dmpnn_message(xd, plan.out_ptr, plan.rev, want_s=True, want_q=False)
    assert none is None and torch.equal(S_alone, S)
    prefilled = torch.full((B, d), float("nan"), device=DEV)
    T, dx = ops.dmpnn_message(gd, plan.out_ptr, plan.rev, transposed=True, add=dSd, want_s=True, q_out=prefilled)
    assert dx is prefilled and not bool(torch.isnan(dx).any())  # every bond row was written
    q, S, dx, T = (t.cpu().numpy() for t in (q, S, dx, T))
    inside("q", q, q64.numpy(), bq.numpy())
    inside("S", S, S64.numpy(), bS.numpy())
    inside("dx", dx, dx64.numpy(), bdx.numpy())
    if B == 0:
        assert not S.any() and S.shape == (A, d)
        return
    T64 = torch.zeros((A, d), dtype=torch.float64).index_add_(0, R.bond_source(h["out_ptr"])[0], t64(g))
    within("T", T, T64.numpy(), 1e-6)
    # the two halves of the adjoint alone: g without dS, dS without g
    only_g = ops.dmpnn_message(gd, plan.out_ptr, plan.rev, transposed=True)[1].cpu().numpy()
    only_s = ops.dmpnn_message(None, plan.out_ptr, plan.rev, transposed=True, add=dSd)[1].cpu().numpy()
    for label, got, g_, dS_ in (("dx(g)", only_g, t64(g), torch.zeros_like(t64(dS))),
                                ("dx(dS)", only_s, torch.zeros_like(t64(g)), t64(dS))):
        half, bound = R.message_t(g_, dS_, h["out_ptr"], rev64, bounds=True)
        inside(label, got, half.numpy(), bound.numpy())
    # <M x, (g, dS)> = <x, M^T (g, dS)>, evaluated in float64 on the GPU's outputs
    lhs = float((q.astype(np.float64) * g).sum() + (S.astype(np.float64) * dS).sum())
    rhs = float((x.astype(np.float64) * dx).sum())
    room = R.U * float((bq.numpy() * np.abs(g)).sum() + (bS.numpy() * np.abs(dS)).sum() + (bdx.numpy() * np.abs(x)).sum())
    print("adjoint", lhs, rhs, abs(lhs - rhs), "room", room)
    assert abs(lhs - rhs) <= room


@pytest.mark.parametrize("d", [300, 20, 3])
def test_message_on_strided_and_unaligned_rows(d):
    """Rows inside a wider matrix, starting one float off a 16-byte boundary: the scalar path; same numbers."""
    batch = bonds_only(MIXED).to(DEV)
    plan, B = batch.plan, batch.n_bonds
    wide = torch.randn((B, d + 5), device=DEV)
    x = wide[:, 1:1 + d]
    S0, q0 = ops.dmpnn_message(x.contiguous(), plan.out_ptr, plan.rev, want_s=True)
    out = torch.full((B, d + 5), float("nan"), device=DEV)
    S1, q1 = ops.dmpnn_message(x, plan.out_ptr, plan.rev, want_s=True, q_out=out[:, 1:1 + d])
    assert torch.equal(S0, S1) and torch.equal(q0, q1)
    assert bool(torch.isnan(out[:, 0]).all()) and bool(torch.isnan(out[:, 1 + d:]).all())  # nothing beside the rows


def test_message_wrapper_errors_before_launch():
    batch = bonds_only(MIXED).to(DEV)
    plan, B = batch.plan, batch.n_bonds
    x = torch.zeros((B, 8), device=DEV)
    with pytest.raises(ValueError, match="rows"):
        ops.dmpnn_message(x[:-1], plan.out_ptr, plan.rev)
    with pytest.raises(ValueError, match="transposed"):
        ops.dmpnn_message(x, plan.out_ptr, plan.rev, add=torch.zeros((batch.n_atoms, 8), device=DEV))
    with pytest.raises(_lib.GcmiError, match="int32"):
        ops.dmpnn_message(x, plan.out_ptr.long(), plan.rev)
    with pytest.raises(_lib.GcmiError, match="in place"):
        ops.dmpnn_message(x, plan.out_ptr, plan.rev, q_out=x)


# ------------------------------------------------------------------------------------------------ the update
@pytest.mark.parametrize("relu", [False, True], ids=["none", "relu"])
@pytest.mark.parametrize("d", [300, 64, 40, 8])
@pytest.mark.parametrize("name", sorted(BATCHES))
def test_update_forward_fused_and_decomposed(name, d, relu):
    """h = act(input + (S[a] - x[rev[b]]) . W_h^T): the fused kernel, and the message kernel + segmented product, each
    against float64 within the bar."""
    batch = bonds_only(BATCHES[name]).to(DEV)
    plan, h = batch.plan, batch.host
    if batch.n_bonds == 0:
        empty = torch.zeros((0, d), device=DEV)
        assert MessageUpdateFn.apply(empty, empty, torch.zeros((d, d), device=DEV), plan, relu).shape == (0, d)
        return
    rng = np.random.RandomState(d + relu)
    x, inp = (rng.normal(0, 1, (batch.n_bonds, d)).astype(np.float32) for _ in range(2))
    W = rng.normal(0, 1 / np.sqrt(d), (d, d)).astype(np.float32)
    q64, _ = R.message(torch.as_tensor(x.astype(np.float64)), h["out_ptr"], torch.as_tensor(h["rev"], dtype=torch.int64))
    want = inp.astype(np.float64) + q64.numpy() @ W.astype(np.float64).T
    want = np.maximum(want, 0) if relu else want
    xd, id_, Wd = (torch.tensor(a, device=DEV) for a in (x, inp, W))
    within("h fused", MessageUpdateFn.apply(xd, id_, Wd, plan, relu, True).cpu().numpy(), want)
    within("h decomposed", MessageUpdateFn.apply(xd, id_, Wd, plan, relu, False).cpu().numpy(), want)


def test_update_above_the_width_cap_takes_the_decomposed_path():
    batch = bonds_only(BATCHES["straddle32"]).to(DEV)
    d = 324
    rng = np.random.RandomState(0)
    x, inp = (rng.normal(0, 1, (batch.n_bonds, d)).astype(np.float32) for _ in range(2))
    W = rng.normal(0, 1 / np.sqrt(d), (d, d)).astype(np.float32)
    q64, _ = R.message(torch.as_tensor(x.astype(np.float64)), batch.host["out_ptr"],
                       torch.as_tensor(batch.host["rev"], dtype=torch.int64))
    xd, id_, Wd = (torch.tensor(a, device=DEV) for a in (x, inp, W))
    within("h 324", MessageUpdateFn.apply(xd, id_, Wd, batch.plan, True).cpu().numpy(),
           np.maximum(inp.astype(np.float64) + q64.numpy() @ W.astype(np.float64).T, 0))
    with pytest.raises(ValueError, match="d_hidden <= 320"):
        ops.dmpnn_update_fwd(xd, id_, Wd, batch.plan.out_ptr, batch.plan.rev, batch.plan.bond_src, True,
                             torch.zeros(ops.dmpnn_update_scratch_floats(324), device=DEV))


def test_fused_update_holds_no_aggregated_rows():
    """About 20 000 bond rows at d = 300: the call may allocate its output (24 MB) and little else -- the aggregated rows
    alone would be another 24 MB, the reference's gathered tensor several times that."""
    d = 300
    batch = bonds_only([(R.random_bonds(np.random.RandomState(m), 24, 2), 24) for m in range(400)]).to(DEV)
    B = batch.n_bonds
    assert 19000 <= B <= 21000
    x, inp = torch.randn((B, d), device=DEV), torch.randn((B, d), device=DEV)
    W = torch.randn((d, d), device=DEV) / 17
    MessageUpdateFn.apply(x, inp, W, batch.plan, True)  # (warm: the allocator, the image scratch)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    h = MessageUpdateFn.apply(x, inp, W, batch.plan, True)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    print("rise", rise, "output bytes", h.numel() * 4)
    assert rise <= 1.25 * h.numel() * 4
    q = ops.dmpnn_message(x, batch.plan.out_ptr, batch.plan.rev)[1]
    want = torch.relu(inp.double() + q.double() @ W.double().t())
    within("h 20k", h.cpu().numpy(), want.cpu().numpy())


# ------------------------------------------------------------------------------------------------ gradients
@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("depth", [2, 3, 4])
@pytest.mark.parametrize("mode", ["reference", "paper"])
def test_encoder_gradients_on_the_native_path(mode, depth, act):
    AF, BF, H = 9, 3, 28
    rng = np.random.RandomState(depth)
    graphs = [R.graph(rng, b, n, AF, BF, 2) for b, n in MIXED[:7]] + [R.graph(rng, R.random_bonds(rng, 40, 3), 40, AF, BF, 2)]
    batch = DmpnnBatch.from_graphs(graphs).to(DEV)
    layer = layers.DMPNNEncoderLayer(use_default_fdim=False, atom_fdim=AF, bond_fdim=BF, d_hidden=H, depth=depth,
                                     activation=act, aggregation="mean", message_mode=mode).to(DEV)
    state = {k: v.detach().cpu().numpy() for k, v in layer.state_dict().items()}
    cot = rng.normal(0, 1, (len(graphs), H + 2))
    # float64 autograd of the restatement
    p = {"e." + k: torch.tensor(v.astype(np.float64), requires_grad=True) for k, v in state.items()}
    b64 = R.batch_tensors(batch.host, torch.float64)
    f64, a64 = b64["f_ini_atoms_bonds"].requires_grad_(), b64["atom_features"].requires_grad_()
    out64 = R.encoder(p, "e.", b64, depth, mode, act, "mean", f_ini=f64, atom_features=a64)
    out64.backward(torch.as_tensor(cot))
    # the native path, the two feature matrices as leaves
    batch.f_ini_atoms_bonds = batch.f_ini_atoms_bonds.clone().requires_grad_()
    batch.atom_features = batch.atom_features.clone().requires_grad_()
    out = layer(batch)
    out.backward(torch.tensor(cot.astype(np.float32), device=DEV))
    within("out", out.detach().cpu().numpy(), out64.detach().numpy())
    within("d(input)", batch.f_ini_atoms_bonds.grad.cpu().numpy(), f64.grad.numpy())
    within("d(atom features)", batch.atom_features.grad.cpu().numpy(), a64.grad.numpy())
    for k, prm in layer.named_parameters():
        within("d(%s)" % k, prm.grad.cpu().numpy(), p["e." + k].grad.numpy())
    assert {k for k, _ in layer.named_parameters()} == {"W_i.weight", "W_h.weight", "W_o.weight", "W_o.bias"}


# ------------------------------------------------------------------------------------------------ layers and model
def enc_case(c):
    agg, depth, with_gf, bias, act = [int(v) for v in LAYERS["enc%d_cfg" % c]]
    prefix = "enc%d_p_" % c
    return AGG[agg], depth, bool(with_gf), bool(bias), ACTS[act], \
        {k[len(prefix):]: torch.as_tensor(LAYERS[k]) for k in LAYERS.files if k.startswith(prefix)}


N_ENC = len([k for k in LAYERS.files if k.startswith("enc") and k.endswith("_cfg")])


@pytest.mark.parametrize("c", range(N_ENC))
def test_encoder_on_a_batch_against_the_reference_fixture(c):
    agg, depth, with_gf, bias, act, params = enc_case(c)
    graphs = R.unpack_graphs(LAYERS, "g_")
    if not with_gf:
        graphs = [GraphData(g.node_features, g.edge_index, g.edge_features, global_features=np.empty(0, np.float32))
                  for g in graphs]
    layer = layers.DMPNNEncoderLayer(use_default_fdim=False, atom_fdim=133, bond_fdim=14, d_hidden=20, depth=depth, bias=bias,
                                     activation=act, aggregation=agg, aggregation_norm=7)
    layer.load_state_dict(params)
    with torch.no_grad():
        out = layer.to(DEV)(DmpnnBatch.from_graphs(graphs))  # bias=True: the torch path over to_reference_arrays
    within("enc%d%s" % (c, " (bias)" if bias else ""), out.cpu().numpy(), LAYERS["enc%d_out" % c])


def test_feed_forward_against_the_reference_fixture():
    n = len([k for k in LAYERS.files if k.startswith("ffn") and k.endswith("_cfg")])
    x = torch.tensor(LAYERS["ffn_in"], device=DEV)
    for c in range(n):
        n_layers, at_input = [int(v) for v in LAYERS["ffn%d_cfg" % c]]
        prefix = "ffn%d_p_" % c
        layer = layers.PositionwiseFeedForward(d_input=12, d_hidden=16, d_output=5, activation="relu", n_layers=n_layers,
                                               dropout_at_input_no_act=bool(at_input))
        layer.load_state_dict({k[len(prefix):]: torch.as_tensor(LAYERS[k]) for k in LAYERS.files if k.startswith(prefix)})
        with torch.no_grad():
            within("ffn%d" % c, layer.to(DEV)(x).cpu().numpy(), LAYERS["ffn%d_out" % c])


def model_case(name, **kwargs):
    keys = [str(k) for k in MODEL[name + "_keys"]]
    shapes = {k: tuple(int(v) for v in MODEL["%s_shape_%s" % (name, k)]) for k in keys}
    graphs = R.unpack_graphs(MODEL, "g_")
    if name == "cls":
        graphs = [GraphData(g.node_features, g.edge_index, g.edge_features, global_features=np.empty(0, np.float32))
                  for g in graphs]
    args = dict(mode="regression" if name == "reg" else "classification", n_tasks=2, n_classes=3, batch_size=8,
                global_features_size=4 if name == "reg" else 0, use_default_fdim=False, atom_fdim=133, bond_fdim=14,
                learning_rate=0.001, log_frequency=1)
    args.update(kwargs)
    m = DMPNNModel(**args)
    state0 = R.model_params(shapes, int(MODEL[name + "_seed"]))
    m.model.load_state_dict({k: torch.as_tensor(v) for k, v in state0.items()})
    return m, dc.data.NumpyDataset(np.array(graphs, dtype=object), MODEL["y_" + name], MODEL["w"]), state0


@pytest.mark.parametrize("name", ["reg", "cls"])
def test_model_first_batch_outputs_loss_and_gradients(name):
    m, ds, state0 = model_case(name)
    batch = next(iter(m._batch_generator(ds, deterministic=True)))
    assert isinstance(batch[0], DmpnnBatch)
    inputs, labels, weights = m._prepare_batch(batch)
    outputs = m._forward_lists(inputs)
    loss = m._loss_fn([outputs[i] for i in m._roles.loss], labels, weights)
    loss.backward()
    within(name + " out0", outputs[0].detach().cpu().numpy(), MODEL[name + "_out0"])
    want = float(MODEL[name + "_loss0"])
    print("loss0", float(loss.detach()), want)
    assert abs(float(loss.detach()) - want) <= TOL * abs(want)
    for k, p in m.model.named_parameters():
        within(name + " grad " + k, R.sample(p.grad.cpu().numpy()), MODEL["%s_grad_%s" % (name, k)])
    # ... and every gradient in full against float64 autograd of the restatement
    ref = R.DMPNNRef(state0, torch.float64, mode=m.model.mode, n_tasks=2, n_classes=3)
    y, w = MODEL["y_" + name][:8], MODEL["w"][:8]
    (R.l2_loss if name == "reg" else R.sparse_ce_loss)(ref(batch[0].host), y, w).backward()
    for k, p in m.model.named_parameters():
        within(name + " grad64 " + k, p.grad.cpu().numpy(), ref.table()[k].grad.numpy())


@pytest.mark.parametrize("name", ["reg", "cls"])
def test_model_fit_and_predict_follow_the_reference(name):
    m, ds, _ = model_case(name)
    within(name + " predict0", m.predict(ds), MODEL[name + "_predict0"])
    losses = []
    m.fit(ds, nb_epoch=2, deterministic=True, checkpoint_interval=0, all_losses=losses)
    want, e_ref = MODEL[name + "_fit_losses"], MODEL[name + "_e_ref"]
    errs = np.abs(np.asarray(losses) - want) / np.abs(want)
    print("fit", losses, errs, e_ref)
    assert len(losses) == 6
    for k in range(6):
        assert errs[k] <= max(TOL, 4 * e_ref[k]), (k, errs[k])
    for k, v in m.model.state_dict().items():
        within(name + " final " + k, R.sample(v.cpu().numpy()), MODEL["%s_final_%s" % (name, k)])
    within(name + " predict", m.predict(ds), MODEL[name + "_predict"])


def test_model_save_restore_predicts_identically(tmp_path):
    m, ds, _ = model_case("reg", model_dir=str(tmp_path))
    m.fit(ds, nb_epoch=1, deterministic=True, checkpoint_interval=0)
    before = m.predict(ds)
    m.save_checkpoint()
    m2, _, _ = model_case("reg", model_dir=str(tmp_path))
    m2.restore()
    assert np.array_equal(m2.predict(ds), before)


def test_graph_list_batches_equal_the_cached_gather():
    a, ds, _ = model_case("reg")
    b, _, _ = model_case("reg")
    la, lb = [], []
    a.fit(ds, nb_epoch=1, deterministic=True, checkpoint_interval=0, all_losses=la)
    b.fit_generator(b.default_generator(ds, epochs=1, deterministic=True), checkpoint_interval=0, all_losses=lb)
    errs = np.abs(np.asarray(la) - np.asarray(lb)) / np.abs(np.asarray(lb))
    print("gather vs graph lists", errs)
    assert len(la) == len(lb) == 3 and errs.max() <= 1e-6  # same batches through the same kernels


def test_paper_mode_differs_and_bias_takes_the_torch_path():
    m, ds, _ = model_case("reg")
    p, _, _ = model_case("reg", message_mode="paper")
    assert R.rel_err(p.predict(ds), m.predict(ds)) > 1e-3
    biased = DMPNN(global_features_size=4, use_default_fdim=False, atom_fdim=133, bond_fdim=14, enc_hidden=16, ffn_hidden=16,
                   bias=True).to(DEV)
    graphs = R.unpack_graphs(MODEL, "g_")[:5]
    with torch.no_grad():
        on_gpu = biased(DmpnnBatch.from_graphs(graphs)).cpu().numpy()
        on_cpu = biased.cpu()(DmpnnBatch.from_graphs(graphs)).numpy()
    within("bias=True", on_gpu, on_cpu)


# ------------------------------------------------------------------------------------------------ end to end
def test_fit_on_smiles_end_to_end():
    graphs, y, w = R.e2e_data()
    cfg = R.E2E
    m = DMPNNModel(batch_size=cfg["batch_size"], learning_rate=cfg["lr"], log_frequency=1, **R.e2e_model_args())
    shapes = {k: tuple(v.shape) for k, v in m.model.state_dict().items()}
    state0 = R.model_params(shapes, cfg["seed"])
    m.model.load_state_dict({k: torch.as_tensor(v) for k, v in state0.items()})
    losses = []
    m.fit(dc.data.NumpyDataset(graphs, y, w), nb_epoch=cfg["epochs"], deterministic=True, checkpoint_interval=0,
          all_losses=losses)
    want = np.asarray(R.fit(R.DMPNNRef(state0, torch.float64, n_tasks=1), R.e2e_steps(graphs, y, w), cfg["lr"]))
    assert np.allclose(want, E2E["fit_losses64"], rtol=1e-9)
    errs = np.abs(np.asarray(losses) - want) / np.abs(want)
    print("e2e", losses, errs, E2E["e_ref"])
    assert len(losses) == len(want) == 12
    for k in range(12):
        assert errs[k] <= max(TOL, 4 * E2E["e_ref"][k]), (k, errs[k])
    assert losses[-1] < losses[0]
