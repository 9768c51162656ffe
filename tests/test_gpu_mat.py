"""MAT on the GPU: the bias and attention kernels (csrc/mat.hip) against the float64 restatement of tests/mat_refs.py,
the layers against the reference's layer fixtures, and ``MATModel`` against the reference's recorded first batch,
gradients, fit trajectory and predictions (tests/golden/mat_*.npz).

Bar of the kernels: they are plain fp32, so they are measured against what fp32 can do.  Per output tensor, the largest
error against float64 is at most 4 times the largest error of the float32 restatement on the CPU for the same inputs
(the margin the project gives trajectories, ``max(1e-4, 4 e_ref)``: it covers another summation order and the device
``exp``), with a floor of one fp32 ulp of the tensor's largest entry.  The ratios are printed.
Bar of layers and model: 1e-4 of each tensor's largest entry, as tests/test_gpu_dtnn.py.
"""
import os

import numpy as np
import pandas as pd
import pytest
import torch

import deepchem_amd as dc
from deepchem_amd import ops
from deepchem_amd.feat import MATFeaturizer
from deepchem_amd.models.torch_models import MAT, MATModel, MatBatch, layers
from tests import mat_refs as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-4
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LAYERS = np.load(os.path.join(GOLDEN, "mat_layers.npz"))
MODEL = np.load(os.path.join(GOLDEN, "mat_model.npz"))
KEYS = [str(k) for k in MODEL["keys"]]
WIDTH = dict(sa_hsize=32, d_input=32, d_hidden=32, d_output=32, encoder_hsize=32)
CAP = ops.MAT_MAX_ATOMS
# one wave and two, each wave boundary from both sides, the cap from below and at it
SIZES = [1, 2, 3, 31, 32, 33, 63, 64, 65, CAP - 1, CAP]


def bar(got, want64, got32, name):
    """The accuracy bar of the module docstring; returns the ratio error / fp32 error."""
    want64 = np.asarray(want64, np.float64)
    e = float(np.max(np.abs(np.asarray(got, np.float64) - want64)))
    e32 = float(np.max(np.abs(np.asarray(got32, np.float64) - want64)))
    floor = float(np.spacing(np.float32(np.max(np.abs(want64)))))
    ratio = e / max(e32, 1e-300)
    print("%s: error %.3g, fp32 restatement %.3g, ratio %.2f, floor %.3g" % (name, e, e32, ratio, floor))
    assert np.all(np.isfinite(np.asarray(got))), name
    assert e <= max(4 * e32, floor), (name, e, e32, floor)
    return ratio if e > floor else 0.0


# ------------------------------------------------------------------------------------------------ bias kernel
def bias_case():
    rng = np.random.RandomState(4)
    mols = [R.synthetic_molecule(n - 1, rng) for n in (1, 2, 33, CAP)]
    return R.pack(mols)


@pytest.mark.parametrize("kind", ["softmax", "exp"])
def test_bias_kernel(kind):
    n_list, _, adj, dist = bias_case()
    offs = ops.MatOffsets(n_list, DEV)
    got = ops.mat_bias(torch.tensor(adj, dtype=torch.float32, device=DEV), torch.tensor(dist, dtype=torch.float32, device=DEV),
                       offs, kind, 0.33, 0.34).cpu().numpy()
    want = R.bias_blocks(adj, dist, n_list, kind, 0.33, 0.34, 1e-6, torch.float64).numpy()
    got32 = R.bias_blocks(adj, dist, n_list, kind, 0.33, 0.34, 1e-6, torch.float32).numpy()
    bar(got, want, got32, "bias " + kind)
    for m, n in enumerate(n_list):
        B = got[offs.pair_off[m]:offs.pair_off[m + 1]].reshape(n, n)
        # the dummy row (all distances 1e6, no bonds): uniform weights; real rows: an exact 0 in the dummy's column
        assert np.all(B[0] == B[0, 0]) and B[0, 0] == (np.float32(0.33) * (np.float32(1) / np.float32(n)) if kind == "softmax" else 0.0)
        assert np.all(B[1:, 0] == 0.0)
        assert np.all(B[1:].sum(1) > 0.3)  # (the nearest atom alone carries lambda_distance exp(0) or more)


# ------------------------------------------------------------------------------------------------ attention kernels
_CASES = {}


def attention_case(h, d_k, lam=0.33, q_scale=1.0, shared=False):
    """Inputs, the float64 and float32 restatements (outputs and gradients), computed once per case."""
    key = (h, d_k, lam, q_scale, shared)
    if key in _CASES:
        return _CASES[key]
    rng = np.random.RandomState(100 * h + d_k)
    mols = [R.synthetic_molecule(n - 1, rng) for n in SIZES]
    n_list, _, adj, dist = R.pack(mols)
    N, W = sum(n_list), h * d_k
    c = {"n_list": n_list, "h": h, "d_k": d_k, "lam": lam, "shared": shared,
         "bias": R.bias_blocks(adj, dist, n_list, "softmax", 0.33, 0.34, 1e-6, torch.float32).numpy(),
         "q": (q_scale * rng.normal(0, 1, (N, W))).astype(np.float32), "dO": rng.normal(0, 1, (N, W)).astype(np.float32)}
    c["k"] = c["q"] if shared else rng.normal(0, 1, (N, W)).astype(np.float32)
    c["v"] = c["q"] if shared else rng.normal(0, 1, (N, W)).astype(np.float32)
    for dtype, name in ((torch.float64, "f64"), (torch.float32, "f32")):
        q = torch.tensor(c["q"], dtype=dtype, requires_grad=True)
        k, v = (q, q) if shared else (torch.tensor(c["k"], dtype=dtype, requires_grad=True),
                                      torch.tensor(c["v"], dtype=dtype, requires_grad=True))
        o = R.attention(q, k, v, torch.tensor(c["bias"], dtype=dtype), n_list, h, lam)
        o.backward(torch.tensor(c["dO"], dtype=dtype))
        c[name] = {"O": o.detach().numpy(), "dQ": q.grad.numpy()}
        if not shared:
            c[name].update({"dK": k.grad.numpy(), "dV": v.grad.numpy()})
    _CASES[key] = c
    return c


def wide(x, spare=4):
    """x as the leading columns of a matrix whose spare columns are NaN."""
    t = torch.full((x.shape[0], x.shape[1] + spare), float("nan"), dtype=torch.float32, device=DEV)
    t[:, :x.shape[1]] = torch.as_tensor(x, device=DEV)
    return t


def run_native(c, spare=4):
    """The three ops entries on operands with ``spare`` NaN columns behind the heads; outputs into such buffers too."""
    offs = ops.MatOffsets(c["n_list"], DEV)
    W = c["h"] * c["d_k"]
    bias = torch.tensor(c["bias"], device=DEV)
    Q = wide(c["q"], spare)
    K, V = (Q, Q) if c["shared"] else (wide(c["k"], spare), wide(c["v"], spare))
    q, k, v = Q[:, :W], K[:, :W], V[:, :W]
    dO = wide(c["dO"], spare)
    O = wide(np.zeros_like(c["q"]), spare)
    ops.mat_attention_fwd(q, k, v, bias, offs, c["h"], c["d_k"], c["lam"], out=O[:, :W])
    bufs = [wide(np.zeros_like(c["q"]), spare) for _ in range(1 if c["shared"] else 3)]
    ops.mat_attention_bwd(q, k, v, bias, offs, c["h"], c["d_k"], c["lam"], dO[:, :W], c["shared"],
                          out=bufs[0][:, :W] if c["shared"] else [b[:, :W] for b in bufs])
    out = dict(zip(("O", "dQ", "dK", "dV"), [O] + bufs))
    if spare:
        for name, t in out.items():
            assert bool(torch.isnan(t[:, W:]).all()), "%s: the spare columns were written" % name
    return {name: t[:, :W].cpu().numpy() for name, t in out.items()}


def check_case(c, label):
    got = run_native(c)
    return max(bar(got[name], c["f64"][name], c["f32"][name], "%s %s" % (label, name)) for name in c["f64"])


@pytest.mark.parametrize("d_k", [4, 8, 20, 64])
@pytest.mark.parametrize("h", [1, 3, 16])
def test_attention_three_tensors(h, d_k):
    worst = check_case(attention_case(h, d_k), "h%d d_k%d" % (h, d_k))
    print("worst ratio", worst)


@pytest.mark.parametrize("d_k", [4, 8, 20, 64])
@pytest.mark.parametrize("h", [1, 3, 16])
def test_attention_one_shared_tensor(h, d_k):
    """Q = K = V as ONE tensor with shared=True: dQ + dK + dV in one buffer, against float64 autograd through the one
    leaf and against the three-tensor call on the same values, summed."""
    c = attention_case(h, d_k, shared=True)
    check_case(c, "shared h%d d_k%d" % (h, d_k))
    three = dict(c, shared=False)
    a, b = run_native(c)["dQ"], run_native(three)
    summed = (b["dQ"] + b["dK"]) + b["dV"]
    assert np.array_equal(run_native(c)["O"], b["O"])
    print("shared vs summed", R.rel_err(a, summed))
    assert np.array_equal(a, summed)  # the same three rows added in the same order: bit for bit


@pytest.mark.parametrize("lam", [0.0, 1.0])
def test_attention_lambda_edges(lam):
    c = attention_case(3, 20, lam=lam)
    check_case(c, "lambda %g" % lam)
    if lam == 0.0:  # only the bias path carries a gradient
        got = run_native(c)
        assert np.all(got["dQ"] == 0) and np.all(got["dK"] == 0) and np.any(got["dV"] != 0)


def test_attention_large_scores():
    """Q scaled by 30: scores of a few hundred, the softmax close to one-hot; the row maximum must be subtracted."""
    c = attention_case(3, 8, lam=1.0, q_scale=30.0)
    last = slice(sum(SIZES) - CAP, sum(SIZES))  # head 0 of the largest molecule
    assert np.abs(c["q"][last, :8] @ c["k"][last, :8].T).max() / np.sqrt(8) > 88.0  # exp of it unshifted would overflow
    check_case(c, "q x 30")


def test_attention_backward_is_deterministic():
    c = attention_case(16, 8)
    a, b = run_native(c), run_native(c)
    for name in a:
        assert np.array_equal(a[name], b[name]), name
    s = attention_case(16, 8, shared=True)
    assert np.array_equal(run_native(s)["dQ"], run_native(s)["dQ"])


def test_attention_without_spare_columns_and_errors_before_launch():
    c = attention_case(3, 8)
    got = run_native(c, spare=0)
    for name in c["f64"]:
        bar(got[name], c["f64"][name], c["f32"][name], "ld = width " + name)
    offs = ops.MatOffsets([3, 5], DEV)
    x = torch.zeros((8, 24), device=DEV)
    bias = torch.zeros(34, device=DEV)
    with pytest.raises(ValueError, match="multiple of 4"):
        ops.mat_attention_fwd(x, x, x, bias, offs, 4, 6, 0.33)
    with pytest.raises(ValueError, match="expected 8"):
        ops.mat_attention_fwd(x[:7], x[:7], x[:7], bias, offs, 3, 8, 0.33)
    with pytest.raises(ValueError, match="up to %d atoms" % CAP):
        ops.mat_attention_fwd(x, x, x, bias, ops.MatOffsets([CAP + 1], DEV), 3, 8, 0.33)
    with pytest.raises(ValueError, match="16-byte"):
        y = torch.zeros((8, 26), device=DEV)
        ops.mat_attention_fwd(y[:, :24], y[:, :24], y[:, :24], bias, offs, 3, 8, 0.33)
    with pytest.raises(ValueError, match="one tensor"):
        ops.mat_attention_bwd(x, x.clone(), x, bias, offs, 3, 8, 0.33, x, True)


def test_attention_function_holds_no_per_head_tensor():
    """64 molecules of 64 atoms, 16 heads of 8: forward + backward stay below ONE of the reference's (B, h, N, N) float
    tensors (it holds six per layer); outputs and the three gradients are about 8 MB of that 16.8 MB."""
    rng = np.random.RandomState(1)
    n_list = [64] * 64
    offs = ops.MatOffsets(n_list, DEV)
    bias = torch.tensor(rng.uniform(0, 0.1, offs.n_pairs).astype(np.float32), device=DEV)
    q, k, v = [torch.tensor(rng.normal(0, 1, (offs.n_atoms, 128)).astype(np.float32), device=DEV, requires_grad=True)
               for _ in range(3)]
    dO = torch.tensor(rng.normal(0, 1, (offs.n_atoms, 128)).astype(np.float32), device=DEV)

    def step():
        q.grad = k.grad = v.grad = None
        ops.MatAttentionFn.apply(q, k, v, bias, offs, 16, 0.33).backward(dO)
    step()  # (warm: allocator, LDS limits)
    q.grad = k.grad = v.grad = None
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    step()
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    print("rise", rise, "of", 64 * 16 * 64 * 64 * 4)
    assert rise < 64 * 16 * 64 * 64 * 4


# ------------------------------------------------------------------------------------------------ layers
def layer_batch():
    n = [int(x) for x in LAYERS["n_atoms"]]
    node = np.concatenate([LAYERS["node"][m, :k] for m, k in enumerate(n)])
    adj = np.concatenate([LAYERS["adj"][m, :k, :k].reshape(-1) for m, k in enumerate(n)])
    dist = np.concatenate([LAYERS["dist"][m, :k, :k].reshape(-1) for m, k in enumerate(n)])
    return MatBatch(n, node, adj, dist, DEV), n


def rows(padded, n):
    return np.concatenate([padded[m, :k] for m, k in enumerate(n)])


def load(module, prefix):
    module.load_state_dict({k[len(prefix) + 3:]: torch.as_tensor(LAYERS[k]) for k in LAYERS.files
                            if k.startswith(prefix + "_p_")})
    return module.to(DEV)


def test_layer_fixtures():
    batch, n = layer_batch()
    x_pad, y_pad = torch.as_tensor(LAYERS["x"], device=DEV), torch.as_tensor(LAYERS["y"], device=DEV)
    x, y = torch.as_tensor(rows(LAYERS["x"], n), device=DEV), torch.as_tensor(rows(LAYERS["y"], n), device=DEV)
    node, adj, dist = [torch.as_tensor(LAYERS[k], device=DEV) for k in ("node", "adj", "dist")]
    mask = node.abs().sum(-1) != 0
    errs = {}

    def both(name, packed_out, padded_out, want):
        errs[name + " pad-free"] = R.rel_err(packed_out.detach().cpu().numpy(), rows(want, n) if want.ndim == 3 else want)
        errs[name + " padded"] = R.rel_err(rows(padded_out.detach().cpu().numpy(), n) if want.ndim == 3 else
                                           padded_out.detach().cpu().numpy(), rows(want, n) if want.ndim == 3 else want)

    emb = load(layers.MATEmbedding(36, 32, 0.0), "emb")
    both("embedding", emb(batch.node), emb(node), LAYERS["emb_out"])
    sub = load(layers.SublayerConnection(32, 0.0), "sub")
    both("sublayer", sub(x, y), sub(x_pad, y_pad), LAYERS["sub_out"])
    for kind in ("softmax", "exp"):
        att = load(layers.MultiHeadedMATAttention(kind, 0.33, 0.33, 4, 32), "att_" + kind)
        both("attention " + kind, att(x, x, x, batch=batch), att(x_pad, x_pad, x_pad, mask, adj, dist),
             LAYERS["att_%s_out" % kind])
        # distinct input tensors: three projections, the three-tensor kernel call
        both("attention, three tensors " + kind, att(x, x.clone(), x.clone(), batch=batch),
             att(x_pad, x_pad.clone(), x_pad.clone(), mask, adj, dist), LAYERS["att_%s_out" % kind])
        enc = load(layers.MATEncoderLayer(dist_kernel=kind, h=4, **WIDTH), "enc_" + kind)
        both("encoder " + kind, enc(x, batch=batch), enc(x_pad, mask, adj, dist), LAYERS["enc_%s_out" % kind])
    for agg in ("mean", "grover"):
        gen = load(layers.MATGenerator(32, agg, 2, 1, 0.0, 16, 4), "gen_" + agg)
        both("generator " + agg, gen(x, batch=batch), gen(x_pad, mask), LAYERS["gen_%s_out" % agg])
    print(errs)
    assert max(errs.values()) <= TOL, errs


def test_encoder_layer_takes_the_one_tensor_path(monkeypatch):
    """The encoder projects ONCE and hands the kernels one tensor three times: the forward sees equal pointers, the
    backward is asked for dQ + dK + dV in one buffer.  (Lost identity would still give correct numbers, at three times
    the projection work: hence this test.)"""
    batch, n = layer_batch()
    seen = {"fwd": [], "bwd": [], "linear": 0}
    fwd, bwd, gemm = ops.mat_attention_fwd, ops.mat_attention_bwd, ops.seg_gemm

    def spy_fwd(q, k, v, *args, **kwargs):
        seen["fwd"].append(q.data_ptr() == k.data_ptr() == v.data_ptr())
        return fwd(q, k, v, *args, **kwargs)

    def spy_bwd(q, k, v, bias, offs, n_heads, d_k, lam, dO, shared=False, out=None):
        seen["bwd"].append(bool(shared))
        return bwd(q, k, v, bias, offs, n_heads, d_k, lam, dO, shared, out)

    def spy_gemm(*args, **kwargs):
        seen["linear"] += 1
        return gemm(*args, **kwargs)

    monkeypatch.setattr(ops, "mat_attention_fwd", spy_fwd)
    monkeypatch.setattr(ops, "mat_attention_bwd", spy_bwd)
    monkeypatch.setattr(ops, "seg_gemm", spy_gemm)
    enc = load(layers.MATEncoderLayer(dist_kernel="softmax", h=4, **WIDTH), "enc_softmax")
    x = torch.as_tensor(rows(LAYERS["x"], n), device=DEV).requires_grad_(True)
    out = enc(x, batch=batch)
    assert seen["fwd"] == [True] and seen["linear"] == 3  # one projection, output_linear, the feed-forward layer
    out.sum().backward()
    assert seen["bwd"] == [True]
    seen["fwd"].clear(), seen["bwd"].clear()
    enc.self_attn(x, x.detach().clone(), x.detach().clone(), batch=batch).sum().backward()  # three tensors: three buffers
    assert seen["fwd"] == [False] and seen["bwd"] == [False]


# ------------------------------------------------------------------------------------------------ model
def dataset():
    return R.fixture_dataset(dc, MODEL)


def model_with(prefix, kind="softmax", **kwargs):
    m = MATModel(dist_kernel=kind, n_encoders=2, h=4, batch_size=8, learning_rate=0.001, log_frequency=1, **WIDTH, **kwargs)
    m.model.load_state_dict({k: torch.as_tensor(MODEL[prefix + k]) for k in KEYS})  # a reference-format state dict
    return m


@pytest.mark.parametrize("kind", ["softmax", "exp"])
def test_model_first_batch_outputs_loss_and_gradients(kind):
    pre = "" if kind == "softmax" else "exp_"
    m = model_with("param0_", kind)
    assert list(m.model.state_dict()) == KEYS
    m.model.train()
    batch = next(iter(m._batch_generator(dataset(), deterministic=True)))
    assert isinstance(batch[0], MatBatch)
    inputs, labels, weights = m._prepare_batch(batch)
    out = m.model(inputs)
    assert m.last_route == "native"
    loss = m._loss_fn([out], labels, weights)
    loss.backward()
    errs = {"out0": R.rel_err(out.detach().cpu().numpy(), MODEL[pre + "out0"]),
            "loss0": abs(float(loss.detach()) - float(MODEL[pre + "loss0"])) / abs(float(MODEL[pre + "loss0"]))}
    for k, p in m.model.named_parameters():
        errs["grad_" + k] = R.rel_err(p.grad.cpu().numpy(), MODEL[pre + "grad_" + k])
    print(errs)
    assert len(errs) == 2 + 4 + 2 * 8 and max(errs.values()) <= TOL, errs
    # the padded arrays through MAT.forward: the torch route, the same numbers
    padded = m.model([MODEL["gen_node"], MODEL["gen_adj"], MODEL["gen_dist"]]) if kind == "softmax" else None
    if padded is not None:
        assert m.last_route == "torch"
        assert R.rel_err(padded.detach().cpu().numpy(), out.detach().cpu().numpy()) <= TOL


@pytest.mark.parametrize("kind", ["softmax", "exp"])
def test_model_fit_follows_the_reference(kind):
    pre = "" if kind == "softmax" else "exp_"
    m = model_with("param0_", kind)
    losses = []
    m.fit(dataset(), nb_epoch=2, deterministic=True, checkpoint_interval=0, all_losses=losses)
    assert m.last_route == "native"
    want, e_ref = MODEL[pre + "fit_losses"], MODEL[pre + "e_ref"]
    errs = np.abs(np.asarray(losses) - want) / np.abs(want)
    print("fit", losses, errs, e_ref)
    assert len(losses) == 6
    for k in range(6):
        assert errs[k] <= max(TOL, 4 * e_ref[k]), (k, errs[k])


def test_model_predict_on_reference_trained_parameters():
    m = model_with("final_")
    pred = m.predict(dataset())
    e = R.rel_err(pred, MODEL["predict"])
    print("predict", e)
    assert pred.shape == MODEL["predict"].shape and e <= TOL


def test_model_save_restore_predicts_identically(tmp_path):
    m = model_with("param0_", model_dir=str(tmp_path))
    m.fit(dataset(), nb_epoch=1, deterministic=True, checkpoint_interval=0)
    before = m.predict(dataset())
    m.save_checkpoint()
    m2 = MATModel(n_encoders=2, h=4, batch_size=8, learning_rate=0.001, model_dir=str(tmp_path), **WIDTH)
    m2.restore()
    att = m2.model.encoder[0].self_attn
    assert att.linear_layers[0] is att.linear_layers[2]
    assert np.array_equal(m2.predict(dataset()), before)


def test_molecule_above_the_cap_takes_the_torch_route():
    m = model_with("param0_")
    m.model.eval()
    mols = R.fixture_molecules()[:5]
    big = R.synthetic_molecule(CAP, np.random.RandomState(8))  # cap + 1 atoms with the dummy node
    with torch.no_grad():
        alone = m.model(MatBatch.from_encodings(mols, DEV)).cpu().numpy()
        assert m.last_route == "native"
        mixed = m.model(MatBatch.from_encodings(mols + [big], DEV)).cpu().numpy()
        assert m.last_route == "torch"
        ref = R.MATRef({k: MODEL["param0_" + k] for k in KEYS}, torch.float64, h=4)
        want = ref(R.pack(mols + [big])).numpy()
    e = R.rel_err(mixed, want)
    print("torch route", e, R.rel_err(mixed[:5], alone))
    assert e <= TOL and R.rel_err(mixed[:5], alone) <= TOL
    # a real atom without features: the reference masks it, so the batch is handed to the padded arithmetic
    bad = R.Encoding(mols[1].node_features.copy(), mols[1].adjacency_matrix, mols[1].distance_matrix)
    bad.node_features[2] = 0.0
    with torch.no_grad():
        got = m.model(MatBatch.from_encodings(mols + [bad], DEV)).cpu().numpy()
    assert m.last_route == "torch" and R.rel_err(got[:5], alone) <= TOL
    # dropout on the attention weights while training: the torch route as well
    d = MATModel(n_encoders=1, h=4, sa_dropout_p=0.5, batch_size=8, **WIDTH)
    d.model.train()
    d.model(MatBatch.from_encodings(mols, DEV))
    assert d.last_route == "torch"
    d.model.eval()
    d.model(MatBatch.from_encodings(mols, DEV))
    assert d.last_route == "native"


def test_fit_from_smiles_end_to_end():
    table = pd.read_csv(os.path.join(GOLDEN, "delaney_sample.csv"))[:64]
    y = table.iloc[:, 2].to_numpy(np.float64)[:, None]
    X = MATFeaturizer().featurize(table["smiles"].tolist())
    assert all(hasattr(e, "node_features") for e in X)
    ds = dc.data.NumpyDataset(X, (y - y.mean()) / y.std())
    torch.manual_seed(0)
    m = MATModel(n_encoders=2, h=16, sa_hsize=128, d_input=128, d_hidden=128, d_output=128, encoder_hsize=128,
                 batch_size=32, learning_rate=0.00005, log_frequency=1)
    losses = []
    m.fit(ds, nb_epoch=8, deterministic=True, checkpoint_interval=0, all_losses=losses)
    print("losses", losses)
    assert m.last_route == "native" and len(losses) == 16
    assert np.mean(losses[-2:]) < 0.95 * np.mean(losses[:2])  # the last epoch against the first
    assert m.predict(ds).shape == (64, 1)
