"""A plain-torch restatement of the Molecule Attention Transformer (deepchem/models/torch_models/mat.py and the MAT layers
of torch_models/layers.py of the reference), parametrised by dtype, in two forms:

* PAD-FREE (``bias_blocks``, ``attention``, ``MATRef``): the atoms of a batch concatenated, pair data as per-molecule
  ``n x n`` blocks -- what csrc/mat.hip computes.  float64 is the yardstick the GPU tests measure against, float32 on
  the CPU the yardstick of what plain float32 arithmetic makes of a case.
* PADDED (``padded_forward``): the reference's algorithm on ``(B, N, ...)`` arrays, written anew, for the timing
  comparison of tools/mat_step_time.py and as a cross-check of the pad-free form.

State-dict keys are the reference's (aliases of the shared modules included), so its parameters load directly; a shared
parameter is ONE leaf, so its gradient is the sum over its uses, as in the reference.
"""
import math

import numpy as np
import torch

DEFAULTS = dict(dist_kernel="softmax", lambda_attention=0.33, lambda_distance=0.33, h=16, activation="leakyrelu",
                gen_aggregation_type="mean")


def rel_err(got, want):
    """max |got - want| relative to the largest entry of ``want``."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.max(np.abs(got - want)) / max(float(np.max(np.abs(want))), 1e-30)) if want.size else 0.0


def offsets(n_list):
    n = np.asarray(n_list, np.int64)
    return np.concatenate([[0], np.cumsum(n)]), np.concatenate([[0], np.cumsum(n * n)])


def _t(x, dtype, device=None):
    return (x if torch.is_tensor(x) else torch.as_tensor(np.asarray(x))).to(device=device, dtype=dtype)


def dist_kernel_fn(name):
    return (lambda x: torch.softmax(-x, dim=-1)) if name == "softmax" else (lambda x: torch.exp(-x))


def bias_blocks(adj, dist, n_list, dist_kernel, lambda_distance, lambda_adjacency, eps=1e-6, dtype=torch.float64):
    """lambda_distance g(D) + lambda_adjacency A / (rowsum A + eps) per molecule block, flat."""
    adj, dist = _t(adj, dtype).reshape(-1), _t(dist, dtype, adj.device if torch.is_tensor(adj) else None).reshape(-1)
    g = dist_kernel_fn(dist_kernel)
    _, poff = offsets(n_list)
    out = []
    for m, n in enumerate(n_list):
        A, D = adj[poff[m]:poff[m + 1]].view(n, n), dist[poff[m]:poff[m + 1]].view(n, n)
        out.append((lambda_distance * g(D) + lambda_adjacency * (A / (A.sum(-1, keepdim=True) + eps))).reshape(-1))
    return torch.cat(out)


def attention(q, k, v, bias, n_list, h, lambda_attention):
    """O = (lambda_attention softmax(Q K^T / sqrt(d_k)) + B) V per (molecule, head); q, k, v (atoms, h d_k)."""
    aoff, poff = offsets(n_list)
    d_k = q.shape[1] // h
    out = []
    for m, n in enumerate(n_list):
        sl = slice(int(aoff[m]), int(aoff[m + 1]))
        Q, K, V = [x[sl].view(n, h, d_k).transpose(0, 1) for x in (q, k, v)]  # (h, n, d_k)
        B = bias[poff[m]:poff[m + 1]].view(1, n, n)
        P = lambda_attention * torch.softmax(Q @ K.transpose(-2, -1) / math.sqrt(d_k), dim=-1) + B
        out.append((P @ V).transpose(0, 1).reshape(n, h * d_k))
    return torch.cat(out)


def activation_fn(name):
    return {"relu": torch.relu, "leakyrelu": lambda x: torch.nn.functional.leaky_relu(x, 0.1), "tanh": torch.tanh,
            "elu": torch.nn.functional.elu, "selu": torch.selu, "linear": lambda x: x}[name]


def layer_norm(x, w, b, eps=1e-5):
    return torch.nn.functional.layer_norm(x, (x.shape[-1],), w, b, eps)


class MATRef(torch.nn.Module):
    """MAT with parameters in ``dtype`` (feed-forward ``n_layers = 1``, generator ``n_layers = 1``, no dropout: the
    fixture's model).  ``forward`` takes ``(n_list, node rows, adjacency blocks, distance blocks)``."""

    def __init__(self, state, dtype, **cfg):
        super().__init__()
        self.cfg = dict(DEFAULTS, **cfg)
        self.dtype = dtype
        # aliases (the shared modules) map to ONE leaf
        self.names, leaves, self.alias = [], [], {}
        first = {}
        for k, v in state.items():
            canon = k.replace("linear_layers.1.", "linear_layers.0.").replace("linear_layers.2.", "linear_layers.0.") \
                     .replace("sublayer.1.", "sublayer.0.")
            if canon not in first:
                first[canon] = len(leaves)
                self.names.append(canon)
                leaves.append(torch.nn.Parameter(torch.as_tensor(np.asarray(v)).to(dtype).clone()))
            self.alias[k] = canon
        self.params = torch.nn.ParameterList(leaves)

    def table(self):
        """canonical key -> leaf (each parameter once, as ``named_parameters`` of the reference lists them)."""
        return dict(zip(self.names, self.params))

    def n_encoders(self):
        return len([k for k in self.names if k.endswith("self_attn.output_linear.weight")])

    def encoder_layer(self, p, i, x, att_fn):
        pre = "encoder.%d." % i
        lin = lambda t, name: t @ p[pre + name + ".weight"].t() + (p[pre + name + ".bias"] if pre + name + ".bias" in p else 0)
        nw, nb = p[pre + "sublayer.0.norm.weight"], p[pre + "sublayer.0.norm.bias"]
        att = lin(att_fn(lin(x, "self_attn.linear_layers.0")), "self_attn.output_linear")
        x = x + layer_norm(att, nw, nb)
        ff = activation_fn(self.cfg["activation"])(lin(x, "feed_forward.linears.0"))
        return x + layer_norm(ff, nw, nb)

    def forward(self, inputs):
        n_list, node, adj, dist = inputs
        n_list = [int(n) for n in n_list]
        p = self.table()
        dev = self.params[0].device
        c = self.cfg
        x = _t(node, self.dtype, dev)
        bias = bias_blocks(_t(adj, self.dtype, dev), _t(dist, self.dtype, dev), n_list, c["dist_kernel"],
                           c["lambda_distance"], 1.0 - c["lambda_attention"] - c["lambda_distance"], 1e-6, self.dtype)
        x = x @ p["embedding.linear_unit.weight"].t() + p["embedding.linear_unit.bias"]
        for i in range(self.n_encoders()):
            x = self.encoder_layer(p, i, x, lambda t: attention(t, t, t, bias, n_list, c["h"], c["lambda_attention"]))
        aoff, _ = offsets(n_list)
        mem = torch.as_tensor(np.repeat(np.arange(len(n_list)), n_list), device=dev)
        pooled = torch.zeros((len(n_list), x.shape[1]), dtype=x.dtype, device=dev).index_add_(0, mem, x)
        pooled = pooled / _t(np.asarray(n_list, np.float64), self.dtype, dev).unsqueeze(-1)
        return pooled @ p["generator.proj.weight"].t() + p["generator.proj.bias"]

    def padded_forward(self, node, adj, dist):
        """The reference's padded algorithm: masks, ``(B, h, N, N)`` tensors and all."""
        p = self.table()
        c = self.cfg
        h = c["h"]
        dev = self.params[0].device
        node, adj, dist = _t(node, self.dtype, dev), _t(adj, self.dtype, dev), _t(dist, self.dtype, dev)
        mask = node.abs().sum(-1) != 0  # (B, N)
        B, N = mask.shape
        x = node @ p["embedding.linear_unit.weight"].t() + p["embedding.linear_unit.bias"]
        key_pad = (~mask).view(B, 1, 1, N)
        lam_a = 1.0 - c["lambda_attention"] - c["lambda_distance"]
        g = dist_kernel_fn(c["dist_kernel"])

        def att_fn(t):
            d_k = t.shape[-1] // h
            q = t.view(B, N, h, d_k).transpose(1, 2)
            scores = (q @ q.transpose(-2, -1) / math.sqrt(d_k)).masked_fill(key_pad, -1e12)
            p_attn = torch.softmax(scores, dim=-1)
            p_adj = (adj / (adj.sum(-1, keepdim=True) + 1e-6)).unsqueeze(1).repeat(1, h, 1, 1)
            p_dist = g(dist.masked_fill(key_pad[:, 0], float("inf"))).unsqueeze(1).repeat(1, h, 1, 1)
            w = c["lambda_attention"] * p_attn + c["lambda_distance"] * p_dist + lam_a * p_adj
            return (w @ q).transpose(1, 2).contiguous().view(B, N, h * d_k)

        for i in range(self.n_encoders()):
            x = self.encoder_layer(p, i, x, att_fn)
        m = mask.unsqueeze(-1).to(x.dtype)
        pooled = (x * m).sum(1) / m.sum(1)
        return pooled @ p["generator.proj.weight"].t() + p["generator.proj.bias"]


def l2_loss(out, y, w):
    """TorchModel's _StandardLoss over L2Loss: mean(w * (out - y)^2)."""
    y = _t(y, out.dtype, out.device).reshape(out.shape)
    w = _t(w, out.dtype, out.device).reshape(out.shape)
    return torch.mean(torch.square(out - y) * w)


def fit(model, batches, learning_rate=0.001):
    """One Adam step (torch defaults: the reference's) per batch of ``(inputs, y, w)``; the per-step losses."""
    opt = torch.optim.Adam(model.parameters(), lr=learning_rate)
    losses = []
    for inputs, y, w in batches:
        opt.zero_grad()
        loss = l2_loss(model(inputs), y, w)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    return losses


def pack(encodings):
    """``(n_list, node rows, adjacency blocks, distance blocks)`` of MATEncoding-like objects, float64."""
    n_list = [int(np.shape(e.node_features)[0]) for e in encodings]
    return (n_list, np.concatenate([np.asarray(e.node_features, np.float64) for e in encodings]),
            np.concatenate([np.asarray(e.adjacency_matrix, np.float64).reshape(-1) for e in encodings]),
            np.concatenate([np.asarray(e.distance_matrix, np.float64).reshape(-1) for e in encodings]))


class Encoding:
    """A MATEncoding stand-in for synthetic molecules."""

    def __init__(self, node_features, adjacency_matrix, distance_matrix):
        self.node_features, self.adjacency_matrix, self.distance_matrix = node_features, adjacency_matrix, distance_matrix


def synthetic_molecule(n_real, rng, n_features=36):
    """A random tree of ``n_real`` atoms plus the dummy node, as the featurizer lays a molecule out: one-hot-like 0/1
    node rows without an all-zero row, symmetric adjacency, bond-count distances, dummy row / column 1e6 and 0."""
    n = n_real + 1
    node = np.zeros((n, n_features))
    node[0, 0] = 1.0
    adj = np.zeros((n, n))
    dist = np.full((n, n), 1e6)
    parent = [-1] + [int(rng.randint(0, k)) for k in range(1, n_real)]
    d = np.zeros((n_real, n_real))
    for k in range(1, n_real):
        adj[k + 1, parent[k] + 1] = adj[parent[k] + 1, k + 1] = 1.0
        d[k, :k] = d[parent[k], :k] + 1
        d[:k, k] = d[k, :k]
    dist[1:, 1:] = d
    for k in range(n_real):
        node[k + 1, 1 + rng.randint(0, 11)] = 1.0
        node[k + 1, 12 + rng.randint(0, 6)] = 1.0
        node[k + 1, 34 + rng.randint(0, 2)] = float(rng.randint(0, 2))
    return Encoding(node, adj, dist)


FIXTURE_SIZES = [1, 3, 7, 12, 5, 30, 2, 18, 9, 24, 4, 15, 27, 6, 11, 20, 8, 13, 22, 10]  # real atoms (the dummy node adds one)


def fixture_molecules():
    """The 20 molecules of tests/golden/mat_model.npz, regenerated from their seed."""
    rng = np.random.RandomState(2024)
    return [synthetic_molecule(n, rng) for n in FIXTURE_SIZES]


def fixture_dataset(dc, model_npz):
    mols = fixture_molecules()
    X = np.empty(len(mols), dtype=object)
    X[:] = mols
    return dc.data.NumpyDataset(X, model_npz["y"], model_npz["w"])
