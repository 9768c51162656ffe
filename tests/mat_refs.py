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


# ------------------------------------------------------------------------------------------------ edge cases of csrc/mat.hip
# (shared by tests/test_mat_megnet_edge_cases_host.py and tests/test_gpu_mat_edges.py)
MAT_CAP = 128
MAT_NV = (1, 2, 4, 8, 16)  # float4 columns per head the attention kernels are instantiated for
# the largest n_max whose dynamic LDS stays at or below 64 KiB / the one above it, per NV: (forward, backward)
LDS_TABLE = {1: ((119, 120), (119, 120)), 2: ((116, 117), (115, 116)), 4: ((109, 110), (109, 110)),
             8: ((96, 97), (96, 97)), 16: ((76, 77), (76, 77))}
# n_max -> molecule sizes: at least 48 molecules where the molecules are tiny, else the largest plus a few small ones
N_MAX_BATCHES = {1: [1] * 48, 2: [2, 2, 1] * 16, 3: [3, 2, 1, 3] * 12, 63: [2, 63, 1, 5], 64: [63, 1, 64], 65: [65, 2],
                 127: [3, 127, 1]}
BIAS_EDGE_SIZES = [1] * 5 + [63, 64, 65, 127, 1, 2] + [1] * 6


def nv_of(d_k):
    """The instantiation ``dispatch_mat`` picks for ``d_k``."""
    return next(nv for nv in MAT_NV if d_k // 4 <= nv)


def lds_bytes(nv, n_max, bwd):
    """Dynamic LDS of one attention workgroup, from the layout at the top of csrc/mat.hip: two row tiles of
    n_max x (4 NV + 4) floats, the n_max x (n_max | 1) tile and, backward, n_max row sums."""
    return 4 * (2 * n_max * (4 * nv + 4) + n_max * (n_max | 1) + (n_max if bwd else 0))


def lds_boundary(nv, bwd, limit=65536):
    """(the largest n_max whose LDS is at most ``limit``, the one above it)."""
    fits = [n for n in range(1, MAT_CAP + 1) if lds_bytes(nv, n, bwd) <= limit]
    assert fits == list(range(1, fits[-1] + 1)) and fits[-1] < MAT_CAP
    return fits[-1], fits[-1] + 1


_EDGE_CASES = {}


def attention_edge_case(n_list, h, d_k, shared=False, kv_same=False, lam=0.33):
    """Inputs of one attention call on molecules of the sizes ``n_list`` and the float64 / float32 restatements of its
    outputs and gradients, computed once per case.  ``shared``: q = k = v one leaf; ``kv_same``: k and v equal in value
    (two leaves for autograd, so dK and dV stay apart)."""
    key = (tuple(n_list), h, d_k, shared, kv_same, lam)
    if key in _EDGE_CASES:
        return _EDGE_CASES[key]
    rng = np.random.RandomState(1000 * h + 10 * d_k + len(n_list))
    n_list = [int(n) for n in n_list]
    _, _, adj, dist = pack([synthetic_molecule(n - 1, rng) for n in n_list])
    N, W = sum(n_list), h * d_k
    c = {"n_list": n_list, "h": h, "d_k": d_k, "lam": lam, "shared": shared,
         "bias": bias_blocks(adj, dist, n_list, "softmax", 0.33, 0.34, 1e-6, torch.float32).numpy(),
         "q": rng.normal(0, 1, (N, W)).astype(np.float32), "dO": rng.normal(0, 1, (N, W)).astype(np.float32)}
    c["k"] = c["q"] if shared else rng.normal(0, 1, (N, W)).astype(np.float32)
    c["v"] = c["q"] if shared else c["k"] if kv_same else rng.normal(0, 1, (N, W)).astype(np.float32)
    for dtype, name in ((torch.float64, "f64"), (torch.float32, "f32")):
        q = torch.tensor(c["q"], dtype=dtype, requires_grad=True)
        k, v = (q, q) if shared else (torch.tensor(c["k"], dtype=dtype, requires_grad=True),
                                      torch.tensor(c["v"], dtype=dtype, requires_grad=True))
        o = attention(q, k, v, torch.tensor(c["bias"], dtype=dtype), n_list, h, lam)
        o.backward(torch.tensor(c["dO"], dtype=dtype))
        c[name] = {"O": o.detach().numpy(), "dQ": q.grad.numpy()}
        if not shared:
            c[name].update({"dK": k.grad.numpy(), "dV": v.grad.numpy()})
    _EDGE_CASES[key] = c
    return c


def reorder_case(c, order):
    """The inputs of ``c`` with its molecules in ``order`` (no restatement: compared with ``c`` molecule by molecule)."""
    aoff, poff = offsets(c["n_list"])
    rows = np.concatenate([np.arange(aoff[m], aoff[m + 1]) for m in order])
    pairs = np.concatenate([np.arange(poff[m], poff[m + 1]) for m in order])
    out = {k: c[k] for k in ("h", "d_k", "lam", "shared")}
    out["n_list"] = [c["n_list"][m] for m in order]
    out["bias"] = c["bias"][pairs]
    out["q"] = c["q"][rows]
    out["k"], out["v"] = (out["q"], out["q"]) if c["shared"] else (c["k"][rows], c["v"][rows])
    out["dO"] = c["dO"][rows]
    return out, rows


def _dot4(x, y):
    """x (..., d) . y (..., d) as the kernels add it: four running sums over the float4 columns, then (a + b) + (c + d);
    float32, products and sums rounded one by one (no fused multiply-add)."""
    s = [np.zeros(np.broadcast(x[..., 0], y[..., 0]).shape, np.float32) for _ in range(4)]
    for c in range(0, x.shape[-1], 4):
        for i in range(4):
            s[i] = s[i] + x[..., c + i] * y[..., c + i]
    return (s[0] + s[1]) + (s[2] + s[3])


def _comp_add(total, comp, x):
    """``comp_add`` of csrc/mat.hip: total += x with the rounding error of the addition carried in ``comp``."""
    y = x - comp
    t = total + y
    return t, (t - total) - y


def attention_emulation(c, compensated=True):
    """float32 numpy in the kernels' own order (the header comment of csrc/mat.hip): per query row the scores, their
    maximum, the exponentials and their sum, ``lam * e / l + b``, and every sum over atoms accumulated in atom order;
    the two scalar row sums (the softmax denominator and delta) are compensated as in the kernels, or with
    ``compensated=False`` plain running sums.  What float32 gives for that order without fused multiply-add and with
    numpy's ``exp``."""
    f = np.float32
    h, d_k, lam, shared = c["h"], c["d_k"], f(c["lam"]), c["shared"]
    scale = f(1) / np.sqrt(f(d_k))
    c_ds = lam * scale
    aoff, poff = offsets(c["n_list"])
    out = {name: np.zeros_like(c["q"]) for name in (("O", "dQ") if shared else ("O", "dQ", "dK", "dV"))}
    for m, n in enumerate(c["n_list"]):
        B = c["bias"][poff[m]:poff[m + 1]].reshape(n, n)
        for head in range(h):
            blk = (slice(int(aoff[m]), int(aoff[m + 1])), slice(head * d_k, (head + 1) * d_k))
            Q, K, V, G = c["q"][blk], c["k"][blk], c["v"][blk], c["dO"][blk]
            S = np.stack([_dot4(Q, K[j]) * scale for j in range(n)], 1)
            E = np.exp(S - S.max(1, keepdims=True)).astype(f)
            l, comp = np.zeros(n, f), np.zeros(n, f)
            for j in range(n):
                l, comp = _comp_add(l, comp, E[:, j]) if compensated else (l + E[:, j], comp)
            o = np.zeros((n, d_k), f)
            for j in range(n):
                o = o + (lam * (E[:, j] / l) + B[:, j])[:, None] * V[j]
            out["O"][blk] = o
            P = E / l[:, None]
            dP = np.stack([_dot4(G, V[j]) for j in range(n)], 1)
            delta, comp = np.zeros(n, f), np.zeros(n, f)
            for j in range(n):
                delta, comp = _comp_add(delta, comp, P[:, j] * dP[:, j]) if compensated else (delta + P[:, j] * dP[:, j], comp)
            dS = c_ds * P * (dP - delta[:, None])
            dq, dk, dv = np.zeros((n, d_k), f), np.zeros((n, d_k), f), np.zeros((n, d_k), f)
            for j in range(n):
                dq = dq + dS[:, j][:, None] * K[j]
            for i in range(n):
                dk = dk + dS[i][:, None] * Q[i]
                dv = dv + (lam * P[i] + B[i])[:, None] * G[i]
            if shared:
                out["dQ"][blk] = (dq + dk) + dv
            else:
                out["dQ"][blk], out["dK"][blk], out["dV"][blk] = dq, dk, dv
    return out


def bias_edge_case():
    """(n_list, adjacency blocks, distance blocks) of the bias batch: 333 atoms, one past a multiple of the 4 rows a workgroup takes."""
    rng = np.random.RandomState(11)
    n_list, _, adj, dist = pack([synthetic_molecule(n - 1, rng) for n in BIAS_EDGE_SIZES])
    return n_list, adj, dist
