"""A torch-CPU restatement of DTNN (deepchem/models/torch_models/dtnn.py and the three DTNN layers of
torch_models/layers.py of the reference), parametrised by dtype: float32 reproduces the reference's arithmetic graph
op for op, float64 is the yardstick the GPU tests measure against.  ``scatter`` is a sum by index (``index_add_``).

State-dict keys are the reference's, so its parameters load directly into ``DTNNRef``.
"""
import numpy as np
import torch


def gaussians(distance, distance_min, distance_max, n_distance, dtype=torch.float64):
    """exp(-(d - s_k)^2 / (2 step^2)), s_k = distance_min + k step, computed in ``dtype`` from ``distance``."""
    d = torch.as_tensor(distance, dtype=dtype).reshape(-1, 1)
    step = (distance_max - distance_min) / n_distance
    steps = torch.as_tensor(np.array([distance_min + k * step for k in range(n_distance)]), dtype=dtype).reshape(1, -1)
    return torch.exp(-torch.square(d - steps) / (2 * step**2))


def pair_sum(gauss, ah, mem_i, mem_j, W_df, b_df, W_fc, n_atoms):
    """Y[i] = sum_{p: mem_i[p] = i} tanh(((g_p W_df + b_df) * ah[mem_j[p]]) W_fc)."""
    hidden = (gauss @ W_df + b_df) * ah[mem_j]
    out = torch.tanh(hidden @ W_fc)
    return torch.zeros((n_atoms, W_fc.shape[1]), dtype=out.dtype, device=out.device).index_add_(0, mem_i, out)


def step_forward(p, prefix, x, gauss, mem_i, mem_j):
    W_cf, W_df, W_fc = p[prefix + "W_cf"], p[prefix + "W_df"], p[prefix + "W_fc"]
    b_cf, b_df = p[prefix + "b_cf"], p[prefix + "b_df"]
    ah = x @ W_cf + b_cf
    own = torch.tanh((b_df * ah) @ W_fc)
    return pair_sum(gauss, ah, mem_i, mem_j, W_df, b_df, W_fc, x.shape[0]) - own + x


def gather_forward(p, prefix, x, membership, n_mols, output_activation=True):
    n_layers = len([k for k in p if k.startswith(prefix + "W_list.")])
    for k in range(n_layers):
        x = x @ p[prefix + "W_list.%d" % k] + p[prefix + "b_list.%d" % k]
        if k < n_layers - 1 or output_activation:
            x = torch.tanh(x)
    return torch.zeros((n_mols, x.shape[1]), dtype=x.dtype, device=x.device).index_add_(0, membership, x)


class DTNNRef(torch.nn.Module):
    """DTNN with parameters in ``dtype``; ``forward`` takes the five generator arrays (Gaussians included) or, with
    ``distance=`` one value per pair, computes the Gaussians in ``dtype`` itself."""

    def __init__(self, state, dtype, distance_min=-1, distance_max=18, output_activation=True):
        super().__init__()
        self.dtype, self.distance_min, self.distance_max = dtype, distance_min, distance_max
        self.output_activation = output_activation
        self.names = list(state)
        self.params = torch.nn.ParameterList(
            [torch.nn.Parameter(torch.as_tensor(np.asarray(v)).to(dtype).clone()) for v in state.values()])

    def table(self):
        return dict(zip(self.names, self.params))

    def forward(self, inputs, n_mols=None, distance=None):
        p = self.table()
        atom_number, gauss, membership, mem_i, mem_j = inputs
        dev = self.params[0].device  # (CPU in the tests; tools/dtnn_step_time.py moves the module to the GPU)

        def index(a):
            return (a if torch.is_tensor(a) else torch.as_tensor(np.asarray(a))).to(device=dev, dtype=torch.int64)
        atom_number, membership, mem_i, mem_j = index(atom_number), index(membership), index(mem_i), index(mem_j)
        n_distance = p["dtnn_step.0.W_df"].shape[0]
        if distance is not None:
            gauss = gaussians(distance, self.distance_min, self.distance_max, n_distance, self.dtype).to(dev)
        else:
            gauss = (gauss if torch.is_tensor(gauss) else torch.as_tensor(np.asarray(gauss))).to(device=dev, dtype=self.dtype)
        x = p["dtnn_embedding.embedding_list"][atom_number]
        n_steps = len([k for k in p if k.endswith(".W_cf")])
        for s in range(n_steps):
            x = step_forward(p, "dtnn_step.%d." % s, x, gauss, mem_i, mem_j)
        if n_mols is None:
            n_mols = int(membership.max()) + 1
        g = gather_forward(p, "dtnn_gather.", x, membership, n_mols, self.output_activation)
        return g @ p["linear.weight"].t() + p["linear.bias"]


def l2_loss(out, y, w):
    """TorchModel's _StandardLoss over L2Loss: mean(w * (out - y)^2)."""
    y = (y if torch.is_tensor(y) else torch.as_tensor(np.asarray(y))).to(device=out.device, dtype=out.dtype).reshape(out.shape)
    w = (w if torch.is_tensor(w) else torch.as_tensor(np.asarray(w))).to(device=out.device, dtype=out.dtype).reshape(out.shape)
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


def rel_err(got, want):
    """max |got - want| relative to the largest entry of ``want`` (at least tiny, so that an all-zero tensor compares)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.max(np.abs(got - want)) / max(float(np.max(np.abs(want))), 1e-30)) if want.size else 0.0
