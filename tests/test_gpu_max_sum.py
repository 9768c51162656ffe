"""GraphPool and the neighbour sum of the block above in one window pass (gather_lds.hip, MaxSumOp): exactly
`ops.gather_max` followed by `ops.gather_sum`.  Both stages call the loops the separate kernels call, on the same
values in the same order, so every comparison here is `torch.equal` -- pooled rows, arg bytes and neighbour sums."""
import functools

import numpy as np
import pytest
import torch

from deepchem_amd.utils.synthetic import concat_packed, single_atom_and_edge_cases, synthetic_labels, synthetic_molecules

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

# launch_lpr gives the ordinary windows min(n_norm, 256 * per_cu) workgroups, per_cu <= 8 whatever the thread count
# and the LDS size: above 3 * 256 * 8 ordinary windows some workgroup walks three (both buffers and the third tile
# are used again)
MANY_WINDOWS = 3 * 256 * 8
SMALL_CAP = 16


@functools.lru_cache(maxsize=None)
def _packed(case):
    if case == "small":  # degrees 0 and 10 present, a handful of windows: one per workgroup
        return concat_packed([synthetic_molecules(40, seed=3, max_atoms=40), single_atom_and_edge_cases(75, 1)])
    if case == "many_windows":  # molecules of about ten atoms under a cap of 16: nearly a window each
        return concat_packed([synthetic_molecules(10000, seed=4, mean_atoms=10, max_atoms=SMALL_CAP),
                              single_atom_and_edge_cases(75, 1)])
    assert case == "oversized"  # one molecule above the default cap of 96 atoms among ordinary ones
    return concat_packed([synthetic_molecules(30, seed=5, max_atoms=40),
                          synthetic_molecules(1, seed=6, mean_atoms=118, max_atoms=132, min_atoms=100),
                          synthetic_molecules(30, seed=7, max_atoms=40), single_atom_and_edge_cases(75, 1)])


@functools.lru_cache(maxsize=None)
def _batch(case):
    from deepchem_amd.data.collate import collate_to_device
    kw = {"win_cap": SMALL_CAP} if case == "many_windows" else {}
    b = collate_to_device(_packed(case), None, DEV, **kw)
    c = b.graph.c
    assert c.n_win > 0
    deg = np.diff(_packed(case).adj_ptr)
    assert deg.min() == 0 and deg.max() == 10
    if case == "many_windows":
        assert c.n_win_big == 0 and c.n_win > MANY_WINDOWS
    elif case == "oversized":
        assert c.n_win_big == 1 and c.n_win > 1
    else:
        assert c.n_win_big == 0
    return b


def _inputs(n, width, seed=0):
    """Rows with many ties (small integers times a constant), and BatchNorm vectors with both signs."""
    rng = np.random.RandomState(seed)
    y = torch.from_numpy((rng.randint(-3, 4, size=(n, width)) * 0.37).astype(np.float32)).to(DEV)
    sc = torch.from_numpy(rng.standard_normal(width).astype(np.float32)).to(DEV)
    sh = torch.from_numpy(rng.standard_normal(width).astype(np.float32)).to(DEV)
    return y, sc, sh


def _both(g, y, sc, sh, want_arg):
    """(fused results, separate results, launches of the fused kernel)"""
    from deepchem_amd import ops
    before = ops.max_sum_launches()
    fused = ops.gather_max_sum(g, y, sc, sh, want_arg=want_arg)
    ran = ops.max_sum_launches() - before
    pool, arg = ops.gather_max(g, y, sc, sh, want_arg=want_arg)
    return fused, (pool, arg, ops.gather_sum(g, pool)), ran


def _assert_same(fused, separate, want_arg):
    for name, a, b in zip(("pooled rows", "arg bytes", "neighbour sums"), fused, separate):
        if name == "arg bytes" and not want_arg:
            assert a is None and b is None
            continue
        assert torch.equal(a, b), name


@pytest.mark.parametrize("want_arg", [True, False])
@pytest.mark.parametrize("bn", [True, False])
@pytest.mark.parametrize("width", [64, 128])
@pytest.mark.parametrize("case", ["small", "many_windows", "oversized"])
def test_fused_pass_equals_gather_max_then_gather_sum(case, width, bn, want_arg):
    g = _batch(case).graph
    y, sc, sh = _inputs(g.n_atoms, width)
    fused, separate, ran = _both(g, y, sc if bn else None, sh if bn else None, want_arg)
    assert ran == 1  # (oversized: the one big window took the separate ops, the others this kernel)
    _assert_same(fused, separate, want_arg)
    # lone atoms: pooled row = the (normalised) row itself, no neighbours to sum
    n0 = int(g.deg_start[1])
    assert n0 > 0 and not fused[2][:n0].any()


@pytest.mark.parametrize("shape", ["width76", "unaligned"])
def test_refused_shape_takes_the_two_kernels(shape):
    g = _batch("small").graph
    if shape == "width76":
        y, sc, sh = _inputs(g.n_atoms, 76)
    else:  # rows that start 4 bytes off a 16-byte boundary
        wide, sc, sh = _inputs(g.n_atoms, 68)
        y, sc, sh = wide[:, 1:65], sc[:64].contiguous(), sh[:64].contiguous()
        assert y.data_ptr() % 16 != 0
    fused, separate, ran = _both(g, y, sc, sh, True)
    assert ran == 0
    _assert_same(fused, separate, True)


def test_model_forward_runs_the_fused_pass_between_blocks():
    """One training step and one eval forward of GraphConvModel([64, 64], dense 128): the fused kernel runs L - 1 = 1
    time per forward (the last block's GraphPool feeds the dense product and stays a plain one).  Values: the parity
    tests of the model step."""
    import deepchem_amd as dc
    from deepchem_amd import ops
    from deepchem_amd.metrics import to_one_hot
    packed = _packed("small")
    b = _batch("small")
    g = b.graph
    n, tasks = packed.n_mols, 2
    yl, wl = synthetic_labels(n, tasks, "classification", 1, pos_rate=0.3)
    labels = torch.as_tensor(to_one_hot(yl.flatten(), 2).reshape(-1, tasks, 2).astype(np.float32), device=DEV)
    weights = torch.as_tensor(wl.astype(np.float32), device=DEV)
    torch.manual_seed(11)
    model = dc.models.torch_models.GraphConvModel(tasks, graph_conv_layers=[64, 64], dense_layer_size=128,
                                                  number_input_features=[75, 64], batch_size=n, mode="classification",
                                                  grad_mode="full", device=DEV)
    native = model.model._native_net()
    assert native is not None
    g.set_mols(n)
    model.model.train()
    before = ops.max_sum_launches()
    native.forward(b.atom_features, g, True, want_probs=False)
    assert ops.max_sum_launches() - before == 1
    loss = native.loss_backward(labels, weights, n)
    assert np.isfinite(float(loss)) and ops.max_sum_launches() - before == 1
    model.model.eval()
    before = ops.max_sum_launches()
    logits, _, _ = native.forward(b.atom_features, g, False, want_probs=False)
    torch.cuda.synchronize()
    assert ops.max_sum_launches() - before == 1 and bool(torch.isfinite(logits).all())
