"""No GPU: the helpers that tests/test_gpu_lcnn_edges.py, test_gpu_acnn_edges.py and test_gpu_cgcnn_edges.py rest on.

* The op-level LCNN restatements put together are the block: ``site_fwd_ref`` behind the product equals
  ``lcnn_refs.block`` in float64 to 1e-12, ``running_ref`` (the literal loop) equals the running statistics ``block``
  leaves (its closed form), and ``site_bwd_ref`` / ``rev_sum_ref`` chained give the block's gradient of Y.
* The condition on the op-level inputs: for every tensor of every case the errors of the two float32 slot orders lie
  within 4 times of each other, so ``e32`` is no coin toss.
* The tiled builders give valid ``LcBatch`` / ``GnGraph`` inputs with the stated counts.
* The 32-type AtomConv case uses every slot of the table, the padding type and a type in no slot.
"""
import numpy as np
import pytest
import torch

from tests import lcnn_refs as R
from tests import test_gpu_acnn_edges as A
from tests import test_gpu_cgcnn_edges as C
from tests import test_gpu_lcnn_edges as L
from tests.test_gpu_cgcnn import kernel_case
from tests.test_gpu_lcnn import make_inputs


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("name", ["3x3", "O44"])
def test_op_restatements_put_together_are_the_block(name, training):
    c = make_inputs(name, training)
    dt = torch.float64
    t = {k: torch.tensor(c[k], dtype=dt, requires_grad=True) for k in ("x", "W", "b", "gamma", "beta")}
    st = R.BNState(0, dt, c["rm"], c["rv"])
    want = R.block(t["x"], c["nbr"], t["W"], t["b"], t["gamma"], t["beta"], c["mask"], st, training, "split")
    O, K = c["O"], c["K"]
    Wk = t["W"].view(O, K, -1).permute(1, 0, 2).reshape(K * O, -1)
    Y = (t["x"] @ Wk.t()).detach().requires_grad_(True)
    stats = (None, None) if training else (c["rm"], c["rv"])
    args = (Y, c["nbr"], c["b"], c["gamma"], c["beta"], c["mask"]) + stats + (R.EPS,)
    out, X = R.site_fwd_ref(*args, dt)
    assert float((out - want).detach().abs().max()) <= 1e-12
    if training:
        rm, rv = R.running_ref(X, c["rm"], c["rv"], R.MOMENTUM, dt)
        assert float((rm - st.mean).abs().max()) <= 1e-12 and float((rv - st.var).abs().max()) <= 1e-12
    # the backward ops chained: the gradient of Y, and the parameter gradients of the block
    cot = torch.tensor(c["cot"], dtype=dt)
    dY_want, = torch.autograd.grad((out * cot).sum(), [Y], retain_graph=True)
    dX, dgamma, dbeta, db = R.site_bwd_ref(*args, c["cot"], dt)
    assert float((R.rev_sum_ref(dX, c["nbr"], dt) - dY_want).abs().max()) <= 1e-12
    g = torch.autograd.grad((want * cot).sum(), [t["gamma"], t["beta"], t["b"]])
    for got, w in zip((dgamma, dbeta, db), g):
        assert float((got - w).abs().max()) <= 1e-11 * max(1.0, float(w.abs().max()))


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("O,P,K,n", L.OP_CASES)
def test_the_two_slot_orders_lie_within_4_of_each_other(O, P, K, n, training):
    c = R.op_case(O, P, K, n, training)
    want, e32, spread = R.op_references(c)
    print("O%d P%d K%d n%d: spread %.2f" % (O, P, K, n, spread))
    assert spread <= 4.0
    assert all(np.all(np.isfinite(want[k])) for k in want)
    assert c["nbr"].shape == (n, P, K) and c["Y"].shape == (n, K * O)


def test_running_rows_are_what_the_docstring_says():
    for n in L.CUT_SITES:
        x = L.running_rows(n, True)
        assert x.shape == (n, 6, 19) and np.all(np.isfinite(x.astype(np.float32) ** 2))
        assert np.abs(x[:n - L.LOUD_FROM]).max() > 1e12 and np.abs(x[n - L.LOUD_FROM:]).max() < 10
        rm0, rv0 = L.running_start(n)
        assert np.abs(rm0).max() == np.float32(1e30) and rv0.max() == np.float32(1e30) and rv0.min() > 0
        for m in L.MOMENTA:  # the float64 loop and the closed form agree: the loop is the reference, not a third thing
            rm, rv = R.running_ref(x, rm0, rv0, m, torch.float64)
            xs = torch.as_tensor(x, dtype=torch.float64)
            closed = R.running_closed(xs.mean(1), rm0, m)
            assert float((rm - closed).abs().max()) <= 1e-9 * float(closed.abs().max())


def test_tiled_lattice_batch():
    c = R.op_case(*L.TILED_CASE, True)
    b = L.tiled_batch(c, L.COPIES, "cpu")
    n, P, K = c["N"], c["P"], c["K"]
    assert (b.n_sites, b.n_graphs, b.P, b.K) == (36873, L.COPIES, 2, 8)
    assert -(-b.n_sites // (256 // c["O"])) == 9219 and -(-b.n_sites * K // (256 // c["O"])) == 73746
    nbr = b.nbr.numpy().reshape(L.COPIES, n, P, K)
    for i in range(L.COPIES):
        assert np.array_equal(nbr[i], c["nbr"] + i * n)
    assert np.array_equal(b.node_ptr.numpy(), np.arange(L.COPIES + 1) * n)
    ptr, row = b.rev_ptr.numpy(), b.rev_row.numpy()
    assert ptr[-1] == b.n_sites * P * K and np.all(np.diff(ptr) >= 0)
    # every reverse list names the rows that list its owner in its slot
    flat = b.nbr.numpy().reshape(-1, K)
    for u, j in ((0, 0), (n - 1, K - 1), (n, 0), (b.n_sites - 1, 3)):
        mine = row[ptr[u * K + j]:ptr[u * K + j + 1]]
        assert np.array_equal(mine, np.flatnonzero(flat[:, j] == u))


def test_tiled_crystal_batch():
    c = kernel_case("tile", 128, False)
    assert (c["batch"].size, c["ei"].shape[1], c["G"]) == (2731, 4099, 1)
    g = C.tiled_graph(c, C.TILE_COPIES, "cpu")
    assert (g.n_nodes, g.n_edges, g.n_graphs, g.undirected) == (68275, 102475, C.TILE_COPIES, False)
    h = g.host
    assert np.array_equal(h["node_ptr"], np.arange(C.TILE_COPIES + 1) * 2731)
    assert np.array_equal(h["edge_ptr"], np.arange(C.TILE_COPIES + 1) * 4099)
    assert np.array_equal(h["src"][4099:8198], c["ei"][0] + 2731) and np.array_equal(h["dst"][-4099:], c["ei"][1] + 24 * 2731)
    assert np.diff(h["inc_ptr"]).min() >= 1  # (a cycle through every node: no empty arriving list)
    cap = kernel_case("cap", 128, True)
    assert (cap["batch"].size, cap["ei"].shape[1]) == (8200, 8300)


def test_the_32_type_case_uses_every_slot():
    X, nbrs, Z, params, types, cot = A.case_inputs(*A.FULL_TABLE_CASE)
    assert len(types) == 32 and len(set(np.float32(t) for t in types)) == 32 and {-1.0, 0.5, 118.0} <= set(types)
    assert len(params) == 64 and cot.shape == (2, 3, 2048)
    for t in types:
        assert np.any(Z == np.float32(t)), t
    assert np.any(Z == 0) and np.any(Z == A.FOREIGN) and A.FOREIGN not in types
    assert len(A.KINDS["table33"]) == 33 and len(set(A.KINDS["table33"])) == 33
