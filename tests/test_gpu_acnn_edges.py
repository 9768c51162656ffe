"""The atomic-convolution kernels (csrc/atomconv.hip) at the sizes their launch arithmetic depends on.

Every case goes through ``run_ops`` / ``check_bars`` of tests/test_gpu_acnn.py (the statistics, y and the three filter
gradients under ``bar`` of tests/test_gpu_mat.py: the error against float64 at most 4 times the float32 restatement's,
floor one float32 ulp of the tensor's largest entry) and a second run bit for bit.  A workgroup takes 4 rows (b, n);
ac_bwd leaves one partial row per workgroup of a grid cut to 1024 and ac_bwd_finish gives lane i the partials i, i + 64,
...; the row kernels stride under the 8192 workgroups of ``grid_for``.

Cases (B, N, M, L, types) and what each pins:
* (2, 129, 2, 3, none): 258 rows = 65 partials, the first second partial of a lane of ac_bwd_finish.
* (2, 2049, 2, 3, one): 4098 rows = 1025 row groups: the capped ac_bwd takes a second turn; ac_finish runs on 9
  workgroups (N > 256).
* (2, 16400, 1, 1, none): 32 800 rows = 8200 row groups: the second turn of ac_stats and ac_fwd.
* (2, 5, 12, L, one), L = 127 | 128 | 129: the backward's chunk of 128 filters (gridDim.y 1 | 1 | 2, the second filter
  of a lane missing, full, and a chunk of one filter).
* (2, 5, M, 3, defaults), M = 63 | 64: the LDS arrays of GCMI_AC_MAX_NEIGHBORS = 64 full, no lane takes the
  ``lane >= a.M`` exit.
* (2, 3, 6, 64, 32 types): the full type table, C = 32 * 64 = 2048 exactly.  The table is 32 distinct values including
  -1, 0.5 and 118; Z holds every one of them, 0 (padding) and 200 (in no slot).  M is 6 and not 4: the 34 values need 34
  of the B * N * M entries (tests/test_conv_edge_refs_host.py asserts that every slot occurs).
* the router at the layer: M = 64 native, M = 65 torch; 32 types native, 33 torch; both sides under the bar.

Measured on an MI355X (worst ratio per case, in the order above): 1.07; 3.96 (d re, three numbers; d rs 3.32, the
statistics and y 0.41 to 0.55); 2.98 (d rc); 0.66, 0.79, 1.34; 0.90, 1.30; 0.72; the layer 1.94 (M = 64), 1.00 (M = 65),
1.14 (32 types), 2.88 (33 types).  Worst of the family: 3.96.
"""
import numpy as np
import pytest
import torch

from tests import acnn_refs as R
from tests.test_gpu_acnn import DEV, TYPES, check_bars, layer_on, run_ops

pytestmark = pytest.mark.gpu

TABLE32 = [-1.0, 0.5, 118.0] + [float(v) for v in range(1, 30)]
FOREIGN = 200.0
KINDS = dict(TYPES, table32=TABLE32, table33=TABLE32 + [30.0])
CASES = [(2, 129, 2, 3, "none"), (2, 2049, 2, 3, "one"), (2, 16400, 1, 1, "none"), (2, 5, 12, 127, "one"),
         (2, 5, 12, 128, "one"), (2, 5, 12, 129, "one"), (2, 5, 63, 3, "defaults"), (2, 5, 64, 3, "defaults")]
FULL_TABLE_CASE = (2, 3, 6, 64, "table32")


def case_inputs(B, N, M, L, kind):
    """(X, nbrs, Z, params, types, cot) of a case."""
    rng = np.random.RandomState(B * 100000 + N * 10 + M * 7 + L)
    types = KINDS[kind]
    if kind.startswith("table"):
        X, nbrs, Z = R.random_case(rng, B, N, M, z_values=tuple(types) + (0.0, FOREIGN))
        values = np.asarray(tuple(types) + (0.0, FOREIGN), np.float32)
        flat = Z.reshape(-1)
        flat[rng.permutation(flat.size)[:values.size]] = values  # every slot, the padding and the foreign type occur
    else:
        X, nbrs, Z = R.random_case(rng, B, N, M)
    params = R.random_params(rng, L)
    cot = rng.normal(0, 1, (B, N, max(len(types or ()), 1) * L)).astype(np.float32)
    return X, nbrs, Z, params, types, cot


def check_case(B, N, M, L, kind):
    X, nbrs, Z, params, types, cot = case_inputs(B, N, M, L, kind)
    got = run_ops(X, nbrs, Z, params, types, None, cot)
    check_bars(got, X, nbrs, Z, params, types, None, cot, "B%d N%d M%d L%d %s" % (B, N, M, L, kind))
    again = run_ops(X, nbrs, Z, params, types, None, cot)
    for k in got:
        assert torch.equal(got[k], again[k]), k  # bit for bit


@pytest.mark.parametrize("B,N,M,L,kind", CASES)
def test_kernels_at_the_grid_and_chunk_edges(B, N, M, L, kind):
    check_case(B, N, M, L, kind)


def test_the_full_type_table():
    X, nbrs, Z, params, types, cot = case_inputs(*FULL_TABLE_CASE)
    assert len(set(types)) == 32 and len(types) * len(params) == 2048
    assert all(np.any(Z == np.float32(t)) for t in types) and np.any(Z == 0) and np.any(Z == FOREIGN)
    check_case(*FULL_TABLE_CASE)


def layer_against_the_bar(X, nbrs, Z, params, types, rng, label):
    layer = layer_on(types, params)
    out = layer([X, nbrs, Z])
    cot = rng.normal(0, 1, tuple(out.shape)).astype(np.float32)
    (out * torch.as_tensor(cot, device=DEV)).sum().backward()
    got = dict(y=out, rc=layer.rc.grad.reshape(-1), rs=layer.rs.grad.reshape(-1), re=layer.re.grad.reshape(-1))
    check_bars(got, X, nbrs, Z, params, types, None, cot, label)
    return layer.last_route


def test_the_native_bound_on_the_neighbours():
    """M = 64 is the last neighbour list the kernels hold in LDS; M = 65 lands on the torch route."""
    rng = np.random.RandomState(31)
    params = R.random_params(rng, 3)
    for M, want in ((64, "native"), (65, "torch")):
        X, nbrs, Z = R.random_case(rng, 2, 5, M)
        assert layer_against_the_bar(X, nbrs, Z, params, R.EDGE_TYPES, rng, "M = %d" % M) == want


def test_the_native_bound_on_the_types():
    """32 types fill the kernels' table; 33 land on the torch route."""
    rng = np.random.RandomState(32)
    params = R.random_params(rng, 3)
    for kind, want in (("table32", "native"), ("table33", "torch")):
        types = KINDS[kind]
        X, nbrs, Z = R.random_case(rng, 2, 5, 12, z_values=tuple(types) + (0.0, FOREIGN))
        assert layer_against_the_bar(X, nbrs, Z, params, types, rng, "%d types" % len(types)) == want
