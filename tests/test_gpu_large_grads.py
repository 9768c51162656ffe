"""The large-batch step (csrc/model.hip: gcmi_model_forward / gcmi_model_loss_backward, the step bench.py times) route by
route: every gradient tensor of one step against the float64 oracle at the project's 1e-4, on batches qualified on the
CPU (tests/small_refs.py, DESIGN sections 43 and 46).  The backward walk picks, block by block, between one pass and
separate launches, pooled BatchNorm sums and a pass over dy, the two-stage window pass, the accumulating gather and the
scatter, a one-piece and a three-piece first block, and carries have_psums / dy_ready / acc2 from block to block; the
per-kernel files call the kernels, not the walk.  Here each route is forced by its switch, asserted from the library's
launch counters against what the dispatch predicates say, and every step runs twice on one workspace.

Second run.  Every route accumulates its weight gradients with float atomics across workgroups (bwd_fused.hip,
gemm.hip / gemm_split.hip seg_gemm_wgrad, head_bwd.hip; without reverse slots the GraphPool backward and the scatter
too), so no route is bit-reproducible and bit-equality is asked nowhere; the second run meets the same bound against
float64 and lies within 2e-5 of the first, the bar tests/test_gpu_fused_bwd.py sets for another summation order of the
same arithmetic.

A padded batch run with n_rows = n_real takes the mean of the loss over n_real rows where the zero-weight form (and
the oracle step of tests/small_refs.py) takes it over all B: the same sum over another count, so its reference is the
float64 loss and gradient times B / n_real, exactly; outputs and running statistics are the same."""
import ctypes
import time

import numpy as np
import pytest
import torch

from tests import small_refs as R
from tests.test_gpu_scale import DEV, _device_labels, _native_model, _run_step
from tests.test_gpu_small_grads import _check_buffer, _check_gradient, _check_loss
from tests.test_gpu_width_edges import expected_fused_launches

pytestmark = pytest.mark.gpu

ROUTES = ("default", "three_piece", "separate", "exact", "colsum_stats", "no_rev_slots", "no_windows")
NEEDS_BATCHNORM = ("three_piece", "colsum_stats")  # routes that do not exist on a model without BatchNorm
RERUN_TOL = 2e-5


@pytest.fixture(scope="module", autouse=True)
def _wall_time():
    t0 = time.time()
    yield
    print("\ntests/test_gpu_large_grads.py: %.1f s" % (time.time() - t0))


def _get_option(opt):
    from deepchem_amd import _lib
    v = ctypes.c_int32(0)
    _lib.call("gcmi_get_option", opt, ctypes.byref(v))
    return v.value


def _counters():
    from deepchem_amd import _lib
    return tuple(_get_option(o) for o in (_lib.GCMI_OPT_FUSED_BWD_LAUNCHES, _lib.GCMI_OPT_ONE_PIECE_LAUNCHES,
                                          _lib.GCMI_OPT_MAX_SUM_LAUNCHES))


def _device_batch(packed, y, w, cfg, n_real, route):
    """(features, graph, the collation's small-integer finding) of the whole of ``packed`` as one batch, in the form
    ``route`` wants it."""
    from deepchem_amd.data.collate import collate_to_device
    from deepchem_amd.graph import BatchGraph
    if route == "no_windows":  # the oracle's own layer inputs: no window plan, reverse slots built by the backward
        inputs, _, _ = R.oracle_inputs(packed, y, w, cfg, n_real)
        x = inputs[0].to(torch.float32)
        feats = torch.zeros((x.shape[0], (x.shape[1] + 3) // 4 * 4), dtype=torch.float32)  # 16-byte rows, as collated
        feats[:, :x.shape[1]] = x
        feats = feats.to(DEV)
        g = BatchGraph.from_layer_inputs(inputs[1], inputs[2], list(inputs[4:]), DEV)
        small_int = False
    else:
        dbatch = collate_to_device(packed, None, DEV)
        feats, g, small_int = dbatch.atom_features, dbatch.graph, dbatch.small_int_features
        assert g.c.n_win > 0 and g.rev_pos is not None
        if route == "three_piece":
            g.note_small_int_features(None)
        if route == "no_rev_slots":  # as tests/test_gpu_fused_bwd.py::_step(asymmetric=True)
            g.rev_pos = None
            g.c.d_rev_pos = None
            g.symmetric = False
    g.set_mols(packed.n_mols)
    return feats, g, small_int


def expected_counters(cfg, grad_mode, route, small_int, g):
    """(one-pass backward, one-piece, fused GraphPool + neighbour sum) launches of one step, from the dispatch
    predicates: model.hip block_route / dense_block_one_pass (tests/test_gpu_width_edges.py::expected_fused_launches;
    the dense block's one pass needs BatchNorm), one_piece_block0, gather.hip gcmi_gather_max_sum_fwd."""
    widths, k, bn = tuple(cfg.graph_conv_layers), cfg.number_input_features[0], cfg.batch_normalize
    one_pass_on = route not in ("separate", "exact")
    fused = 0
    if route != "separate":
        fused = expected_fused_launches(k, widths, cfg.dense_layer_size if bn else 0, grad_mode,
                                        "exact" if route == "exact" else "fast")
    one_piece = 0
    if (small_int and route != "three_piece" and one_pass_on and bn and widths[0] == 64 and (k + 3) // 4 * 4 == 76
            and g.c.n_win > 0 and g.rev_pos is not None):
        one_piece = 2 if grad_mode == "full" else 1  # the forward product, and the backward when the block trains
    max_sum = sum(wd in (64, 128) for wd in widths[:-1]) if g.c.n_win > g.c.n_win_big else 0
    return fused, one_piece, max_sum


def _large_step(inputs, grad_mode, route="default", n_rows=None, net=None, runs=2):
    """``runs`` training steps (forward + loss + backward of the whole-model entry points, tests/test_gpu_scale.py
    ::_run_step) from ONE state on one collated batch and one workspace, the route switched as ROUTES says.  Returns
    (net, graph, per run: the tuple of _run_step + num_batches_tracked + the three launch-counter increments)."""
    import deepchem_amd as dc
    from deepchem_amd import _lib
    packed, y, w, cfg, state, n_real = inputs
    n = packed.n_mols
    n_rows = n if n_rows is None else n_rows
    if net is None:
        net = _native_model(n, cfg.n_tasks, grad_mode, state, tuple(cfg.graph_conv_layers), cfg.dense_layer_size, cfg.mode,
                            cfg.n_classes, cfg.number_input_features[0], cfg.batch_normalize)
    model, native = net
    w_b = w.copy()
    w_b[n_real:] = 0
    labels, weights = _device_labels(y[:n_rows], w_b[:n_rows], cfg.n_tasks, cfg.mode, cfg.n_classes)
    feats, g, small_int = _device_batch(packed, y, w, cfg, n_real, route)
    saved = {o: _get_option(o) for o in (_lib.GCMI_OPT_FUSED_BWD, _lib.GCMI_OPT_FUSED_BN_STATS, _lib.GCMI_OPT_GEMM_EXACT)}
    out = []
    try:
        if route == "separate":
            _lib.call("gcmi_set_option", _lib.GCMI_OPT_FUSED_BWD, 0)
        elif route == "colsum_stats":
            _lib.call("gcmi_set_option", _lib.GCMI_OPT_FUSED_BN_STATS, 0)
        elif route == "exact":
            dc.set_gemm_mode("exact")
        for _ in range(runs):
            model.model.load_state_dict({k: v.clone() for k, v in state.items()})
            assert native.views_intact()
            before = _counters()
            step = _run_step(model, native, feats, g, labels, weights, n_rows)
            ran = tuple(a - b for a, b in zip(_counters(), before))
            tracked = [int(bn.num_batches_tracked) for bn in model.model.batch_norms if hasattr(bn, "running_mean")]
            out.append(step + (tracked, ran))
    finally:
        for o, v in saved.items():
            _lib.call("gcmi_set_option", o, v)
    want = expected_counters(cfg, grad_mode, route, small_int, g)
    for step in out:
        assert step[-1] == want, (route, "launch counters (one pass, one piece, max + sum)", step[-1], want)
    if route == "no_windows":
        assert g.c.n_win == 0
    return net, g, out


def _scaled(ref, factor):
    return R.Reference(ref.loss * factor, ref.outs, {k: (None if v is None else v * factor) for k, v in ref.grads.items()},
                       ref.state)


def _check_step(what, step, net, inputs, grad_mode, refs, factor=1.0):
    """One step against its float64 reference: everything the module docstring and DESIGN section 46 list."""
    model, native = net
    packed, y, w, cfg, state, n_real = inputs
    r64, r32 = (_scaled(r, factor) for r in refs) if factor != 1.0 else refs
    loss, logits, fp, grads, slices, (lo, hi), stats, _, tracked, ran = step
    L, bn = native.n_layers, cfg.batch_normalize
    assert lo == (0 if grad_mode == "full" else native.offsets["batch_norms.%d.weight" % (L - 1) if bn else "dense.weight"])
    assert hi == int(native.desc.n_params)
    ratio = _check_gradient(what, grads[lo:hi], lo, hi, slices, r64, r32)
    _check_loss(what, loss, r64)
    ref_logits, ref_fp = (r64.outs[1], r64.outs[2]) if cfg.mode == "classification" else (r64.outs[0], r64.outs[1])
    B = packed.n_mols
    e_lo = float((logits.double().reshape(B, -1) - ref_logits.reshape(B, -1)).abs().max()) / max(float(ref_logits.abs().max()), 1.0)
    e_fp = float((fp.double() - ref_fp).abs().max()) / max(float(ref_fp.abs().max()), 1.0)
    assert e_lo <= 1e-4 and e_fp <= 1e-4, (what, e_lo, e_fp)
    assert len(stats) == (L + 1 if bn else 0) and tracked == [1] * len(stats), (what, tracked)
    for i, (rm, rv) in enumerate(stats):  # r64.state: (1 - m) start + m batch, in float64
        _check_buffer("batch_norms.%d.running_mean" % i, rm.numpy(), r64.state["batch_norms.%d.running_mean" % i].numpy())
        _check_buffer("batch_norms.%d.running_var" % i, rv.numpy(), r64.state["batch_norms.%d.running_var" % i].numpy())
    return ratio


def _check_rerun(what, first, second):
    """The second run on the same workspace against the first: 2e-5 of each tensor's scale, zeros stay zeros."""
    g1, g2, (lo, hi) = first[3].double().numpy(), second[3].double().numpy(), first[5]
    assert second[5] == (lo, hi)
    worst = (0.0, None)
    for name, (off, cnt) in first[4]:
        if not (lo <= off and off + cnt <= hi):
            continue
        a, b = g1[off:off + cnt], g2[off:off + cnt]
        d = float(np.abs(a - b).max() / max(np.abs(a).max(), 1e-6))
        if not a.any():
            assert not b.any(), (what, name)
        if d >= worst[0]:
            worst = (d, name)
    print("%s: second run within %.2e of the first (%s)" % (what, worst[0], worst[1]))
    assert worst[0] <= RERUN_TOL, (what, worst)
    assert abs(first[0] - second[0]) <= 1e-6 * max(abs(first[0]), 1.0)


def _case(model_id, kind):
    return next(c for c in R.LARGE_CASES if (c.model, c.kind) == (model_id, kind))


def _run_and_check(case, grad_mode, route, n_rows=None):
    what = "%s [%s]" % (R.case_id(case, grad_mode), route if n_rows is None else route + ", n_rows = n_real")
    inputs = R.case_inputs(case.model, case.kind, case.seed)
    refs = R.references(case.model, case.kind, case.seed, grad_mode)
    factor = 1.0 if n_rows is None else inputs[0].n_mols / float(n_rows)
    net, g, steps = _large_step(inputs, grad_mode, route, n_rows=n_rows)
    for i, step in enumerate(steps):
        _check_step("%s run %d" % (what, i + 1), step, net, inputs, grad_mode, refs, factor)
    _check_rerun(what, steps[0], steps[1])
    return g, steps


SHAPES = [(c, g) for c in R.LARGE_CASES for g in c.modes]


@pytest.mark.parametrize("case,grad_mode", SHAPES, ids=[R.case_id(c, g) for c, g in SHAPES])
def test_default_route_against_the_float64_oracle(case, grad_mode):
    """Every LARGE_CASES entry as collated (a padded batch: all B rows, the tail's weights zero).  The width cases
    assert their one-pass launches from the same predicates: 33..96 one pass for layer 0, 97 the separate launches."""
    g, steps = _run_and_check(case, grad_mode, "default")
    if case.kind.startswith("width"):
        k = int(case.kind[len("width"):])
        assert steps[0][-1][0] == expected_fused_launches(k, (64, 64), 128, grad_mode, "fast")
        assert steps[0][-1][0] == ((3 if k <= 96 else 2) if grad_mode == "full" else 1)
    if (case.model, case.kind) in (("A", "shaped"), ("A", "tiled")):  # small-integer features: the one-piece first block
        assert steps[0][-1][1] == (2 if grad_mode == "full" else 1)
    if case.model == "A":
        assert steps[0][-1][2] == 1  # L - 1
    if case.model == "E":
        assert steps[0][-1] == ((2 if grad_mode == "full" else 0), 0, 3)
    if case.model == "G":  # one pass (and one piece) for GraphConv 0 below two blocks of separate launches
        assert steps[0][-1] == ((1, 2, 1) if grad_mode == "full" else (0, 1, 1))


PADDED = [(c, g) for c in R.LARGE_CASES if c.kind == "padded" for g in c.modes]


@pytest.mark.parametrize("case,grad_mode", PADDED, ids=[R.case_id(c, g) for c, g in PADDED])
def test_padded_batch_with_n_rows_below_the_batch(case, grad_mode):
    """The padded tail cut off by n_rows = n_real instead of zero weights: the same float64 reference, its loss and
    gradient times B / n_real (module docstring)."""
    n_real = R.case_inputs(case.model, case.kind, case.seed)[5]
    assert n_real == 48 - R.PAD
    _run_and_check(case, grad_mode, "default", n_rows=n_real)


ROUTE_BATCHES = [("A", "tiled"), ("A", "shaped"), ("A", "ordinary"), ("E", "tiled"), ("G", "tiled")]
# one-pass backward launches of the default route (full, reference): A the dense block + both GraphConvs; E (no
# BatchNorm, widths 64 / 128 / 64 / 64, dense 64) GraphConvs 0 and 3; G (64 / 128, dense 128 over 128) GraphConv 0 alone
ONE_PASS = {"A": (3, 1), "E": (2, 0), "G": (1, 0)}
ROUTED = [(r, m, k, g) for r in ROUTES[1:] for m, k in ROUTE_BATCHES for g in R.GRAD_MODES
          if R.MODELS[m].bn or r not in NEEDS_BATCHNORM]


@pytest.mark.parametrize("route,model_id,kind,grad_mode", ROUTED, ids=["%s-%s-%s-%s" % t for t in ROUTED])
def test_route_against_the_float64_oracle(route, model_id, kind, grad_mode):
    g, steps = _run_and_check(_case(model_id, kind), grad_mode, route)
    fused, one_piece, max_sum = steps[0][-1]  # (asserted against expected_counters in _large_step; the table of the issue:)
    full = grad_mode == "full"
    if route in ("three_piece", "no_rev_slots", "no_windows"):
        assert one_piece == 0
        assert fused == ONE_PASS[model_id][0 if full else 1]
    if route in ("separate", "exact"):
        assert fused == 0 and one_piece == 0
    assert max_sum == (0 if route == "no_windows" else len(R.MODELS[model_id].widths) - 1)


@pytest.mark.parametrize("grad_mode", R.GRAD_MODES)
def test_three_piece_step_after_a_one_piece_step(grad_mode):
    """One workspace: the one-piece first block leaves S0 and Xb as bf16 rows and a note for the backward; the next
    step, the same batch with the small-integer property withdrawn, must read fp32 rows again."""
    case = _case("A", "tiled")
    inputs = R.case_inputs(case.model, case.kind, case.seed)
    refs = R.references(case.model, case.kind, case.seed, grad_mode)
    net, _, first = _large_step(inputs, grad_mode, "default", runs=1)
    ws = net[1]._ws.data_ptr()
    _, _, second = _large_step(inputs, grad_mode, "three_piece", net=net, runs=1)
    assert net[1]._ws.data_ptr() == ws
    assert first[0][-1][1] == (2 if grad_mode == "full" else 1) and second[0][-1][1] == 0
    what = R.case_id(case, grad_mode)
    _check_step(what + " one-piece step", first[0], net, inputs, grad_mode, refs)
    _check_step(what + " three-piece step after it", second[0], net, inputs, grad_mode, refs)
    _check_rerun(what, first[0], second[0])


@pytest.mark.parametrize("grad_mode", R.GRAD_MODES)
def test_tiled_batch_after_an_ordinary_one(grad_mode):
    """One workspace, a larger batch (about 500 atoms, 34 molecules, no small-integer features) and then a smaller one
    (264 atoms, 97 molecules, one-piece first block), each from its own state against its own float64 reference."""
    big, small = _case("A", "ordinary"), _case("A", "tiled")
    in_big, in_small = (R.case_inputs(c.model, c.kind, c.seed) for c in (big, small))
    assert in_big[0].n_atoms > in_small[0].n_atoms and in_big[0].n_mols < in_small[0].n_mols
    net, _, first = _large_step(in_big, grad_mode, "default", runs=1)
    ws = net[1]._ws.data_ptr()
    _, _, second = _large_step(in_small, grad_mode, "default", net=net, runs=1)
    assert net[1]._ws.data_ptr() == ws, "the second batch must run in the first one's workspace"
    assert first[0][-1][1] == 0 and second[0][-1][1] == (2 if grad_mode == "full" else 1)
    _check_step(R.case_id(big, grad_mode), first[0], net, in_big, grad_mode,
                R.references(big.model, big.kind, big.seed, grad_mode))
    _check_step(R.case_id(small, grad_mode) + " after it", second[0], net, in_small, grad_mode,
                R.references(small.model, small.kind, small.seed, grad_mode))
