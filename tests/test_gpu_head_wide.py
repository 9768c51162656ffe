"""The task head with 33..256 outputs on the matrix cores (csrc/head_bwd.hip: head_fwd_wide_kernel,
head_bwd_wide_kernel, head_wgrad_wide_kernel) at the shapes its indexing has to survive: outputs that are no multiple
of 16 or 32, a last tile of fewer than 32 molecules, one output per task (regression), three classes per task (the
general loss loop), more tasks than one round of the loss phase covers, and one output beyond what the kernels take
(the former launches must still be right).  Each case: loss, logits, fingerprint and every gradient of the complete
backward against the float32 and float64 oracles (tests/test_gpu_scale.py:_check; nothing flips at these sizes, so the
bound is the plain 1e-4)."""
import numpy as np
import pytest
import torch

from tests.test_gpu_scale import _check, _native_step, _oracle_step

pytestmark = pytest.mark.gpu

CASES = [
    # mode, tasks, classes, molecules, seed of the molecules
    # (seeds: no dense pre-activation within 3e-6 of zero in the float64 oracle.  With seed 95 the first case has one
    # at -5e-7 of a typical 0.76: the default kernels keep it negative like the oracle, the separate-launch forward --
    # GCMI_FUSED_FWD=0, exact mode -- rounds it positive, its ReLU passes a gradient and one column of dense.weight is
    # 2e-3 off: a flipped route as in tests/test_gpu_scale.py, not an error of either)
    ("classification", 20, 2, 75, 98),    # 40 outputs: padded to 48 columns; 75 = 2 x 32 + 11 molecules
    ("classification", 100, 2, 40, 140),  # 200 outputs
    ("classification", 128, 2, 33, 161),  # 256 outputs: the most; a last tile of one molecule
    ("classification", 15, 3, 50, 65),    # 45 outputs, three classes: the general loss loop
    ("regression", 33, 1, 50, 83),        # one output per task, odd count
    ("regression", 200, 1, 37, 237),      # more tasks than one round of the loss phase (128)
    ("classification", 130, 2, 40, 170),  # 260 outputs: beyond the kernels, the separate launches
]


def _head_case(mode, tasks, classes, n, seed):
    """Molecules, labels, weights and the initial state of one case."""
    from oracle import graphconv_oracle as O
    from deepchem_amd.utils.synthetic import synthetic_labels, synthetic_molecules
    packed = synthetic_molecules(n, seed=seed, max_atoms=40)
    rng = np.random.RandomState(tasks)
    if mode == "classification":
        y = rng.randint(0, classes, size=(n, tasks)).astype(np.float64)
        w = (rng.rand(n, tasks) < 0.9).astype(np.float64) * (0.5 + rng.rand(n, tasks))
    else:
        y, w = synthetic_labels(n, tasks, "regression", tasks)
    cfg = O.ModelConfig(tasks, mode=mode, n_classes=classes, batch_size=n)
    return packed, y, w, O.init_state(cfg, 9)


def _check_against_oracle(native, packed, y, w, tasks, state, mode, classes):
    kw = dict(mode=mode, n_classes=classes)

    def outs(o):  # _check reads outs[1] (outputs) and outs[2] (fingerprint)
        return o if mode == "classification" else (o[0], [None, o[1][0], o[1][1]], o[2], o[3])
    checked, report = _check(native, outs(_oracle_step(packed, y, w, tasks, "full", state, **kw)),
                             outs(_oracle_step(packed, y, w, tasks, "full", state, double=True, **kw)))
    assert checked > 40


def wide_head_meets_the_oracle(mode, tasks, classes, n, seed):
    packed, y, w, state = _head_case(mode, tasks, classes, n, seed)
    native = _native_step(packed, y, w, tasks, "full", state, mode=mode, n_classes=classes)
    _check_against_oracle(native, packed, y, w, tasks, state, mode, classes)


@pytest.mark.parametrize("mode,tasks,classes,n,seed", CASES)
def test_wide_head_meets_the_oracle(mode, tasks, classes, n, seed):
    wide_head_meets_the_oracle(mode, tasks, classes, n, seed)


@pytest.mark.parametrize("switch,cases", [
    # the forward declines the wide kernels below the minimum: the backward must not read the images it did not build
    ("GCMI_HEAD_WIDE_MIN=64", [CASES[0], CASES[4]]),
    # the wide kernels below 33 outputs
    ("GCMI_HEAD_WIDE_MIN=16", [("classification", 12, 2, 75, 98)]),
    # the wide kernels off: the separate launches above 32 outputs
    ("GCMI_HEAD_WIDE=0", [CASES[0]]),
])
def test_wide_head_switches_meet_the_oracle(switch, cases):
    """The switches are read once per process: each runs in a child of its own (one GPU process at a time)."""
    import os
    import subprocess
    import sys
    code = ("from tests.test_gpu_head_wide import wide_head_meets_the_oracle\n"
            "for c in %r:\n    wide_head_meets_the_oracle(*c)\nprint('ok')\n" % (cases,))
    name, value = switch.split("=")
    env = dict(os.environ)
    env.pop("GCMI_HEAD_WIDE_MIN", None)
    env.pop("GCMI_HEAD_WIDE", None)
    env[name] = value
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300,
                         cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert out.returncode == 0 and "ok" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]


def test_wide_head_backward_after_a_product_mode_switch():
    """The head matrix's fragment images are made by a fast-mode forward; the weights then change in place, an
    exact-mode forward (which makes no images) runs on them, and the backward runs in fast mode.  It must use the
    weights it is given, not the images of the earlier ones."""
    import deepchem_amd as dc
    from deepchem_amd.data.collate import collate_to_device
    from deepchem_amd.metrics import to_one_hot
    mode, tasks, classes, n, seed = CASES[0]
    packed, y, w, state = _head_case(mode, tasks, classes, n, seed)
    w2 = state["reshape_dense.weight"].flip(0) * 1.5  # W2: other values, the same scale
    state2 = dict(state, **{"reshape_dense.weight": w2.clone()})
    dev = torch.device("cuda:0")
    dbatch = collate_to_device(packed, None, dev)
    labels = torch.as_tensor(to_one_hot(y.flatten(), classes).reshape(-1, tasks, classes).astype(np.float32), device=dev)
    weights = torch.as_tensor(w.astype(np.float32), device=dev)
    model = dc.models.torch_models.GraphConvModel(tasks, number_input_features=[75, 64], mode=mode, n_classes=classes,
                                                  batch_size=n, grad_mode="full", device=dev)
    model.model.load_state_dict({k: v.clone() for k, v in state.items()})
    native = model.model._native_net()
    g = dbatch.graph
    g.set_mols(n)
    off = native.offsets["reshape_dense.weight"]
    try:
        dc.set_gemm_mode("fast")
        model.model.eval()
        native.forward(dbatch.atom_features, g, False, want_probs=False)  # makes the images of W1
        native.flat[off:off + w2.numel()].copy_(w2.reshape(-1).to(dev))
        model.model.train()
        dc.set_gemm_mode("exact")
        logits, _, fp = native.forward(dbatch.atom_features, g, True, want_probs=False)
        dc.set_gemm_mode("fast")
        loss = native.loss_backward(labels, weights, n)
        torch.cuda.synchronize()
    finally:
        dc.set_gemm_mode("fast")
    names = [k for k, _ in model.model.named_parameters()]
    native_out = (float(loss), logits.cpu(), fp.cpu(), native.grad_flat.clone().cpu(), list(zip(names, native._slices)),
                  native.grad_range, None, g)
    _check_against_oracle(native_out, packed, y, w, tasks, state2, mode, classes)


@pytest.mark.parametrize("rows,n_out,with_scratch", [(100, 24, True), (75, 40, True), (8192, 256, True), (333, 256, False),
                                                     (64, 200, True)])
def test_task_head_forward_op(rows, n_out, with_scratch):
    """gcmi_task_head_forward (prepared images with a scratch, the segmented product without, or up to 32 outputs)
    against the float64 product: 1e-5 of the output's scale (fp32-accurate split products)."""
    from deepchem_amd import ops
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(rows + n_out)
    a = torch.randn((rows, 256), generator=gen)
    w = torch.randn((n_out, 256), generator=gen) * 0.1
    b = torch.randn(n_out, generator=gen)
    scratch = torch.empty(ops.task_head_scratch_floats(), dtype=torch.float32, device=dev) if with_scratch else None
    out = ops.task_head_forward(a.to(dev), w.to(dev), b.to(dev), scratch)
    ref = a.double() @ w.double().T + b.double()
    err = float((out.cpu().double() - ref).abs().max()) / float(ref.abs().max())
    assert out.shape == (rows, n_out) and err <= 1e-5, err
