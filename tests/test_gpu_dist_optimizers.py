"""Data parallel under the other optimizers: two ranks over gloo on one GPU (started the way tests/test_gpu_dist.py
starts its workers), three steps of 8 + 8 molecules.  Both ranks hold bit-identical parameters afterwards -- for Lamb
that is the determinism of its norms: the same all-reduced gradient, the same reduction tree -- and those lie within
1e-4 (of each tensor's scale) of a single process stepping on the concatenated batches, the bound of the Adam case in
tests/test_gpu_dist.py.  One case runs AdamW under ``shard_model(sync_batchnorm=True)``."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

COMMON = r'''
def optimizer(name):
    import deepchem_amd as dc
    O = dc.models.optimizers
    return {"Lamb": lambda: O.Lamb(1e-3), "RMSProp": lambda: O.RMSProp(1e-3), "AdamW": lambda: O.AdamW(1e-3)}[name]()

def data():
    from deepchem_amd.utils.synthetic import synthetic_labels, synthetic_molecules
    n, T = 48, 3
    packed = synthetic_molecules(n, seed=31, max_atoms=30)
    y, w = synthetic_labels(n, T, "classification", 31, pos_rate=0.4)
    return n, T, packed, y, w
'''

WORKER = r'''
import os, sys
import numpy as np
import torch
import torch.distributed as dist
sys.path.insert(0, %(root)r)
rank, out_dir, name, sync_bn = int(os.environ["RANK"]), sys.argv[1], sys.argv[2], sys.argv[3] == "1"
dist.init_process_group("gloo")
torch.cuda.set_device(0)
import deepchem_amd as dc
from deepchem_amd.dist import shard_model
exec(open(os.path.join(out_dir, "common.py")).read())
dc.set_gemm_mode("exact")
n, T, packed, y, w = data()
# global batch k = molecules [16 k, 16 k + 16): rank r takes its half of every global batch
idx = np.concatenate([np.arange(16 * k + 8 * rank, 16 * k + 8 * rank + 8) for k in range(n // 16)])
torch.manual_seed(70 + rank)  # different initial weights per rank: the broadcast must fix that
model = dc.models.torch_models.GraphConvModel(T, number_input_features=[75, 64], batch_size=8, batch_normalize=sync_bn,
                                              grad_mode="full", optimizer=optimizer(name),
                                              device=torch.device("cuda:0"), log_frequency=1)
shard_model(model, sync_batchnorm=sync_bn)
before = {k: v.detach().cpu().clone() for k, v in model.model.state_dict().items()}
losses = []
model.fit(dc.data.PackedDataset(packed.select(idx), y[idx], w[idx]), nb_epoch=1, deterministic=True,
          checkpoint_interval=0, all_losses=losses)
from deepchem_amd.models.optimizers import FlatOptimizer
assert isinstance(model._pytorch_optimizer, FlatOptimizer)
assert model.model.__dict__.get("_native") is not None, "the native step did not run"
engine_ran = model.__dict__.get("_small") is not None
assert engine_ran == (name == "RMSProp"), "wrong path"  # Lamb and synchronised BatchNorm: the per-batch native step
torch.cuda.synchronize()
torch.save({"before": before, "after": {k: v.detach().cpu() for k, v in model.model.state_dict().items()},
            "losses": losses, "steps": model.get_global_step()}, os.path.join(out_dir, "rank%%d.pt" %% rank))
dist.barrier()
dist.destroy_process_group()
'''


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.mark.timeout(600)
@pytest.mark.parametrize("name,sync_bn", [("Lamb", False), ("RMSProp", False), ("AdamW", True)])
def test_two_ranks_hold_identical_parameters_and_follow_the_single_process_run(tmp_path, name, sync_bn):
    import deepchem_amd as dc
    (tmp_path / "common.py").write_text(COMMON)
    script = tmp_path / "worker.py"
    script.write_text(WORKER % {"root": ROOT})
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
           "127.0.0.1", "--master-port", str(_free_port()), str(script), str(tmp_path), name, "1" if sync_bn else "0"]
    done = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=500)
    assert done.returncode == 0, done.stdout[-2000:] + done.stderr[-4000:]
    r0 = torch.load(str(tmp_path / "rank0.pt"), weights_only=False)
    r1 = torch.load(str(tmp_path / "rank1.pt"), weights_only=False)
    assert r0["steps"] == r1["steps"] == 3
    for k in r0["before"]:
        assert torch.equal(r0["before"][k], r1["before"][k]), k
        assert torch.equal(r0["after"][k], r1["after"][k]), k
    ns = {}
    exec(COMMON, ns)
    n, T, packed, y, w = ns["data"]()
    dc.set_gemm_mode("exact")
    try:
        model = dc.models.torch_models.GraphConvModel(T, number_input_features=[75, 64], batch_size=16,
                                                      batch_normalize=sync_bn, grad_mode="full",
                                                      optimizer=ns["optimizer"](name), device=torch.device("cuda:0"),
                                                      log_frequency=1)
        model.model.load_state_dict({k: v.clone() for k, v in r0["before"].items()})
        losses = []
        model.fit(dc.data.PackedDataset(packed, y, w), nb_epoch=1, deterministic=True, checkpoint_interval=0,
                  all_losses=losses)
    finally:
        dc.set_gemm_mode("fast")
    assert model.get_global_step() == 3
    both = 0.5 * (np.array(r0["losses"]) + np.array(r1["losses"]))
    print("%s: losses of the ranks (mean) %s, single process %s" % (name, both, losses))
    assert np.allclose(both, np.array(losses), rtol=2e-4, atol=1e-6), (both, losses)
    worst, changed = 0.0, 0
    for k, v in model.model.state_dict().items():
        if not v.is_floating_point():
            continue
        a, b = r0["after"][k].double(), v.detach().cpu().double()
        rel = float((a - b).abs().max()) / max(float(b.abs().max()), 1e-3)
        worst = max(worst, rel)
        changed += int(not torch.equal(r0["before"][k], r0["after"][k]))
        assert rel <= 1e-4, (k, rel)
    print("%s: largest difference to the single-process run, relative to the tensor's scale: %.3g" % (name, worst))
    assert changed >= 30
