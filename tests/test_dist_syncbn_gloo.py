"""The host side of synchronised BatchNorm on CPU: ``shard_model(..., sync_batchnorm=...)`` accepts the keyword and
refuses what the native step cannot synchronise, the statistics exchanger sums a float64 buffer over a world-2 gloo
group, and the header declares the two ``_dp`` entry points with the callback type."""
import inspect
import os
import re
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from deepchem_amd.dist import StatAllReduce, shard_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


class _Holder:
    """The attributes shard_model touches on a TorchModel, around a module without a native step."""

    def __init__(self, module):
        self.model = module
        self._grad_sync = None


def _worker(rank, world, port, tmp):
    import deepchem_amd as dc
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        # the default: today's behaviour, no exchanger
        plain = _Holder(torch.nn.Linear(4, 2))
        shard_model(plain)
        assert plain._stat_sync is None
        shard_model(plain, sync_batchnorm=False)
        assert plain._stat_sync is None
        # a model without a native step
        with pytest.raises(ValueError, match="no native training step"):
            shard_model(_Holder(torch.nn.Linear(4, 2)), sync_batchnorm=True)
        cpu = torch.device("cpu")
        # nothing to synchronise
        no_bn = dc.models.torch_models.GraphConvModel(3, number_input_features=[75, 64], batch_size=8,
                                                      batch_normalize=False, device=cpu)
        with pytest.raises(ValueError, match="no BatchNorm"):
            shard_model(no_bn, sync_batchnorm=True)
        assert getattr(no_bn, "_stat_sync", None) is None and no_bn._grad_sync is None  # refused before anything was set
        # the uncertainty head trains through autograd
        unc = dc.models.torch_models.GraphConvModel(3, number_input_features=[75, 64], batch_size=8, mode="regression",
                                                    uncertainty=True, dropout=0.1, device=cpu)
        with pytest.raises(ValueError, match="uncertainty"):
            shard_model(unc, sync_batchnorm=True)
        # non-standard BatchNorm
        odd = dc.models.torch_models.GraphConvModel(3, number_input_features=[75, 64], batch_size=8, device=cpu)
        odd.model.batch_norms[1] = torch.nn.BatchNorm1d(64, affine=False)
        with pytest.raises(ValueError, match="non-standard BatchNorm"):
            shard_model(odd, sync_batchnorm=True)
        # the default model is accepted and gets the exchanger
        model = dc.models.torch_models.GraphConvModel(3, number_input_features=[75, 64], batch_size=8, device=cpu)
        shard_model(model, sync_batchnorm=True)
        ex = model._stat_sync
        assert isinstance(ex, StatAllReduce) and ex.world_size == world
        # ... which sums a float64 buffer [sums | row count] over the ranks, in place
        buf = torch.arange(9, dtype=torch.float64) * (rank + 1)
        buf[-1] = 100.0 + rank
        ex.reduce_stats(buf)
        want = torch.arange(9, dtype=torch.float64) * 3
        want[-1] = 201.0
        assert torch.equal(buf, want), buf
        with pytest.raises(ValueError, match="float64"):
            ex.reduce_stats(torch.zeros(4, dtype=torch.float32))
        # a step that cannot run natively raises instead of training with per-rank statistics
        with pytest.raises(RuntimeError, match="cannot be synchronised"):
            model._train_step(None, [None], [None], lambda *a: None, None)
        open(os.path.join(tmp, "ok%d" % rank), "w").close()
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(180)
def test_shard_model_keyword_refusals_and_the_exchanger_on_two_ranks(tmp_path):
    mp.spawn(_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    assert os.path.exists(tmp_path / "ok0") and os.path.exists(tmp_path / "ok1")


def test_shard_model_signature_and_docstring():
    sig = inspect.signature(shard_model)
    assert list(sig.parameters) == ["model", "group", "sync_batchnorm"]
    assert sig.parameters["sync_batchnorm"].default is False
    assert "small-batch engine" in shard_model.__doc__


def test_exchanger_of_one_rank_is_the_identity():
    buf = torch.arange(5, dtype=torch.float64)
    StatAllReduce(world_size=1).reduce_stats(buf)
    assert torch.equal(buf, torch.arange(5, dtype=torch.float64))


def test_header_declares_the_dp_entry_points():
    text = open(os.path.join(ROOT, "include", "gcmi.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"typedef\s+int\s*\(\*gcmi_stat_sync_fn\)\(void\*\s*ctx,\s*double\*\s*d_buf,\s*int64_t\s+n_doubles,"
                     r"\s*void\*\s*stream\)", code)
    for name in ("gcmi_model_forward_dp", "gcmi_model_loss_backward_dp"):
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\);" % name, code)
        assert m, name
        assert "gcmi_stat_sync_fn sync" in m.group(1) and "void* sync_ctx" in m.group(1), name
    from deepchem_amd import _lib
    for name in ("gcmi_model_forward_dp", "gcmi_model_loss_backward_dp", "gcmi_bn_sync_sums", "gcmi_bn_sync_finalize",
                 "gcmi_bn_sync_bwd_sums", "gcmi_bn_sync_bwd_coef"):
        assert name in _lib.EXPORTS and hasattr(_lib.load(), name), name
