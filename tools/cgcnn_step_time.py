"""Time of one CGCNN training step on the GPU: the native route (``csrc/cgcnn.hip`` between the two products of a layer)
against the torch route (the reference's order: concatenated rows, BatchNorm module, index_add) of the SAME
``CGCNNModel`` on the same GPU and batch.

    python tools/cgcnn_step_time.py [--batches 1024 4096] [--warmup 5] [--steps 30]

The default-width model (in_node_dim 92, hidden 64, in_edge_dim 41, num_conv 3, predictor 128) on crystal-like graphs:
about 20 nodes (at least 4, at most 36), every node with 12 arriving edges from random nodes of its graph (a
multigraph, as the neighbour lists of a crystal are).  Per route: warm-up steps, then the MEDIAN of repeated steps,
Adam included, each ended by a device synchronise; peak memory = ``torch.cuda.max_memory_allocated`` over the timed
steps.  ``*_ms`` builds and uploads the ``CgcnnBatch`` in every step, as ``fit`` does; ``*_uploaded_ms`` reuses an uploaded
batch.  ``build_ms``: the host-side build and upload alone.  One JSON line per batch size.
"""
import argparse
import gc
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NEIGHBOURS = 12


def crystal(rng, Fn=92, Fe=41):
    from deepchem_amd.feat import GraphData
    n = int(np.clip(rng.normal(20, 4.5), 4, 36))
    dst = np.repeat(np.arange(n), NEIGHBOURS)
    src = rng.randint(0, n, dst.size)
    return GraphData(rng.normal(0, 1, (n, Fn)).astype(np.float32), np.stack([src, dst]),
                     rng.normal(0, 1, (dst.size, Fe)).astype(np.float32))


def timed(step, warmup, steps):
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    times = []
    for _ in range(steps):
        t0 = time.perf_counter()
        step()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return float(np.median(times)) * 1e3, torch.cuda.max_memory_allocated() / 2**20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[1024, 4096])
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=30)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("cgcnn_step_time needs the GPU: nothing is measured without one")
    import deepchem_amd as dc
    from deepchem_amd.models.torch_models import CgcnnBatch
    for B in args.batches:
        rng = np.random.RandomState(17)
        graphs = [crystal(rng) for _ in range(B)]
        y, w = rng.normal(0, 1, (B, 1)), np.ones((B, 1))
        row = {"batch": B}
        for route, tag in (("auto", "native"), ("torch", "torch")):
            torch.manual_seed(0)
            model = dc.models.CGCNNModel(batch_size=B, learning_rate=1e-4, route=route)
            model._ensure_built()
            model.model.train()
            labels, weights = [model._to_device(y)], [model._to_device(w)]

            def build():
                return CgcnnBatch(graphs, model.device)

            def step():
                model._train_step(build(), labels, weights, model._loss_fn, model._pytorch_optimizer)

            uploaded = build()

            def uploaded_step():
                model._train_step(uploaded, labels, weights, model._loss_fn, model._pytorch_optimizer)

            row[tag + "_uploaded_ms"], row[tag + "_uploaded_peak_mib"] = (round(v, 3) for v in
                                                                          timed(uploaded_step, args.warmup, args.steps))
            assert model.last_route == tag
            row[tag + "_ms"], row[tag + "_peak_mib"] = (round(v, 3) for v in timed(step, args.warmup, args.steps))
            if tag == "native":
                row["build_ms"] = round(timed(build, 2, 10)[0], 3)
                row["nodes"], row["edges"] = uploaded.graph.n_nodes, uploaded.graph.n_edges
            del model, uploaded, build, step, uploaded_step, labels, weights  # (the closures hold the model)
            gc.collect()
            torch.cuda.empty_cache()
        row["torch_over_native_uploaded"] = round(row["torch_uploaded_ms"] / row["native_uploaded_ms"], 3)
        row["torch_over_native"] = round(row["torch_ms"] / row["native_ms"], 3)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
