"""Time of one LCNN training step on the GPU: the native route (``csrc/lcnn.hip`` behind the one product of a block)
against the torch route (the reference's arithmetic, vectorised: the gathered (N, P, K * F) rows through one Linear,
statistics over dim 1) of the SAME ``LCNNModel`` on the same GPU and batch.

    python tools/lcnn_step_time.py [--batches 8 1024 4096] [--warmup 5] [--steps 30]

The default model (n_occupancy 3, 19 neighbour sites, 6 permutations, n_features 44, 2 convolutions) on 7 x 9 periodic
triangular lattices (63 sites, one-hot occupancies).  Per route: warm-up steps, then the MEDIAN of repeated steps, Adam
included, each ended by a device synchronise; peak memory = ``torch.cuda.max_memory_allocated`` over the timed steps.
``*_ms`` builds and uploads the ``LcnnBatch`` in every step through ``_prepare_batch``, as ``fit`` does (per-item tables
cached); ``*_uploaded_ms`` reuses an uploaded batch.  ``build_ms``: the host-side build and upload alone.  One JSON line
per batch size.
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
    ap.add_argument("--batches", type=int, nargs="+", default=[8, 1024, 4096])
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=30)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lcnn_step_time needs the GPU: nothing is measured without one")
    import deepchem_amd as dc
    from deepchem_amd.feat import GraphData
    from tests.lcnn_refs import edges_of, torus_table
    edges = edges_of(torus_table(7, 9))
    for B in args.batches:
        rng = np.random.RandomState(17)
        X = np.empty(B, dtype=object)
        X[:] = [GraphData(np.eye(3, dtype=np.float32)[rng.randint(0, 3, 63)], edges) for _ in range(B)]
        y, w = rng.normal(0, 1, (B, 1)), np.ones((B, 1))
        row = {"batch": B, "sites": 63 * B}
        for route, tag in (("auto", "native"), ("torch", "torch")):
            torch.manual_seed(0)
            model = dc.models.LCNNModel(batch_size=B, learning_rate=1e-4, route=route)
            model._ensure_built()
            model.model.train()

            def build():
                return model._prepare_batch(([X], [y], [w]))

            def step():
                inputs, labels, weights = build()
                model._train_step(inputs, labels, weights, model._loss_fn, model._pytorch_optimizer)

            uploaded, labels, weights = build()

            def uploaded_step():
                model._train_step(uploaded, labels, weights, model._loss_fn, model._pytorch_optimizer)

            row[tag + "_uploaded_ms"], row[tag + "_uploaded_peak_mib"] = (round(v, 3) for v in
                                                                          timed(uploaded_step, args.warmup, args.steps))
            row[tag + "_route"] = model.last_route
            row[tag + "_ms"], row[tag + "_peak_mib"] = (round(v, 3) for v in timed(step, args.warmup, args.steps))
            if tag == "native":
                row["build_ms"] = round(timed(build, 2, 10)[0], 3)
            del model, uploaded, build, step, uploaded_step, labels, weights  # (the closures hold the model)
            gc.collect()
            torch.cuda.empty_cache()
        row["torch_over_native_uploaded"] = round(row["torch_uploaded_ms"] / row["native_uploaded_ms"], 3)
        row["torch_over_native"] = round(row["torch_ms"] / row["native_ms"], 3)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
