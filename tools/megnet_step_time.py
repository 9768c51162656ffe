"""Time of one MEGNet training step on the GPU: the native route (``csrc/megnet.hip`` between the products, the set2set
kernels) against the torch route (the reference's order: doubled edges, concatenated rows, scatter-means) of the SAME
``MEGNetModel`` on the same GPU and batch.

    python tools/megnet_step_time.py [--batches 32 64 128 256 512 1024 4096] [--warmup 5] [--steps 30]

The default-width model (Fn = Fe = Fg = 32, n_blocks = 3, undirected) on molecule-like graphs: a random tree of about
18 nodes (at least 3, at most 29) plus up to two ring closures, every bond listed in both directions.  Per route:
warm-up steps, then the MEDIAN of repeated steps, each ended by a device synchronise; peak memory =
``torch.cuda.max_memory_allocated`` over the timed steps.  ``*_ms`` builds and uploads the ``MegnetBatch`` in every step,
as ``fit`` did before the graph set; ``*_uploaded_ms`` reuses an uploaded batch.  ``build_ms``: the host-side build and
upload alone.  The two routes ``fit`` takes over a ``NumpyDataset`` now, both over the cached ``MegnetGraphSet`` of the same
graphs and a fixed permutation of them: ``native_setcollate_ms`` gathers the batch in numpy and uploads it,
``native_devcollate_ms`` is plan, index upload, ``gcmi_gn_collate`` over the ``ResidentMegnetSet`` and the step together.
One JSON line per batch size.
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
SIZES = dict(n_node_features=32, n_edge_features=32, n_global_features=32)


def molecule(rng, F=32):
    from deepchem_amd.feat import GraphData
    n = int(np.clip(rng.normal(18, 4.5), 3, 29))
    a = np.arange(1, n)
    b = np.asarray([rng.randint(0, k) for k in a])
    for _ in range(rng.randint(0, 3)):  # ring closures
        i, j = rng.choice(n, 2, replace=False)
        a, b = np.append(a, i), np.append(b, j)
    ei = np.stack([np.concatenate([a, b]), np.concatenate([b, a])])
    bond = rng.normal(0, 1, (a.size, F)).astype(np.float32)
    return GraphData(rng.normal(0, 1, (n, F)).astype(np.float32), ei, np.concatenate([bond, bond]),
                     global_features=rng.normal(0, 1, (1, F)).astype(np.float32))


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
    ap.add_argument("--batches", type=int, nargs="+", default=[32, 64, 128, 256, 512, 1024, 4096])
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=30)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("megnet_step_time needs the GPU: nothing is measured without one")
    import deepchem_amd as dc
    from deepchem_amd.models.torch_models import MegnetBatch
    for B in args.batches:
        rng = np.random.RandomState(17)
        graphs = [molecule(rng) for _ in range(B)]
        y, w = rng.normal(0, 1, (B, 1)), np.ones((B, 1))
        row = {"batch": B}
        for route, tag in (("auto", "native"), ("torch", "torch")):
            torch.manual_seed(0)
            model = dc.models.MEGNetModel(n_blocks=3, batch_size=B, learning_rate=1e-4, route=route, **SIZES)
            model._ensure_built()
            model.model.train()
            labels, weights = [model._to_device(y)], [model._to_device(w)]

            def build():
                return MegnetBatch(graphs, True, model.device)

            def step():
                model._train_step(build(), labels, weights, model._loss_fn, model._pytorch_optimizer)

            uploaded = build()

            def uploaded_step():
                model._train_step(uploaded, labels, weights, model._loss_fn, model._pytorch_optimizer)

            row[tag + "_ms"], row[tag + "_peak_mib"] = (round(v, 3) for v in timed(step, args.warmup, args.steps))
            assert model.last_route == tag
            row[tag + "_uploaded_ms"], row[tag + "_uploaded_peak_mib"] = (round(v, 3) for v in
                                                                          timed(uploaded_step, args.warmup, args.steps))
            if tag == "native":
                X = np.empty(B, dtype=object)
                X[:] = graphs
                order = np.random.RandomState(3).permutation(B)
                held, resident = model.graph_set(X), model.resident_set(X)
                for name, make in (("native_setcollate", lambda: held.batch(order, model.device)),
                                   ("native_devcollate", lambda: resident.batch(order))):
                    def collated_step():
                        model._train_step(make(), labels, weights, model._loss_fn, model._pytorch_optimizer)
                    row[name + "_ms"], row[name + "_peak_mib"] = (round(v, 3) for v in
                                                                  timed(collated_step, args.warmup, args.steps))
                    assert model.last_route == "native"
                row["set_mib"] = round(resident.nbytes / 2**20, 3)
                del X, held, resident, make, collated_step
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
