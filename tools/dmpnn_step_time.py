"""Time of one D-MPNN training step on the GPU: ``DMPNNModel`` (message kernel, fused update, segmented products, flat
native optimizer step) against the float32 pad-free torch restatement of tests/dmpnn_refs.py moved to the same GPU with
its batch already uploaded -- eager torch on the SAME algorithm (index_add_ instead of the reference's padded gather),
so the comparison is kind to torch: the reference's own ``message[mapping].sum(1)`` moves max_degree times more.

    python tools/dmpnn_step_time.py [--batches 64 4096] [--modes reference paper] [--warmup 5] [--steps 30]

Synthetic molecules from ``deepchem_amd.utils.synthetic`` (18.5 atoms on average) with 133 atom and 14 bond features,
the default model (enc_hidden 300, depth 3).  Per configuration: warm-up steps, then the MEDIAN of repeated steps,
each ended by a device synchronise; peak memory = ``torch.cuda.max_memory_allocated`` over the timed steps.
``native_ms`` has its batch on the device already, like the torch step; ``native_collate_ms`` also gathers the batch
from the cached graph set in numpy and uploads it every step (what ``fit`` does with ``collate="host"``);
``native_devcollate_ms`` collates it on the device from the resident set instead, index upload included (what ``fit``
does from ``DMPNN_DEVICE_COLLATE_MIN`` molecules per batch up).  One JSON line per batch size and mode.
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
sys.path.insert(0, os.path.join(ROOT, "tests"))


def synthetic_graphs(n_mols, seed, atom_fdim=133, bond_fdim=14):
    from deepchem_amd.feat import GraphData
    from deepchem_amd.utils.synthetic import synthetic_molecules
    packed = synthetic_molecules(n_mols, n_feat=atom_fdim, seed=seed)
    rng = np.random.RandomState(seed)
    graphs = []
    for m in range(n_mols):
        feats, adj = packed.molecule(m)
        bonds = np.array([(i, j) for i, nb in enumerate(adj) for j in nb if i < j], np.int64).reshape(-1, 2)
        edge_index = np.stack([bonds.reshape(-1), bonds[:, ::-1].reshape(-1)])
        graphs.append(GraphData(np.asarray(feats, np.float32), edge_index,
                                np.repeat(rng.normal(0, 1, (len(bonds), bond_fdim)).astype(np.float32), 2, axis=0),
                                global_features=np.empty(0, np.float32)))
    return np.array(graphs, dtype=object)


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
    ap.add_argument("--batches", type=int, nargs="+", default=[64, 4096])
    ap.add_argument("--modes", nargs="+", default=["reference", "paper"])
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=30)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dmpnn_step_time needs the GPU: nothing is measured without one")
    import deepchem_amd as dc
    import dmpnn_refs
    for B in args.batches:
        X = synthetic_graphs(B, 17)
        rng = np.random.RandomState(1)
        y, w = rng.normal(0, 1, (B, 1)), np.ones((B, 1))
        for mode in args.modes:
            model = dc.models.DMPNNModel(batch_size=B, learning_rate=1e-3, message_mode=mode)
            model._ensure_built()
            model.model.train()
            graphs = model.graph_set(X)
            idx = np.arange(B)
            labels, weights = [model._to_device(y)], [model._to_device(w)]
            batch = graphs.batch(idx).to(model.device)

            def native_step():
                model._train_step(batch, labels, weights, model._loss_fn, model._pytorch_optimizer)

            def native_collate_step():
                model._train_step(graphs.batch(idx).to(model.device), labels, weights, model._loss_fn,
                                  model._pytorch_optimizer)

            resident = model.resident_set(X)

            def native_devcollate_step():
                model._train_step(resident.batch(idx), labels, weights, model._loss_fn, model._pytorch_optimizer)

            t_native, m_native = timed(native_step, args.warmup, args.steps)
            t_collate, _ = timed(native_collate_step, args.warmup, args.steps)
            t_devcollate, _ = timed(native_devcollate_step, args.warmup, args.steps)
            state = {k: v.detach().cpu().numpy() for k, v in model.model.state_dict().items()}
            host, n_atoms, n_bonds = batch.host, batch.n_atoms, batch.n_bonds
            del model, batch, graphs, resident, native_step, native_collate_step, native_devcollate_step
            gc.collect()
            torch.cuda.empty_cache()

            ref = dmpnn_refs.DMPNNRef(state, torch.float32, n_tasks=1, message_mode=mode).to("cuda")
            on_gpu = dmpnn_refs.batch_tensors(host, torch.float32, "cuda")
            ty, tw = torch.as_tensor(y, device="cuda"), torch.as_tensor(w, device="cuda")
            opt = torch.optim.Adam(ref.parameters(), lr=1e-3)

            def torch_step():
                opt.zero_grad()
                dmpnn_refs.l2_loss(ref(on_gpu), ty, tw).backward()
                opt.step()

            t_torch, m_torch = timed(torch_step, args.warmup, args.steps)
            del ref, on_gpu, opt, torch_step
            gc.collect()
            torch.cuda.empty_cache()
            print(json.dumps({"batch": B, "mode": mode, "atoms": n_atoms, "bond_rows": n_bonds,
                              "native_ms": round(t_native, 4), "native_collate_ms": round(t_collate, 4),
                              "native_devcollate_ms": round(t_devcollate, 4),
                              "torch_ms": round(t_torch, 4), "ratio": round(t_torch / t_native, 3),
                              "native_peak_mib": round(m_native, 1), "torch_peak_mib": round(m_torch, 1)}), flush=True)


if __name__ == "__main__":
    main()
