"""Time of one MAT training step on the GPU: ``MATModel`` (pad-free ``MatBatch``, bias once per batch, fused attention
kernel) against ``padded_forward``, the reference's padded algorithm restated in eager float32 torch (tests/mat_refs.py),
on the same GPU with its padded batch already uploaded -- what a user has without this model, minus the host generator.

    python tools/mat_step_time.py [--models default test] [--batches 32 100 1024] [--warmup 5] [--steps 30]

Synthetic molecules (tests/mat_refs.py: random trees laid out as the featurizer lays a molecule out): 18 real atoms on
average, 29 at most, plus the dummy node.  ``default`` is the default model (8 encoder layers, 16 heads, width 1024),
``test`` the reference's own test model (width 128).  Per configuration: warm-up steps, then the MEDIAN of repeated
steps, each ended by a device synchronise; peak memory = ``torch.cuda.max_memory_allocated`` over the timed steps.
``native_ms`` builds and uploads the ``MatBatch`` in every step, as ``fit`` does; ``native_uploaded_ms`` reuses an
uploaded batch (its bias is recomputed), the like-for-like figure against ``torch_ms``.  One JSON line per configuration.
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

MODELS = {"default": dict(n_encoders=8, h=16),
          "test": dict(n_encoders=8, h=16, sa_hsize=128, d_input=128, d_hidden=128, d_output=128, encoder_hsize=128)}


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
    ap.add_argument("--models", nargs="+", default=["default", "test"], choices=sorted(MODELS))
    ap.add_argument("--batches", type=int, nargs="+", default=[32, 100, 1024])
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=30)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mat_step_time needs the GPU: nothing is measured without one")
    import deepchem_amd as dc
    import mat_refs
    for name in args.models:
        for B in args.batches:
            rng = np.random.RandomState(17)
            mols = [mat_refs.synthetic_molecule(int(np.clip(rng.normal(18, 4.5), 3, 29)), rng) for _ in range(B)]
            X = np.empty(B, dtype=object)
            X[:] = mols
            y, w = rng.normal(0, 1, (B, 1)), np.ones((B, 1))
            model = dc.models.MATModel(batch_size=B, learning_rate=1e-4, **MODELS[name])
            model._ensure_built()
            model.model.train()
            hs = model.host_set(X)
            idx = np.arange(B)
            labels, weights = [model._to_device(y)], [model._to_device(w)]

            def native_step():
                model._train_step(hs.batch(idx, model.device), labels, weights, model._loss_fn, model._pytorch_optimizer)

            t_native, m_native = timed(native_step, args.warmup, args.steps)
            assert model.last_route == "native"
            uploaded = hs.batch(idx, model.device)

            def native_uploaded_step():
                uploaded._bias.clear()
                model._train_step(uploaded, labels, weights, model._loss_fn, model._pytorch_optimizer)

            t_up, m_up = timed(native_uploaded_step, args.warmup, args.steps)
            n_atoms, n_pairs = uploaded.offs.n_atoms, uploaded.offs.n_pairs
            state = {k: v.detach().cpu().numpy() for k, v in model.model.state_dict().items()}
            padded = [torch.as_tensor(np.asarray(a, np.float32), device="cuda")
                      for a in next(iter(model.default_generator(dc.data.NumpyDataset(X, y, w))))[0]]
            del model, hs, uploaded, native_step, native_uploaded_step, labels, weights  # (the closures hold the model)
            gc.collect()
            torch.cuda.empty_cache()

            ref = mat_refs.MATRef(state, torch.float32, h=MODELS[name]["h"]).to("cuda")
            ty, tw = torch.as_tensor(y, device="cuda"), torch.as_tensor(w, device="cuda")
            opt = torch.optim.Adam(ref.parameters(), lr=1e-4)

            def torch_step():
                opt.zero_grad()
                mat_refs.l2_loss(ref.padded_forward(*padded), ty, tw).backward()
                opt.step()

            t_torch, m_torch = timed(torch_step, args.warmup, args.steps)
            n_pad = int(padded[0].shape[1])
            del ref, padded, opt, torch_step, ty, tw
            gc.collect()
            torch.cuda.empty_cache()
            print(json.dumps({"model": name, "batch": B, "atoms": n_atoms, "pairs": n_pairs, "padded_to": n_pad,
                              "native_ms": round(t_native, 3), "native_uploaded_ms": round(t_up, 3),
                              "torch_ms": round(t_torch, 3), "torch_over_native_uploaded": round(t_torch / t_up, 3),
                              "native_peak_mib": round(m_native, 1), "torch_peak_mib": round(m_torch, 1)}), flush=True)


if __name__ == "__main__":
    main()
