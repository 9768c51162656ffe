"""The dense-layer backward (ops.fused_dense_bwd, fp32 rows) on seeded standard-normal data, for comparing two builds
of libgcmi.so bit for bit.

    python tools/dense_bwd_dump.py dump DIR        # writes DIR/<case>_{dp,dw,db,psums}.npy with the library that loads
    python tools/dense_bwd_dump.py compare A B     # exit status 1 unless what must be equal is equal

Cases: ``one_tile`` (64 rows: one tile, one workgroup, so the float atomics of dW and db land on zeros in a fixed
order and all four outputs must be equal) and ``rows700`` (11 tiles, 11 workgroups: dP and psums must be equal -- each
workgroup adds into its own psums replica --; dW and db differ by the order of the atomics, as between two runs of one
build, and are only reported)."""
import os
import sys

import numpy as np

CASES = {"one_tile": 64, "rows700": 700}
MUST_EQUAL = {"one_tile": ("dp", "dw", "db", "psums"), "rows700": ("dp", "psums")}
K, W = 64, 128


def run_case(rows, seed):
    import torch
    from deepchem_amd import ops
    rng = np.random.default_rng(seed)
    sizes = []
    while sum(sizes) < rows:
        sizes.append(min(int(rng.integers(1, 40)), rows - sum(sizes)))
    n_mols = len(sizes)
    membership = np.repeat(np.arange(n_mols), sizes).astype(np.int32)
    first = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    arg = (first[:, None] + rng.integers(0, 40, (n_mols, W)) % np.array(sizes)[:, None]).astype(np.int32)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    f32 = lambda *shape: rng.standard_normal(shape).astype(np.float32)
    g2, gc, coef, p, w = dev(f32(n_mols, 2 * W)), dev(f32(rows, W)), dev(f32(3 * W)), dev(f32(rows, K)), dev(f32(W * K))
    dw, db = torch.zeros(W * K, device="cuda:0"), torch.zeros(W, device="cuda:0")
    dp = torch.zeros(rows, K, device="cuda:0")
    psums = torch.zeros(66 * K, dtype=torch.float64, device="cuda:0")
    ops.fused_dense_bwd([0], [rows], [0], [0], dev(membership), g2, dev(arg), gc, coef, p, w, dw, db, dp, psums=psums)
    torch.cuda.synchronize()
    return dict(dp=dp.cpu().numpy(), dw=dw.cpu().numpy(), db=db.cpu().numpy(), psums=psums.cpu().numpy())


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "dump":
        sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        os.makedirs(sys.argv[2], exist_ok=True)
        for i, (name, rows) in enumerate(CASES.items()):
            for key, a in run_case(rows, 20 + i).items():
                np.save(os.path.join(sys.argv[2], "%s_%s.npy" % (name, key)), a)
        return 0
    if len(sys.argv) == 4 and sys.argv[1] == "compare":
        bad = 0
        for name in CASES:
            for key in ("dp", "dw", "db", "psums"):
                a, b = (np.load(os.path.join(d, "%s_%s.npy" % (name, key))) for d in sys.argv[2:4])
                same = a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))
                must = key in MUST_EQUAL[name]
                diff = 0.0 if same else float(np.abs(a.astype(np.float64) - b.astype(np.float64)).max())
                print("%-9s %-5s %s  max |a - b| %.3g%s" % (name, key, "bit-equal" if same else "DIFFERENT", diff,
                                                          "" if must else "  (atomics: reported only)"))
                bad += must and not same
        return 1 if bad else 0
    raise SystemExit(__doc__)


if __name__ == "__main__":
    sys.exit(main())
