"""Per-scan timing of the dense-precision Gaussian family (k_explore_dense_slice / k_explore_dense + the swap launch) -- DESIGN 4.16's table.

    python tools/bench_dense.py [--out FILE.json] [--dims 16,64,...]

Shapes: d = 16, 64, 128, 256, 512, Q = U diag(lambda) U' with log-spaced lambda and cond(Q) = 100, a random mean, 1024 chains, reference
ScaledPrecisionNormalLogPotential(1, d).  SliceSampler and AutoMALA adapt for four rounds (the schedule; AutoMALA also its step size and
preconditioner), then run three timed blocks of 16 scans (run_scans; best of three, wall clock around a synchronised call): ms per scan.

The yardstick is the centred hierarchical normal-means family at the same d in the same run, launch for launch: an elementwise density
with O(d) work per evaluation.  SliceSampler there evaluates the density in full at every proposal; here a proposal is O(1) and a commit
one matrix row.  AutoMALA there reads 3 d doubles per gradient, here the whole matrix (8 d ld bytes from L2).  The ratio dense / hier is
printed per cell, and with it the matrix bytes the scan requests from L2 per second (SliceSampler: n_passes + 2 matrices per scan --
one row per coordinate and pass, one full evaluation at each end of the call)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "pigeons.jl_amd")]
import numpy as np
import torch
import pigeons_amd as P
from pigeons_amd.pt import reduce_recorders, adapt

N_CHAINS, BLOCK, REPS = 1024, 16, 3
DIMS = (16, 64, 128, 256, 512)
EXPLORERS = (("SliceSampler", lambda: P.SliceSampler(), 4), ("AutoMALA", lambda: P.AutoMALA(), 4))


def dense_target(d, cond=100.0):
    g = np.random.default_rng(2000 + d)
    U, _ = np.linalg.qr(g.normal(size=(d, d)))
    lam = np.exp(np.linspace(-0.5 * np.log(cond), 0.5 * np.log(cond), d))
    return P.DenseNormal(g.normal(0.0, 1.0, d), (U * lam) @ U.T)


def hier_target(d):
    J = d - 2
    g = np.random.default_rng(1000 + J)
    sigma = g.uniform(0.5, 2.0, J)
    y = 0.5 + g.normal(0.0, 1.0, J) + sigma * g.normal(0.0, 1.0, J)
    return P.HierarchicalNormalMeans(y, sigma, mu_sd=5.0, tau_scale=5.0, parameterization="centered")


def measure(target, explorer, adapt_rounds):
    pt = P.PT(P.Inputs(target=target, reference=P.ScaledPrecisionNormalLogPotential(1.0, target.dim), n_chains=N_CHAINS, n_rounds=20,
                       explorer=explorer, show_report=False, record=[P.round_trip, P.log_sum_ratio]))
    e = pt.replicas
    for r in range(1, adapt_rounds + 1):
        e.run_scans(1, 2 ** r)
        adapt(pt, reduce_recorders(pt))
    best = 1e9
    for _ in range(REPS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e.run_scans(2, BLOCK)
        torch.cuda.synchronize()
        best = min(best, (time.perf_counter() - t0) / BLOCK * 1e3)
    name = e.kernel_name()
    e.close()
    return best, name


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--dims", default=",".join(map(str, DIMS)))
    args = ap.parse_args()
    rows = []
    for d in [int(v) for v in args.dims.split(",")]:
        row = dict(d=d, n_chains=N_CHAINS, hier={}, kernel={})
        for name, mk, rounds in EXPLORERS:
            try:
                row["hier"][name] = measure(hier_target(d), mk(), rounds)[0]
            except P.PteError as exc:          # (no yardstick for that cell)
                print("d=%-4d hier %s: %s" % (d, name, exc), flush=True)
                row["hier"][name] = None
            row[name], row["kernel"][name] = measure(dense_target(d), mk(), rounds)
        ld = 64 * (1 if d <= 64 else 2 if d <= 128 else 4 if d <= 256 else 8)
        passes = P.SliceSampler().n_passes
        row["slice_matrix_GB_per_s"] = (passes + 2) * 8.0 * d * ld * (N_CHAINS - 1) / (row["SliceSampler"] * 1e-3) / 1e9
        rows.append(row)
        ratio = lambda n: "x %.2f of hier %.3f" % (row[n] / row["hier"][n], row["hier"][n]) if row["hier"][n] else "no yardstick"
        print("d=%-4d " % d + "  ".join("%s %8.3f ms/scan (%s)" % (n, row[n], ratio(n)) for n, _, _ in EXPLORERS)
              + "  slice: %.0f GB/s of matrix rows from L2" % row["slice_matrix_GB_per_s"], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(rows, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
