"""Per-scan timing of the variable-selection family (k_explore_varsel + the swap launch) -- DESIGN 4.12's table.

    python tools/bench_varsel.py [--glm] [--out FILE.json]

Shapes (n observations, d columns; the state has 2 d coordinates): (1024, 16), (1024, 64), (4096, 32), (512, 256), logistic spike-and-slab
regression on synthetic data in which every second column is active, 1024 chains, reference ScaledPrecisionNormalLogPotential(1, d),
inclusion probability 0.5.  SliceSampler adapts the schedule for four rounds, then runs three timed blocks of 16 scans (run_scans; best of
three, wall clock around a synchronised call): ms per scan, as tools/bench_glm.py measures.

From the explorer recorders of the timed blocks: the density evaluations per scan that the recorders count -- per visit of a Float64
coordinate the two end points, the doubling steps and the shrinkage steps (explorer_n_steps), per visit of a Bool coordinate one; the
re-evaluations inside slice_accept are not recorded, so this is a lower bound -- and from it the evaluations per second and the bytes of
Xc and y they request from L2 at most (8 * 2 * n_pad each; an evaluation whose effective coefficient does not move makes no pass).

--glm: also tools/bench_glm.py's SliceSampler rows (the Bayesian-GLM family, which evaluates eta in full per proposal) in the same
process, for the comparison of DESIGN 4.12."""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "pigeons.jl_amd"), os.path.join(ROOT, "tools")]
import numpy as np
import torch
import pigeons_amd as P
from pigeons_amd.pt import reduce_recorders, adapt

N_CHAINS, BLOCK, REPS = 1024, 16, 3
SHAPES = ((1024, 16), (1024, 64), (4096, 32), (512, 256))


def target(n, d):
    g = np.random.default_rng(n * 1000 + d)
    X = g.normal(0.0, 1.0 / math.sqrt(d), (n, d))
    eta = X @ (g.normal(0.0, 1.0, d) * (np.arange(d) % 2 == 0))
    y = (g.uniform(size=n) < 1 / (1 + np.exp(-eta))).astype(float)
    return P.SpikeSlabRegression(X, y), P.ScaledPrecisionNormalLogPotential(1.0, d)


def measure(n, d, adapt_rounds=4):
    t, ref = target(n, d)
    ex = P.SliceSampler()
    pt = P.PT(P.Inputs(target=t, reference=ref, n_chains=N_CHAINS, n_rounds=20, explorer=ex, show_report=False,
                       record=[P.round_trip, P.log_sum_ratio]))
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
    e.reduce()
    _, _, steps_sum, steps_n = e.explorer_stats()
    scans = REPS * BLOCK
    # per Float64 visit two recorder entries (doubling steps, shrinkage steps) and the two end points; per Bool visit one evaluation
    evals = (float(np.sum(steps_sum)) + float(np.sum(steps_n))) / scans + (N_CHAINS - 1) * d * ex.n_passes
    out = dict(ms_per_scan=best, kernel=e.kernel_name(), evals_per_scan=evals)
    e.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--glm", action="store_true", help="also the Bayesian-GLM family's SliceSampler rows (tools/bench_glm.py)")
    args = ap.parse_args()
    rows = []
    for n, d in SHAPES:
        m = measure(n, d)
        n_pad = (n + 63) // 64 * 64
        per_s = m["evals_per_scan"] / (m["ms_per_scan"] * 1e-3)
        row = dict(n=n, d=d, n_chains=N_CHAINS, family="variable_selection", SliceSampler=m["ms_per_scan"], kernel=m["kernel"],
                   evals_per_scan=m["evals_per_scan"], evals_per_s=per_s, l2_bytes_per_s_at_most=per_s * 16.0 * n_pad)
        rows.append(row)
        print("varsel n=%-5d d=%-4d  SliceSampler %9.3f ms/scan  >= %.3g evaluations/scan, %.3g /s, <= %.2f TB/s of Xc and y from L2"
              % (n, d, row["SliceSampler"], row["evals_per_scan"], per_s, row["l2_bytes_per_s_at_most"] / 1e12), flush=True)
    if args.glm:
        import bench_glm
        for n, d in bench_glm.SHAPES:
            ms = bench_glm.measure(n, d, P.SliceSampler())["ms_per_scan"]
            rows.append(dict(n=n, d=d, n_chains=bench_glm.N_CHAINS, family="bayesian_glm", SliceSampler=ms))
            print("glm    n=%-5d d=%-4d  SliceSampler %9.3f ms/scan" % (n, d, ms), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(rows, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
