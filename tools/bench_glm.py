"""Per-scan timing of the Bayesian-GLM family (k_explore_glm + the swap launch) -- DESIGN 4.9's table.

    python tools/bench_glm.py [--out FILE.json]

Shapes (n observations, d coefficients): (1024, 16), (1024, 64), (4096, 32), (256, 512), logistic regression on synthetic data, 1024 chains,
reference ScaledPrecisionNormalLogPotential(1, d).  SliceSampler and AutoMALA adapt for four rounds (the schedule; AutoMALA also its step size
and preconditioner), then run three timed blocks of 16 scans (run_scans; best of three, wall clock around a synchronised call): ms per scan.

A third row per shape, MALA with a fixed step size, counts its work exactly: every non-reference replica evaluates the gradient 1 + n_refresh
times per scan (2 n d fused multiply-adds and 2 n d 8 bytes of X each, from L2) and the log density once more (n d of each); the reference
replica once.  From the same timing: the X bytes per second the kernel streams (algorithmic, and what its loads request: whole 64-lane rows
of Xr) and the FP64 multiply-adds per second it issues."""
import argparse
import json
import math
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
SHAPES = ((1024, 16), (1024, 64), (4096, 32), (256, 512))


def target(n, d):
    g = np.random.default_rng(n * 1000 + d)
    X = g.normal(0.0, 1.0 / math.sqrt(d), (n, d))
    eta = X @ g.normal(0.0, 1.0, d)
    y = (g.uniform(size=n) < 1 / (1 + np.exp(-eta))).astype(float)
    return P.BayesianGLM(X, y), P.ScaledPrecisionNormalLogPotential(1.0, d)


def measure(n, d, explorer, adapt_rounds=4):
    t, ref = target(n, d)
    pt = P.PT(P.Inputs(target=t, reference=ref, n_chains=N_CHAINS, n_rounds=20, explorer=explorer, show_report=False,
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
    out = dict(ms_per_scan=best, kernel=e.kernel_name())
    e.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    rows = []
    for n, d in SHAPES:
        row = dict(n=n, d=d, n_chains=N_CHAINS)
        for name, mk in (("SliceSampler", P.SliceSampler), ("AutoMALA", P.AutoMALA)):
            row[name] = measure(n, d, mk())["ms_per_scan"]
        mala = P.MALA(step_size=0.02)
        n_refresh = mala.base_n_refresh * int(math.ceil(d ** mala.exponent_n_refresh))
        ms = measure(n, d, mala, adapt_rounds=1)["ms_per_scan"]
        grads = (N_CHAINS - 1) * (1 + n_refresh)
        fma = grads * 2 * n * d + N_CHAINS * n * d
        # what the loads fetch: Xc [d][n_pad] per evaluation, and per gradient whole 64-lane rows of Xr (64 E doubles for each observation)
        E = 1 if d <= 64 else 2 if d <= 128 else 4 if d <= 256 else 8
        n_pad = (n + 63) // 64 * 64
        requested = 8.0 * (grads * (d * n_pad + 64 * E * n) + N_CHAINS * d * n_pad)
        row.update(MALA=ms, mala_n_refresh=n_refresh, x_bytes_per_s=8.0 * fma / (ms * 1e-3), x_requested_bytes_per_s=requested / (ms * 1e-3),
                   fp64_fma_per_s=fma / (ms * 1e-3))
        rows.append(row)
        print("n=%-5d d=%-4d  SliceSampler %8.3f ms/scan  AutoMALA %8.3f ms/scan  MALA(n_refresh=%d) %8.3f ms/scan: X from L2 %.2f TB/s "
              "(requested %.2f TB/s), FP64 FMA %.2f T/s" % (n, d, row["SliceSampler"], row["AutoMALA"], n_refresh, ms, row["x_bytes_per_s"] / 1e12,
                                                           row["x_requested_bytes_per_s"] / 1e12, row["fp64_fma_per_s"] / 1e12), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(rows, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
