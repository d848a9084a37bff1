"""Per-scan timing of the Gaussian-mixture family (k_explore_mixture + the swap launch) next to Funnel(d) from the same run (DESIGN 4.8's table).

    python tools/bench_mixture.py [--out FILE.json]

Shapes: GaussianMixture with K = 2 and K = 8 components at d = 128 and d = 512, and Funnel(d) -- 1024 chains each, with SliceSampler and
AutoMALA.  Every engine adapts for four rounds (the schedule; AutoMALA also its step size and preconditioner), then runs three timed blocks of
16 scans (run_scans; best of three, wall clock around a synchronised call).  Reported: ms per scan, and the mixture's ratio to the funnel."""
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


def target(kind, d, K):
    if kind == "funnel":
        return P.Funnel(d), P.ScaledPrecisionNormalLogPotential(1 / 9., d)
    g = np.random.default_rng(K * 1000 + d)
    return P.GaussianMixture(g.uniform(0.5, 2.0, K), g.normal(0.0, 2.0, (K, d)), g.uniform(0.5, 1.5, (K, d))), \
        P.ScaledPrecisionNormalLogPotential(1 / 9., d)


def measure(kind, d, K, explorer):
    t, ref = target(kind, d, K)
    pt = P.PT(P.Inputs(target=t, reference=ref, n_chains=N_CHAINS, n_rounds=20, explorer=explorer, show_report=False,
                       record=[P.round_trip, P.log_sum_ratio]))
    e = pt.replicas
    for r in range(1, 5):
        e.run_scans(1, 2 ** r)
        adapt(pt, reduce_recorders(pt))
    best = 1e9
    for _ in range(REPS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e.run_scans(1, BLOCK)
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
    for name, mk in (("SliceSampler", P.SliceSampler), ("AutoMALA", P.AutoMALA)):
        for d in (128, 512):
            try:
                fun = measure("funnel", d, 0, mk())
            except P.PteError as exc:                  # (SliceSampler on the funnel's neck can exhaust slice_shrink's iterations at 1024 chains)
                fun = dict(ms_per_scan=float("nan"), error=str(exc))
            for K in (2, 8):
                mix = measure("mixture", d, K, mk())
                row = dict(explorer=name, d=d, K=K, n_chains=N_CHAINS, mixture=mix, funnel=fun, ratio=mix["ms_per_scan"] / fun["ms_per_scan"])
                rows.append(row)
                print("%-12s d=%-4d K=%d  mixture %.3f ms/scan  funnel %.3f ms/scan  ratio %.2f"
                      % (name, d, K, mix["ms_per_scan"], fun["ms_per_scan"], row["ratio"]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(rows, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
