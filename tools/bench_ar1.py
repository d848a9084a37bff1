"""Per-scan timing of the latent-AR(1) state-space family (k_explore_ar1 + the swap launch) -- DESIGN 4.15's table.

    python tools/bench_ar1.py [--out FILE.json] [--obs 12,61,509]

Shapes: T = 12, 61, 509 observations (d = T + 3 = 15, 64, 512), both observation models, a synthetic AR(1) path observed through the model,
1024 chains, reference ScaledPrecisionNormalLogPotential(1, d).  SliceSampler and AutoMALA adapt for four rounds (the schedule; AutoMALA also
its step size and preconditioner), then run three timed blocks of 16 scans (run_scans; best of three, wall clock around a synchronised
call): ms per scan.  MALA runs with a fixed step size after one round.

The yardstick is HierarchicalNormalMeans (centred) at the same d in the same run, launch for launch (explore + swap per scan; neither family
has a one-launch scan loop): the same body and the same register-resident data.  This family has a tanh and a log more on uniform values
(and, under stochastic volatility, an exp per coordinate), three gradient sums instead of two, and two DPP wave shifts per block and
evaluation.  The ratio ar1 / hier is printed per row."""
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
OBS = (12, 61, 509)
EXPLORERS = (("SliceSampler", lambda: P.SliceSampler(), 4), ("AutoMALA", lambda: P.AutoMALA(), 4), ("MALA", lambda: P.MALA(step_size=0.02), 1))


def ar1_target(T, lik):
    g = np.random.default_rng(1000 + T)
    h = np.empty(T)
    h[0] = g.normal(0.0, 0.5 / 0.6)
    for t in range(1, T):
        h[t] = 0.8 * h[t - 1] + 0.5 * g.normal()
    y = h + 0.5 * g.normal(0.0, 1.0, T) if lik == "normal_identity" else np.exp(h / 2.0) * g.normal(0.0, 1.0, T)
    return P.LatentAR1(y, likelihood=lik, obs_sd=0.5)


def hier_target(J):
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
    ap.add_argument("--obs", default=",".join(str(t) for t in OBS))
    args = ap.parse_args()
    rows = []
    for T in (int(t) for t in args.obs.split(",")):
        d = T + 3
        hier = {}
        for name, mk, rounds in EXPLORERS:
            try:
                hier[name] = measure(hier_target(d - 2), mk(), rounds)[0]
            except P.PteError as exc:          # (no yardstick for that cell)
                print("d=%-4d hier %s: %s" % (d, name, exc), flush=True)
                hier[name] = None
        fmt = lambda v: "%8.3f ms/scan" % v if v is not None else "     n/a"
        print("d=%-4d hier (centred)         " % d + "  ".join("%s %s" % (n, fmt(hier[n])) for n, _, _ in EXPLORERS), flush=True)
        for lik in ("stochastic_volatility", "normal_identity"):
            row = dict(T=T, d=d, n_chains=N_CHAINS, likelihood=lik, hier=hier)
            for name, mk, rounds in EXPLORERS:
                try:
                    row[name], row["kernel"] = measure(ar1_target(T, lik), mk(), rounds)
                except P.PteError as exc:
                    print("d=%-4d %s %s: %s" % (d, lik, name, exc), flush=True)
                    row[name] = None
            rows.append(row)
            cell = lambda n: ("%8.3f ms/scan (%s)" % (row[n], "x %.2f" % (row[n] / hier[n]) if hier[n] else "no yardstick")) if row[n] is not None else "     n/a"
            print("d=%-4d %-22s " % (d, lik) + "  ".join("%s %s" % (n, cell(n)) for n, _, _ in EXPLORERS), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(rows, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
