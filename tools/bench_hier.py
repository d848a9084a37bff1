"""Per-scan timing of the hierarchical normal-means family (k_explore_hier + the swap launch) -- DESIGN 4.14's table.

    python tools/bench_hier.py [--out FILE.json]

Shapes: J = 8, 62, 510 groups (d = J + 2 = 10, 64, 512), both parameterisations, synthetic group estimates, 1024 chains, reference
ScaledPrecisionNormalLogPotential(1, d).  SliceSampler and AutoMALA adapt for four rounds (the schedule; AutoMALA also its step size and
preconditioner), then run three timed blocks of 16 scans (run_scans; best of three, wall clock around a synchronised call): ms per scan.
MALA runs with a fixed step size after one round.

The yardstick is Neal's funnel at the same d in the same run, launch for launch (explore + swap per scan; the funnel's one-launch scan loop
is switched off): the same body; this family has one exp (centred) and a log1p more, two gradient sums instead of one, and none of the
funnel's 2 E divisions per evaluation.  The ratio hier / funnel is printed per row."""
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
from pigeons_amd import _lib
from pigeons_amd.pt import reduce_recorders, adapt

N_CHAINS, BLOCK, REPS = 1024, 16, 3
GROUPS = (8, 62, 510)
EXPLORERS = (("SliceSampler", lambda: P.SliceSampler(), 4), ("AutoMALA", lambda: P.AutoMALA(), 4), ("MALA", lambda: P.MALA(step_size=0.02), 1))


def hier_target(J, param):
    g = np.random.default_rng(1000 + J)
    sigma = g.uniform(0.5, 2.0, J)
    y = 0.5 + g.normal(0.0, 1.0, J) + sigma * g.normal(0.0, 1.0, J)
    return P.HierarchicalNormalMeans(y, sigma, mu_sd=5.0, tau_scale=5.0, parameterization=param)


def measure(target, explorer, adapt_rounds):
    pt = P.PT(P.Inputs(target=target, reference=P.ScaledPrecisionNormalLogPotential(1.0, target.dim), n_chains=N_CHAINS, n_rounds=20,
                       explorer=explorer, show_report=False, record=[P.round_trip, P.log_sum_ratio]),
              debug_kernel=_lib.KERNEL_TWO_LAUNCHES if isinstance(target, P.Funnel) else 0)
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
    args = ap.parse_args()
    rows = []
    for J in GROUPS:
        d = J + 2
        funnel = {}
        for name, mk, rounds in EXPLORERS:
            try:
                funnel[name] = measure(P.Funnel(d), mk(), rounds)[0]
            except P.PteError as exc:          # (the funnel's neck can exhaust slice_shrink's iterations at a small d: no yardstick for that cell)
                print("d=%-4d funnel %s: %s" % (d, name, exc), flush=True)
                funnel[name] = None
        fmt = lambda v: "%8.3f ms/scan" % v if v is not None else "     n/a"
        print("d=%-4d funnel        " % d + "  ".join("%s %s" % (n, fmt(funnel[n])) for n, _, _ in EXPLORERS), flush=True)
        for param in ("centered", "noncentered"):
            row = dict(J=J, d=d, n_chains=N_CHAINS, parameterization=param, funnel=funnel)
            for name, mk, rounds in EXPLORERS:
                row[name], row["kernel"] = measure(hier_target(J, param), mk(), rounds)
            rows.append(row)
            ratio = lambda n: "x %.2f" % (row[n] / funnel[n]) if funnel[n] else "no yardstick"
            print("d=%-4d %-13s " % (d, param) + "  ".join("%s %8.3f ms/scan (%s)" % (n, row[n], ratio(n)) for n, _, _ in EXPLORERS), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(rows, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
