"""Per-scan timing of the Poisson change-point family (k_explore_changepoint + the swap launch) under both evaluation forms -- DESIGN
4.13's table.

    python tools/bench_changepoint.py [--out FILE.json]

Shapes (n observations, K change points; the state has 2 K + 1 coordinates): (1024, 7), (65536, 7), (4096, 31), (4096, 63), synthetic
piecewise-constant Poisson counts with K + 1 segments of equal length, 1024 chains, reference ScaledPrecisionNormalLogPotential(1, K + 1).
One engine per shape: SliceSampler adapts the schedule for four rounds, then the two forms -- the full evaluation and the cached one,
pte_set_changepoint_form -- take turns at timed blocks of 16 scans (run_scans; best of three per form, wall clock around a synchronised
call): ms per scan.  The forms compute the same bits, so both continue the one run.

From the explorer recorders of a form's timed blocks: the density evaluations per scan that the recorders count -- per visit of a
coordinate the two end points, the doubling steps and the shrinkage steps (explorer_n_steps); the re-evaluations inside slice_accept are
not recorded, so this is a lower bound -- and from it the evaluations per second."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "pigeons.jl_amd"), os.path.join(ROOT, "tools")]
import numpy as np
import torch
import pigeons_amd as P
from pigeons_amd import _lib
from pigeons_amd.pt import reduce_recorders, adapt

N_CHAINS, BLOCK, REPS = 1024, 16, 3
SHAPES = ((1024, 7), (65536, 7), (4096, 31), (4096, 63))
FORMS = (("full", _lib.CHANGEPOINT_FORM_FULL), ("cached", _lib.CHANGEPOINT_FORM_CACHED))


def target(n, K):
    g = np.random.default_rng(n * 1000 + K)
    rates = g.uniform(0.5, 12.0, K + 1)
    y = g.poisson(rates[np.minimum(np.arange(n) * (K + 1) // n, K)]).astype(float)
    return P.PoissonChangePoint(y, K), P.ScaledPrecisionNormalLogPotential(1.0, K + 1)


def measure(n, K, adapt_rounds=4):
    t, ref = target(n, K)
    pt = P.PT(P.Inputs(target=t, reference=ref, n_chains=N_CHAINS, n_rounds=20, explorer=P.SliceSampler(), show_report=False,
                       record=[P.round_trip, P.log_sum_ratio]))
    e = pt.replicas
    for r in range(1, adapt_rounds + 1):
        e.run_scans(1, 2 ** r)
        adapt(pt, reduce_recorders(pt))
    out = {name: dict(ms_per_scan=1e9, steps=0.0) for name, _ in FORMS}
    for _ in range(REPS):
        for name, form in FORMS:                # interleaved: a drift of the clocks meets both forms alike
            e.set_changepoint_form(form)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e.run_scans(2, BLOCK)
            torch.cuda.synchronize()
            out[name]["ms_per_scan"] = min(out[name]["ms_per_scan"], (time.perf_counter() - t0) / BLOCK * 1e3)
            e.reduce()                          # the recorders of this block alone
            _, _, steps_sum, steps_n = e.explorer_stats()
            out[name]["steps"] += float(np.sum(steps_sum)) + float(np.sum(steps_n))
    for name, _ in FORMS:
        out[name]["evals_per_scan"] = out[name].pop("steps") / (REPS * BLOCK)
    out["kernel"] = e.kernel_name()
    e.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    rows = []
    for n, K in SHAPES:
        m = measure(n, K)
        for name, _ in FORMS:
            r = m[name]
            per_s = r["evals_per_scan"] / (r["ms_per_scan"] * 1e-3)
            rows.append(dict(n=n, K=K, n_chains=N_CHAINS, family="change_point", form=name, SliceSampler=r["ms_per_scan"], kernel=m["kernel"],
                             evals_per_scan=r["evals_per_scan"], evals_per_s=per_s))
            print("changepoint n=%-5d K=%-2d %-6s SliceSampler %9.3f ms/scan  >= %.3g evaluations/scan, %.3g /s"
                  % (n, K, name, r["ms_per_scan"], r["evals_per_scan"], per_s), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(rows, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
