"""Per-scan timing of AAPS (k_explore_aaps + the swap launch) against AutoMALA at the same shapes, from the same run (DESIGN 4.7's table).

    python tools/bench_aaps.py [--out FILE.json]

Shapes: toy_mvn_target(128), toy_mvn_target(512), Funnel(128) -- 1024 chains each.  Every engine adapts for four rounds (the schedule and
the preconditioner's std deviations; AutoMALA also its step size), then runs three timed blocks of 16 scans (run_scans; best of three,
wall clock around a synchronised call).  Reported per shape and explorer: ms per scan; for AAPS also the mean leapfrog steps per replica
and scan (explorer_n_steps over the timed scans, reference chain excluded), its maximum over the chains, and us per mean leapfrog step."""
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


def inputs(shape, explorer):
    kind, d = shape
    if kind == "funnel":
        return P.Inputs(target=P.Funnel(d), reference=P.ScaledPrecisionNormalLogPotential(1 / 9., d), n_chains=N_CHAINS, n_rounds=20,
                        explorer=explorer, show_report=False, record=[P.round_trip, P.log_sum_ratio])
    return P.Inputs(target=P.toy_mvn_target(d), n_chains=N_CHAINS, n_rounds=20, explorer=explorer, show_report=False,
                    record=[P.round_trip, P.log_sum_ratio])


def measure(shape, explorer):
    pt = P.PT(inputs(shape, explorer))
    e = pt.replicas
    for r in range(1, 5):
        e.run_scans(1, 2 ** r)
        adapt(pt, reduce_recorders(pt))
    best = 1e9
    for _ in range(REPS):
        torch.cuda.synchronize()
        t = time.perf_counter()
        e.run_scans(1, BLOCK)
        torch.cuda.synchronize()
        best = min(best, (time.perf_counter() - t) / BLOCK * 1e3)
    e.reduce()
    _, _, ss, sn = e.explorer_stats()
    out = dict(ms_per_scan=best, kernel=e.kernel_name())
    if isinstance(explorer, P.AAPS):
        live = sn > 0
        per = ss[live] / sn[live]
        out.update(mean_steps=float(ss[live].sum() / sn[live].sum()), max_chain_mean_steps=float(per.max()))
        out["us_per_step"] = best * 1e3 / out["mean_steps"]
    e.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    rows = []
    for shape in (("mvn", 128), ("mvn", 512), ("funnel", 128)):
        aaps = measure(shape, P.AAPS())
        am = measure(shape, P.AutoMALA())
        row = dict(shape="%s(%d)" % shape, n_chains=N_CHAINS, aaps=aaps, automala=am)
        rows.append(row)
        print("%-12s N=%d  AAPS %.3f ms/scan  %.1f steps/replica/scan (chain max %.1f)  %.2f us/step   AutoMALA %.3f ms/scan"
              % (row["shape"], N_CHAINS, aaps["ms_per_scan"], aaps["mean_steps"], aaps["max_chain_mean_steps"], aaps["us_per_step"],
                 am["ms_per_scan"]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(rows, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
