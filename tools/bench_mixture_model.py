"""Per-scan timing of the mixture-model-posterior family (k_explore_mixture_model + the swap launch) -- DESIGN 4.11's table.

    python tools/bench_mixture_model.py [--out FILE.json]

Shapes (n observations, K components): (1024, 2), (4096, 2), (4096, 8), (65536, 4), synthetic standardised data, 1024 chains, reference
ScaledPrecisionNormalLogPotential(1, 3 K).  SliceSampler and AutoMALA adapt for four rounds (the schedule; AutoMALA also its step size and
preconditioner), then run three timed blocks of 16 scans (run_scans; best of three, wall clock around a synchronised call): ms per scan.

A third row per shape, MALA with a fixed step size, counts its work exactly: every non-reference replica evaluates the density with its
gradient 1 + n_refresh times per scan and the density alone once more, the reference replica the density once; an evaluation is one pass
over the n_pad observations with K exp each (and one log per observation).  From the same timing: the exp evaluations per second over the
chip, and the time of one evaluation (the scan's time over the 2 + n_refresh evaluations a replica makes one after the other; the swap
launch and the momentum draws are in it, so it overstates) against the issue floor of the inner loop: VALU instructions per (i, k) counted in
the ISA (--valu-grad / --valu-density, DESIGN 4.11's resource table) x 4 cycles x n_pad / 64 x K at --clock-ghz, one wave alone on its SIMD."""
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
SHAPES = ((1024, 2), (4096, 2), (4096, 8), (65536, 4))
# VALU instructions per (observation, component) of the loop over observations, from the generated code (tools/codegen.py loops()): the
# gradient pass and the density-only pass of the MALA kernel, by component bucket
VALU_GRAD = {2: 108.6, 4: 84.4, 8: 73.5}
VALU_DENSITY = {2: 83.1, 4: 59.1, 8: 48.4}


def target(n, K):
    g = np.random.default_rng(n * 1000 + K)
    k = g.integers(0, K, n)
    y = g.normal(np.linspace(-2.0, 2.0, K)[k], 0.3)
    return P.MixtureModelPosterior((y - y.mean()) / y.std(), K), P.ScaledPrecisionNormalLogPotential(1.0, 3 * K)


def measure(n, K, explorer, adapt_rounds=4):
    t, ref = target(n, K)
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
    ap.add_argument("--clock-ghz", type=float, default=2.4)
    args = ap.parse_args()
    rows = []
    for n, K in SHAPES:
        row = dict(n=n, K=K, n_chains=N_CHAINS)
        for name, mk in (("SliceSampler", P.SliceSampler), ("AutoMALA", P.AutoMALA)):
            row[name] = measure(n, K, mk())["ms_per_scan"]
        mala = P.MALA(step_size=0.01)
        n_refresh = mala.base_n_refresh * int(math.ceil((3 * K) ** mala.exponent_n_refresh))
        ms = measure(n, K, mala, adapt_rounds=1)["ms_per_scan"]
        n_pad = (n + 63) // 64 * 64
        evals = (N_CHAINS - 1) * (2 + n_refresh) + 1
        exps = evals * n_pad * K
        per_eval_us = ms * 1e3 / (2 + n_refresh)
        cycles = 4.0 * (n_pad / 64) * K * ((1 + n_refresh) * VALU_GRAD[K] + VALU_DENSITY[K]) / (2 + n_refresh)
        floor_us = cycles / (args.clock_ghz * 1e3)
        row.update(MALA=ms, mala_n_refresh=n_refresh, exp_per_s=exps / (ms * 1e-3), eval_us=per_eval_us, eval_floor_us=floor_us)
        rows.append(row)
        print("n=%-5d K=%d  SliceSampler %8.3f ms/scan  AutoMALA %8.3f ms/scan  MALA(n_refresh=%d) %8.3f ms/scan: %.2f T exp/s, "
              "%.1f us per evaluation against an issue floor of %.1f us (x%.2f)"
              % (n, K, row["SliceSampler"], row["AutoMALA"], n_refresh, ms, row["exp_per_s"] / 1e12, per_eval_us, floor_us, per_eval_us / floor_us),
              flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(rows, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
