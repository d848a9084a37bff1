"""Per-scan timing of CheckerboardMetropolis on the 3-D spin glass against the 2-D packed kernel, from the same process (DESIGN 4.19's table).

    python tools/bench_lattice3d.py [--out FILE.json] [--chains 512]

512 chains, n_steps = 3.  Five engines: SpinGlass3DLogPotential.edwards_anderson(1.0, L, seed=1) at L = 8, 16, 32 (k_explore_checkerboard3d)
and, as the yardstick, the unchanged 2-D k_explore_checkerboard on SpinGlassLogPotential.edwards_anderson(1.0, 64) and (1.0, 256): 4096 and
65536 sites against 16^3 = 4096 and 32^3 = 32768.  The method is tools/bench_checkerboard.py's: every engine adapts its ladder for three rounds
(2, 4, 8 scans), then three blocks of 16 scans are timed per engine, the engines interleaved block by block (wall clock around a synchronised
run_scans).  Every block's time is kept; reported: ms per scan (best block) and site updates per ns (chains x sites x n_steps per scan).

The comparison is PER SCAN, not per unit of mixing: the lattices differ in dimension, and a 3-D site costs six neighbour terms and three
thresholds against four and two."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "pigeons.jl_amd")]
import torch
import pigeons_amd as P
from pigeons_amd.pt import reduce_recorders, adapt

BLOCK, REPS, N_STEPS = 16, 3, 3


def engine(target, n_chains):
    pt = P.PT(P.Inputs(target=target, n_chains=n_chains, n_rounds=20, explorer=P.CheckerboardMetropolis(N_STEPS), show_report=False,
                       record=[P.round_trip, P.log_sum_ratio]))
    for r in range(1, 4):
        pt.replicas.run_scans(1, 2 ** r)
        adapt(pt, reduce_recorders(pt))
    return pt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--chains", type=int, default=512)
    args = ap.parse_args()
    N = args.chains
    pts = [("ea3d_L%d" % L, engine(P.SpinGlass3DLogPotential.edwards_anderson(1.0, L, seed=1), N)) for L in (8, 16, 32)]
    pts += [("ea2d_L%d" % L, engine(P.SpinGlassLogPotential.edwards_anderson(1.0, L, seed=1), N)) for L in (64, 256)]
    blocks = {name: [] for name, _ in pts}
    for _ in range(REPS):
        for name, pt in pts:
            torch.cuda.synchronize()
            t = time.perf_counter()
            pt.replicas.run_scans(1, BLOCK)
            torch.cuda.synchronize()
            blocks[name].append((time.perf_counter() - t) / BLOCK * 1e3)
    best = {name: min(v) for name, v in blocks.items()}
    sites = {name: pt.replicas.d for name, pt in pts}
    rate = {name: N * sites[name] * N_STEPS / (best[name] * 1e6) for name in best}          # site updates per ns
    out = dict(n_chains=N, n_steps=N_STEPS, block=BLOCK, reps=REPS, sites=sites, kernels={name: pt.replicas.kernel_name() for name, pt in pts},
               ms_per_scan_blocks=blocks, ms_per_scan=best, site_updates_per_ns=rate)
    for name, pt in pts:
        print("%-10s %-26s %6d sites %8.3f ms/scan %7.2f updates/ns   blocks: %s"
              % (name, pt.replicas.kernel_name(), sites[name], best[name], rate[name], " ".join("%.3f" % v for v in blocks[name])), flush=True)
        pt.replicas.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(out, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
