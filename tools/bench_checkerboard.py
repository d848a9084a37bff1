"""Per-scan timing of CheckerboardMetropolis against IsingMetropolis at the C5 shard shape, from the same process (DESIGN 4.18's table).

    python tools/bench_checkerboard.py [--out FILE.json] [--base-length 256] [--chains 512]

256 x 256 spins, 512 chains, n_steps = 3.  Four engines: (a) IsingMetropolis on IsingLogPotential(1.0, L) -- k_explore_ising_spec, unchanged, the
yardstick; (b) CheckerboardMetropolis on the same target; (c) CheckerboardMetropolis on edwards_anderson(1.0, L, seed=1); (d) instance (c) on
the sites kernel (debug_kernel = PTE_KERNEL_ISING_BYTES).  Every engine adapts its ladder for three rounds (2, 4, 8 scans), then three blocks
of 16 scans are timed per engine, the engines interleaved block by block (wall clock around a synchronised run_scans).  Every block's time is
kept; reported: ms per scan of each (best block), the ratios (b)/(a) and (d)/(c).

The comparison is PER SCAN, not per unit of mixing: a checkerboard sweep and a raster sweep are different Markov kernels with the same cost
model (n_steps updates of every site)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "pigeons.jl_amd")]
import torch
import pigeons_amd as P
from pigeons_amd import _lib
from pigeons_amd.pt import reduce_recorders, adapt

BLOCK, REPS = 16, 3


def engine(target, explorer, n_chains, debug_kernel=0):
    pt = P.PT(P.Inputs(target=target, n_chains=n_chains, n_rounds=20, explorer=explorer, show_report=False,
                       record=[P.round_trip, P.log_sum_ratio]), debug_kernel=debug_kernel)
    for r in range(1, 4):
        pt.replicas.run_scans(1, 2 ** r)
        adapt(pt, reduce_recorders(pt))
    return pt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--base-length", type=int, default=256)
    ap.add_argument("--chains", type=int, default=512)
    args = ap.parse_args()
    L, N = args.base_length, args.chains
    ea = P.SpinGlassLogPotential.edwards_anderson(1.0, L, seed=1)
    pts = [("a_ising_raster", engine(P.IsingLogPotential(1.0, L), P.IsingMetropolis(3), N)),
           ("b_ising_checkerboard", engine(P.IsingLogPotential(1.0, L), P.CheckerboardMetropolis(3), N)),
           ("c_ea_checkerboard", engine(ea, P.CheckerboardMetropolis(3), N)),
           ("d_ea_checkerboard_sites", engine(ea, P.CheckerboardMetropolis(3), N, debug_kernel=_lib.KERNEL_ISING_BYTES))]
    blocks = {name: [] for name, _ in pts}
    for _ in range(REPS):
        for name, pt in pts:
            torch.cuda.synchronize()
            t = time.perf_counter()
            pt.replicas.run_scans(1, BLOCK)
            torch.cuda.synchronize()
            blocks[name].append((time.perf_counter() - t) / BLOCK * 1e3)
    best = {name: min(v) for name, v in blocks.items()}
    out = dict(base_length=L, n_chains=N, n_steps=3, block=BLOCK, reps=REPS,
               kernels={name: pt.replicas.kernel_name() for name, pt in pts}, ms_per_scan_blocks=blocks, ms_per_scan=best,
               ratio_b_over_a=best["b_ising_checkerboard"] / best["a_ising_raster"],
               ratio_d_over_c=best["d_ea_checkerboard_sites"] / best["c_ea_checkerboard"])
    for name, pt in pts:
        print("%-26s %-30s %8.3f ms/scan   blocks: %s" % (name, pt.replicas.kernel_name(), best[name], " ".join("%.3f" % v for v in blocks[name])), flush=True)
        pt.replicas.close()
    print("(b)/(a) %.4f   (d)/(c) %.2f" % (out["ratio_b_over_a"], out["ratio_d_over_c"]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(out, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
