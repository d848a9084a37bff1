"""Per-scan timing of the spin-glass family against the Ising family at the C5 shard shape, from the same run (DESIGN 4.17's table).

    python tools/bench_spinglass.py [--out FILE.json] [--base-length 256] [--chains 512]

256 x 256 spins, 512 chains, IsingMetropolis(3).  Four engines: (a) IsingLogPotential(1.0, L) -- k_explore_ising_spec, the reference of the
comparison; (b) the spin glass with every bond +1; (c) an Edwards-Anderson instance (seed 1); (d) instance (c) on the byte kernel
(debug_kernel = PTE_KERNEL_ISING_BYTES).  Every engine adapts its ladder for three rounds (2, 4, 8 scans), then three blocks of 16 scans are
timed per engine, the engines interleaved block by block (wall clock around a synchronised run_scans; best of three).  Reported: ms per scan
of each, the ratios (b)/(a), (c)/(a) and (d)/(c)."""
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

BLOCK, REPS = 16, 3


def engine(target, n_chains, debug_kernel=0):
    pt = P.PT(P.Inputs(target=target, n_chains=n_chains, n_rounds=20, explorer=P.IsingMetropolis(3), show_report=False,
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
    ones = np.ones((L, L), dtype=np.int8)
    ea = P.SpinGlassLogPotential.edwards_anderson(1.0, L, seed=1)
    pts = [("ising", engine(P.IsingLogPotential(1.0, L), N)),
           ("spin_glass_all_ferro", engine(P.SpinGlassLogPotential(1.0, ones, ones), N)),
           ("spin_glass_ea", engine(ea, N)),
           ("spin_glass_ea_bytes", engine(ea, N, debug_kernel=_lib.KERNEL_ISING_BYTES))]
    best = {name: 1e9 for name, _ in pts}
    for _ in range(REPS):
        for name, pt in pts:
            torch.cuda.synchronize()
            t = time.perf_counter()
            pt.replicas.run_scans(1, BLOCK)
            torch.cuda.synchronize()
            best[name] = min(best[name], (time.perf_counter() - t) / BLOCK * 1e3)
    out = dict(base_length=L, n_chains=N, n_steps=3, block=BLOCK, reps=REPS,
               kernels={name: pt.replicas.kernel_name() for name, pt in pts}, ms_per_scan=best,
               ratio_all_ferro_over_ising=best["spin_glass_all_ferro"] / best["ising"],
               ratio_ea_over_ising=best["spin_glass_ea"] / best["ising"],
               ratio_bytes_over_spec_ea=best["spin_glass_ea_bytes"] / best["spin_glass_ea"])
    for name, pt in pts:
        print("%-22s %-26s %8.3f ms/scan" % (name, pt.replicas.kernel_name(), best[name]), flush=True)
        pt.replicas.close()
    print("(b)/(a) %.3f   (c)/(a) %.3f   bytes/spec on (c) %.2f" % (out["ratio_all_ferro_over_ising"], out["ratio_ea_over_ising"],
                                                                    out["ratio_bytes_over_spec_ea"]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(out, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
