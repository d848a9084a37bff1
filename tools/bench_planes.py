"""What the plane autocorrelation of a lattice pair (k_overlap_planes) adds per scan, from one process (DESIGN 4.22's table).

    python tools/bench_planes.py [--out FILE.json] [--chains 512]

512 chains of edwards_anderson(1.0, L, seed=1) under CheckerboardMetropolis(3): the cube (SpinGlass3DLogPotential) at L = 16 and 32 and the
256 x 256 square (SpinGlassLogPotential), the largest lattice the recorder admits.  Per setting: a pair of PTs (seeds 1 and 2) with an
Overlap between them, adapted together for three rounds (2, 4, 8 scans: run_pair_round / adapt_pair).  Then blocks of paired scans
(pte_overlap_run_scans: both engines' explore and swap, one record per scan) are timed with the feature off and on, interleaved block by
block (wall clock around synchronised calls, the method of tools/bench_overlap.py):

    (off)  the pair as it is without the feature: the baseline
    (on)   the same pair with Overlap.set_planes(True): one launch of k_overlap_planes more per scan

Every block's time is kept; reported: ms per scan (best block and median), the difference on - off in microseconds per scan and per chain,
and the ratio on / off.  Nothing is asserted."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "pigeons.jl_amd")]
import torch
import pigeons_amd as P
from pigeons_amd.pt import next_round

REPS, N_STEPS = 7, 3
SETTINGS = [("cube16", "cube", 16, 16), ("cube32", "cube", 32, 16), ("square256", "square", 256, 8)]      # name, family, L, scans per block


def setting(family, L, n_chains):
    family_of = {"cube": P.SpinGlass3DLogPotential, "square": P.SpinGlassLogPotential}
    target = family_of[family].edwards_anderson(1.0, L, seed=1)
    a, b = (P.PT(P.Inputs(target=target, n_chains=n_chains, n_rounds=20, seed=seed, explorer=P.CheckerboardMetropolis(N_STEPS), show_report=False,
                          record=[P.round_trip, P.log_sum_ratio])) for seed in (1, 2))
    pair = P.PTPair(a, b, P.Overlap(a.replicas, b.replicas))
    for _ in range(3):
        next_round(a); next_round(b)
        P.adapt_pair(pair, *P.run_pair_round(pair))
    return pair


def timed(f, block):
    torch.cuda.synchronize()
    t = time.perf_counter()
    f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / block * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--chains", type=int, default=512)
    args = ap.parse_args()
    N = args.chains
    out = dict(n_chains=N, n_steps=N_STEPS, reps=REPS, settings={})
    for name, family, L, block in SETTINGS:
        pair = setting(family, L, N)
        ov = pair.recorder
        blocks = {"off": [], "on": []}
        for on in (False, True):                               # one untimed block each: the first launch of a kernel loads its code
            ov.set_planes(on)
            ov.run_scans(1, 2)
        for _ in range(REPS):
            for key, on in (("off", False), ("on", True)):
                ov.set_planes(on)
                blocks[key].append(timed(lambda: ov.run_scans(1, block), block))
        best = {k: min(v) for k, v in blocks.items()}
        med = {k: statistics.median(v) for k, v in blocks.items()}
        rec = ov.reduce()
        cl = rec.correlation_length()
        out["settings"][name] = dict(family=family, L=L, sites=ov.d, block=block, kernel=pair.a.replicas.kernel_name(), ms_per_scan_blocks=blocks,
                                     ms_per_scan=best, ms_per_scan_median=med, added_us_per_scan=(best["on"] - best["off"]) * 1e3,
                                     added_us_per_scan_median=(med["on"] - med["off"]) * 1e3, added_ns_per_chain=(best["on"] - best["off"]) * 1e6 / N,
                                     on_over_off=best["on"] / best["off"], records_per_chain=int(rec.n[0]), plane_records_per_chain=int(rec.plane_n[0]),
                                     xi_over_L_target_chain=float(cl["xi_over_L"][-1]))
        for k in ("off", "on"):
            print("%-10s %-3s %9.4f ms/scan (median %9.4f)   blocks: %s" % (name, k, best[k], med[k], " ".join("%.4f" % v for v in blocks[k])), flush=True)
        print("%-10s on - off %+8.1f us/scan (median %+8.1f)   on / off %.4f   plane records per chain %d of %d" %
              (name, (best["on"] - best["off"]) * 1e3, (med["on"] - med["off"]) * 1e3, best["on"] / best["off"], int(rec.plane_n[0]), int(rec.n[0])), flush=True)
        ov.close()
        for e in (pair.a.replicas, pair.b.replicas):
            e.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(out, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
