"""What Houdayer's cluster move costs per scan and how much of the disagreeing sites it flips, from one process (DESIGN 4.21's tables).

    python tools/bench_cluster.py [--out FILE.json] [--chains 512] [--lib PATH]

512 chains of edwards_anderson(1.0, L, seed=1) under CheckerboardMetropolis(3): the cube at L = 16 and L = 32, the 2-D glass at 256 x 256.
Per setting: a pair of PTs (seeds 1 and 2) with an Overlap between them, adapted together for five rounds (2 .. 32 scans: run_pair_round /
adapt_pair) with the move off.  Then blocks of 16 scans of pte_overlap_run_scans are timed, the two arrangements interleaved block by block
(wall clock around synchronised calls, the method of tools/bench_overlap.py):

    (a) off      HoudayerMove(every=0): today's launches
    (b) every 1  HoudayerMove(every=1): one move per scan, after both swaps and ahead of the record

Every block's time is kept; reported: ms per scan (best block) of both, their difference and ratio -- read (b) against (a) of the same process,
not against another table -- and per chain mean_fraction() = size_sum / k_sum and the passes of the kernel's fixed-point loop per move, over the
moves of the (b) blocks.  --lib: another build of libpte (the one-wave build of the kernel, -DPTE_CLUSTER_THREADS=64).  Nothing is asserted."""
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
from pigeons_amd.pt import next_round

BLOCK, REPS, N_STEPS, ROUNDS = 16, 5, 3, 5
SETTINGS = [("cube L16", lambda: P.SpinGlass3DLogPotential.edwards_anderson(1.0, 16, seed=1)),
            ("cube L32", lambda: P.SpinGlass3DLogPotential.edwards_anderson(1.0, 32, seed=1)),
            ("square L256", lambda: P.SpinGlassLogPotential.edwards_anderson(1.0, 256, seed=1))]


def make_pt(target, n_chains, seed):
    return P.PT(P.Inputs(target=target, n_chains=n_chains, n_rounds=20, seed=seed, explorer=P.CheckerboardMetropolis(N_STEPS), show_report=False,
                         record=[P.round_trip, P.log_sum_ratio]))


def setting(target, n_chains):
    a, b = (make_pt(target, n_chains, seed) for seed in (1, 2))
    pair = P.PTPair(a, b, P.Overlap(a.replicas, b.replicas))
    for _ in range(ROUNDS):
        next_round(a); next_round(b)
        P.adapt_pair(pair, *P.run_pair_round(pair))
    return pair


def timed(f):
    torch.cuda.synchronize()
    t = time.perf_counter()
    f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / BLOCK * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--chains", type=int, default=512)
    ap.add_argument("--lib", default=None)
    ap.add_argument("--only", default=None, help="a setting's name, e.g. 'cube L32'")
    args = ap.parse_args()
    if args.lib:
        P._lib.use_library(os.path.abspath(args.lib))
    N = args.chains
    out = dict(n_chains=N, n_steps=N_STEPS, block=BLOCK, reps=REPS, lib=args.lib, settings={})
    for name, make_target in SETTINGS:
        if args.only and args.only != name:
            continue
        pair = setting(make_target(), N)
        ov = pair.recorder
        off, on = P.HoudayerMove(every=0, seed=1), P.HoudayerMove(every=1, seed=1)
        ov.reduce()

        def run(move):
            ov.set_cluster_move(move)
            ov.run_scans(1, BLOCK)
        blocks = {"off": [], "every1": []}
        for _ in range(REPS):
            blocks["off"].append(timed(lambda: run(off)))
            blocks["every1"].append(timed(lambda: run(on)))
        best = {k: min(v) for k, v in blocks.items()}
        ov.reduce()
        cl = ov.reduce_clusters()
        moved = np.maximum(cl.n - cl.empty, 1)
        frac, passes = cl.mean_fraction(), cl.passes_sum / moved
        out["settings"][name] = dict(sites=pair.a.replicas.d, kernel=pair.a.replicas.kernel_name(), ms_per_scan_blocks=blocks, ms_per_scan=best,
                                     move_ms=best["every1"] - best["off"], every1_over_off=best["every1"] / best["off"],
                                     moves_per_chain=int(cl.n[0]), moves_launched=cl.moves_launched, betas=cl.betas.tolist(),
                                     mean_fraction=frac.tolist(), passes_per_move=passes.tolist(), mean_size=(cl.size_sum / moved).tolist(),
                                     mean_k=(cl.k_sum / moved).tolist())
        for k in ("off", "every1"):
            print("%-12s %-7s %8.3f ms/scan   blocks: %s" % (name, k, best[k], " ".join("%.3f" % v for v in blocks[k])), flush=True)
        print("%-12s move %+.3f ms/scan   every1 / off %.3f   moves per chain %d" % (name, best["every1"] - best["off"], best["every1"] / best["off"], int(cl.n[0])), flush=True)
        for c in sorted(set(list(range(0, N, max(1, N // 8))) + [N - 1])):
            print("%-12s chain %4d beta %.4f   fraction %.4f   passes / move %7.2f   |C| %9.1f   k %9.1f" % (name, c, cl.betas[c], frac[c], passes[c], cl.size_sum[c] / moved[c], cl.k_sum[c] / moved[c]), flush=True)
        ov.close()
        for e in (pair.a.replicas, pair.b.replicas):
            e.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(out, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
