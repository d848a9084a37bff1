"""What the replica-overlap recorder costs per scan, from one process (DESIGN 4.20's table).

    python tools/bench_overlap.py [--out FILE.json] [--chains 512]

512 chains of SpinGlass3DLogPotential.edwards_anderson(1.0, L, seed=1) at L = 16 and 32 under CheckerboardMetropolis(3).  Per L: a pair of PTs
(seeds 1 and 2) with an Overlap between them, adapted together for three rounds (2, 4, 8 scans: run_pair_round / adapt_pair), and a third PT
(seed 3) adapted alone the same way.  Then blocks of 16 scans are timed, the arrangements interleaved block by block (wall clock around
synchronised calls, the method of tools/bench_lattice3d.py -- whose rows are the yardstick for (c)):

    (a) pair     pte_overlap_run_scans: both engines' explore and swap on their own streams, one record per scan
    (b) serial   the pair's two engines, pte_run_scans one after the other, no record
    (c) alone    the third engine's pte_run_scans

Every block's time is kept; reported: ms per scan (best block) and the ratios (a) / (b), (a) / (2 c).  Nothing is asserted."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "pigeons.jl_amd")]
import torch
import pigeons_amd as P
from pigeons_amd.pt import adapt, next_round, reduce_recorders

BLOCK, REPS, N_STEPS = 16, 5, 3


def make_pt(target, n_chains, seed):
    return P.PT(P.Inputs(target=target, n_chains=n_chains, n_rounds=20, seed=seed, explorer=P.CheckerboardMetropolis(N_STEPS), show_report=False,
                         record=[P.round_trip, P.log_sum_ratio]))


def setting(L, n_chains):
    target = P.SpinGlass3DLogPotential.edwards_anderson(1.0, L, seed=1)
    a, b, c = (make_pt(target, n_chains, seed) for seed in (1, 2, 3))
    pair = P.PTPair(a, b, P.Overlap(a.replicas, b.replicas))
    for r in range(1, 4):
        next_round(a); next_round(b)
        P.adapt_pair(pair, *P.run_pair_round(pair))
        c.replicas.run_scans(1, 2 ** r)
        adapt(c, reduce_recorders(c))
    return pair, c


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
    args = ap.parse_args()
    N = args.chains
    out = dict(n_chains=N, n_steps=N_STEPS, block=BLOCK, reps=REPS, settings={})
    for L in (16, 32):
        pair, c = setting(L, N)
        ea, eb, ec = pair.a.replicas, pair.b.replicas, c.replicas

        def serial():
            ea.run_scans(1, BLOCK)
            eb.run_scans(1, BLOCK)
        arrangements = [("pair", lambda: pair.recorder.run_scans(1, BLOCK)), ("serial", serial), ("alone", lambda: ec.run_scans(1, BLOCK))]
        blocks = {name: [] for name, _ in arrangements}
        for _ in range(REPS):
            for name, f in arrangements:
                blocks[name].append(timed(f))
        best = {name: min(v) for name, v in blocks.items()}
        rec = pair.recorder.reduce()
        out["settings"]["L%d" % L] = dict(sites=ea.d, kernel=ea.kernel_name(), ms_per_scan_blocks=blocks, ms_per_scan=best,
                                          pair_over_serial=best["pair"] / best["serial"], pair_over_two_alone=best["pair"] / (2 * best["alone"]),
                                          records_per_chain=int(rec.n[0]), q2_target_chain=float(rec.moments()["q2"][-1]))
        for name, _ in arrangements:
            print("L=%-3d %-7s %8.3f ms/scan   blocks: %s" % (L, name, best[name], " ".join("%.3f" % v for v in blocks[name])), flush=True)
        print("L=%-3d pair / serial %.3f   pair / (2 alone) %.3f   records per chain %d" % (L, best["pair"] / best["serial"], best["pair"] / (2 * best["alone"]), int(rec.n[0])), flush=True)
        pair.recorder.close()
        for e in (ea, eb, ec):
            e.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(out, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
