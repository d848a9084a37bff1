#!/usr/bin/env python3
"""SQ counters of the fused slice kernel per wave and SCAN, dispatch by dispatch, from rocprofv3 result DBs of `bench.py --steps K --warmup W`
(tools/prof_pmc.sh).  rocpd_summary.py prints the mean over dispatches; the bench's launches hold 64 + 64 (preparation) + W + K scans, so the
mean mixes launch sizes.  Here every k_scans_slice8 dispatch is divided by its own number of scans (given in launch order) and its 1024 waves.
*_CYCLES, WAIT_* and ACTIVE_* count quad-cycles (x 4 = cycles).
Usage: python tools/pmc_per_scan.py 64,64,2,4 <p_results.db> [<q_results.db> ...]"""
import sqlite3
import sys


def main():
    scans = [int(s) for s in sys.argv[1].split(",")]
    for path in sys.argv[2:]:
        con = sqlite3.connect(path)
        rows = con.execute("select dispatch_id, counter_name, sum(value), max(duration) from counters_collection "
                           "where kernel_name like '%k_scans_slice8%' group by dispatch_id, counter_name order by dispatch_id").fetchall()
        ids = sorted(set(r[0] for r in rows))
        assert len(ids) == len(scans), (ids, scans)
        print("== %s" % path)
        for d, n in zip(ids, scans):
            c = {r[1]: r[2] for r in rows if r[0] == d}
            w = c.get("SQ_WAVES", 1024.0)
            per = {k: v / w / n for k, v in c.items() if k != "SQ_WAVES"}
            line = "dispatch %4d, %3d scans:" % (d, n) + "".join("  %s %.0f" % (k[3:], v) for k, v in sorted(per.items()))
            if "SQ_WAVE_CYCLES" in per:
                wc = per["SQ_WAVE_CYCLES"]
                line += "  | wave cycles %.3f M" % (4 * wc / 1e6)
                for k in ("SQ_WAIT_ANY", "SQ_WAIT_INST_ANY", "SQ_ACTIVE_INST_ANY"):
                    if k in per:
                        line += "  %s/cycles %.3f" % (k[3:], per[k] / wc)
            print(line)
        con.close()


if __name__ == "__main__":
    main()
