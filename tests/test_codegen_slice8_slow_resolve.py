"""The generated code of round 11 (pte_slice8.hpp): the fill of a draw window decides the slow-path exponentials it can and leaves a record per
lane in LDS; behind the slow-mask branch lane 0 looks its position up before it runs the sequential procedure of round 10.

Held here, in k_scans_slice8<4, 9> (the kernel the metric runs) and k_explore_slice8<4, 9>, on the product's assembly with the shipped flags
(tools/codegen.py, cached under build/codegen/):
  * the likely path of the round is the one recorded in profiles/r09_slice8_round_loop.txt -- 259 = 192 VALU + 57 scalar + 10 LDS instructions in
    8 blocks, five dynamic v_readlane, no spill, no scratch -- and the kernels stay within their register and LDS budgets;
  * the region behind the slow-mask branch BEGINS with the lookup: the record words are read from LDS (the table lies behind the policy word,
    at byte 14344 and beyond) ahead of everything else that waits, and the region holds no vector-memory instruction and no vmcnt wait;
  * the record table is written by the fills only: inside the round loop, in the blocks reachable from the refill branch (the first branch out
    of the likely path) and nowhere else -- not on the likely path, not behind the slow-mask branch;
  * the fill's two ZIG_FE words are its only vector-memory instructions."""
import os
import re
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from test_codegen_slice8_slow_exp import KERNELS, _recorded, _region, _round

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")

TABLE_AT = 14344                 # u, e (2 x 4096), x (2048), we, ke (2 x 2048), policy (8): the records lie behind them


@pytest.fixture(scope="module")
def cg():
    import codegen as C
    units = C.compile_units()
    return C, C.resources(units), C.asm_lines(units)


def _table_access(t, op):
    return t.startswith(op) and any(int(o) >= TABLE_AT for o in re.findall(r"offset[01]?:(\d+)", t))


@pytest.mark.parametrize("kernel,sub,depth", KERNELS)
def test_likely_path_and_budgets(cg, kernel, sub, depth):
    C, res, lines = cg
    body, hot, names = _round(C, lines, sub, depth)
    t, rec = C.totals(hot), _recorded()
    print(kernel, t)
    assert rec == {"v": 192, "s": 57, "l": 10, "m": 0, "instructions": 259, "blocks": 8}
    assert {k: t[k] for k in rec} == rec, (t, rec)
    assert t["dyn"] == 5 and t["w"] == 0 and t["r"] == 0 and t["scratch"] == 0, t
    r = res[kernel]
    print(kernel, r)
    assert r["spilled_vgpr"] == 0 and r["scratch_B_per_lane"] == 0 and r["vgpr"] <= (200 if depth == 3 else 248) and r["lds_B"] <= 16384, r


@pytest.mark.parametrize("kernel,sub,depth", KERNELS)
def test_slow_mask_region_begins_with_the_lookup(cg, kernel, sub, depth):
    C, res, lines = cg
    body, hot, names = _round(C, lines, sub, depth)
    b = next(b for b in hot if any(t.startswith("s_movrels_b32") for t in b["text"]))
    assert len(b["branches"]) == 1 and b["branches"][0] not in names, b["branches"]
    reg = _region(C, body, b["branches"][0], names)
    entry = next(r for r in reg if r["name"] == b["branches"][0])
    text = [t for r in reg for t in r["text"]]
    print(kernel, "entry block:", entry["text"])
    # the first instructions of the entry block that touch memory or wait are the reads of the record's words
    mem = [t for t in entry["text"] if re.match(r"^(ds_|s_load|s_waitcnt|global_|flat_|buffer_|scratch_)", t)]
    n_reads = next(i for i, t in enumerate(mem + ["end"]) if not t.startswith("ds_read"))
    assert n_reads >= 1 and all(_table_access(t, "ds_read") for t in mem[:n_reads]), mem
    assert mem[n_reads].startswith("s_waitcnt") and "vmcnt" not in mem[n_reads], mem
    assert not any(t.startswith("v_rndne_f64") for t in entry["text"]), "the sequential procedure runs ahead of the lookup"
    assert sum(r["m"] for r in reg) == 0, [t for t in text if re.match(r"^(global|scratch|buffer|flat)_", t)]
    assert not any(t.startswith("s_waitcnt") and "vmcnt" in t for t in text)
    assert not any(_table_access(t, "ds_write") for t in text)


@pytest.mark.parametrize("kernel,sub,depth", KERNELS)
def test_the_table_is_written_by_the_fills_only(cg, kernel, sub, depth):
    C, res, lines = cg
    body, hot, names = _round(C, lines, sub, depth)
    header = next(h for d, h in C.loop_headers(body) if d == depth)
    assert not any(_table_access(t, "ds_write") for b in hot for t in b["text"])
    first = next(t for b in hot for t in b["branches"] if t not in names)          # p > REFILL_AT is the round's first test
    refill = _region(C, body, first, names)
    inside = set(r["name"] for r in refill)
    writers = [b for b in C.blocks_of(body) if any(_table_access(t, "ds_write") for t in b["text"])]
    in_loop = [b for b in writers if b["head"] == header or header in b.get("parents", [])]
    print(kernel, "blocks that write the table:", [(b["name"], b["depth"]) for b in writers], "refill region:", sorted(inside))
    assert in_loop and all(b["name"] in inside for b in in_loop), [b["name"] for b in in_loop]
    assert any(b not in in_loop for b in writers), "the first fill of an explore step writes the table too"
    # the refill: window stores, the record's two words, and the gather of the two ZIG_FE words as its only vector memory
    text = [t for r in refill for t in r["text"]]
    assert sum(r["m"] for r in refill) == 2 and all(t.startswith("global_load_dwordx2") for t in text if re.match(r"^(global|scratch|buffer|flat)_", t)), \
        [t for t in text if re.match(r"^(global|scratch|buffer|flat)_", t)]
    assert sum(_table_access(t, "ds_write") for t in text) == 2
