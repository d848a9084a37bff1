"""Lane 0's slow-path head exponential in the speculative round of the default SliceSampler kernel after round 10 (pte_slice8.hpp).

Before round 10 every entry into the slow path (2.3 % of the coordinates) paid for the policy word of the ziggurat TAIL (3e-4 of the draws): hipcc
had hoisted the loop-invariant load of g_rng_policy out of the candidate loop to the entry of the path -- a pc-relative address, a scalar load
of it, a global_load_dword and an s_waitcnt vmcnt(0).  Now the kernel keeps the word in LDS and reads it on the tail branch only, and the table
words of a candidate are requested together and waited for once (randexp_from_raw_hot, pte_device.hpp).

Held here, in k_scans_slice8<4, 9> (the kernel the metric runs) and k_explore_slice8<4, 9>, on the product's assembly with the shipped flags
(tools/codegen.py, cached under build/codegen/):
  * the blocks reachable from the target of the slow-mask branch without passing through the round's likely path -- the entry block, the
    wedge path, the candidate loop, and the tail with them -- hold no vector-memory instruction and do not name g_rng_policy;
  * a candidate's four table words are loaded in ONE block, with one wait behind them;
  * the likely path of the round has exactly the totals recorded for the parent (profiles/r09_slice8_round_loop.txt).
(The refill's pre-scaled table, which round 10 also built, was measured, found within the noise and taken out again: the refill block is the
parent's and nothing is asserted on it.  profiles/r10_slice8_summary.txt)"""
import os
import re
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")

KERNELS = [("k_scans_slice8<4, 9>", "k_scans_slice8ILi4ELi9E", 4), ("k_explore_slice8<4, 9>", "k_explore_slice8ILi4ELi9E", 3)]


def _recorded():
    """the parent's likely path: VALU, scalar, LDS, vector memory, instructions, blocks"""
    text = open(os.path.join(ROOT, "profiles", "r09_slice8_round_loop.txt")).read()
    assert "k_scans_slice8<4, 9>" in text
    m = re.search(r"# HOT path per round: (\d+) VALU \+ (\d+) SALU \+ (\d+) LDS \+ (\d+) VMEM = (\d+) instructions in (\d+) blocks", text)
    return dict(zip(("v", "s", "l", "m", "instructions", "blocks"), map(int, m.groups())))


@pytest.fixture(scope="module")
def cg():
    import codegen as C
    units = C.compile_units()
    return C, C.resources(units), C.asm_lines(units)


def _region(C, body, entry, stop):
    """the blocks reachable from the label `entry` by branches and fall-through without entering a block named in `stop`, in layout order"""
    bl = C.blocks_of(body)
    at = {b["name"]: i for i, b in enumerate(bl)}
    seen, todo = set(), [entry]
    while todo:
        n = todo.pop()
        if n in seen or n in stop:
            continue
        seen.add(n)
        b = bl[at[n]]
        todo += b["branches"]
        last = b["text"][-1] if b["text"] else ""
        if not re.match(r"^(s_branch|s_endpgm|s_setpc)", last) and at[n] + 1 < len(bl):
            todo.append(bl[at[n] + 1]["name"])
    return [bl[i] for i in sorted(at[n] for n in seen)]


def _round(C, lines, sub, depth):
    name, body = C.kernel_body(lines, sub)
    header = next(h for d, h in C.loop_headers(body) if d == depth)
    hot = C.hot_path(body, header)
    return body, hot, set(b["name"] for b in hot)


@pytest.mark.parametrize("kernel,sub,depth", KERNELS)
def test_slow_path_exponential_reads_no_vector_memory_and_no_policy_word(cg, kernel, sub, depth):
    C, res, lines = cg
    body, hot, names = _round(C, lines, sub, depth)
    # the slow-mask test: bit p of the mask tuple selected through M0, a bit test, ONE conditional branch out of the likely path
    b = next(b for b in hot if any(t.startswith("s_movrels_b32") for t in b["text"]))
    assert len(b["branches"]) == 1 and b["branches"][0] not in names, b["branches"]
    reg = _region(C, body, b["branches"][0], names)
    text = [t for r in reg for t in r["text"]]
    print(kernel, "slow-path exponential:", [(r["name"], r["v"], r["s"], r["l"], r["m"]) for r in reg])
    assert any(t.startswith("v_rndne_f64") for t in text), "this is not the ziggurat's wedge test (exp(-x) rounds its argument to a multiple of ln 2)"
    assert sum(r["m"] for r in reg) == 0, [t for t in text if re.match(r"^(global|scratch|buffer|flat)_", t)]
    assert not any("g_rng_policy" in t for t in text), [t for t in text if "g_rng_policy" in t]
    assert not any(t.startswith("s_waitcnt") and "vmcnt" in t for t in text)
    # the tail is in the region (it reads the kernel's own copy of the word from LDS)
    assert any(t.startswith("ds_read_b32") for t in text)
    # the candidate's table words -- we[idx], ke[idx], fe[idx - 1], fe[idx] -- are requested in one block, ahead of the first wait in it
    cand = [r for r in reg if sum(t.startswith("s_load_dwordx") for t in r["text"]) > 0]
    assert len(cand) == 1, [r["name"] for r in cand]
    ops = [t.split()[0] for t in cand[0]["text"] if t.startswith(("s_load_dwordx", "s_waitcnt"))]
    assert ops == ["s_load_dwordx2"] * 4 + ["s_waitcnt"], ops


@pytest.mark.parametrize("kernel,sub,depth", KERNELS)
def test_likely_path_is_the_parents(cg, kernel, sub, depth):
    C, res, lines = cg
    body, hot, names = _round(C, lines, sub, depth)
    t, rec = C.totals(hot), _recorded()
    print(kernel, t)
    assert {k: t[k] for k in rec} == rec, (t, rec)
    assert t["dyn"] == 5 and t["w"] == 0 and t["r"] == 0 and t["scratch"] == 0, t
    r = res[kernel]
    # (VGPRs: tests/test_codegen_frozen.py's 200 for the per-scan kernel; the fused kernel held 248 before round 10 and 204 after it)
    assert r["spilled_vgpr"] == 0 and r["scratch_B_per_lane"] == 0 and r["vgpr"] <= (200 if depth == 3 else 248) and r["lds_B"] <= 16384, r
