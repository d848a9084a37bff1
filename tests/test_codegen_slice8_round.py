"""The speculative round of the default SliceSampler kernel, frozen at its round-7 size.

Round 7 took instructions OUT of the round (a lone wave per SIMD pays an issue slot for every one of them): every slice test is one v_fma_f64
where it was v_mul_f64 + v_add_f64, and the doubling step of the default kernel extends the interval arithmetically -- two v_cndmask halves and
four v_fma_f64 -- where it computed both candidates and selected five 64-bit values.  301 -> 268 instructions per round in the default
kernel, 375 -> 354 in the many-replica twin.  tests/test_codegen_frozen.py keeps its (upper) bounds from before; this module holds the
round loop to the new numbers plus at most four instructions of slack each, so that a change which puts the selects or the separate
multiplies back fails here.  Same source of truth as there: tools/codegen.py compiles the product's translation units with the shipped flags
(cached under build/codegen/) and counts the blocks from the round loop's header to its back edge."""
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")

SLACK = 4
ROUND = {"instructions": 268, "v": 205, "s": 53}             # 205 VALU + 53 scalar + 10 LDS, as shipped
TWIN = {4: 354, 5: 354, 6: 354}                              # k_explore_slice8_lds10k<NLU, 9>: 262 VALU + 82 scalar + 10 LDS


@pytest.fixture(scope="module")
def cg():
    import codegen as C
    units = C.compile_units()
    return C, C.resources(units), C.asm_lines(units)


def _round(C, lines, sub, depth):
    name, body = C.kernel_body(lines, sub)
    header = next(h for d, h in C.loop_headers(body) if d == depth)
    return C.totals(C.hot_path(body, header))


def _check_default(t):
    for k, v in ROUND.items():
        assert t[k] <= v + SLACK, (k, t)
    assert t["l"] <= 10 and t["dyn"] == 5, t                  # the chase's five v_readlane are the only lane instructions
    assert t["w"] == 0 and t["r"] == 0 and t["scratch"] == 0 and t["m"] == 0, t
    assert t["blocks"] <= 8, t


@pytest.mark.parametrize("nlu", [4, 6])
def test_explore_round_loop(cg, nlu):
    """k_explore_slice8<NLU, 9> (d = 1024 and d = 4096), replica -> pass -> block -> ROUND: 268 instructions = 205 VALU + 53 scalar + 10 LDS in
    8 blocks, five lane instructions, no spill, no scratch (round 6: 301 = 238 + 53 + 10)."""
    C, res, lines = cg
    _check_default(_round(C, lines, "k_explore_slice8ILi%dELi9E" % nlu, 3))
    r = res["k_explore_slice8<%d, 9>" % nlu]
    assert r["spilled_vgpr"] == 0 and r["scratch_B_per_lane"] == 0, r


@pytest.mark.parametrize("nlu", [0, 4, 5])
def test_scan_loop_round_loop(cg, nlu):
    """k_scans_slice8<NLU, 9> (the fused scan loop; the metric runs <4, 9>), scan -> pass -> block -> ROUND: the same 268 = 205 + 53 + 10 in 8
    blocks; the three constant registers of the doubling block (two zero dwords, the high word of 1.0) are set once per scan, outside the
    round loop, and the kernel stays free of VGPR spills and scratch."""
    C, res, lines = cg
    _check_default(_round(C, lines, "k_scans_slice8ILi%dELi9E" % nlu, 4))
    r = res["k_scans_slice8<%d, 9>" % nlu]
    assert r["spilled_vgpr"] == 0 and r["scratch_B_per_lane"] == 0 and r["vgpr"] <= 256, r


@pytest.mark.parametrize("nlu", [4, 5, 6])
def test_many_replica_twin_round_loop(cg, nlu):
    """k_explore_slice8_lds10k<NLU, 9> (EXEC-mask doubling steps, 128 VGPRs): 354 instructions = 262 VALU + 82 scalar + 10 LDS on the round
    loop's likely path (round 6: 375 = 282 + 83 + 10); nothing spilled or reloaded inside it."""
    C, res, lines = cg
    t = _round(C, lines, "k_explore_slice8_lds10kILi%dELi9E" % nlu, 3)
    assert t["instructions"] <= TWIN[nlu] + SLACK, t
    assert t["dyn"] == 5 and t["scratch"] == 0 and t["m"] == 0 and t["w"] == 0, t
