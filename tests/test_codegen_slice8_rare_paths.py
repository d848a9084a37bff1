"""The speculative round of the default SliceSampler kernel after round 8: the three "does lane 0 need its out-of-line path?" tests are scalar
bit tests (pte_slice8.hpp), and the compares, lane-0 masks and mask arithmetic that used to feed them are gone from the round.

The size of the round's likely path is recorded in profiles/r08_slice8_round_loop.txt (tools/round_loop_lanes.py k_scans_slice8ILi4ELi9E);
this module holds k_scans_slice8<4, 9> -- the kernel the metric runs -- and k_explore_slice8<4, 9> to that number plus the four instructions of
slack tests/test_codegen_slice8_round.py allows, and the number itself below the 268 of round 7.  Same source of truth as there:
tools/codegen.py compiles the product's translation units with the shipped flags (cached under build/codegen/).

The window's slow-path mask lives in sixteen SGPRs and is indexed through M0 (s_movrels_b32): no lane instruction joins the five v_readlane of
the chase, nothing is spilled, reloaded or sent to scratch inside the loop, and the likely path stays at eight blocks."""
import os
import re
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")

SLACK = 4
ROUND7 = 268


def _recorded():
    text = open(os.path.join(ROOT, "profiles", "r08_slice8_round_loop.txt")).read()
    assert "k_scans_slice8<4, 9>" in text
    return int(re.search(r"# HOT path per round: .* = (\d+) instructions in (\d+) blocks", text).group(1))


@pytest.fixture(scope="module")
def cg():
    import codegen as C
    units = C.compile_units()
    return C, C.resources(units), C.asm_lines(units)


def test_recorded_round_is_smaller_than_round_7():
    assert _recorded() < ROUND7


@pytest.mark.parametrize("kernel,sub,depth", [("k_scans_slice8<4, 9>", "k_scans_slice8ILi4ELi9E", 4), ("k_explore_slice8<4, 9>", "k_explore_slice8ILi4ELi9E", 3)])
def test_round_loop(cg, kernel, sub, depth):
    C, res, lines = cg
    name, body = C.kernel_body(lines, sub)
    header = next(h for d, h in C.loop_headers(body) if d == depth)
    t = C.totals(C.hot_path(body, header))
    print(kernel, t)
    assert t["instructions"] <= _recorded() + SLACK, t
    assert t["blocks"] <= 8 and t["dyn"] == 5, t
    assert t["w"] == 0 and t["r"] == 0 and t["scratch"] == 0 and t["m"] == 0, t
    assert res[kernel]["spilled_vgpr"] == 0, res[kernel]
