"""The generated code of k_explore_aaps (pigeons.jl_amd/csrc/pte_aaps.hpp), compiled with the shipped flags through tools/codegen.py as
tests/test_codegen_frozen.py does: every instantiation keeps its seven vectors in registers -- no VGPR spill, no scratch -- and those with
at most four blocks per lane (d <= 256) leave room for two waves per SIMD."""
import os
import re
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")


@pytest.fixture(scope="module")
def res():
    import codegen as C
    return C.resources(C.compile_units())


def test_every_instantiation_is_there(res):
    names = sorted(k for k in res if k.startswith("k_explore_aaps<"))
    assert len(names) == 16, names                     # E in {1, 2, 4, 8} x {MVN, funnel} x {ragged, whole blocks}


def test_no_spill_no_scratch(res):
    for k, r in res.items():
        if not k.startswith("k_explore_aaps<"):
            continue
        E = int(re.match(r"k_explore_aaps<(\d+),", k).group(1))
        assert r["spilled_vgpr"] == 0 and r["scratch_B_per_lane"] == 0, (k, r)
        if E <= 4:
            assert r["waves_per_simd"] >= 2, (k, r)
