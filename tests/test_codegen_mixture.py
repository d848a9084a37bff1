"""The generated code of k_explore_mixture and k_refresh_mixture_stats (pigeons.jl_amd/csrc/pte_mixture.hpp), compiled with the shipped flags
through tools/codegen.py as tests/test_codegen_frozen.py does: no instantiation touches scratch.  (The largest ones -- AutoMALA / MALA at
E = 8 blocks per lane with KB = 4 or 8 components -- keep part of their vectors in AGPRs)"""
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
    names = sorted(k for k in res if k.startswith("k_explore_mixture<"))
    assert len(names) == 36, names                     # E in {1, 2, 4, 8} x KB in {2, 4, 8} x {slice, ragged, whole blocks}
    names = sorted(k for k in res if k.startswith("k_refresh_mixture_stats<"))
    assert len(names) == 12, names


def test_no_scratch(res):
    seen = 0
    for k, r in res.items():
        if not (k.startswith("k_explore_mixture<") or k.startswith("k_refresh_mixture_stats<")):
            continue
        seen += 1
        assert r["scratch_B_per_lane"] == 0, (k, r)
        E = int(re.match(r"k_\w+<(\d+),", k).group(1))
        if E <= 2:
            assert r["spilled_vgpr"] == 0 and r["waves_per_simd"] >= 2, (k, r)
    assert seen == 48
