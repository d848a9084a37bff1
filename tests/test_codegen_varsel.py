"""The generated code of k_explore_varsel and k_refresh_varsel_stats (pigeons.jl_amd/csrc/pte_varsel.hpp), compiled with the shipped flags
through tools/codegen.py as tests/test_codegen_frozen.py does: every instantiation is there, none touches scratch, none at E <= 2 blocks per
lane spills, and none has static LDS in front of the dynamic region (eta and the staged state)
(DESIGN 4.12)."""
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


def _varsel(res):
    return {k: r for k, r in res.items() if k.startswith("k_explore_varsel<") or k.startswith("k_refresh_varsel_stats<")}


def test_every_instantiation_is_there(res):
    names = sorted(k for k in res if k.startswith("k_explore_varsel<"))
    assert len(names) == 16, names                     # E in {1, 2, 4, 8} x two likelihoods x {ragged, whole blocks}
    names = sorted(k for k in res if k.startswith("k_refresh_varsel_stats<"))
    assert len(names) == 8, names


def test_no_scratch_and_no_spills_at_two_blocks(res):
    vs = _varsel(res)
    assert len(vs) == 24
    for k, r in vs.items():
        assert r["scratch_B_per_lane"] == 0, (k, r)
        assert r["lds_B"] == 0, (k, r)                 # the dynamic region starts at the workgroup's LDS base
        E = int(re.match(r"k_\w+<(\d+),", k).group(1))
        if E <= 2:
            assert r["spilled_vgpr"] == 0 and r["waves_per_simd"] >= 2, (k, r)

