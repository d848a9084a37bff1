"""The generated code of k_explore_changepoint and k_refresh_changepoint_stats (pigeons.jl_amd/csrc/pte_changepoint.hpp), compiled with the
shipped flags through tools/codegen.py as tests/test_codegen_frozen.py does: every instantiation is there, none touches scratch, none
spills a VGPR, none has static LDS, and every one leaves room for two waves per SIMD."""
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")

# both evaluation forms of the explorer (the template flag CACHED) and the refresh kernel; the state takes two registers per lane at every
# dim, so the kernels have no blocks-per-lane parameter
NAMES = ["k_explore_changepoint<false>", "k_explore_changepoint<true>", "k_refresh_changepoint_stats"]


@pytest.fixture(scope="module")
def res():
    import codegen as C
    return C.resources(C.compile_units())


def test_every_instantiation_is_there(res):
    assert sorted(k for k in res if "changepoint" in k) == NAMES


@pytest.mark.parametrize("name", NAMES)
def test_no_scratch_no_spilled_vgpr_no_lds_and_two_waves(res, name):
    r = res[name]
    assert r["scratch_B_per_lane"] == 0, (name, r)
    assert r["spilled_vgpr"] == 0, (name, r)
    assert r["lds_B"] == 0, (name, r)
    assert r["waves_per_simd"] >= 2, (name, r)
