"""The generated code of the CheckerboardMetropolis kernels (pigeons.jl_amd/csrc/pte_checkerboard.hpp), cross-compiled for gfx950 with the shipped
flags of their unit (__graft_entry__.CHECKERBOARD_UNITS) through tools/codegen.py: resource figures only.  Both k_explore_checkerboard
instantiations are spill- and scratch-free; their VGPR counts are pinned at the values DESIGN 4.18 tabulates (LDS is dynamic: L * L / 8 bytes per
plane, one plane on the Ising target and three on the spin glass -- 0 static bytes)."""
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")

NAMES = ["k_explore_checkerboard<false>", "k_explore_checkerboard<true>", "k_explore_checkerboard_sites<false>", "k_explore_checkerboard_sites<true>"]
VGPRS = {"k_explore_checkerboard<false>": 54, "k_explore_checkerboard<true>": 54}


@pytest.fixture(scope="module")
def cg():
    import codegen as C
    import __graft_entry__ as g
    units = C.compile_units(units=g.CHECKERBOARD_UNITS)
    return C, C.resources(units)


def test_every_kernel_is_there(cg):
    _, res = cg
    assert sorted(k for k in res if "checkerboard" in k) == NAMES


@pytest.mark.parametrize("name", sorted(VGPRS))
def test_packed_kernels_have_no_spill_and_no_scratch(cg, name):
    r = cg[1][name]
    assert r["scratch_B_per_lane"] == 0 and r["spilled_vgpr"] == 0 and r["spilled_sgpr"] == 0 and r["lds_B"] == 0, (name, r)
    assert r["vgpr"] == VGPRS[name] and (r["agpr"] or 0) == 0, (name, r)
    assert r["waves_per_simd"] >= 7, (name, r)


@pytest.mark.parametrize("name", [n for n in NAMES if "sites" in n])
def test_sites_kernels_have_no_scratch(cg, name):
    r = cg[1][name]
    assert r["scratch_B_per_lane"] == 0 and r["spilled_vgpr"] == 0 and r["lds_B"] == 0, (name, r)
