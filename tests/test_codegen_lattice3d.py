"""The generated code of the 3-D spin-glass kernels (pigeons.jl_amd/csrc/pte_lattice3d.hpp), cross-compiled for gfx950 with the shipped flags of
their unit (__graft_entry__.LATTICE3D_UNITS) through tools/codegen.py: resource figures only.  k_explore_checkerboard3d spills no VGPR and
touches no scratch; its LDS is dynamic (16 L^2 bytes: the lattice and three bond planes -- 0 static bytes); its occupancy is held at the
7 waves per SIMD DESIGN 4.19 tabulates (48 VGPRs when that table was made)."""
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")

NAMES = ["k_explore_checkerboard3d", "k_refresh_lattice3d_stats"]


@pytest.fixture(scope="module")
def cg():
    import codegen as C
    import __graft_entry__ as g
    units = C.compile_units(units=g.LATTICE3D_UNITS)
    return C, C.resources(units)


def test_every_kernel_is_there(cg):
    _, res = cg
    assert sorted(k for k in res if "lattice3d" in k or "checkerboard3d" in k) == NAMES
    assert not [k for k in res if k != "__order__" and k not in NAMES], "the unit holds the family's two kernels and nothing else"


@pytest.mark.parametrize("name", NAMES)
def test_no_vgpr_spill_no_scratch_and_dynamic_lds_only(cg, name):
    r = cg[1][name]
    print(name, r)
    assert r["scratch_B_per_lane"] == 0 and r["spilled_vgpr"] == 0 and r["lds_B"] == 0 and (r["agpr"] or 0) == 0, (name, r)


def test_the_sweep_keeps_its_occupancy(cg):
    r = cg[1]["k_explore_checkerboard3d"]
    assert r["waves_per_simd"] >= 7, r
