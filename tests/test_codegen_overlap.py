"""The generated code of the replica-overlap kernel (pigeons.jl_amd/csrc/pte_overlap.hpp), cross-compiled for gfx950 with the shipped flags of
its unit (__graft_entry__.OVERLAP_UNITS) through tools/codegen.py: resource figures only.  k_overlap touches no scratch and spills no VGPR;
its LDS is dynamic -- 4 ceil(d / 32) bytes, 8 KiB at the largest d the launcher admits, 0 static bytes -- and it reaches the 8 waves per
SIMD of a kernel that is all memory latency (45 VGPRs when DESIGN 4.20 was written)."""
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
    import __graft_entry__ as g
    return C.resources(C.compile_units(units=g.OVERLAP_UNITS))


def test_the_unit_holds_the_kernel_and_nothing_else(res):
    assert [k for k in res if k != "__order__"] == ["k_overlap"]


def test_no_scratch_no_spill_full_occupancy(res):
    r = res["k_overlap"]
    print(r)
    assert r["scratch_B_per_lane"] == 0 and r["spilled_vgpr"] == 0 and r["spilled_sgpr"] == 0 and (r["agpr"] or 0) == 0, r
    assert r["waves_per_simd"] == 8, r


def test_at_most_8_KiB_of_lds(res):
    """no static LDS in the kernel's resource note; the dynamic size is 4 bytes per word of t, and the launcher refuses d > OVERLAP_MAX_DIM"""
    import __graft_entry__ as g
    r = res["k_overlap"]
    assert r["lds_B"] == 0, r
    params = open(os.path.join(g.CSRC, "pte_overlap_params.hpp")).read()
    src = open(os.path.join(g.CSRC, "pte_overlap.hpp")).read()
    max_dim = int(re.search(r"constexpr int OVERLAP_MAX_DIM = (\d+);", params).group(1))
    assert 4 * ((max_dim + 31) // 32) <= 8192
    assert "if (d < 1 || d > OVERLAP_MAX_DIM || N < 1) return 1;" in src
    assert "sizeof(unsigned) * (size_t)((d + 31) >> 5), stream," in src
