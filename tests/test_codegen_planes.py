"""The generated code of the plane-correlation kernel (pigeons.jl_amd/csrc/pte_overlap_planes.hpp), cross-compiled for gfx950 with the shipped
flags of its unit (__graft_entry__.PLANES_UNITS) through tools/codegen.py: resource figures only.  k_overlap_planes touches no scratch and
spills nothing; its LDS is dynamic -- 4 ceil(d / 32) + 4 n_axes L bytes, 4480 B on the 32^3 cube and 10 KiB at 256 x 256, the largest d
the launcher admits, 0 static bytes.  It holds 69 VGPRs in the build DESIGN 4.22 was written from -- sixteen loads of a and of b in flight
in the loop that forms t, six bit-sliced counters -- which is 7 waves per SIMD: with one wave per chain, 28 waves per CU are more than a
ladder puts there, and at the largest d the LDS (10 KiB per wave) allows 16."""
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
    return C.resources(C.compile_units(units=g.PLANES_UNITS))


def test_the_unit_holds_the_kernel_and_nothing_else(res):
    assert [k for k in res if k != "__order__"] == ["k_overlap_planes"]


def test_no_scratch_no_spill_seven_waves_per_simd(res):
    r = res["k_overlap_planes"]
    print(r)
    assert r["scratch_B_per_lane"] == 0 and r["spilled_vgpr"] == 0 and r["spilled_sgpr"] == 0 and (r["agpr"] or 0) == 0, r
    assert r["waves_per_simd"] == 7, r


def test_the_lds_is_dynamic_and_the_launcher_sizes_and_bounds_it(res):
    """no static LDS in the kernel's resource note; the dynamic size is 4 bytes per word of t and per plane count, and the launcher refuses
    d > OVERLAP_MAX_DIM and every shape without a geometry"""
    import __graft_entry__ as g
    r = res["k_overlap_planes"]
    assert r["lds_B"] == 0, r
    params = open(os.path.join(g.CSRC, "pte_overlap_planes_params.hpp")).read()
    src = open(os.path.join(g.CSRC, "pte_overlap_planes.hpp")).read()
    max_dim = int(re.search(r"constexpr int OVERLAP_MAX_DIM = (\d+);", open(os.path.join(g.CSRC, "pte_overlap_params.hpp")).read()).group(1))
    assert ("constexpr size_t planes_lds_bytes(int d, int geom, int L) { return sizeof(unsigned) * (size_t)((d + 31) >> 5) + "
            "sizeof(int) * (size_t)(planes_axes(geom) * L); }") in params
    assert "constexpr int planes_axes(int geom) { return geom == OVERLAP_GEOM_CUBE ? 3 : geom == OVERLAP_GEOM_SQUARE ? 2 : 0; }" in params
    assert 4 * ((32 ** 3 + 31) // 32) + 4 * 3 * 32 == 4480 and 4 * ((max_dim + 31) // 32) + 4 * 2 * 256 == 10240 and max_dim == 256 * 256
    assert "if (d < 1 || d > OVERLAP_MAX_DIM || N < 1) return 1;" in src
    assert "dim3((unsigned)N), dim3(64), planes_lds_bytes(d, geom, L), stream," in src
    assert "__shared__" in src and src.count("__shared__") == 1 and "extern __shared__ unsigned t[];" in src
