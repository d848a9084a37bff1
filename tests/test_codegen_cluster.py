"""The generated code of the cluster-move kernel (pigeons.jl_amd/csrc/pte_cluster.hpp), cross-compiled for gfx950 with the shipped flags of its
unit (__graft_entry__.CLUSTER_UNITS) through tools/codegen.py: resource figures only.  k_cluster_move touches no scratch and spills neither
a VGPR nor an SGPR; its LDS is dynamic -- 64 bytes of scratch and three arrays of one word per row (cube) or per 32 sites (square), 64 bytes
+ 24 KiB at the largest d the launcher admits, 0 static bytes -- and its registers leave room for 8 waves per SIMD (51 VGPRs, 81 SGPRs when
DESIGN 4.21 was written): what the LDS admits per compute unit, six workgroups of four waves at the largest d, is the bound in force."""
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
    return C.resources(C.compile_units(units=g.CLUSTER_UNITS))


def test_the_unit_holds_the_kernel_and_nothing_else(res):
    assert [k for k in res if k != "__order__"] == ["k_cluster_move"]


def test_no_scratch_no_spill_full_occupancy(res):
    r = res["k_cluster_move"]
    print(r)
    assert r["scratch_B_per_lane"] == 0 and r["spilled_vgpr"] == 0 and r["spilled_sgpr"] == 0 and (r["agpr"] or 0) == 0, r
    assert r["waves_per_simd"] == 8 and r["vgpr"] <= 64, r


def test_at_most_24_KiB_and_64_bytes_of_lds(res):
    """no static LDS in the kernel's resource note; the dynamic size is cluster_lds_bytes, and the launcher refuses d > OVERLAP_MAX_DIM, a cube
    beyond L = 32 and every geometry but the two"""
    import __graft_entry__ as g
    r = res["k_cluster_move"]
    assert r["lds_B"] == 0, r
    params = open(os.path.join(g.CSRC, "pte_cluster_params.hpp")).read()
    overlap = open(os.path.join(g.CSRC, "pte_overlap_params.hpp")).read()
    src = open(os.path.join(g.CSRC, "pte_cluster.hpp")).read()
    max_dim = int(re.search(r"constexpr int OVERLAP_MAX_DIM = (\d+);", overlap).group(1))
    assert "return 64 + 3 * sizeof(unsigned) * (size_t)(geom == OVERLAP_GEOM_CUBE ? L * L : (d + 31) >> 5); }" in params
    assert max(64 + 3 * 4 * ((max_dim + 31) // 32), 64 + 3 * 4 * 32 * 32) == 64 + 24576
    assert 6 * (64 + 24576) <= 160 * 1024 < 7 * (64 + 24576)             # workgroups per compute unit at the largest d
    assert "if (d < 1 || d > OVERLAP_MAX_DIM || mv.N < 1) return 1;" in src
    assert "(L < 2 || L > 32 || L % 2 != 0 || L * L * L != d || !mv.jw)" in src and "(L < 32 || L % 32 != 0 || L * L != d) : true) return 1;" in src
    assert "dim3(PTE_CLUSTER_THREADS), cluster_lds_bytes(d, mv.geom, L), stream," in src
    assert re.search(r"#define PTE_CLUSTER_THREADS 256\n", params)
    assert "extern __shared__ uint4 cluster_lds[];" in src               # a 16-byte element type: the dynamic-LDS base is 16-byte aligned
