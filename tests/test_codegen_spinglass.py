"""The generated code of the spin-glass kernels (pigeons.jl_amd/csrc/pte_spinglass.hpp), cross-compiled for gfx950 with the shipped flags of
their unit (__graft_entry__.LATTICE_UNITS) through tools/codegen.py: both k_explore_spinglass_spec instantiations are spill- and
scratch-free and keep the waves per SIMD of k_explore_ising_spec; the per-word loop's instruction counts are frozen at the values DESIGN 4.17
reports next to the Ising loop's 204 VALU + 52 scalar + 4 LDS."""
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")

NAMES = ["k_explore_spinglass", "k_explore_spinglass_spec<false>", "k_explore_spinglass_spec<true>", "k_refresh_spinglass_stats"]
# waves per SIMD of k_explore_ising_spec<false> / <true> (97 / 85 VGPRs: tests/test_codegen_frozen.py asks >= 4 of the first)
ISING_WAVES = {"k_explore_spinglass_spec<false>": 4, "k_explore_spinglass_spec<true>": 5}


@pytest.fixture(scope="module")
def cg():
    import codegen as C
    import __graft_entry__ as g
    units = C.compile_units(units=g.LATTICE_UNITS)
    return C, C.resources(units), C.asm_lines(units)


def test_every_kernel_is_there(cg):
    _, res, _ = cg
    assert sorted(k for k in res if "spinglass" in k) == NAMES


@pytest.mark.parametrize("name", NAMES)
def test_no_scratch_and_no_spilled_vgpr(cg, name):
    r = cg[1][name]
    assert r["scratch_B_per_lane"] == 0 and r["spilled_vgpr"] == 0 and r["lds_B"] == 0, (name, r)      # (LDS is dynamic: 0 static bytes)


@pytest.mark.parametrize("name", sorted(ISING_WAVES))
def test_speculative_kernels_keep_the_waves_of_the_ising_kernel(cg, name):
    r = cg[1][name]
    assert r["waves_per_simd"] >= ISING_WAVES[name], (name, r)
    assert r["vgpr"] <= (99 if name.endswith("<false>") else 87), (name, r)


def test_word_loop_counts(cg):
    """k_explore_spinglass_spec<false>: per 32-site word the likely path is 6 blocks, 228 VALU + 57 scalar + 7 LDS instructions, without a
    spill write or reload: 24 VALU, 5 scalar and 3 LDS instructions more than the Ising loop (DESIGN 4.17 says which)"""
    C, _, lines = cg
    _, body = C.kernel_body(lines, "k_explore_spinglass_specILb0E")
    header = next(h for d, h in C.loop_headers(body) if d == 3)          # replica -> sweep -> row -> WORD
    t = C.totals(C.hot_path(body, header))
    assert t["blocks"] <= 6, t
    assert t["w"] == 0 and t["r"] == 0 and t["scratch"] == 0, t
    assert (t["v"], t["s"], t["l"], t["m"]) == (228, 57, 7, 0), t


def test_one_word_row_loop_counts(cg):
    """k_explore_spinglass_spec<true> (L = 32: a row is one word, the word loop is gone): the row loop's likely path, 283 VALU + 64 scalar + 7
    LDS against the Ising instantiation's 243 + 55 + 4"""
    C, _, lines = cg
    _, body = C.kernel_body(lines, "k_explore_spinglass_specILb1E")
    header = [h for d, h in C.loop_headers(body) if d == 2][1]           # (the first depth-2 loop is the refresh of the reference chain)
    t = C.totals(C.hot_path(body, header))
    assert t["w"] == 0 and t["r"] == 0 and t["scratch"] == 0, t
    assert (t["v"], t["s"], t["l"], t["m"]) == (283, 64, 7, 0), t
