"""The generated code of k_explore_ar1 and k_refresh_ar1_stats (pigeons.jl_amd/csrc/pte_ar1.hpp), compiled with the shipped flags through
tools/codegen.py as tests/test_codegen_hier.py does: every instantiation is there, none touches scratch, none at E <= 2 blocks per lane spills
a vector register or drops below two waves per SIMD -- the bar the GLM, mixture and hierarchical families are held to -- and the
neighbour values travel by DPP wave shifts: no LDS instruction beyond the Langevin kernels' ziggurat tables, no LDS allocation beyond them."""
import os
import re
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")


@pytest.fixture(scope="module")
def units():
    import codegen as C
    return C.compile_units()


@pytest.fixture(scope="module")
def res(units):
    import codegen as C
    return C.resources(units)


def _ar1(res):
    return {k: r for k, r in res.items() if k.startswith("k_explore_ar1<") or k.startswith("k_refresh_ar1_stats<")}


def test_every_instantiation_is_there(res):
    names = sorted(k for k in res if k.startswith("k_explore_ar1<"))
    assert len(names) == 24, names                     # E in {1, 2, 4, 8} x two observation models x {slice, ragged, whole blocks}
    assert sorted(set(int(re.match(r"k_\w+<(\d+), (\d+)", k).group(2)) for k in names)) == [0, 1]
    assert sorted(set(int(re.match(r"k_\w+<(\d+),", k).group(1)) for k in names)) == [1, 2, 4, 8]
    names = sorted(k for k in res if k.startswith("k_refresh_ar1_stats<"))
    assert len(names) == 8, names


def test_no_scratch_and_no_spills_at_two_blocks(res):
    ar1 = _ar1(res)
    assert len(ar1) == 32
    for k, r in ar1.items():
        assert r["scratch_B_per_lane"] == 0, (k, r)                    # at every E: the build achieves 0 (DESIGN 4.15's table)
        E = int(re.match(r"k_\w+<(\d+),", k).group(1))
        if E <= 2:
            assert r["spilled_vgpr"] == 0 and r["waves_per_simd"] >= 2, (k, r)


def test_no_dynamic_lds(res):
    """the data stays in registers or comes from L2, the neighbours come by DPP: the only LDS is automala_body's ziggurat tables (6 KiB, the
    Langevin kernels alone)"""
    for k, r in _ar1(res).items():
        args = k[k.index("<") + 1:k.rindex(">")].split(", ")           # E, LIK, [SLICE, FULL]
        want = 6144 if k.startswith("k_explore_ar1<") and args[2] == "false" else 0
        assert r["lds_B"] == want, (k, r)


def test_neighbours_travel_by_wave_shifts(units):
    """one log-density evaluation is 2 E v_mov_b32_dpp wave_shr:1 (the predecessors, two dwords a double); the refresh kernel holds exactly
    one evaluation and no gradient, so no wave_shl:1, and no LDS instruction at all.  The explore kernels hold both directions when they
    take gradients and wave_shr alone in slice mode."""
    path = next(p for src, _, p, _ in units if src == "pte_glm.hip")
    bodies = {}                                                       # mangled name -> text, the latent-AR(1) kernels only
    for part in open(path).read().split("\n.Lfunc_end")[:-1]:
        m = None
        for m in re.finditer(r"^(_ZN3pte\w*ar1\w*):", part, re.M):
            pass
        if m:
            bodies[m.group(1)] = part[m.start():]

    def body(sub):
        return next(t for k, t in bodies.items() if sub in k)
    assert len(bodies) == 32
    for E in (1, 2, 4, 8):
        for lik in (0, 1):
            text = body("k_refresh_ar1_statsILi%dELi%dE" % (E, lik))
            assert text.count("wave_shr:1") == 2 * E and text.count("wave_shl:1") == 0, (E, lik)
            assert not re.search(r"^\s*ds_", text, re.M), (E, lik)
            text = body("k_explore_ar1ILi%dELi%dELb1ELb0E" % (E, lik))
            assert text.count("wave_shr:1") >= 2 * E and text.count("wave_shl:1") == 0, (E, lik)
            text = body("k_explore_ar1ILi%dELi%dELb0ELb0E" % (E, lik))
            assert text.count("wave_shr:1") >= 2 * E and text.count("wave_shl:1") >= 2 * E, (E, lik)
