"""The generated code of k_explore_hier and k_refresh_hier_stats (pigeons.jl_amd/csrc/pte_hier.hpp), compiled with the shipped flags through
tools/codegen.py as tests/test_codegen_glm.py does: every instantiation is there, none touches scratch (the coefficients of exp / log1p are
not spilled around the step-size search), and none at E <= 2 blocks per lane spills or drops below two waves per SIMD -- the bar
the GLM and mixture families are held to."""
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


def _hier(res):
    return {k: r for k, r in res.items() if k.startswith("k_explore_hier<") or k.startswith("k_refresh_hier_stats<")}


def test_every_instantiation_is_there(res):
    names = sorted(k for k in res if k.startswith("k_explore_hier<"))
    assert len(names) == 24, names                     # E in {1, 2, 4, 8} x two parameterisations x {slice, ragged, whole blocks}
    assert sorted(set(int(re.match(r"k_\w+<(\d+), (\d+)", k).group(2)) for k in names)) == [0, 1]
    names = sorted(k for k in res if k.startswith("k_refresh_hier_stats<"))
    assert len(names) == 8, names


def test_no_scratch_and_no_spills_at_two_blocks(res):
    hier = _hier(res)
    assert len(hier) == 32
    for k, r in hier.items():
        assert r["scratch_B_per_lane"] == 0, (k, r)
        E = int(re.match(r"k_\w+<(\d+),", k).group(1))
        if E <= 2:
            assert r["spilled_vgpr"] == 0 and r["waves_per_simd"] >= 2, (k, r)


def test_no_dynamic_lds(res):
    """the data stays in registers or comes from L2: the only LDS is automala_body's ziggurat tables (6 KiB, the Langevin kernels alone)"""
    for k, r in _hier(res).items():
        args = k[k.index("<") + 1:k.rindex(">")].split(", ")           # E, PARAM, [SLICE, FULL]
        want = 6144 if k.startswith("k_explore_hier<") and args[2] == "false" else 0
        assert r["lds_B"] == want, (k, r)
