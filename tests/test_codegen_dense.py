"""The generated code of k_explore_dense, k_explore_dense_slice and k_refresh_dense_stats (pigeons.jl_amd/csrc/pte_dense.hpp), compiled with
the shipped flags through tools/codegen.py as tests/test_codegen_hier.py does: every instantiation is there, none touches scratch, the
Langevin kernels at E <= 2 blocks per lane spill no vector register and keep at least two waves per SIMD -- the bar the other families are
held to -- the slice kernel at E <= 2 spills none, and only the Langevin kernels allocate LDS (automala_body's ziggurat tables).  The
E = 4 and E = 8 figures are DESIGN 4.16's table; beyond scratch they are not asserted."""
import os
import re
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")

PREFIXES = ("k_explore_dense<", "k_explore_dense_slice<", "k_refresh_dense_stats<")


@pytest.fixture(scope="module")
def res():
    import codegen as C
    return C.resources(C.compile_units())


def _dense(res):
    return {k: r for k, r in res.items() if k.startswith(PREFIXES)}


def _E(k):
    return int(re.match(r"k_\w+<(\d+)", k).group(1))


def test_every_instantiation_is_there(res):
    lang = sorted(k for k in res if k.startswith("k_explore_dense<"))
    assert len(lang) == 8, lang                        # E in {1, 2, 4, 8} x {ragged, whole blocks}; SLICE = false alone
    assert all(k.split(", ")[1] == "false" for k in lang) and sorted(set(map(_E, lang))) == [1, 2, 4, 8]
    sl = sorted(k for k in res if k.startswith("k_explore_dense_slice<"))
    assert len(sl) == 8 and sorted(set(map(_E, sl))) == [1, 2, 4, 8], sl
    rf = sorted(k for k in res if k.startswith("k_refresh_dense_stats<"))
    assert len(rf) == 4 and sorted(map(_E, rf)) == [1, 2, 4, 8], rf
    assert len(_dense(res)) == 20


def test_no_scratch_and_no_spills_at_two_blocks(res):
    for k, r in _dense(res).items():
        assert r["scratch_B_per_lane"] == 0, (k, r)
        if _E(k) <= 2:
            assert r["spilled_vgpr"] == 0, (k, r)
            if k.startswith("k_explore_dense<"):
                assert r["waves_per_simd"] >= 2, (k, r)


def test_lds_is_the_langevin_tables_alone(res):
    """z_k is broadcast by a read-lane and the rows come from L2: the only LDS is automala_body's ziggurat tables (6 KiB)"""
    for k, r in _dense(res).items():
        assert r["lds_B"] == (6144 if k.startswith("k_explore_dense<") else 0), (k, r)
