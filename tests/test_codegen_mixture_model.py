"""The generated code of k_explore_mixture_model and k_refresh_mixture_model_stats (pigeons.jl_amd/csrc/pte_mixture_model.hpp), compiled with
the shipped flags through tools/codegen.py as tests/test_codegen_frozen.py does: the instantiation list is exactly KB in {2, 4, 8} x
{Langevin, slice} plus the one refresh kernel, none touches scratch or spills a VGPR, and every one leaves room for two waves per SIMD
(DESIGN 4.11)."""
import os
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


def _family(res):
    return {k: r for k, r in res.items() if k.startswith("k_explore_mixture_model<") or k.startswith("k_refresh_mixture_model_stats")}


def test_the_instantiation_list_is_exact(res):
    assert sorted(k for k in res if k.startswith("k_explore_mixture_model<")) == sorted(
        "k_explore_mixture_model<%d, %s>" % (kb, s) for kb in (2, 4, 8) for s in ("false", "true"))
    assert [k for k in res if k.startswith("k_refresh_mixture_model_stats")] == ["k_refresh_mixture_model_stats"]
    assert not [k for k in res if "mixture_model" in k and k not in _family(res)]


def test_no_scratch_no_spilled_vgprs_and_two_waves_per_simd(res):
    fam = _family(res)
    assert len(fam) == 7
    for k, r in fam.items():
        assert r["scratch_B_per_lane"] == 0 and r["spilled_vgpr"] == 0, (k, r)
        assert r["waves_per_simd"] >= 2, (k, r)
