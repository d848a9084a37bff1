"""The case table of tests/family_blocks.py, checked without a device: that it reaches every instantiation it is there for, and that the
restatement's own MALA, from the table's inputs, accepts some proposals and rejects others in every MALA case -- so that the parity test
of tests/test_gpu_family_blocks.py sees both branches of the accept / reject step.  The AutoMALA cases likewise: the restatement alone
(tests/automala_ref.py), from the engine's RNG words, must not raise, must take both outcomes of the MH step and of the reversibility
check in every case that has them, must only grow, only shrink, or meet non-finite trials where the case's regime says so, and none of its
decisions may be closer than 1e-6 to going the other way: a device that differs from the restatement in the last bits could otherwise
rightly decide otherwise.  1e-6 is the floor tests/test_gpu_family_edges.py uses for |u - alpha|; at |lp| + |ke| <= ~1e3 it is 100 x the
project's log-density tolerance of 1e-11 relative.  The whole AutoMALA part takes about 15 s, half of it dense at d = 512.

A cell is (family, variant, mode, E, whole): E = blocks_per_lane of the state dimension, whole = the state fills its E blocks.  The
launchers (pte_<family>.hpp, <family>_launch) take the FULL instantiation -- no per-lane validity masks -- at whole for MALA everywhere
and for SliceSampler on the dense and variable-selection families; the other families' slice mode has the masked instantiation only,
which eight whole blocks then run with every lane valid."""
import math

import numpy as np
import pytest

import family_blocks as B

GLM, HIER, AR1, VARSEL = ("bernoulli_logit", "normal_identity"), ("c", "nc"), ("sv", "n"), ("bernoulli_logit", "normal_identity")
VARIANTS = {"glm": GLM, "hier": HIER, "ar1": AR1, "mixture": (None,), "dense": (None,), "varsel": VARSEL}
FOUR_CELLS = [(4, False), (4, True), (8, False), (8, True)]
MAX_STATE_DIM = {"glm": 512, "hier": 510 + 2, "ar1": 509 + 3, "mixture": 512, "dense": 512, "varsel": 2 * 256}


def blocks_per_lane(d):
    """pte.hip: the number of 64-coordinate blocks a lane holds"""
    return 1 if d <= 64 else 2 if d <= 128 else 4 if d <= 256 else 8 if d <= 512 else 16


def cell(case):
    E = blocks_per_lane(case.d)                       # (varsel: case.d is the state's 2 d)
    return (case.family, case.variant, case.mode, E, case.d == 64 * E)


def mixture_bucket(K):
    """pte_mixture_params.hpp"""
    return 2 if K <= 2 else 4 if K <= 4 else 8


def required_cells():
    """[(cell, variants that may fill it)]: one case of any of the variants fills the cell"""
    out = []
    for f in ("glm", "hier", "ar1", "mixture"):        # slice: no FULL instantiation -- 129 / 130, 257, 512
        for v in VARIANTS[f]:
            out += [((f, v, "slice", 4, False), (v,)), ((f, v, "slice", 8, False), (v,))]
            if f != "glm":
                out.append(((f, v, "slice", 8, True), (v,)))
    out.append((("glm", None, "slice", 8, True), GLM))               # one likelihood at 512: the restatement's pass takes seconds a replica
    for f in ("dense", "varsel"):                      # slice kernels of their own, with FULL instantiations
        for v in VARIANTS[f]:
            out += [((f, v, "slice", E, whole), (v,)) for E, whole in FOUR_CELLS]
    out += [(("varsel", v, "slice", 2, True), (v,)) for v in VARSEL]            # 2 d = 128: two whole blocks
    for f in ("glm", "hier", "ar1", "mixture", "dense"):
        for v in VARIANTS[f]:
            out += [((f, v, "mala", E, whole), (v,)) for E, whole in FOUR_CELLS]
    return out


def test_the_table_reaches_every_cell():
    have = {}
    for c in B.CASES:
        have.setdefault(cell(c)[0:1] + cell(c)[2:], []).append(c)
    empty = []
    for (f, v, mode, E, whole), variants in required_cells():
        if not any(c.variant in variants for c in have.get((f, mode, E, whole), [])):
            empty.append("%s %s %s E = %d %s" % (f, v if v is not None else "/".join(map(str, variants)), mode, E, "whole" if whole else "ragged"))
    assert not empty, "no case reaches: " + "; ".join(empty)


def test_every_dimension_is_the_smallest_or_the_most_ragged_of_its_cell():
    """E = 4 ragged: 129 or 130 (block 2 holds one or two coordinates, block 3 none); E = 8 ragged: 257 (block 4 holds one coordinate, blocks
    5 to 7 none; varsel's even state: 258); whole: 64 E"""
    for c in B.CASES:
        _, _, _, E, whole = cell(c)
        assert E in (2, 4, 8), c
        want = (64 * E,) if whole else {4: (129, 130), 8: (258,) if c.family == "varsel" else (257,)}.get(E, ())
        assert c.d in want, (c, want)
        assert c.family != "varsel" or c.d % 2 == 0, c


def test_slice_cases_run_one_pass_of_the_defaults_and_mixture_meets_every_bucket():
    for c in B.SLICE_CASES:
        assert (c.kw["w"], c.kw["p"], c.kw["n_passes"]) == (10.0, 20, 1), c
    for mode in ("slice", "mala"):
        buckets = {mixture_bucket(c.kw["K"]) for c in B.CASES if c.family == "mixture" and c.mode == mode and blocks_per_lane(c.d) >= 4}
        assert buckets == {2, 4, 8}, (mode, buckets)


def test_every_family_meets_every_preconditioner():
    for f in ("glm", "hier", "ar1", "mixture", "dense"):
        for v in VARIANTS[f]:
            seen = {c.kw["precond"] for c in B.MALA_CASES if c.family == f and c.variant == v}
            assert seen == {"identity", "diagonal", "mix"}, (f, v, seen)
    for E, whole in FOUR_CELLS:                          # ... and every cell more than one of them
        assert len({c.kw["precond"] for c in B.MALA_CASES if cell(c)[3:] == (E, whole)}) == 3, (E, whole)


def test_no_case_is_beyond_its_family_s_limits():
    """J <= 510, T <= 509, varsel d <= 256, n d <= 131072 (pte.h); replicas: 6, or 3 where the restatement's pass is slowest"""
    for c in B.CASES + B.LOG_DENSITY_CASES:
        assert c.d <= MAX_STATE_DIM[c.family], c
        if c.family in ("glm", "varsel"):
            cols = c.d // 2 if c.family == "varsel" else c.d
            assert 1 <= c.kw["n"] and c.kw["n"] * cols <= 131072, c
            assert c.mode == "lp" or c.kw["n"] <= 20, c
        assert c.mode == "lp" or c.N == (3 if c.mode == "slice" and c.family in ("glm", "dense") and c.d == 512 else 6), c
        betas, x, chain = B.layout(c)
        assert x.shape == (c.N, c.d) and sorted(chain) == list(range(c.N)) and betas[0] == 0.0 and betas[-1] == 1.0
        assert np.all(np.diff(betas) > 0), c


def test_the_refresh_kernels_left_out_so_far_are_in_the_log_density_cases():
    """glm E = 2 and 4, mixture E = 4, varsel E = 4 and a ragged E = 8"""
    got = sorted((c.family, blocks_per_lane(c.d), c.d == 64 * blocks_per_lane(c.d)) for c in B.LOG_DENSITY_CASES)
    assert got == [("glm", 2, False), ("glm", 4, False), ("mixture", 4, False), ("varsel", 4, False), ("varsel", 8, False)], got


@pytest.fixture(scope="module")
def words():
    """the engine's RNG words (every MALA case has 6 replicas)"""
    return B.init_rng_words(6)


@pytest.mark.parametrize("case", B.MALA_CASES, ids=[c.id for c in B.MALA_CASES])
def test_the_restatement_accepts_and_rejects(case, words):
    betas, x, chain = B.layout(case)
    res, accepted, rejected = B.mala_reference(case, betas, x, chain, words)
    print("%s, step %g: %d proposals accepted, %d rejected (when the step was chosen: %s)" % (case.id, case.kw["step"], accepted, rejected, case.kw["seen"]))
    assert len(res) == case.N - 1 and accepted + rejected == (case.N - 1) * B.n_refresh(case.d)
    assert accepted > 0 and rejected > 0, (accepted, rejected)
    assert all(np.all(np.isfinite(r["x"])) for r in res.values())


# ---- AutoMALA --------------------------------------------------------------------------------------------------------------------------
PAIRS = [(f, v) for f in ("glm", "hier", "ar1", "mixture", "dense") for v in VARIANTS[f]]
MARGIN_FLOOR = 1e-6


def test_automala_cases_cover_regimes_dimensions_and_preconditioners():
    A = B.AUTOMALA_CASES
    assert len(A) == 32 and all(c.N == 6 and c.mode == "automala" for c in A)
    assert sorted((c.family, c.variant, c.d) for c in A) == sorted((f, v, d) for f, v in PAIRS for d in B.AUTOMALA_DIMS)
    for f, v in PAIRS:                                   # every (family, variant) meets every regime
        assert sorted(c.kw["regime"] for c in A if (c.family, c.variant) == (f, v)) == sorted(B.AUTOMALA_REGIMES), (f, v)
    for regime in B.AUTOMALA_REGIMES:                    # every regime meets every dimension class and every preconditioner
        mine = [c for c in A if c.kw["regime"] == regime]
        assert {cell(c)[3:] for c in mine} == set(FOUR_CELLS), regime
        assert {c.kw["precond"] for c in mine} == {"identity", "diagonal", "mix"}, regime
    assert B.n_refresh(129, base=1) == 6 and B.n_refresh(512, base=1) == 9
    for c in A:                                          # the MALA case's inputs, its step where the regime does not set one
        (m,) = [k for k in B.MALA_CASES if (k.family, k.variant, k.d) == (c.family, c.variant, c.d)]
        assert c.kw["step"] == {"grow": 2.0 ** -12, "shrink": 2.0 ** 8}.get(c.kw["regime"], m.kw["step"]), c
        assert c.kw["scan"] == (1 if c.kw["regime"] == "scan1" else 2), c
        assert B.model(c).ref_prec == 1.0 and all(np.array_equal(a, b) for a, b in zip(B.layout(c), B.layout(m))), c
        assert {k: c.kw[k] for k in ("n", "K") if k in m.kw} == {k: m.kw[k] for k in ("n", "K") if k in m.kw}, c


@pytest.mark.parametrize("case", B.AUTOMALA_CASES, ids=[c.id for c in B.AUTOMALA_CASES])
def test_the_automala_restatement_meets_the_case_s_conditions(case, words):
    betas, x, chain = B.layout(case)
    res = B.automala_reference(case, betas, x, chain, words)          # (raises at a start without density or a step that reaches 0)
    seen, margin = B.automala_seen(case, x, res)
    accepted, rejected, passed, failed, lo, hi, nonfinite, moved = seen
    regime, nr = case.kw["regime"], B.n_refresh(case.d, base=B.AUTOMALA_BASE_N_REFRESH)
    print("%s %s %s step %g: %s, least margin %.2e (in the table: %s, %.2e)" % (case.id, regime, case.kw["precond"], case.kw["step"], seen, margin,
                                                                               case.kw["seen"], case.kw["margin"]))
    assert len(res) == case.N - 1 and all(np.all(np.isfinite(r["x"])) for r in res.values())
    if regime == "scan1":
        assert moved == case.N - 1 and accepted + rejected == 0 and passed + failed == 0
        assert all(len(r["exponents"]) == nr for r in res.values())
    else:
        assert accepted + rejected == passed + failed == (case.N - 1) * nr
        assert all(len(r["exponents"]) == 2 * nr for r in res.values())
        assert accepted > 0 and rejected > 0 and passed > 0 and failed > 0, seen
    if regime == "grow":
        assert lo > 0, seen
    if regime == "shrink":
        assert hi < 0, seen
        if (case.family, case.variant) in (("hier", "c"), ("ar1", "sv"), ("ar1", "n")):
            assert nonfinite > 0, seen
    assert margin >= MARGIN_FLOOR, margin
    assert seen == case.kw["seen"] and math.isclose(margin, case.kw["margin"], rel_tol=0.01), (seen, margin)
