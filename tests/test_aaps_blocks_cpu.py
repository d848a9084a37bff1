"""The case table of tests/aaps_blocks.py, checked without a device: that it reaches every instantiation of k_explore_aaps and the lane
layouts it is there for, what the restatement (tests/aaps_ref.py) does on each case from the engine's initial RNG words, that none of the
restatement's decisions is a near tie -- so that a kernel within tolerance has to take the same decisions -- and how far rounding alone
moves these trajectories, by rerunning them with np.longdouble state arithmetic.

A cell is (target, E, whole): E = blocks_per_lane(d), whole = the state fills its E blocks (pte.hip, launch_explore: full = d == 64 E takes
the instantiation without per-lane validity masks).  A layout is (E, occupied blocks, lanes of the last occupied block): it says which
trailing blocks are whole, partly filled or empty, which is what the nl arithmetic of the momentum draw and of the variational refresh
meets."""
import math

import numpy as np
import pytest

import aaps_blocks as B

MARGIN = 1e-7                    # least distance of a decision from its tie; the device agrees with the restatement to 1e-9 relative
LD_RTOL = 1e-10                  # RTOL / 10 of tests/test_gpu_aaps_blocks.py

# (target, variant) -> layouts; every layout is filled by exactly one case of kind "parity"
REQUIRED = {
    ("mvn", "plain"): [(1, 1, 33), (1, 1, 64), (2, 2, 36), (2, 2, 64), (4, 3, 1), (4, 4, 1), (4, 4, 63), (4, 4, 64),
                       (8, 5, 1), (8, 5, 64), (8, 8, 63), (8, 8, 64)],
    ("funnel", "plain"): [(1, 1, 20), (1, 1, 64), (2, 2, 1), (2, 2, 63), (2, 2, 64), (4, 3, 1), (4, 3, 64), (4, 4, 63), (4, 4, 64),
                          (8, 5, 1), (8, 5, 64), (8, 8, 63), (8, 8, 64)],
    ("funnel", "vref"): [(2, 2, 1), (4, 3, 1), (4, 4, 64), (8, 5, 1), (8, 8, 64)],
    ("funnel", "identity"): [(4, 4, 8), (8, 6, 64)],
    ("funnel", "diagonal"): [(4, 3, 2), (8, 5, 44)],
    ("funnel", "K0"): [(8, 7, 64)],
    ("mvn", "K9"): [(8, 7, 16)],
}


def blocks_per_lane(d):
    """pte.hip: the number of 64-coordinate blocks a lane holds"""
    return 1 if d <= 64 else 2 if d <= 128 else 4 if d <= 256 else 8 if d <= 512 else 16


def full(d):
    """pte.hip, launch_explore: no ragged last block"""
    return d == 64 * blocks_per_lane(d)


def cell(case):
    return (case.target, blocks_per_lane(case.d), full(case.d))


def layout(d):
    occupied = (d + 63) // 64
    return (blocks_per_lane(d), occupied, d - 64 * (occupied - 1))


def variant(case):
    return "vref" if case.vref else case.precond if case.precond != "mix" else "K%d" % case.K if case.K != 4 else "plain"


def _cell_name(target, E, whole):
    return "%s E = %d %s" % (target, E, "whole" if whole else "ragged")


PARITY = [c for c in B.CASES if c.kind == "parity"]


def test_the_parity_cases_reach_all_sixteen_instantiations():
    have = {cell(c) for c in PARITY if variant(c) == "plain"}
    empty = [_cell_name(t, E, w) for t in ("mvn", "funnel") for E in (1, 2, 4, 8) for w in (False, True) if (t, E, w) not in have]
    assert not empty, "no parity case reaches: " + "; ".join(empty)


def test_the_variational_reference_reaches_two_four_and_eight_blocks():
    have = {cell(c)[1:] for c in B.VREF_CASES}
    empty = [_cell_name("funnel vref", E, w) for E, w in ((2, False), (4, False), (4, True), (8, False), (8, True)) if (E, w) not in have]
    assert not empty, "no case reaches: " + "; ".join(empty)
    assert all(c.target == "funnel" and c.vref and c.kind == "parity" for c in B.VREF_CASES)
    inp = B.inputs(B.VREF_CASES[0])
    pairs = {(int(inp.uses[c]), int(inp.uses[c + 1])) for c in range(len(inp.uses) - 1)}
    assert inp.uses[0] == 1 and 2 * int(np.sum(inp.uses)) == len(inp.uses) and pairs == {(0, 0), (0, 1), (1, 0), (1, 1)}


def test_four_and_eight_blocks_meet_empty_trailing_blocks_and_a_single_lane():
    """for every E >= 4 and both targets: a d whose last blocks hold nothing, and a d = 64 j + 1 (one lane in the last occupied block)"""
    missing = []
    for target in ("mvn", "funnel"):
        for E in (4, 8):
            ds = [c.d for c in PARITY if c.target == target and blocks_per_lane(c.d) == E]
            if not any((d + 63) // 64 < E for d in ds):
                missing.append("%s E = %d: an empty trailing block" % (target, E))
            if not any(d % 64 == 1 for d in ds):
                missing.append("%s E = %d: d = 64 j + 1" % (target, E))
            if not any(d % 64 == 1 and (d + 63) // 64 < E for d in ds):
                missing.append("%s E = %d: one lane in a block with empty blocks behind it" % (target, E))
    assert not missing, "no parity case has " + "; ".join(missing)


def test_every_layout_has_its_case_and_no_case_is_spare():
    """removing any parity case empties a layout, which is named"""
    have = {}
    for c in PARITY:
        have.setdefault((c.target, variant(c), layout(c.d)), []).append(c)
    want = {(t, v, lay) for (t, v), lays in REQUIRED.items() for lay in lays}
    empty = ["%s %s E = %d, %d blocks occupied, %d lanes in the last" % ((t, v) + lay) for t, v, lay in sorted(want - set(have))]
    assert not empty, "no case reaches: " + "; ".join(empty)
    assert set(have) == want and all(len(cs) == 1 for cs in have.values()), have
    at = lambda v: {blocks_per_lane(c.d) for c in PARITY if variant(c) == v}
    assert at("identity") == {4, 8} and at("diagonal") == {4, 8} and at("K0") == {8} and at("K9") == {8}


def test_the_settings_of_the_cases():
    for c in PARITY:
        assert c.N == 8 and c.seed in (1, 2, 3), c
        assert c.step == (0.25 if c.target == "mvn" else 0.05 if c.d >= 511 else 0.1), c
        assert c.precond == "mix" or (c.target == "funnel" and c.K == 4), c
    assert sorted((c.target, c.d, c.step, c.N, c.K, c.precond) for c in B.UNSTABLE_CASES) == [
        ("funnel", 130, 0.3, 8, 4, "mix"), ("funnel", 300, 0.3, 8, 4, "mix"), ("mvn", 130, 0.4, 8, 4, "mix")]
    assert sorted((c.target, c.d, c.step, c.N, c.K) for c in B.CAP_CASES) == [("funnel", 130, 1e-7, 4, 2), ("mvn", 130, 1e-6, 4, 2)]
    for c in B.CASES:
        inp = B.inputs(c)
        assert inp.x.shape == (c.N, c.d) and sorted(inp.chain) == list(range(c.N)) and inp.betas[0] == 0.0 and inp.betas[-1] == 1.0
        assert np.all(np.diff(inp.betas) > 0) and inp.words.shape == (c.N, 2), c
        if c.kind == "unstable":                         # _one_step's own states
            g = np.random.default_rng(c.seed)
            g.uniform(0.0, 1.0, c.N - 2)
            assert np.array_equal(inp.x, g.standard_normal((c.N, c.d)) * (0.5 if c.target == "funnel" else 0.4)), c
    want = {(t, E) for t in ("mvn", "funnel") for E in (2, 4, 8)}
    assert {(c.target, blocks_per_lane(c.d)) for c in B.STATISTICS_CASES if not c.vref} == want
    assert {cell(c)[1:] for c in B.STATISTICS_CASES if c.vref} == {(4, False), (4, True), (8, False), (8, True)}
    assert all(c.kind == "parity" for c in B.STATISTICS_CASES)


@pytest.mark.parametrize("case", B.CASES, ids=[c.id for c in B.CASES])
def test_what_the_restatement_does(case):
    """aaps_ref.transition from the engine's initial RNG words; the instrumented copy is the same function, to the bit"""
    ref, pr = B.reference(case), B.probes(case)
    failed, moved, lo, hi, total = B.census(ref)
    print("%s: %d failed, %d moved of %d; steps %d .. %d, summed %d (when the case was written: %s)" % (case.id, failed, moved, len(ref), lo, hi, total, case.steps))
    assert len(ref) == case.N - 1 and sorted(ref) == sorted(pr)
    for i, r in ref.items():
        p = pr[i]
        assert np.array_equal(r["x"], p["x"]) and p["x"].dtype == np.float64, (case, i)
        assert (r["acc"], r["steps"], r["Kf"], r["failed"], r["words"]) == (p["acc"], p["steps"], p["Kf"], p["failed"], p["words"]), (case, i)
        assert r["failed"] or np.all(np.isfinite(r["x"])), (case, i)
    assert total == case.steps, (case, total)
    if case.kind == "parity":
        assert failed == 0 and moved >= 5, (case, failed, moved)
        assert all(p["n_candidates"] >= 1 for p in pr.values()), case
    elif case.kind == "unstable":                        # a failure below the cap is a non-finite point
        assert failed >= 1 and moved >= 1 and all(r["steps"] < B.A.MAX_LEAPFROGS for r in ref.values()), (case, failed, moved)
    else:                                                # the cap: every replica stays after 4096 steps and 4096 candidate uniforms
        assert failed == len(ref) and moved == 0 and (lo, hi) == (B.A.MAX_LEAPFROGS,) * 2, (case, failed, lo, hi)
        assert all(p["n_candidates"] == B.A.MAX_LEAPFROGS for p in pr.values()), case


def test_an_unstable_replica_fails_after_more_than_one_step():
    """... somewhere in the table: the failure is then met inside the loop, with candidates already visited and uniforms drawn"""
    late = [(c.id, r["steps"]) for c in B.UNSTABLE_CASES for r in B.reference(c).values() if r["failed"] and r["steps"] > 1]
    print("failed after more than one step:", late)
    assert late


@pytest.mark.parametrize("case", B.CASES, ids=[c.id for c in B.CASES])
def test_no_decision_is_a_near_tie(case):
    """over every computed point: the sign of h against the size of its terms, the uniform of the choice against its probability, and the
    mix preconditioner's uniform against its two thresholds"""
    pr, inp = B.probes(case), B.inputs(case)
    h = min(p["h_margin"] for p in pr.values())
    u = min(p["u_margin"] for p in pr.values())
    pc = min(B.preconditioner_margin(case, inp.words[i]) for i in pr)
    print("%s: least |h| / sum |p g~| = %.1e, least |u - exp(w - L)| = %.1e, preconditioner %.1e" % (case.id, h, u, pc))
    assert h >= MARGIN and u >= MARGIN and pc >= MARGIN, (case, h, u, pc)


@pytest.mark.parametrize("case", PARITY, ids=[c.id for c in PARITY])
def test_rounding_alone_does_not_move_the_trajectory(case):
    """the same transitions with x, p, g~, M and the density's sums in np.longdouble (the draws and logaddexp as they are): the same steps,
    RNG words and selected candidate, the final state within 1e-10 relative -- a tenth of the device tests' tolerance; measured: 4e-12
    at the most (tests/aaps_blocks.py holds the figure of every case)"""
    pr, ld = B.probes(case), B.probes(case, np.longdouble)
    worst = 0.0
    for i, p in pr.items():
        q = ld[i]
        assert (q["steps"], q["Kf"], q["failed"], q["words"], q["selected"], q["n_candidates"]) == \
               (p["steps"], p["Kf"], p["failed"], p["words"], p["selected"], p["n_candidates"]), (case, i)
        x = q["x"].astype(np.float64)
        worst = max(worst, float(np.max(np.abs(x - p["x"]) / np.maximum(np.abs(p["x"]), 1e-300))))
        np.testing.assert_allclose(x, p["x"], rtol=LD_RTOL, atol=1e-13, err_msg="%s replica %d" % (case.id, i))
        assert math.isclose(q["acc"], p["acc"], rel_tol=LD_RTOL, abs_tol=1e-13), (case, i, q["acc"], p["acc"])
    print("%s: largest relative distance of a final coordinate %.1e" % (case.id, worst))
