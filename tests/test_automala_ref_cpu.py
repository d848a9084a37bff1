"""tests/automala_ref.py held to the C oracle (oracle/pt_oracle.c, automala_step) without a device, on the two paths the oracle has: the
scaled-precision MVN path and the funnel.  Every branch of the restatement is pinned here before any device is compared with it
(tests/test_gpu_family_blocks.py, tests/test_gpu_family_edges.py): the last test asserts that the union of the cases sees a shrinking, a
growing and an unmoved search, a failed and a passed reversibility check, an accepted and a rejected proposal and a non-finite trial.

One oracle shard of 4 chains per case, states and chain permutation set, the step and the preconditioner's standard deviations through
set_explorer_adaptation, one explore(scan); the restatement runs every replica off the reference chain from the same RNG words.
RNG words and counting recorders equal; states equal on the MVN path (the gradient -prec x has no reduction in it), within the project's
1e-9 relative + 1e-12 on the funnel (NumPy's pairwise sums against the oracle's fixed tree); the recorders' means (OnlineStats' running
mean in the oracle, a sum here) within 1e-12."""
import math

import numpy as np
import pytest

import aaps_ref as A
import automala_ref as R
import oracle as O

N = 4
BASE_N_REFRESH = 2
FUNNEL_REF_PREC = 1.0 / 9.0
PRECOND = {"identity": 0, "diagonal": 1, "mix": 2}
STEPS = {"mvn": (0.7, 2.0 ** -6, 64.0), "funnel": (0.5, 2.0 ** -6, 64.0)}        # tuned, far too small, far too large
DIMS = [("mvn", d) for d in (1, 10, 64, 65, 130, 300)] + [("funnel", d) for d in (2, 8, 70)]
CASES = [(t, d, step, scan, pc) for t, d in DIMS for step in STEPS[t] for scan in (1, 2) for pc in PRECOND]
IDS = ["%s-d%d-step%g-scan%d-%s" % c for c in CASES]


def n_refresh(d):
    return BASE_N_REFRESH * int(math.ceil(d ** 0.35))


def run(case):
    """-> (the oracle's (x, words, explorer_stats, am_stats), chain, {replica: the restatement's dict + words})"""
    target, d, step, scan, pc = case
    funnel = target == "funnel"
    g = np.random.default_rng(1000 * d + 10 * scan + PRECOND[pc])
    kw = dict(p0=FUNNEL_REF_PREC) if funnel else {}
    sh = O.OracleShard(target=O.TARGET_FUNNEL if funnel else O.TARGET_MVN, explorer=O.EXPLORER_AUTOMALA, n_chains=N, dim=d,
                       am_base_n_refresh=BASE_N_REFRESH, am_preconditioner=PRECOND[pc], seed=d, **kw)
    betas = np.concatenate([[0.0], np.sort(g.uniform(0.0, 1.0, N - 2)), [1.0]])
    sh.set_schedule(betas)
    x = g.normal(0.0, 1.0 if funnel else 0.5, (N, d))
    chain = g.permutation(N).astype(np.int64)
    _, _, rng = sh.states()
    sh.set_states(x, chain, rng)
    std = g.uniform(0.5, 2.0, d)
    sh.set_explorer_adaptation(step, std)
    sh.explore(scan)
    x1, c1, r1 = sh.states()
    assert np.array_equal(c1, chain)
    sh.reduce()
    got = (x1, r1, sh.explorer_stats(), sh.am_stats())
    want = {}
    for i in range(N):
        c = int(chain[i])
        if c == 0:
            continue
        r = O.OracleRng(state=(int(rng[i, 0]), int(rng[i, 1])))
        M = A.build_preconditioner(r, d, PRECOND[pc], 1.0 / 3.0, 1.0 / 3.0, std)
        ch = A.FunnelChain(betas[c], FUNNEL_REF_PREC) if funnel else A.mvn_chain(1.0, 10.0, betas[c])
        want[i] = R.automala_transition(x[i], r, ch, step, n_refresh(d), M, scan != 1)
        want[i]["words"] = r.state
        want[i]["x0"] = x[i]
    return got, chain, want


@pytest.fixture(scope="module")
def results():
    return {}


def _result(results, case):
    if case not in results:
        results[case] = run(case)
    return results[case]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_restatement_equals_the_oracle(results, case):
    target, d, step, scan, pc = case
    (x1, r1, (am, an, ss, sn), (fm, fn, rm, rn)), chain, want = _result(results, case)
    nr = n_refresh(d)
    for i, w in want.items():
        c = int(chain[i])
        what = "%s replica %d chain %d" % (IDS[CASES.index(case)], i, c)
        assert (int(r1[i, 0]), int(r1[i, 1])) == tuple(w["words"]), what
        if target == "mvn":
            assert np.array_equal(x1[i], w["x"]), what
        else:
            np.testing.assert_allclose(x1[i], w["x"], rtol=1e-9, atol=1e-12, err_msg=what)
        searches = nr * (2 if scan != 1 else 1)
        assert w["steps_n"] == w["fac_n"] == searches == len(w["exponents"]), what
        assert w["acc_n"] == w["rev_n"] == (nr if scan != 1 else 0), what
        assert (an[c], sn[c], ss[c], fn[c], rn[c]) == (w["acc_n"], w["steps_n"], w["steps_sum"], w["fac_n"], w["rev_n"]), what
        assert w["fac_sum"] == sum(math.ldexp(1.0, e) for e in w["exponents"]), what
        assert math.isclose(fm[c], w["fac_sum"] / w["fac_n"], rel_tol=1e-12), what
        if scan != 1:
            assert math.isclose(rm[c], w["rev_sum"] / w["rev_n"], rel_tol=1e-12, abs_tol=1e-15), what
            assert math.isclose(am[c], w["acc_sum"] / w["acc_n"], rel_tol=1e-9, abs_tol=1e-12), what
        else:
            assert not np.array_equal(w["x"], w["x0"]), what                 # no MH step: the chain is where the proposal ended


def test_the_cases_reach_every_branch(results):
    """over all the cases: every outcome of a search, of the reversibility check and of the MH step, and a non-finite trial"""
    seen = dict(shrink=0, grow=0, unmoved=0, passed=0, failed=0, accepted=0, rejected=0, nonfinite=0)
    for case in CASES:
        _, _, want = _result(results, case)
        for w in want.values():
            seen["shrink"] += sum(e < 0 for e in w["exponents"])
            seen["grow"] += sum(e > 0 for e in w["exponents"])
            seen["unmoved"] += sum(e == 0 for e in w["exponents"])
            seen["passed"] += w["rev_sum"]
            seen["failed"] += w["rev_n"] - w["rev_sum"]
            seen["nonfinite"] += w["nonfinite"]
            seen["accepted"] += w["accepted"]
            seen["rejected"] += w["acc_n"] - w["accepted"]
    print(seen)
    assert all(v > 0 for v in seen.values()), seen


def test_the_start_must_have_a_finite_density_and_the_step_must_stay_positive():
    r = O.OracleRng(seed=3)
    with pytest.raises(R.AutoMalaError, match="positive density"):
        R.automala_transition(np.array([np.inf, 0.0]), r, A.MvnChain(1.0), 0.5, 1, np.ones(2), True)

    class Nowhere:                                   # every point but the start has no density: the search halves the step down to 0
        def lp_grad(self, x):
            return (0.0 if not np.any(x) else -math.inf), np.zeros_like(x)

    with pytest.raises(R.AutoMalaError, match="positive step size"):
        R.automala_transition(np.zeros(2), r, Nowhere(), 0.5, 1, np.ones(2), True)
