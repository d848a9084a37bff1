"""The families' explore kernels at four and eight blocks per lane (E = 4: d = 129 .. 256, E = 8: 257 .. 512) against the restatements at
one transition, over the case table of tests/family_blocks.py: k_explore_glm, k_explore_hier, k_explore_ar1, k_explore_mixture,
k_explore_dense, k_explore_dense_slice and k_explore_varsel, every (E, LIK or PARAM, slice or Langevin, FULL) instantiation that the
launchers reach from E = 4 on (the Langevin ones under MALA and under AutoMALA, whose step-size search visits the huge and non-finite points) -- the sizes where the hierarchical and AR(1) data leave the registers for L2, the block-sum tree takes its
E >= 4 branch, the dense slice kernel carries its cached u, A and S over up to 512 coordinates and variable selection's Bool coordinate
d + j lies in block (d + j) / 64.  tests/test_family_blocks_cpu.py holds the table to its coverage.

The assertions and tolerances are those of the families' own parity tests (tests/test_gpu_<family>.py): RNG words, Bool coordinates and
the counting recorders equal, Float64 coordinates and the mean acceptance within 1e-9 relative (states: + 1e-12), log densities within
1e-11 relative + 1e-11.  Nearly all of the time is the restatements' arithmetic on the CPU."""
import math

import numpy as np
import pytest

import automala_ref as R
import family_blocks as B
import oracle as O

pytestmark = pytest.mark.gpu

RTOL = 1e-9
LP_RTOL = 1e-11


@pytest.fixture(scope="module")
def P():
    import pigeons_amd
    return pigeons_amd


def _pt(P, case, explorer, **kw):
    target, ref_dim = B.model(case).device(P)
    return P.PT(P.Inputs(target=target, reference=P.ScaledPrecisionNormalLogPotential(B.model(case).ref_prec, ref_dim), n_chains=case.N,
                         n_rounds=2, explorer=explorer, show_report=False, **kw))


def _random_states(pt, case):
    """the case's schedule, states and chain permutation on the engine, which keeps its own RNG words -> (betas, x, chain, rng)"""
    eng = pt.replicas
    betas, x, chain = B.layout(case)
    eng.set_schedule(betas)
    _, _, rng = eng.states()
    eng.set_states(x, chain, rng)
    return betas, x, chain, rng


@pytest.mark.parametrize("case", B.SLICE_CASES, ids=[c.id for c in B.SLICE_CASES])
def test_one_slice_transition_parity(P, case):
    """one SliceSampler pass (w = 10, p = 20) of every replica against oracle.MixedSliceSampler on the restatement's path_lp from the same
    RNG words; variable selection also the reference chain's i.i.d. draw: d thetas, then d Bools"""
    m, d, N = B.model(case), case.d, case.N
    pt = _pt(P, case, P.SliceSampler(w=case.kw["w"], p=case.kw["p"], n_passes=case.kw["n_passes"]))
    betas, x, chain, rng = _random_states(pt, case)
    eng = pt.replicas
    eng.explore(1)
    x1, c1, r1 = eng.states()
    eng.reduce()
    am, an, ss, sn = eng.explorer_stats()
    assert np.array_equal(c1, chain)
    exact = m.kinds != O.COORD_FLOAT64
    moved = flipped = 0
    for i in range(N):
        c = int(chain[i])
        what = "%s replica %d chain %d" % (case.id, i, c)
        if c == 0:
            if case.family != "varsel":                  # the reference chain draws i.i.d.: the families' own tests hold that
                continue
            cols = d // 2                                # sample_iid!: randn / sqrt(p) per theta, then rand(rng, Bool) per indicator
            r = O.OracleRng(state=(int(rng[i, 0]), int(rng[i, 1])))
            yv = np.array([r.randn() / math.sqrt(m.ref_prec) for _ in range(cols)] + [float(r.rand_bool()) for _ in range(cols)])
            words = r.state
            assert an[c] == 0 and sn[c] == 0, what
        else:
            yv, words, stats = B.slice_reference(case, betas[c], x[i], rng[i])
            assert an[c] == stats.acc_n and sn[c] == stats.steps_n and ss[c] == stats.steps_sum, what
            np.testing.assert_allclose(am[c], stats.acc_mean, rtol=RTOL, err_msg=what)
            moved += int(np.sum(yv[~exact] != x[i][~exact]))
            flipped += int(np.sum(yv[exact] != x[i][exact]))
        assert (int(r1[i, 0]), int(r1[i, 1])) == tuple(words), what
        assert np.array_equal(x1[i][exact], yv[exact]), what
        np.testing.assert_allclose(x1[i][~exact], yv[~exact], rtol=RTOL, atol=1e-12, err_msg=what)
    assert moved > 0 and (flipped > 0 or not exact.any())


@pytest.mark.parametrize("case", B.MALA_CASES, ids=[c.id for c in B.MALA_CASES])
def test_one_mala_transition_parity(P, case):
    """one MALA transition (3 ceil(d^0.35) refreshes) against aaps_ref.build_preconditioner + mixture_ref.mala_transition, refresh by
    refresh, so that the test sees that the restatement accepts some proposals and rejects others"""
    d, N, step = case.d, case.N, case.kw["step"]
    pc = {"identity": P.IdentityPreconditioner, "diagonal": P.DiagonalPreconditioner, "mix": P.MixDiagonalPreconditioner}[case.kw["precond"]]()
    ex = P.MALA(step_size=step, preconditioner=pc)
    pt = _pt(P, case, ex)
    betas, x, chain, rng = _random_states(pt, case)
    assert np.array_equal(rng, B.init_rng_words(N))      # the words tests/test_family_blocks_cpu.py counted the proposals with
    eng = pt.replicas
    eng.set_explorer_adaptation(step, B.target_std(case))
    eng.explore(2)
    x1, c1, r1 = eng.states()
    eng.reduce()
    am, an, ss, sn = eng.explorer_stats()
    assert np.array_equal(c1, chain)
    nr = ex.base_n_refresh * int(math.ceil(d ** ex.exponent_n_refresh))
    assert nr == B.n_refresh(d)
    res, accepted, rejected = B.mala_reference(case, betas, x, chain, rng)
    for i, want in res.items():
        c = int(chain[i])
        what = "%s replica %d chain %d" % (case.id, i, c)
        assert (int(r1[i, 0]), int(r1[i, 1])) == tuple(want["words"]), what
        np.testing.assert_allclose(x1[i], want["x"], rtol=RTOL, atol=1e-12, err_msg=what)
        assert an[c] == nr and sn[c] == nr and ss[c] == nr, what
        np.testing.assert_allclose(am[c], want["acc_sum"] / nr, rtol=RTOL, atol=1e-12, err_msg=what)
    print("MALA %s, step %g: %d proposals accepted, %d rejected" % (case.id, step, accepted, rejected))
    assert accepted > 0 and rejected > 0


@pytest.mark.parametrize("case", B.AUTOMALA_CASES, ids=[c.id for c in B.AUTOMALA_CASES])
def test_one_automala_transition_parity(P, case):
    """one AutoMALA transition (base_n_refresh = 1: ceil(d^0.35) refreshes) in the case's regime -- its step, with the MH step (scan 2) or
    without (scan 1) -- against aaps_ref.build_preconditioner + automala_ref.automala_transition: RNG words, the counting recorders, the sum
    of the step-size factors and the number of reversibility checks passed equal, states and mean acceptance within RTOL.
    tests/test_family_blocks_cpu.py holds the restatement alone to what makes the comparison meaningful (both outcomes of every decision,
    none of them closer than 1e-6 to the other)"""
    d, N, step = case.d, case.N, case.kw["step"]
    pc = {"identity": P.IdentityPreconditioner, "diagonal": P.DiagonalPreconditioner, "mix": P.MixDiagonalPreconditioner}[case.kw["precond"]]()
    ex = P.AutoMALA(base_n_refresh=B.AUTOMALA_BASE_N_REFRESH, step_size=step, preconditioner=pc)
    assert ex.base_n_refresh * int(math.ceil(d ** ex.exponent_n_refresh)) == B.n_refresh(d, base=B.AUTOMALA_BASE_N_REFRESH)
    pt = _pt(P, case, ex)
    betas, x, chain, rng = _random_states(pt, case)
    assert np.array_equal(rng, B.init_rng_words(N))      # the words tests/test_family_blocks_cpu.py held the restatement to its conditions with
    eng = pt.replicas
    eng.set_explorer_adaptation(step, B.target_std(case))
    eng.explore(case.kw["scan"])
    res = B.automala_reference(case, betas, x, chain, rng)
    assert len(res) == N - 1
    R.assert_engine_matches(eng, chain, res, RTOL, lambda i: case.id)


@pytest.mark.parametrize("case", B.LOG_DENSITY_CASES, ids=[c.id for c in B.LOG_DENSITY_CASES])
def test_log_density_at_every_beta(P, case):
    """the refresh kernels that no family's test_log_density_at_every_beta visits (glm E = 2 and 4, mixture E = 4, varsel E = 4 and a ragged
    E = 8), by the method of those tests: the extended trace of one step against the restatement at the state the step left"""
    m, d, N = B.model(case), case.d, case.N
    pt = _pt(P, case, P.SliceSampler(n_passes=1), record=[P.traces], extended_traces=True)
    betas, x0, _, _ = _random_states(pt, case)
    eng = pt.replicas
    eng.explore(1)
    eng.swap(1)                                   # (a scan ends at its swap: the traces count it from there)
    eng.reduce()
    tr = eng.traces()
    assert tr.shape == (1, N, d + 1)
    for c in range(N):
        after = tr[0, c, :d]
        assert not any(np.array_equal(after, x0[i]) for i in range(N))        # the state is the step's, not the one that was set
        ch = m.chain(betas[c])
        want = ch.lp_full(after) if case.family == "varsel" else ch.path_lp(after)
        assert math.isclose(tr[0, c, d], want, rel_tol=LP_RTOL, abs_tol=1e-11), (case.id, c, betas[c], tr[0, c, d], want)
