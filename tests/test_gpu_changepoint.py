"""The Poisson change-point family on the device (k_explore_changepoint, pigeons.jl_amd/csrc/pte_changepoint.hpp) against its NumPy
restatement (tests/changepoint_ref.py): the log density at every chain's beta, one SliceSampler transition of every replica from random
states -- Float64 and Integer coordinates, draw for draw against oracle.MixedSliceSampler -- under both evaluation forms, the reference
chain's draw, whole runs against the exact change-point posterior and evidence from enumeration, determinism, the chain-sharded engine,
checkpoint / resume and replacing the data.

RNG words, Integer coordinates and step counts are compared exactly; Float64 coordinates to 1e-12 and log densities to 1e-13 relative: the
one difference between the device and the restatement is exp (ocml against libm, an ulp), every other operation is the same IEEE one.
These are tighter than the figures of tests/family_gpu.py, whose shared checks take them as arguments."""
import math

import numpy as np
import pytest

import family_gpu as G
import oracle as O
import changepoint_ref as R
from family_gpu import P  # noqa: F401  (the module's fixture)

pytestmark = pytest.mark.gpu

X_RTOL = 1e-12
LP_RTOL = 1e-13


def _data(n, K, seed=1):
    """piecewise-constant Poisson counts: K + 1 segments of about equal length with rates drawn from 0.5..12"""
    g = np.random.default_rng(seed)
    rates = g.uniform(0.5, 12.0, K + 1)
    seg = np.minimum((np.arange(n) * (K + 1)) // max(n, 1), K)
    return g.poisson(rates[seg]).astype(np.float64)


def _pt(P, y, K, prec, N, n_passes=3, record=(), slice_kw=None, **kw):
    return P.PT(P.Inputs(target=P.PoissonChangePoint(y, K), reference=P.ScaledPrecisionNormalLogPotential(prec, K + 1), n_chains=N,
                         n_rounds=2, explorer=P.SliceSampler(n_passes=n_passes, **(slice_kw or {})), record=list(record), show_report=False, **kw))


def _random_states(pt, N, K, n, seed, scale=1.0):
    """random schedule, rates N(0, scale^2) around log 4, taus uniform on 0..n -- with a tie in the replicas that have two taus or more, and a tau at
    0 or at n in turn --, a random chain permutation; the streams stay the engine's"""
    eng = pt.replicas
    g = np.random.default_rng(seed)
    betas = np.concatenate([[0.0], np.sort(g.uniform(0.0, 1.0, N - 2)), [1.0]])
    eng.set_schedule(betas)
    tau = g.integers(0, n + 1, (N, K)).astype(np.float64)
    tau[0::2, K // 2] = 0.0
    tau[1::2, K // 2] = float(n)
    if K >= 2:
        rows = slice(0, None, 3) if K == 2 else slice(None)       # (K = 2: the tie takes the column of the 0 / n in every third replica)
        tau[rows, -1] = tau[rows, 0]
    x = np.concatenate([math.log(4.0) + g.normal(0.0, scale, (N, K + 1)), tau], axis=1)
    chain = g.permutation(N).astype(np.int64)
    _, _, rng = eng.states()
    eng.set_states(x, chain, rng)
    return betas, x, chain, rng


def test_state_calls_need_the_data_and_the_setter_validates(P):
    L = P._lib
    eng = P.Engine(n_chains=4, target=L.TARGET_CHANGE_POINT, dim=7, explorer=L.EXPLORER_SLICE, target_params=[1.0])
    for call in (lambda: eng.explore(1), lambda: eng.swap(1), lambda: eng.run_scans(1, 2), lambda: eng.states()):
        with pytest.raises(P.PteError, match="call pte_set_target_changepoint first"):
            call()
    y = _data(10, 3)
    cases = [
        (np.zeros(0), r"1\.\.65536 observations \(got 0\)"),
        (np.zeros(65537), r"1\.\.65536 observations \(got 65537\)"),
        (np.where(np.arange(10) == 2, np.inf, y), r"y\[2\] must be an integer count in 0\.\.2\^20 \(got inf\)"),
        (np.where(np.arange(10) == 3, np.nan, y), r"y\[3\] must be an integer count"),
        (np.where(np.arange(10) == 4, 0.5, y), r"y\[4\] must be an integer count in 0\.\.2\^20 \(got 0\.5\)"),
        (np.where(np.arange(10) == 5, -1.0, y), r"y\[5\] must be an integer count"),
        (np.where(np.arange(10) == 9, 2.0 ** 20 + 1, y), r"y\[9\] must be an integer count"),
    ]
    for arg, msg in cases:
        with pytest.raises(P.PteError, match=msg):
            eng.set_target_changepoint(arg)
    with pytest.raises(P.PteError, match="null argument"):
        eng._chk(eng.L.pte_set_target_changepoint(eng.h, None, 10))
    with pytest.raises(P.PteError, match="form must be PTE_CHANGEPOINT_FORM_AUTO"):
        eng.set_changepoint_form(3)
    other = P.Engine(n_chains=4, target=L.TARGET_FUNNEL, dim=7, explorer=L.EXPLORER_SLICE, target_params=[1.0])
    with pytest.raises(P.PteError, match="not PTE_TARGET_CHANGE_POINT"):
        other.set_target_changepoint(y)
    with pytest.raises(P.PteError, match="not PTE_TARGET_CHANGE_POINT"):
        other.set_changepoint_form(1)
    eng.set_target_changepoint(np.where(np.arange(10) == 9, 2.0 ** 20, y))          # the largest count is accepted
    eng.set_target_changepoint(y)
    with pytest.raises(P.PteError, match="only the interpolated \\(funnel\\) path has a replaceable reference"):
        eng.set_variational_reference(np.zeros(7), np.ones(7), np.ones(4, dtype=np.int32))
    x0 = eng.states()[0]
    assert np.all(x0 == 0.0)                      # the initial state: K empty segments and one whole-series segment
    eng.explore(1)
    x = eng.states()[0]
    assert x.shape == (4, 7) and eng.kernel_name() == "k_explore_changepoint" and eng.scan_loop_name() == ""
    assert np.all(x[:, 4:] == np.floor(x[:, 4:])) and x[:, 4:].min() >= 0 and x[:, 4:].max() <= 10


@pytest.mark.parametrize("n,K", [(1, 1), (40, 3), (200, 31), (130, 32), (300, 63), (65536, 2)])
def test_log_density_at_every_beta(P, n, K):
    """the device's log density (extended traces of one explore step of no passes, which evaluates the state in full and leaves it) against
    the restatement, every chain's beta: one observation, a ragged block (dim 63), the taus straddling the two blocks (dim 65), all 64 lanes
    segments (dim 127) and the prefix table's full range; ties, taus at 0 and taus at n among the states"""
    y = _data(n, K, seed=n + K)
    N, prec, dim = 12, 0.5, 2 * K + 1
    pt = _pt(P, y, K, prec, N, n_passes=0, record=[P.traces], extended_traces=True)
    betas, x, chain, _ = _random_states(pt, N, K, n, seed=K, scale=0.7)
    tr = G.log_densities(pt, N, dim)
    cp = R.ChangePoint(y, K, prec)
    kept = 0
    for c in range(N):
        tau = tr[c, K + 1:dim]
        assert np.all(tau == np.floor(tau)) and tau.min() >= 0 and tau.max() <= n
        kept += int(any(np.array_equal(tr[c, :dim], x[i]) for i in range(N)))
    wants = G.assert_log_density_at_every_beta(tr, betas, dim, lambda beta: R.ChangePointChain(cp, beta, prec).path_lp, LP_RTOL, abs_tol=0.0)
    assert all(math.isfinite(want) for want in wants)
    assert kept >= N - 1                                    # every state but the reference chain's fresh draw is one of those handed in
    taus = tr[:, K + 1:dim]
    assert np.any(taus == 0.0) and np.any(taus == float(n))
    if K >= 2:
        assert any(len(set(row)) < K for row in taus)


_NARROW = dict(w=2.0, p=2)           # a first interval that the doubling cap p keeps from covering the slice (the default w = 10, p = 20 never
                                     # binds); w stays integral: the Integer method's midpoints are integral only then


_PARITY = [(40, 3, "auto", {}), (200, 31, "auto", {}), (130, 32, "auto", {}), (300, 63, "auto", {}), (200, 31, "other", {}),
           (40, 3, "auto", _NARROW), (40, 3, "other", _NARROW)]


@pytest.mark.parametrize("n,K,form,slice_kw", _PARITY, ids=["-".join(map(str, c[:3])) + ("-narrow" if c[3] else "") for c in _PARITY])
def test_one_slice_transition_parity(P, n, K, form, slice_kw):
    """every replica's transition from its own RNG words against oracle.MixedSliceSampler on the restatement's call-back: the same draws in
    the same order (final RNG words equal), every Integer coordinate equal, the Float64 ones within X_RTOL, the explorer recorders equal;
    the reference chain's i.i.d. draw: K + 1 normals, then rand(rng, 0:n) per tau.  The "other" cases run the evaluation form that the
    engine does not choose by itself, the last two cases both forms with the doubling cut short at p = 2"""
    y = _data(n, K, seed=7 * n + K)
    N, prec, dim = 8, 0.5, 2 * K + 1
    pt = _pt(P, y, K, prec, N, slice_kw=slice_kw)
    eng = pt.replicas
    if form == "other":
        eng.set_changepoint_form(P._lib.CHANGEPOINT_FORM_FULL)      # (the engine's own choice is the cached form: DESIGN 4.13)
    betas, x, chain, rng = _random_states(pt, N, K, n, seed=n, scale=0.5)
    eng.explore(1)
    x1, c1, r1 = eng.states()
    eng.reduce()
    am, an, ss, sn = eng.explorer_stats()
    assert np.array_equal(c1, chain)
    cp = R.ChangePoint(y, K, prec)
    kinds = np.array([O.COORD_FLOAT64] * (K + 1) + [O.COORD_INTEGER] * K, dtype=np.int32)
    moved = 0
    for i in range(N):
        c = int(chain[i])
        r = O.OracleRng(state=(int(rng[i, 0]), int(rng[i, 1])))
        if c == 0:                                # sample_iid! at the reference: randn / sqrt(p) per rate, then rand(rng, 0:n) per tau
            yv = np.array([r.randn() / math.sqrt(prec) for _ in range(K + 1)] + [float(r.rand_range(0, n)) for _ in range(K)])
            assert an[c] == 0 and sn[c] == 0
        else:
            s = O.MixedSliceSampler(R.ChangePointChain(cp, betas[c], prec).path_lp, kinds, **slice_kw)
            yv = x[i].copy()
            s.step(r, yv)
            assert an[c] == s.stats.acc_n and sn[c] == s.stats.steps_n and ss[c] == s.stats.steps_sum, (i, c)
            np.testing.assert_allclose(am[c], s.stats.acc_mean, rtol=1e-12)
            moved += int(np.sum(yv[K + 1:] != x[i, K + 1:]))
        assert int(r1[i, 0]) == r.state[0] and int(r1[i, 1]) == r.state[1], (i, c)
        assert np.array_equal(x1[i, K + 1:], yv[K + 1:]), (i, c, x1[i, K + 1:], yv[K + 1:])
        np.testing.assert_allclose(x1[i, :K + 1], yv[:K + 1], rtol=X_RTOL, atol=1e-12, err_msg="replica %d chain %d" % (i, c))
    assert moved > 0


def test_the_shrink_cap_is_an_error_with_the_coordinate(P):
    """slice_shrink!'s "Maximum number of iterations reached" (SliceSampler.jl:179-185): w = 4096 with max_iter = 2.  The oracle on the same
    streams ends in its own error in every chain but the reference; the engine reports a tempered chain and one of the 2 K + 1 coordinates"""
    n, K, N, prec = 40, 3, 8, 0.5
    slice_kw = dict(w=4096.0, max_iter=2)
    y = _data(n, K, seed=7 * n + K)
    pt = _pt(P, y, K, prec, N, slice_kw=slice_kw)
    betas, x, chain, rng = _random_states(pt, N, K, n, seed=n, scale=0.5)
    cp = R.ChangePoint(y, K, prec)
    kinds = np.array([O.COORD_FLOAT64] * (K + 1) + [O.COORD_INTEGER] * K, dtype=np.int32)
    for i in range(N):
        c = int(chain[i])
        if c != 0:
            s = O.MixedSliceSampler(R.ChangePointChain(cp, betas[c], prec).path_lp, kinds, **slice_kw)
            with pytest.raises(RuntimeError, match="maximum number of iterations"):
                s.step(O.OracleRng(state=(int(rng[i, 0]), int(rng[i, 1]))), x[i].copy())
    eng = pt.replicas
    with pytest.raises(P.PteError, match=r"Maximum number of iterations reached in slice_shrink! \(chain [1-7], index [0-6]\)"):
        eng.explore(1)
        eng.reduce()


def test_both_forms_give_the_same_bits(P):
    """two engines from the same seed, one per evaluation form, four scans with swaps: every state word, stream word and swap statistic equal"""
    y = _data(500, 20, seed=3)
    out = []
    for form in (P._lib.CHANGEPOINT_FORM_FULL, P._lib.CHANGEPOINT_FORM_CACHED):
        pt = _pt(P, y, 20, 0.5, 8, record=[P.traces], extended_traces=True, seed=9)
        pt.replicas.set_changepoint_form(form)
        pt.replicas.run_scans(1, 4)
        pt.replicas.reduce()
        out.append((pt.replicas.states(), pt.replicas.traces()))
    (sa, ta), (sb, tb) = out
    assert all(np.array_equal(a, b) for a, b in zip(sa, sb)) and np.array_equal(ta, tb)
    assert len(np.unique(ta[:, -1, 21:41])) > 10


# ---- whole runs ------------------------------------------------------------------------------------------------------------------------
def _run(P, target, prec, seed, n_rounds):
    return G.run_rounds(P, target, prec, seed, n_rounds, P.SliceSampler(), n_chains=16, ref_dim=target.n_rates,
                        record=["round_trip", "online", "traces", "log_sum_ratio", "index_process"])[0]


_RUN = dict(y=[3, 0, 1, 2, 0, 0, 0, 1, 8, 6, 2, 3, 8, 6, 8, 4, 3, 2, 4, 2, 2, 2, 1, 3], K=2, prec=0.25, n_rounds=10, seeds=(1, 2, 3), B=32)


@pytest.fixture(scope="module")
def runs(P):
    t = P.PoissonChangePoint(_RUN["y"], _RUN["K"])
    return {seed: _run(P, t, _RUN["prec"], seed, _RUN["n_rounds"]) for seed in _RUN["seeds"]}, t


@pytest.fixture(scope="module")
def exact():
    """(log p(y), P(s_1 = 8), E[s_1], E[s_2]) from the 25^2 placements, every segment's rate integrated out by quadrature"""
    log_ev, post = R.ChangePoint(_RUN["y"], _RUN["K"], _RUN["prec"]).exact()
    p8 = sum(w for s, w in post.items() if s[0] == 8)
    m1 = sum(w * s[0] for s, w in post.items())
    m2 = sum(w * s[1] for s, w in post.items())
    return log_ev, p8, m1, m2


def test_the_data_can_tell_the_posterior_from_the_prior(exact):
    """from the reference alone: the exact P(smaller change point = 8) is more than 8 standard errors from the prior's
    ((25 - 8)^2 - (24 - 8)^2) / 25^2 = 0.0528, with the standard error of the indicator's mean over the last round's 2^10 scans taken at a
    quarter of their number as effective sample size -- so a sampler that ignored the data would fail the tests below"""
    log_ev, p8, m1, m2 = exact
    prior8 = (17 ** 2 - 16 ** 2) / 625.0
    T_eff = 2 ** _RUN["n_rounds"] / 4.0
    se = math.sqrt(p8 * (1.0 - p8) / T_eff)
    print("exact: log p(y) %.4f, P(s_1 = 8) %.4f (prior %.4f), E[s_1] %.3f, E[s_2] %.3f" % (log_ev, p8, prior8, m1, m2))
    assert abs(p8 - prior8) / se > 8.0, (p8, prior8, se)
    assert 0.1 < p8 < 0.9                                     # not frozen: the batch-means errors below are not degenerate
    assert abs(m1 - 24 * 1 / 3.0) > 0.5 or abs(m2 - 24 * 2 / 3.0) > 0.5      # the prior's means of the two order statistics are 8 and 16


@pytest.mark.parametrize("seed", _RUN["seeds"])
def test_run_against_the_exact_change_point_posterior(P, runs, exact, seed):
    """16 chains, SliceSampler, 10 rounds.  On the target chain's trace of the last round: the frequency of (smaller change point = 8) and
    the means of the two sorted change points against the enumeration, each within 5 Monte Carlo standard errors, the error by batch means
    over B = 32 batches.  (Measured on an MI355X, in standard errors: DESIGN 4.13.)"""
    pts, _ = runs
    pt = pts[seed]
    K, B = _RUN["K"], _RUN["B"]
    _, p8, m1, m2 = exact
    tr = pt.reduced_recorders.traces[:, -1, :2 * K + 1]             # the target chain
    assert tr.shape[0] == 2 ** _RUN["n_rounds"]
    tau = tr[:, K + 1:]
    assert np.all(tau == np.floor(tau)) and tau.min() >= 0 and tau.max() <= len(_RUN["y"])
    s = np.sort(tau, axis=1)
    stats = np.stack([(s[:, 0] == 8).astype(float), s[:, 0], s[:, 1]], axis=1)
    T = stats.shape[0] // B * B
    bm = stats[:T].reshape(B, T // B, 3).mean(axis=1)
    se = bm.std(axis=0, ddof=1) / math.sqrt(B)
    dev = (stats.mean(axis=0) - np.array([p8, m1, m2])) / se
    print("seed %d: P(s_1 = 8), E[s_1], E[s_2] deviations / se %s" % (seed, np.round(dev, 2)))
    assert np.all(se > 0) and np.all(np.abs(dev) < 5.0), (stats.mean(axis=0), (p8, m1, m2), se)
    assert P.n_round_trips(pt) > 0


def test_runs_against_the_exact_evidence(P, runs, exact):
    """stepping_stone - evidence_offset of the three seeds against the exact log evidence: the mean within 5 standard errors, the standard
    error from the spread over the seeds"""
    pts, t = runs
    log_ev = exact[0]
    assert math.isclose(t.evidence_offset(_RUN["prec"]), R.ChangePoint(_RUN["y"], _RUN["K"], _RUN["prec"]).evidence_offset(), rel_tol=1e-15)
    est = np.array([P.stepping_stone(pts[s]) - t.evidence_offset(_RUN["prec"]) for s in _RUN["seeds"]])
    se = est.std(ddof=1) / math.sqrt(len(est))
    print("log evidence: estimates %s, exact %.4f, deviation / se %.2f" % (np.round(est, 4), log_ev, (est.mean() - log_ev) / se))
    assert abs(est.mean() - log_ev) < 5.0 * se, (est, log_ev, se)


def _inputs(P, seed=1, n_rounds=5, checkpoint=False):
    y = _data(80, 5, seed=23)
    return P.Inputs(target=P.PoissonChangePoint(y, 5), reference=P.ScaledPrecisionNormalLogPotential(0.5, 6),
                    n_chains=12, n_rounds=n_rounds, seed=seed, explorer=P.SliceSampler(), checkpoint=checkpoint,
                    record=[P.round_trip, P.traces, P.log_sum_ratio, P.index_process, P.swap_acceptance_pr, P.energy_ac1], show_report=False)


def test_two_runs_are_equal_bit_for_bit(P):
    a = G.assert_two_runs_equal(P, lambda: _inputs(P, seed=3))
    assert np.all(np.isfinite(a.reduced_recorders.traces)) and len(np.unique(a.reduced_recorders.traces[:, 6:11])) > 10


def test_sharded_equals_single_engine(P):
    G.assert_sharded_equals_single(P, lambda: G.with_recorders(P, _inputs(P, seed=4, n_rounds=4), "online"), n_shards=2)


def test_checkpoint_resume_equals_uninterrupted(P, tmp_path):
    G.assert_checkpoint_resume(P, lambda **kw: _inputs(P, seed=5, **kw), tmp_path)


def test_new_data_replaces_the_old(P):
    """set_target_changepoint again (another n on the same engine): the swap statistics are refreshed at once, and the log densities of the
    next step are the new data's"""
    K, N, prec = 4, 8, 0.5
    y1, y2 = _data(60, K, seed=31), _data(90, K, seed=32)
    pt = _pt(P, y1, K, prec, N, n_passes=0, record=[P.traces], extended_traces=True)
    betas, _, _, _ = _random_states(pt, N, K, 60, seed=3, scale=0.5)
    pt.replicas.set_target_changepoint(y2)
    tr = G.log_densities(pt, N, 2 * K + 1)
    new, old = R.ChangePoint(y2, K, prec), R.ChangePoint(y1, K, prec)
    G.assert_log_density_at_every_beta(tr, betas, 2 * K + 1, lambda beta: R.ChangePointChain(new, beta, prec).path_lp, LP_RTOL, abs_tol=0.0)
    G.assert_log_density_is_not(tr, betas, 2 * K + 1, lambda beta: R.ChangePointChain(old, beta, prec).path_lp)
