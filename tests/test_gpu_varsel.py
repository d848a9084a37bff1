"""The variable-selection family on the device (k_explore_varsel, pigeons.jl_amd/csrc/pte_varsel.hpp) against its NumPy restatement
(tests/varsel_ref.py): the log density at every chain's beta, one SliceSampler transition of every replica from random states -- Float64 and
Bool coordinates, draw for draw against oracle.MixedSliceSampler -- and the reference chain's draw, whole runs against the exact inclusion
probabilities, coefficient means and evidence of the conjugate normal-identity model, determinism, the chain-sharded engine, checkpoint /
resume and replacing the data.

RNG words and Bool coordinates are compared exactly; Float64 coordinates, recorders and log densities to the RTOL and LP_RTOL of
tests/family_gpu.py, which holds the shared checks and says why: this family is of the GLM's arithmetic class."""
import math

import numpy as np
import pytest

import family_gpu as G
import oracle as O
import varsel_ref as R
from family_gpu import LP_RTOL, RTOL, P  # noqa: F401  (P: the module's fixture)

pytestmark = pytest.mark.gpu


def _data(n, d, lik, seed=1, noise_sd=1.0):
    """X with entries N(0, 1 / d) (eta of order |theta|), y drawn from the model at theta ~ N(0, I) with every second column switched off"""
    g = np.random.default_rng(seed)
    X = g.normal(0.0, 1.0 / math.sqrt(d), (n, d))
    eta = X @ (g.normal(0.0, 1.0, d) * (np.arange(d) % 2 == 0))
    y = (g.uniform(size=n) < 1 / (1 + np.exp(-eta))).astype(float) if lik == "bernoulli_logit" else eta + noise_sd * g.normal(size=n)
    return X, y


def _pt(P, X, y, lik, prec, N, pi=0.5, noise_sd=1.0, n_passes=3, record=(), slice_kw=None, **kw):
    return P.PT(P.Inputs(target=P.SpikeSlabRegression(X, y, likelihood=lik, noise_sd=noise_sd, inclusion_prob=pi),
                         reference=P.ScaledPrecisionNormalLogPotential(prec, X.shape[1]), n_chains=N, n_rounds=2,
                         explorer=P.SliceSampler(n_passes=n_passes, **(slice_kw or {})), record=list(record), show_report=False, **kw))


def _random_states(pt, N, d, seed, scale=1.5):
    """random schedule, thetas N(0, scale^2), indicators fair coins, a random chain permutation; the streams stay the engine's"""
    eng = pt.replicas
    g = np.random.default_rng(seed)
    betas = np.concatenate([[0.0], np.sort(g.uniform(0.0, 1.0, N - 2)), [1.0]])
    eng.set_schedule(betas)
    x = np.concatenate([g.normal(0.0, scale, (N, d)), (g.uniform(size=(N, d)) < 0.5).astype(float)], axis=1)
    chain = g.permutation(N).astype(np.int64)
    _, _, rng = eng.states()
    eng.set_states(x, chain, rng)
    return betas, x, chain, rng


def test_state_calls_need_the_data_and_the_setter_validates(P):
    L = P._lib
    eng = P.Engine(n_chains=4, target=L.TARGET_VARIABLE_SELECTION, dim=6, explorer=L.EXPLORER_SLICE, target_params=[1.0])
    for call in (lambda: eng.explore(1), lambda: eng.swap(1), lambda: eng.run_scans(1, 2), lambda: eng.states()):
        with pytest.raises(P.PteError, match="call pte_set_target_varsel first"):
            call()
    X, y = _data(10, 3, "bernoulli_logit")
    cases = [
        ((7, X, y, 1.0, 0.5), "likelihood must be PTE_GLM_BERNOULLI_LOGIT"),
        ((0, np.zeros((10, 4)), y, 1.0, 0.5), r"this engine holds dim / 2 = 3 columns \(got 4\)"),
        ((0, np.zeros((4097, 3)), np.zeros(4097), 1.0, 0.5), r"1\.\.4096 observations"),
        ((0, np.zeros((0, 3)), np.zeros(0), 1.0, 0.5), r"1\.\.4096 observations"),
        ((0, np.where(np.arange(30).reshape(10, 3) == 4, np.nan, X), y, 1.0, 0.5), r"X\[1\]\[1\] must be finite"),
        ((0, X, np.where(np.arange(10) == 2, np.inf, y), 1.0, 0.5), r"y\[2\] must be finite"),
        ((0, X, np.where(np.arange(10) == 3, 0.5, y), 1.0, 0.5), r"needs y in \{0, 1\}"),
        ((1, X, y, 0.0, 0.5), "noise_sd positive and finite"),
        ((0, X, y, 1.0, 0.0), r"inclusion_prob must be in \(0, 1\) \(got 0\)"),
        ((0, X, y, 1.0, 1.0), r"inclusion_prob must be in \(0, 1\)"),
        ((0, X, y, 1.0, float("nan")), r"inclusion_prob must be in \(0, 1\)"),
    ]
    for args, msg in cases:
        with pytest.raises(P.PteError, match=msg):
            eng.set_target_varsel(*args)
    big = P.Engine(n_chains=4, target=L.TARGET_VARIABLE_SELECTION, dim=128, explorer=L.EXPLORER_SLICE, target_params=[1.0])
    with pytest.raises(P.PteError, match=r"n_obs \* d must be <= 131072"):
        big.set_target_varsel(0, np.zeros((2049, 64)), np.zeros(2049), 1.0, 0.5)
    with pytest.raises(P.PteError, match="null argument"):
        eng._chk(eng.L.pte_set_target_varsel(eng.h, None, None, 10, 3, 0, 1.0, 0.5))
    eng.set_target_varsel(0, X, y, 1.0, 0.5)
    with pytest.raises(P.PteError, match="only the interpolated \\(funnel\\) path has a replaceable reference"):
        eng.set_variational_reference(np.zeros(6), np.ones(6), np.ones(4, dtype=np.int32))
    eng.explore(1)
    x = eng.states()[0]
    assert x.shape == (4, 6) and eng.kernel_name() == "k_explore_varsel" and eng.scan_loop_name() == ""
    assert set(np.unique(x[:, 3:])) <= {0.0, 1.0}


@pytest.mark.parametrize("lik,n,d,pi", [("bernoulli_logit", 1, 1, 0.5), ("bernoulli_logit", 300, 40, 0.3), ("normal_identity", 100, 5, 0.5),
                                        ("normal_identity", 130, 64, 0.7), ("bernoulli_logit", 4096, 32, 0.5),
                                        ("normal_identity", 512, 256, 0.2)])
def test_log_density_at_every_beta(P, lik, n, d, pi):
    """the device's log density (extended traces of one explore step) against the restatement at the state the step left, every chain's
    beta: ragged n and d, whole blocks (2 d = 64, 128, 512), the largest n, the largest d and the largest n d"""
    X, y = _data(n, d, lik, seed=n + d, noise_sd=0.8)
    N, prec = 12, 0.5
    pt = _pt(P, X, y, lik, prec, N, pi=pi, noise_sd=0.8, n_passes=1, record=[P.traces], extended_traces=True)
    betas, _, _, _ = _random_states(pt, N, d, seed=d, scale=0.5)
    tr = G.log_densities(pt, N, 2 * d)
    vs = R.VarSel(X, y, lik, 0.8, prec, pi)
    for c in range(N):
        assert set(np.unique(tr[c, d:2 * d])) <= {0.0, 1.0}
    G.assert_log_density_at_every_beta(tr, betas, 2 * d, lambda beta: R.VarSelChain(vs, beta, prec).lp_full, LP_RTOL, abs_tol=1e-11)


_NARROW = dict(w=0.25, p=3)          # a first interval that the doubling cap p keeps from covering the slice (the default w = 10, p = 20 never binds)


_PARITY = [("bernoulli_logit", 50, 3, 0.5, {}), ("normal_identity", 70, 5, 0.3, {}), ("bernoulli_logit", 130, 40, 0.2, {}),
           ("normal_identity", 90, 32, 0.5, {}), ("bernoulli_logit", 50, 3, 0.5, _NARROW), ("normal_identity", 70, 5, 0.3, _NARROW)]


@pytest.mark.parametrize("lik,n,d,pi,slice_kw", _PARITY, ids=["-".join(map(str, c[:4])) + ("-narrow" if c[4] else "") for c in _PARITY])
def test_one_slice_transition_parity(P, lik, n, d, pi, slice_kw):
    """every replica's transition from its own RNG words against oracle.MixedSliceSampler on the restatement's cached-predictor call-back:
    the same draws in the same order (final RNG words equal), every Bool coordinate equal, the Float64 ones within RTOL, the explorer
    recorders equal (the Bool method records nothing); the reference chain's i.i.d. draw: d thetas, then d Bools.  The last two cases run
    with the doubling cut short at p = 3"""
    X, y = _data(n, d, lik, seed=7 * n + d)
    N, prec = 10, 0.5
    pt = _pt(P, X, y, lik, prec, N, pi=pi, slice_kw=slice_kw)
    betas, x, chain, rng = _random_states(pt, N, d, seed=n, scale=1.0)
    eng = pt.replicas
    eng.explore(1)
    x1, c1, r1 = eng.states()
    eng.reduce()
    am, an, ss, sn = eng.explorer_stats()
    assert np.array_equal(c1, chain)
    vs = R.VarSel(X, y, lik, 1.0, prec, pi)
    kinds = np.array([O.COORD_FLOAT64] * d + [O.COORD_BOOL] * d, dtype=np.int32)
    flipped = 0
    for i in range(N):
        c = int(chain[i])
        r = O.OracleRng(state=(int(rng[i, 0]), int(rng[i, 1])))
        if c == 0:                                # sample_iid! at the reference: randn / sqrt(p) per theta, then rand(rng, Bool) per indicator
            yv = np.array([r.randn() / math.sqrt(prec) for _ in range(d)] + [float(r.rand_bool()) for _ in range(d)])
            assert an[c] == 0 and sn[c] == 0
        else:
            s = O.MixedSliceSampler(R.VarSelChain(vs, betas[c], prec).path_lp, kinds, **slice_kw)
            yv = x[i].copy()
            s.step(r, yv)
            assert an[c] == s.stats.acc_n and sn[c] == s.stats.steps_n and ss[c] == s.stats.steps_sum, (i, c)
            np.testing.assert_allclose(am[c], s.stats.acc_mean, rtol=RTOL)
            flipped += int(np.sum(yv[d:] != x[i, d:]))
        assert int(r1[i, 0]) == r.state[0] and int(r1[i, 1]) == r.state[1], (i, c)
        assert np.array_equal(x1[i, d:], yv[d:]), (i, c, x1[i, d:], yv[d:])
        np.testing.assert_allclose(x1[i, :d], yv[:d], rtol=RTOL, atol=1e-12, err_msg="replica %d chain %d" % (i, c))
    assert flipped > 0


def test_the_shrink_cap_is_an_error_with_the_coordinate(P):
    """slice_shrink!'s "Maximum number of iterations reached" (SliceSampler.jl:179-185): w = 1000 with max_iter = 2.  The oracle on the same
    streams ends in its own error in every chain but the reference; the engine reports a tempered chain and one of the thetas (the Bool
    method has no cap)"""
    n, d, N, prec = 50, 3, 8, 0.5
    slice_kw = dict(w=1000.0, max_iter=2)
    X, y = _data(n, d, "bernoulli_logit", seed=7 * n + d)
    pt = _pt(P, X, y, "bernoulli_logit", prec, N, slice_kw=slice_kw)
    betas, x, chain, rng = _random_states(pt, N, d, seed=n, scale=1.0)
    vs = R.VarSel(X, y, "bernoulli_logit", 1.0, prec, 0.5)
    kinds = np.array([O.COORD_FLOAT64] * d + [O.COORD_BOOL] * d, dtype=np.int32)
    for i in range(N):
        c = int(chain[i])
        if c != 0:
            s = O.MixedSliceSampler(R.VarSelChain(vs, betas[c], prec).path_lp, kinds, **slice_kw)
            with pytest.raises(RuntimeError, match="maximum number of iterations"):
                s.step(O.OracleRng(state=(int(rng[i, 0]), int(rng[i, 1]))), x[i].copy())
    eng = pt.replicas
    with pytest.raises(P.PteError, match=r"Maximum number of iterations reached in slice_shrink! \(chain [1-7], index [0-2]\)"):
        eng.explore(1)
        eng.reduce()


# ---- whole runs ------------------------------------------------------------------------------------------------------------------------
def _run(P, target, prec, seed, n_rounds):
    return G.run_rounds(P, target, prec, seed, n_rounds, P.SliceSampler(), n_chains=16, ref_dim=target.n_columns,
                        record=["round_trip", "online", "traces", "log_sum_ratio", "index_process"])


_RUN = dict(d=4, n=30, prec=1.0, sd=1.0, pi=0.5, n_rounds=10, seeds=(1, 2, 3), B=32)


def _run_data():
    """n = 30 observations of d = 4 standard-normal columns, two of them active (coefficients 0.6 and -0.5), unit noise"""
    g = np.random.default_rng(42)
    X = g.normal(0.0, 1.0, (_RUN["n"], _RUN["d"]))
    y = X @ np.array([0.6, -0.5, 0.0, 0.0]) + _RUN["sd"] * g.normal(size=_RUN["n"])
    return X, y


@pytest.fixture(scope="module")
def runs(P):
    X, y = _run_data()
    t = P.SpikeSlabRegression(X, y, likelihood="normal_identity", noise_sd=_RUN["sd"], inclusion_prob=_RUN["pi"])
    return {seed: _run(P, t, _RUN["prec"], seed, _RUN["n_rounds"])[0] for seed in _RUN["seeds"]}, t


def _exact():
    X, y = _run_data()
    return R.VarSel(X, y, "normal_identity", _RUN["sd"], _RUN["prec"], _RUN["pi"])


def test_the_data_can_tell_the_posterior_from_the_prior():
    """from the reference alone: an inclusion probability of the exact enumeration is more than 8 standard errors from the prior's pi, with
    the standard error of an indicator's mean over the last round's 2^10 scans taken at a quarter of their number as effective sample size
    (sqrt(q (1 - q) / 256)) -- so a sampler that ignored the data would fail the test below"""
    incl, b, _ = _exact().exact()
    T_eff = 2 ** _RUN["n_rounds"] / 4.0
    se = np.sqrt(incl * (1.0 - incl) / T_eff)
    assert np.max(np.abs(incl - _RUN["pi"]) / se) > 8.0, (incl, se)
    assert np.all((incl > 0.1) & (incl < 0.9)), incl          # no indicator is frozen: the batch-means errors below are not degenerate
    assert np.sum(np.abs(b) > 0.3) == 2, b                       # the two active columns


@pytest.mark.parametrize("seed", _RUN["seeds"])
def test_run_against_the_exact_inclusion_probabilities_and_coefficients(P, runs, seed):
    """16 chains, SliceSampler, 10 rounds.  The target chain's `online` means of the gamma coordinates against the exact posterior inclusion
    probabilities, and the means of theta_j gamma_j over the last round's trace against the exact E[b_j]; each within 5 Monte Carlo standard
    errors, the error by batch means over B = 32 batches of the last round's target-chain trace.  (Measured on an MI355X, in standard
    errors: DESIGN 4.12.)"""
    pts, _ = runs
    pt = pts[seed]
    d, B = _RUN["d"], _RUN["B"]
    incl, b, _ = _exact().exact()
    m, v, cnt = pt.reduced_recorders.online
    assert cnt == 2 ** _RUN["n_rounds"]
    tr = pt.reduced_recorders.traces[:, -1, :2 * d]                 # the target chain
    assert tr.shape[0] == cnt and set(np.unique(tr[:, d:])) <= {0.0, 1.0}
    gb = G.batches(tr[:, d:], B)
    se_g = gb.mean(axis=1).std(axis=0, ddof=1) / math.sqrt(B)
    dev_g = (np.asarray(m)[d:2 * d] - incl) / se_g
    bb = G.batches(tr[:, :d] * tr[:, d:], B)
    se_b = bb.mean(axis=1).std(axis=0, ddof=1) / math.sqrt(B)
    dev_b = ((tr[:, :d] * tr[:, d:]).mean(axis=0) - b) / se_b
    print("seed %d: inclusion deviations / se %s, coefficient deviations / se %s" % (seed, np.round(dev_g, 2), np.round(dev_b, 2)))
    np.testing.assert_allclose(np.asarray(m)[d:2 * d], tr[:, d:].mean(axis=0), rtol=1e-12)      # online and traces record the same samples
    assert np.all(np.abs(dev_g) < 5.0), (np.asarray(m)[d:2 * d], incl, se_g)
    assert np.all(np.abs(dev_b) < 5.0), ((tr[:, :d] * tr[:, d:]).mean(axis=0), b, se_b)
    assert P.n_round_trips(pt) > 0


def test_runs_against_the_exact_evidence(P, runs):
    """stepping_stone - evidence_offset of the three seeds against the exact log evidence of the 2^4 models: the mean within 5 standard
    errors, the standard error from the spread over the seeds"""
    pts, t = runs
    vs = _exact()
    _, _, log_ev = vs.exact()
    assert math.isclose(t.evidence_offset(_RUN["prec"]), vs.evidence_offset(), rel_tol=1e-15)
    est = np.array([P.stepping_stone(pts[s]) - t.evidence_offset(_RUN["prec"]) for s in _RUN["seeds"]])
    se = est.std(ddof=1) / math.sqrt(len(est))
    print("log evidence: estimates %s, exact %.4f, deviation / se %.2f" % (np.round(est, 4), log_ev, (est.mean() - log_ev) / se))
    assert abs(est.mean() - log_ev) < 5.0 * se, (est, log_ev, se)


def _inputs(P, seed=1, n_rounds=5, checkpoint=False):
    X, y = _data(80, 6, "bernoulli_logit", seed=23)
    return P.Inputs(target=P.SpikeSlabRegression(X, y, inclusion_prob=0.4), reference=P.ScaledPrecisionNormalLogPotential(0.5, 6),
                    n_chains=12, n_rounds=n_rounds, seed=seed, explorer=P.SliceSampler(), checkpoint=checkpoint,
                    record=[P.round_trip, P.traces, P.log_sum_ratio, P.index_process, P.swap_acceptance_pr, P.energy_ac1], show_report=False)


def test_two_runs_are_equal_bit_for_bit(P):
    a = G.assert_two_runs_equal(P, lambda: _inputs(P, seed=3))
    assert np.all(np.isfinite(a.reduced_recorders.traces)) and len(np.unique(a.reduced_recorders.traces[:, 6:12])) == 2


def test_sharded_equals_single_engine(P):
    G.assert_sharded_equals_single(P, lambda: G.with_recorders(P, _inputs(P, seed=4, n_rounds=4), "online"), n_shards=2)


def test_checkpoint_resume_equals_uninterrupted(P, tmp_path):
    G.assert_checkpoint_resume(P, lambda **kw: _inputs(P, seed=5, **kw), tmp_path)


def test_new_data_replaces_the_old(P):
    """set_target_varsel again (another n, another noise, another pi on the same engine): the swap statistics are refreshed at once, and the
    log densities of the next step are the new data's"""
    d, N, prec = 7, 8, 0.5
    X1, y1 = _data(90, d, "normal_identity", seed=31)
    pt = _pt(P, X1, y1, "normal_identity", prec, N, n_passes=1, record=[P.traces], extended_traces=True)
    betas, _, _, _ = _random_states(pt, N, d, seed=3, scale=0.5)
    X2, y2 = _data(200, d, "normal_identity", seed=32, noise_sd=2.0)
    pt.replicas.set_target_varsel(P._lib.GLM_NORMAL_IDENTITY, X2, y2, 2.0, 0.25)
    tr = G.log_densities(pt, N, 2 * d)
    new, old = R.VarSel(X2, y2, "normal_identity", 2.0, prec, 0.25), R.VarSel(X1, y1, "normal_identity", 1.0, prec, 0.5)
    G.assert_log_density_at_every_beta(tr, betas, 2 * d, lambda beta: R.VarSelChain(new, beta, prec).lp_full, LP_RTOL, abs_tol=1e-11)
    G.assert_log_density_is_not(tr, betas, 2 * d, lambda beta: R.VarSelChain(old, beta, prec).lp_full)
