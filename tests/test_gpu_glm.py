"""The Bayesian-GLM family on the device (k_explore_glm, pigeons.jl_amd/csrc/pte_glm.hpp) against its NumPy restatement (tests/glm_ref.py):
the log density at every chain's beta, one SliceSampler and one MALA transition of every replica from random states, whole runs against the
exact posterior and evidence of the conjugate normal-identity model and a quadrature evidence of a logistic one, determinism, Compose, the
chain-sharded engine, checkpoint / resume and replacing the data.

The shared checks and their tolerances (RTOL, LP_RTOL, and why) are in tests/family_gpu.py."""
import math

import numpy as np
import pytest

import family_gpu as G
import glm_ref as R
from family_gpu import LP_RTOL, P  # noqa: F401  (P: the module's fixture)

pytestmark = pytest.mark.gpu


def _data(n, d, lik, seed=1, noise_sd=1.0):
    """X with entries N(0, 1 / d) (eta of order |theta|), y drawn from the model at theta ~ N(0, I)"""
    g = np.random.default_rng(seed)
    X = g.normal(0.0, 1.0 / math.sqrt(d), (n, d))
    eta = X @ g.normal(0.0, 1.0, d)
    y = (g.uniform(size=n) < 1 / (1 + np.exp(-eta))).astype(float) if lik == "bernoulli_logit" else eta + noise_sd * g.normal(size=n)
    return X, y


def test_state_calls_need_the_data_and_the_setter_validates(P):
    L = P._lib
    eng = P.Engine(n_chains=4, target=L.TARGET_BAYESIAN_GLM, dim=3, explorer=L.EXPLORER_SLICE, target_params=[1.0])
    for call in (lambda: eng.explore(1), lambda: eng.swap(1), lambda: eng.run_scans(1, 2), lambda: eng.states()):
        with pytest.raises(P.PteError, match="call pte_set_target_glm first"):
            call()
    X, y = _data(10, 3, "bernoulli_logit")
    cases = [
        ((7, X, y, 1.0), "likelihood must be PTE_GLM_BERNOULLI_LOGIT"),
        ((0, np.zeros((4097, 3)), np.zeros(4097), 1.0), r"1\.\.4096 observations"),
        ((0, np.zeros((0, 3)), np.zeros(0), 1.0), r"1\.\.4096 observations"),
        ((0, np.where(np.arange(30).reshape(10, 3) == 4, np.nan, X), y, 1.0), r"X\[1\]\[1\] must be finite"),
        ((0, X, np.where(np.arange(10) == 2, np.inf, y), 1.0), r"y\[2\] must be finite"),
        ((0, X, np.where(np.arange(10) == 3, 0.5, y), 1.0), r"needs y in \{0, 1\}"),
        ((1, X, y, 0.0), "noise_sd positive and finite"),
        ((1, X, y, np.nan), "noise_sd positive and finite"),
    ]
    for args, msg in cases:
        with pytest.raises(P.PteError, match=msg):
            eng.set_target_glm(*args)
    big = P.Engine(n_chains=4, target=L.TARGET_BAYESIAN_GLM, dim=64, explorer=L.EXPLORER_SLICE, target_params=[1.0])
    with pytest.raises(P.PteError, match=r"n_obs \* dim must be <= 131072"):
        big.set_target_glm(0, np.zeros((2049, 64)), np.zeros(2049), 1.0)
    with pytest.raises(P.PteError, match="null argument"):
        eng._chk(eng.L.pte_set_target_glm(eng.h, 0, 10, None, None, 1.0))
    eng.set_target_glm(0, X, y, 1.0)
    eng.explore(1)
    assert eng.states()[0].shape == (4, 3) and eng.kernel_name() == "k_explore_glm" and eng.scan_loop_name() == ""


@pytest.mark.parametrize("lik,n,d", [("bernoulli_logit", 1, 1), ("bernoulli_logit", 300, 64), ("normal_identity", 100, 5),
                                     ("bernoulli_logit", 4096, 32), ("normal_identity", 256, 512)])
def test_log_density_at_every_beta(P, lik, n, d):
    """the device's log density (extended traces of one explore step) against the restatement at the state the step left, every chain's
    beta: a ragged n and d, the largest n and the largest n d"""
    X, y = _data(n, d, lik, seed=n + d, noise_sd=0.8)
    N, prec = 12, 0.5
    pt = P.PT(P.Inputs(target=P.BayesianGLM(X, y, likelihood=lik, noise_sd=0.8), reference=P.ScaledPrecisionNormalLogPotential(prec, d),
                       n_chains=N, n_rounds=2, explorer=P.SliceSampler(n_passes=1), record=[P.traces], extended_traces=True, show_report=False))
    betas, _, _, _ = G.random_states(pt, N, d, seed=d, scale=0.5)
    tr = G.log_densities(pt, N, d)
    glm = R.Glm(X, y, lik, 0.8, prec)
    G.assert_log_density_at_every_beta(tr, betas, d, lambda beta: R.GlmChain(glm, beta, prec).path_lp, LP_RTOL, abs_tol=1e-11)


@pytest.mark.parametrize("lik,n,d", [("bernoulli_logit", 50, 3), ("normal_identity", 70, 5), ("bernoulli_logit", 130, 66)])
def test_one_slice_transition_parity(P, lik, n, d):
    X, y = _data(n, d, lik, seed=7 * n + d)
    N, prec = 10, 0.5
    pt = P.PT(P.Inputs(target=P.BayesianGLM(X, y, likelihood=lik), reference=P.ScaledPrecisionNormalLogPotential(prec, d), n_chains=N,
                       n_rounds=2, explorer=P.SliceSampler(), show_report=False))
    betas, x, chain, rng = G.random_states(pt, N, d, seed=n, scale=1.0)
    glm = R.Glm(X, y, lik, 1.0, prec)
    G.assert_slice_transition(pt.replicas, betas, x, chain, rng, lambda beta: R.GlmChain(glm, beta, prec).path_lp)


@pytest.mark.parametrize("lik,n,d,precond", [("bernoulli_logit", 40, 6, "mix"), ("normal_identity", 64, 10, "diagonal"),
                                             ("bernoulli_logit", 100, 64, "identity"), ("normal_identity", 90, 70, "mix")])
def test_one_mala_transition_parity(P, lik, n, d, precond):
    X, y = _data(n, d, lik, seed=3 * n + d)
    N, step, prec = 10, 0.1, 1.0
    ex = G.mala_explorer(P, step, precond)
    pt = P.PT(P.Inputs(target=P.BayesianGLM(X, y, likelihood=lik), reference=P.ScaledPrecisionNormalLogPotential(prec, d), n_chains=N,
                       n_rounds=2, explorer=ex, show_report=False))
    betas, x, chain, rng = G.random_states(pt, N, d, seed=d, scale=0.5)
    glm = R.Glm(X, y, lik, 1.0, prec)
    G.assert_mala_transition(pt.replicas, ex, precond, betas, x, chain, rng, lambda beta: R.GlmChain(glm, beta, prec),
                             std_range=(0.5, 2.0), form="whole")


# ---- whole runs ------------------------------------------------------------------------------------------------------------------------
def _run(P, glm_target, prec, seed, n_rounds, explorer):
    return G.run_rounds(P, glm_target, prec, seed, n_rounds, explorer, n_chains=16,
                        record=["round_trip", "online", "traces", "log_sum_ratio", "index_process"])


def _stepping_stone_se(tr, betas, glm):
    """G.stepping_stone_se on this family's target - reference = log likelihood + the constants"""
    l, _ = glm.terms(tr[:, :, :glm.d] @ glm.X.T)
    return G.stepping_stone_se(l.sum(-1) + glm.c_prior + glm.c_obs, betas)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_normal_identity_run_against_the_exact_posterior_and_evidence(P, seed):
    """d = 4, n = 64, 16 chains, AutoMALA, 10 rounds.  Tolerances from the run's own Monte Carlo error (batch means over B = 16 batches of the
    last round's target-chain trace): |mean - m| < 5 se_mean; the online variance is mean((x - m)^2) - (mean - m)^2, so
    |var - v| < 5 se_sq + (5 se_mean)^2 with se_sq the batch-means error of (x - m)^2.  stepping_stone + (d/2) log(2 pi / p) against the exact
    log evidence within 5 se of _stepping_stone_se.  Five standard errors: a false failure has probability below 1e-3 over all 3 x 9
    comparisons even with se estimated from 8-16 batches (t tails)."""
    d, n, prec, sd = 4, 64, 0.5, 0.8
    X, y = _data(n, d, "normal_identity", seed=40 + seed, noise_sd=sd)
    t = P.BayesianGLM(X, y, likelihood="normal_identity", noise_sd=sd)
    pt, grids = _run(P, t, prec, seed, 10, P.AutoMALA())
    glm = R.Glm(X, y, "normal_identity", sd, prec)
    m_exact, cov = glm.posterior()
    v_exact = np.diag(cov)
    m, v, cnt = pt.reduced_recorders.online
    assert cnt > 0
    tr_all = pt.reduced_recorders.traces                          # [scan][chain][d + 1]
    tr = tr_all[:, -1, :d]                                        # the target chain
    xb = G.batches(tr, 16)
    se_mean = xb.mean(axis=1).std(axis=0, ddof=1) / 4.0
    se_sq = ((xb - m_exact) ** 2).mean(axis=1).std(axis=0, ddof=1) / 4.0
    assert np.all(np.abs(np.asarray(m) - m_exact) < 5 * se_mean), (m, m_exact, se_mean)
    assert np.all(np.abs(np.asarray(v) - v_exact) < 5 * se_sq + (5 * se_mean) ** 2), (v, v_exact, se_sq)
    se_ss = _stepping_stone_se(tr_all, grids, glm)
    est = P.stepping_stone(pt) - glm.evidence_offset()
    assert abs(est - glm.log_evidence()) < 5 * se_ss, (est, glm.log_evidence(), se_ss)
    assert P.n_round_trips(pt) > 0


def test_logistic_evidence_against_quadrature(P):
    """d = 2: stepping_stone + (d/2) log(2 pi / p) against log of the integral of prior x likelihood on a 601 x 601 grid (+-10 posterior
    standard deviations around the mode), within 5 Monte Carlo standard errors (_stepping_stone_se)"""
    d, n, prec = 2, 40, 0.5
    X, y = _data(n, d, "bernoulli_logit", seed=17)
    glm = R.Glm(X, y, "bernoulli_logit", 1.0, prec)
    pt, grids = _run(P, P.BayesianGLM(X, y), prec, 4, 10, P.SliceSampler())
    tr = pt.reduced_recorders.traces[:, -1, :d]
    c, s = tr.mean(0), tr.std(0)
    a = np.linspace(c[0] - 10 * s[0], c[0] + 10 * s[0], 601)
    b = np.linspace(c[1] - 10 * s[1], c[1] + 10 * s[1], 601)
    Ag, Bg = np.meshgrid(a, b, indexing="ij")
    T = np.stack([Ag.ravel(), Bg.ravel()], axis=1)
    eta = T @ X.T
    ll = np.sum(y * eta - (np.maximum(eta, 0) + np.log1p(np.exp(-np.abs(eta)))), axis=1)
    logf = ll + (-(d / 2) * np.log(2 * np.pi / prec) - 0.5 * prec * (T ** 2).sum(1))
    mx = logf.max()
    log_z = mx + math.log(np.exp(logf - mx).sum() * (a[1] - a[0]) * (b[1] - b[0]))
    se_ss = _stepping_stone_se(pt.reduced_recorders.traces, grids, glm)
    est = P.stepping_stone(pt) - glm.evidence_offset()
    assert abs(est - log_z) < 5 * se_ss, (est, log_z, se_ss)


def _inputs(P, seed=1, explorer=None, n_rounds=5, checkpoint=False):
    X, y = _data(80, 6, "bernoulli_logit", seed=23)
    return P.Inputs(target=P.BayesianGLM(X, y), reference=P.ScaledPrecisionNormalLogPotential(0.5, 6), n_chains=12, n_rounds=n_rounds,
                    seed=seed, explorer=explorer or P.SliceSampler(), checkpoint=checkpoint,
                    record=[P.round_trip, P.traces, P.log_sum_ratio, P.index_process, P.swap_acceptance_pr, P.energy_ac1], show_report=False)


def test_two_runs_are_equal_bit_for_bit(P):
    G.assert_two_runs_equal(P, lambda: _inputs(P, seed=3, explorer=P.AutoMALA()))


def test_compose_slice_automala_runs(P):
    G.assert_compose_runs(P, _inputs(P, seed=2, explorer=P.Compose(P.SliceSampler(), P.AutoMALA())), "k_explore_glm")


@pytest.mark.parametrize("explorer", ["slice", "automala"])
def test_sharded_equals_single_engine(P, explorer):
    mk = lambda: G.with_recorders(P, _inputs(P, seed=4, n_rounds=4, explorer=P.SliceSampler() if explorer == "slice" else P.AutoMALA()), "online")
    G.assert_sharded_equals_single(P, mk, n_shards=2)


def test_checkpoint_resume_equals_uninterrupted(P, tmp_path):
    G.assert_checkpoint_resume(P, lambda **kw: _inputs(P, seed=5, explorer=P.MALA(step_size=0.2), **kw), tmp_path)


def test_new_data_replaces_the_old(P):
    """set_target_glm again (another n, another likelihood's data on the same engine): the swap statistics are refreshed at once, and the
    log densities of the next step are the new data's"""
    d, N, prec = 7, 8, 0.5
    X1, y1 = _data(90, d, "normal_identity", seed=31)
    pt = P.PT(P.Inputs(target=P.BayesianGLM(X1, y1, likelihood="normal_identity"), reference=P.ScaledPrecisionNormalLogPotential(prec, d),
                       n_chains=N, n_rounds=2, explorer=P.SliceSampler(n_passes=1), record=[P.traces], extended_traces=True, show_report=False))
    betas, _, _, _ = G.random_states(pt, N, d, seed=3, scale=0.5)
    X2, y2 = _data(200, d, "normal_identity", seed=32, noise_sd=2.0)
    pt.replicas.set_target_glm(P._lib.GLM_NORMAL_IDENTITY, X2, y2, 2.0)
    tr = G.log_densities(pt, N, d)
    new, old = R.Glm(X2, y2, "normal_identity", 2.0, prec), R.Glm(X1, y1, "normal_identity", 1.0, prec)
    G.assert_log_density_at_every_beta(tr, betas, d, lambda beta: R.GlmChain(new, beta, prec).path_lp, LP_RTOL, abs_tol=1e-11)
    G.assert_log_density_is_not(tr, betas, d, lambda beta: R.GlmChain(old, beta, prec).path_lp)
