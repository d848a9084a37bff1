"""The Bayesian-GLM family on the device (k_explore_glm, pigeons.jl_amd/csrc/pte_glm.hpp) against its NumPy restatement (tests/glm_ref.py):
the log density at every chain's beta, one SliceSampler and one MALA transition of every replica from random states, whole runs against the
exact posterior and evidence of the conjugate normal-identity model and a quadrature evidence of a logistic one, determinism, Compose, the
chain-sharded engine, checkpoint / resume and replacing the data.

RNG words are compared exactly; states and recorders to 1e-9 relative, log densities to 1e-11 relative -- the device's exp / log1p differ
from libm by an ulp, and its fused multiply-adds from the restatement's twice-rounded ones in rare ties."""
import math

import numpy as np
import pytest

import aaps_ref as A
import glm_ref as R
import mixture_ref as M
import oracle as O

pytestmark = pytest.mark.gpu

RTOL = 1e-9
LP_RTOL = 1e-11


@pytest.fixture(scope="module")
def P():
    import pigeons_amd
    return pigeons_amd


def _data(n, d, lik, seed=1, noise_sd=1.0):
    """X with entries N(0, 1 / d) (eta of order |theta|), y drawn from the model at theta ~ N(0, I)"""
    g = np.random.default_rng(seed)
    X = g.normal(0.0, 1.0 / math.sqrt(d), (n, d))
    eta = X @ g.normal(0.0, 1.0, d)
    y = (g.uniform(size=n) < 1 / (1 + np.exp(-eta))).astype(float) if lik == "bernoulli_logit" else eta + noise_sd * g.normal(size=n)
    return X, y


def _random_states(pt, N, d, seed, scale=1.5):
    eng = pt.replicas
    g = np.random.default_rng(seed)
    betas = np.concatenate([[0.0], np.sort(g.uniform(0.0, 1.0, N - 2)), [1.0]])
    eng.set_schedule(betas)
    x = g.normal(0.0, scale, (N, d))
    chain = g.permutation(N).astype(np.int64)
    _, _, rng = eng.states()
    eng.set_states(x, chain, rng)
    return betas, x, chain, rng


def _log_densities(P, pt, N, d):
    eng = pt.replicas
    eng.explore(1)
    eng.swap(1)                                   # (a scan ends at its swap: the traces count it from there)
    eng.reduce()
    tr = eng.traces()
    assert tr.shape == (1, N, d + 1)
    return tr[0]


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
    betas, _, _, _ = _random_states(pt, N, d, seed=d, scale=0.5)
    tr = _log_densities(P, pt, N, d)
    glm = R.Glm(X, y, lik, 0.8, prec)
    for c in range(N):
        want = R.GlmChain(glm, betas[c], prec).path_lp(tr[c, :d])
        assert math.isclose(tr[c, d], want, rel_tol=LP_RTOL, abs_tol=1e-11), (c, betas[c], tr[c, d], want)


@pytest.mark.parametrize("lik,n,d", [("bernoulli_logit", 50, 3), ("normal_identity", 70, 5), ("bernoulli_logit", 130, 66)])
def test_one_slice_transition_parity(P, lik, n, d):
    X, y = _data(n, d, lik, seed=7 * n + d)
    N, prec = 10, 0.5
    pt = P.PT(P.Inputs(target=P.BayesianGLM(X, y, likelihood=lik), reference=P.ScaledPrecisionNormalLogPotential(prec, d), n_chains=N,
                       n_rounds=2, explorer=P.SliceSampler(), show_report=False))
    betas, x, chain, rng = _random_states(pt, N, d, seed=n, scale=1.0)
    eng = pt.replicas
    eng.explore(1)
    x1, c1, r1 = eng.states()
    eng.reduce()
    am, an, ss, sn = eng.explorer_stats()
    assert np.array_equal(c1, chain)
    glm = R.Glm(X, y, lik, 1.0, prec)
    for i in range(N):
        c = int(chain[i])
        if c == 0:
            continue
        r = O.OracleRng(state=(int(rng[i, 0]), int(rng[i, 1])))
        s = O.MixedSliceSampler(R.GlmChain(glm, betas[c], prec).path_lp, np.zeros(d, dtype=np.int32))
        yv = x[i].copy()
        s.step(r, yv)
        assert int(r1[i, 0]) == r.state[0] and int(r1[i, 1]) == r.state[1], (i, c)
        np.testing.assert_allclose(x1[i], yv, rtol=RTOL, atol=1e-12, err_msg="replica %d chain %d" % (i, c))
        assert an[c] == s.stats.acc_n and sn[c] == s.stats.steps_n and ss[c] == s.stats.steps_sum, (i, c)
        np.testing.assert_allclose(am[c], s.stats.acc_mean, rtol=RTOL)


@pytest.mark.parametrize("lik,n,d,precond", [("bernoulli_logit", 40, 6, "mix"), ("normal_identity", 64, 10, "diagonal"),
                                             ("bernoulli_logit", 100, 64, "identity"), ("normal_identity", 90, 70, "mix")])
def test_one_mala_transition_parity(P, lik, n, d, precond):
    mode, pc = {"identity": (0, P.IdentityPreconditioner()), "diagonal": (1, P.DiagonalPreconditioner()),
                "mix": (2, P.MixDiagonalPreconditioner())}[precond]
    X, y = _data(n, d, lik, seed=3 * n + d)
    N, step, prec = 10, 0.1, 1.0
    ex = P.MALA(step_size=step, preconditioner=pc)
    pt = P.PT(P.Inputs(target=P.BayesianGLM(X, y, likelihood=lik), reference=P.ScaledPrecisionNormalLogPotential(prec, d), n_chains=N,
                       n_rounds=2, explorer=ex, show_report=False))
    betas, x, chain, rng = _random_states(pt, N, d, seed=d, scale=0.5)
    eng = pt.replicas
    std = np.random.default_rng(d).uniform(0.5, 2.0, d)
    eng.set_explorer_adaptation(step, std)
    eng.explore(2)
    x1, c1, r1 = eng.states()
    eng.reduce()
    am, an, ss, sn = eng.explorer_stats()
    n_refresh = ex.base_n_refresh * int(math.ceil(d ** ex.exponent_n_refresh))
    glm = R.Glm(X, y, lik, 1.0, prec)
    moved = 0
    for i in range(N):
        c = int(chain[i])
        if c == 0:
            continue
        r = O.OracleRng(state=(int(rng[i, 0]), int(rng[i, 1])))
        Mv = A.build_preconditioner(r, d, mode, 1.0 / 3.0, 1.0 / 3.0, std)
        res = M.mala_transition(x[i], r, R.GlmChain(glm, betas[c], prec), step, n_refresh, Mv)
        assert int(r1[i, 0]) == r.state[0] and int(r1[i, 1]) == r.state[1], (i, c)
        np.testing.assert_allclose(x1[i], res["x"], rtol=RTOL, atol=1e-12, err_msg="replica %d chain %d" % (i, c))
        assert an[c] == res["acc_n"] and sn[c] == n_refresh and ss[c] == res["steps"], (i, c)
        np.testing.assert_allclose(am[c], res["acc_sum"] / res["acc_n"], rtol=RTOL, atol=1e-12)
        moved += int(not np.array_equal(res["x"], x[i]))
    assert moved > 0


# ---- whole runs ------------------------------------------------------------------------------------------------------------------------
def _run(P, glm_target, prec, seed, n_rounds, explorer, checkpoint=False, record=None):
    """pigeons' round loop by hand: the schedule the last round ran with is kept (adapt replaces it after the round)"""
    pt = P.PT(P.Inputs(target=glm_target, reference=P.ScaledPrecisionNormalLogPotential(prec, glm_target.dim), n_chains=16,
                       n_rounds=n_rounds, seed=seed, explorer=explorer, checkpoint=checkpoint, extended_traces=True, show_report=False,
                       record=record or [P.round_trip, P.online, P.traces, P.log_sum_ratio, P.index_process]))
    grids = None
    while P.next_round(pt):
        grids = np.array(pt.shared.tempering.schedule.grids)
        red = P.run_one_round(pt)
        pt = P.adapt(pt, red)
    return pt, grids


def _batches(a, B):
    T = a.shape[0] // B * B
    return a[:T].reshape(B, T // B, *a.shape[1:])


def _stepping_stone_se(tr, betas, glm, B=8):
    """Monte Carlo standard error of stepping_stone by batch means: the last round's scans (extended traces, every chain) in B consecutive
    batches, the estimator -- (forward + backward) / 2 of sum_k log mean_t exp(+-(beta_k+1 - beta_k) (target - reference)(x_t)) -- on each,
    se = sd(batch estimates) / sqrt(B).  (Shorter batches make each estimate noisier, never less: se is not understated.)"""
    X = tr[:, :, :glm.d]
    l, _ = glm.terms(X @ glm.X.T)
    delta = l.sum(-1) + glm.c_prior + glm.c_obs                   # target - reference = log likelihood + the constants
    db = _batches(delta, B)                                       # [B][t][chain]
    dbeta = np.diff(betas)

    def lme(a):
        m = a.max(axis=1, keepdims=True)
        return (m + np.log(np.mean(np.exp(a - m), axis=1, keepdims=True)))[:, 0]
    fw = lme(db[:, :, :-1] * dbeta).sum(-1)
    bw = -lme(-db[:, :, 1:] * dbeta).sum(-1)
    return float(np.std((fw + bw) / 2.0, ddof=1) / math.sqrt(B))


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
    xb = _batches(tr, 16)
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
    a, b = P.pigeons(P.PT(_inputs(P, seed=3, explorer=P.AutoMALA()))), P.pigeons(P.PT(_inputs(P, seed=3, explorer=P.AutoMALA())))
    xa, ca, ga = a.replicas.states(); xb, cb, gb = b.replicas.states()
    assert np.array_equal(xa, xb) and np.array_equal(ca, cb) and np.array_equal(ga, gb)
    assert np.array_equal(a.reduced_recorders.traces, b.reduced_recorders.traces)
    assert np.array_equal(a.shared.tempering.schedule.grids, b.shared.tempering.schedule.grids)
    assert P.stepping_stone(a) == P.stepping_stone(b)


def test_compose_slice_automala_runs(P):
    pt = P.pigeons(P.PT(_inputs(P, seed=2, explorer=P.Compose(P.SliceSampler(), P.AutoMALA()))))
    assert pt.replicas.kernel_name() == "k_explore_glm"
    assert np.all(np.isfinite(pt.reduced_recorders.traces)) and np.isfinite(P.stepping_stone(pt))
    m, n = pt.reduced_recorders.explorer_acceptance_pr
    assert np.all(n[1:] > 0)


@pytest.mark.parametrize("explorer", ["slice", "automala"])
def test_sharded_equals_single_engine(P, explorer):
    mk = lambda: _inputs(P, seed=4, n_rounds=4, explorer=P.SliceSampler() if explorer == "slice" else P.AutoMALA())
    one, many = P.PT(mk()), P.PT(mk(), n_shards=2)
    for _ in range(4):
        assert P.next_round(one) and P.next_round(many)
        ra = P.run_one_round(one); P.adapt(one, ra)
        rb = P.run_one_round(many); P.adapt(many, rb)
        assert np.array_equal(ra.index_process, rb.index_process) and np.array_equal(ra.traces, rb.traces)
    xa, ca, ga = one.replicas.states(); xb, cb, gb = many.shards.states()
    assert np.array_equal(xa, xb) and np.array_equal(ca, cb) and np.array_equal(ga, gb)


def test_checkpoint_resume_equals_uninterrupted(P, tmp_path):
    straight = P.pigeons(P.PT(_inputs(P, seed=5, n_rounds=6, explorer=P.MALA(step_size=0.2))))
    folder = str(tmp_path / "exec")
    P.pigeons(P.PT(_inputs(P, seed=5, n_rounds=3, explorer=P.MALA(step_size=0.2), checkpoint=True)), exec_folder=folder)
    resumed = P.pigeons(P.load_checkpoint(folder, n_rounds_increment=3))
    ra, rb = straight.reduced_recorders, resumed.reduced_recorders
    assert np.array_equal(ra.index_process, rb.index_process) and np.array_equal(ra.traces, rb.traces)
    assert np.array_equal(straight.shared.tempering.schedule.grids, resumed.shared.tempering.schedule.grids)
    xa, ca, ga = straight.replicas.states(); xb, cb, gb = resumed.replicas.states()
    assert np.array_equal(xa, xb) and np.array_equal(ca, cb) and np.array_equal(ga, gb)


def test_new_data_replaces_the_old(P):
    """set_target_glm again (another n, another likelihood's data on the same engine): the swap statistics are refreshed at once, and the
    log densities of the next step are the new data's"""
    d, N, prec = 7, 8, 0.5
    X1, y1 = _data(90, d, "normal_identity", seed=31)
    pt = P.PT(P.Inputs(target=P.BayesianGLM(X1, y1, likelihood="normal_identity"), reference=P.ScaledPrecisionNormalLogPotential(prec, d),
                       n_chains=N, n_rounds=2, explorer=P.SliceSampler(n_passes=1), record=[P.traces], extended_traces=True, show_report=False))
    betas, _, _, _ = _random_states(pt, N, d, seed=3, scale=0.5)
    X2, y2 = _data(200, d, "normal_identity", seed=32, noise_sd=2.0)
    pt.replicas.set_target_glm(P._lib.GLM_NORMAL_IDENTITY, X2, y2, 2.0)
    tr = _log_densities(P, pt, N, d)
    new, old = R.Glm(X2, y2, "normal_identity", 2.0, prec), R.Glm(X1, y1, "normal_identity", 1.0, prec)
    for c in range(N):
        want = R.GlmChain(new, betas[c], prec).path_lp(tr[c, :d])
        assert math.isclose(tr[c, d], want, rel_tol=LP_RTOL, abs_tol=1e-11), (c, tr[c, d], want)
        if betas[c] > 0:
            assert not math.isclose(tr[c, d], R.GlmChain(old, betas[c], prec).path_lp(tr[c, :d]), rel_tol=1e-6)
