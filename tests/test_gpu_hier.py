"""The hierarchical normal-means family on the device (k_explore_hier, pigeons.jl_amd/csrc/pte_hier.hpp) against its NumPy restatement
(tests/hier_ref.py): the log density at every chain's beta, one SliceSampler and one MALA transition of every replica from random states,
whole runs on the eight-schools data against the quadrature's posterior means and evidence, determinism, Compose, the chain-sharded engine,
checkpoint / resume and replacing the data.

The shared checks and their tolerances (RTOL, LP_RTOL, and why) are in tests/family_gpu.py."""
import numpy as np
import pytest

import family_gpu as G
import hier_ref as R
from family_gpu import LP_RTOL, P  # noqa: F401  (P: the module's fixture)

pytestmark = pytest.mark.gpu

SCHOOLS_Y = (28.0, 8.0, -3.0, 7.0, -1.0, 1.0, 18.0, 12.0)
SCHOOLS_SIGMA = (15.0, 10.0, 16.0, 11.0, 9.0, 11.0, 10.0, 18.0)
PARAM = {"c": "centered", "nc": "noncentered"}


def _data(J, seed=1):
    """group effects theta ~ N(0.5, 1), standard errors in 0.5..2, y drawn from the model"""
    g = np.random.default_rng(seed)
    sigma = g.uniform(0.5, 2.0, J)
    return 0.5 + g.normal(0.0, 1.0, J) + sigma * g.normal(0.0, 1.0, J), sigma


def _pt(P, y, sigma, param, prec, N, explorer, mu_sd=2.0, tau_scale=1.5, **kw):
    t = P.HierarchicalNormalMeans(y, sigma, mu_sd=mu_sd, tau_scale=tau_scale, parameterization=PARAM.get(param, param))
    return P.PT(P.Inputs(target=t, reference=P.ScaledPrecisionNormalLogPotential(prec, t.dim), n_chains=N, n_rounds=2, explorer=explorer,
                         show_report=False, **kw))


def test_state_calls_need_the_data_and_the_setter_validates(P):
    L = P._lib
    eng = P.Engine(n_chains=4, target=L.TARGET_HIERARCHICAL_NORMAL, dim=5, explorer=L.EXPLORER_SLICE, target_params=[1.0])
    for call in (lambda: eng.explore(1), lambda: eng.swap(1), lambda: eng.run_scans(1, 2), lambda: eng.states()):
        with pytest.raises(P.PteError, match="the hierarchical-normal target has no data yet; call pte_set_target_hier first"):
            call()
    y, s = np.array([1.0, -2.0, 0.5]), np.array([1.0, 2.0, 0.5])
    cases = [
        ((2, y, s, 5.0, 5.0), r"parameterization must be PTE_HIER_CENTERED \(0\) or PTE_HIER_NONCENTERED \(1\) \(got 2\)"),
        ((0, y[:2], s[:2], 5.0, 5.0), r"n_groups must be dim - 2 = 3 \(got 2\)"),
        ((0, np.zeros(4), np.ones(4), 5.0, 5.0), r"n_groups must be dim - 2 = 3 \(got 4\)"),
        ((0, np.where(np.arange(3) == 1, np.nan, y), s, 5.0, 5.0), r"y\[1\] must be finite"),
        ((0, np.where(np.arange(3) == 2, np.inf, y), s, 5.0, 5.0), r"y\[2\] must be finite"),
        ((1, y, np.where(np.arange(3) == 0, 0.0, s), 5.0, 5.0), r"sigma\[0\] must be positive and finite \(got 0\)"),
        ((1, y, np.where(np.arange(3) == 2, -1.0, s), 5.0, 5.0), r"sigma\[2\] must be positive and finite \(got -1\)"),
        ((1, y, np.where(np.arange(3) == 1, np.inf, s), 5.0, 5.0), r"sigma\[1\] must be positive and finite \(got inf\)"),
        ((0, y, s, 0.0, 5.0), r"mu_sd must be positive and finite \(got 0\)"),
        ((0, y, s, np.nan, 5.0), r"mu_sd must be positive and finite \(got nan\)"),
        ((0, y, s, 5.0, -3.0), r"tau_scale must be positive and finite \(got -3\)"),
        ((0, y, s, 5.0, np.inf), r"tau_scale must be positive and finite \(got inf\)"),
    ]
    for args, msg in cases:
        with pytest.raises(P.PteError, match=msg):
            eng.set_target_hier(*args)
    with pytest.raises(P.PteError, match="null argument"):
        eng._chk(eng.L.pte_set_target_hier(eng.h, 0, 3, None, None, 5.0, 5.0))
    with pytest.raises(P.PteError, match="has no data yet"):          # a refused call left the engine as it was
        eng.explore(1)
    funnel = P.Engine(n_chains=4, target=L.TARGET_FUNNEL, dim=5, explorer=L.EXPLORER_SLICE, target_params=[1.0])
    with pytest.raises(P.PteError, match="pte_set_target_hier: this engine's target is 2, not PTE_TARGET_HIERARCHICAL_NORMAL"):
        funnel.set_target_hier(0, y, s, 5.0, 5.0)
    eng.set_target_hier(0, y, s, 5.0, 5.0)
    eng.explore(1)
    assert eng.states()[0].shape == (4, 5) and eng.kernel_name() == "k_explore_hier" and eng.scan_loop_name() == ""


@pytest.mark.parametrize("J,param", [(1, "c"), (62, "c"), (63, "nc"), (130, "c"), (510, "nc")])
def test_log_density_at_every_beta(P, J, param):
    """the device's log density (extended traces of one explore step) against the restatement at the state the step left, every chain's
    beta: d = 3; 64 (one whole block); 65 (two blocks, ragged); 132 (four, ragged: the data re-read from L2); 512 (eight whole blocks)"""
    y, s = _data(J, seed=J)
    N, prec, d = 8, 0.5, J + 2
    pt = _pt(P, y, s, param, prec, N, P.SliceSampler(n_passes=1), record=[P.traces], extended_traces=True)
    betas, _, _, _ = G.random_states(pt, N, d, seed=d, scale=1.5)
    tr = G.log_densities(pt, N, d)
    hier = R.Hier(y, s, 2.0, 1.5, PARAM[param])
    G.assert_log_density_at_every_beta(tr, betas, d, lambda beta: R.HierChain(hier, beta, prec).path_lp, LP_RTOL, abs_tol=1e-11)


@pytest.mark.parametrize("J,param,w,p", [(3, "c", 10.0, 20), (8, "nc", 10.0, 20), (66, "c", 10.0, 20), (8, "c", 0.25, 3)])
def test_one_slice_transition_parity(P, J, param, w, p):
    """(w = 0.25, p = 3: the doubling stops at its cap, the slice is wider than the interval)"""
    y, s = _data(J, seed=7 * J)
    N, prec, d = 10, 0.5, J + 2
    pt = _pt(P, y, s, param, prec, N, P.SliceSampler(w=w, p=p))
    betas, x, chain, rng = G.random_states(pt, N, d, seed=J, scale=1.0)
    hier = R.Hier(y, s, 2.0, 1.5, PARAM[param])
    G.assert_slice_transition(pt.replicas, betas, x, chain, rng, lambda beta: R.HierChain(hier, beta, prec).path_lp, w=w, p=p)


@pytest.mark.parametrize("J,param,precond", [(4, "c", "mix"), (8, "nc", "diagonal"), (62, "c", "identity")])
def test_one_mala_transition_parity(P, J, param, precond):
    """(J = 62: d = 64, the whole-block instantiation)"""
    y, s = _data(J, seed=3 * J)
    N, step, prec, d = 10, 0.2, 1.0, J + 2               # (at this step the chains accept some proposals and reject others)
    ex = G.mala_explorer(P, step, precond)
    pt = _pt(P, y, s, param, prec, N, ex)
    betas, x, chain, rng = G.random_states(pt, N, d, seed=d, scale=0.5)
    hier = R.Hier(y, s, 2.0, 1.5, PARAM[param])
    G.assert_mala_transition(pt.replicas, ex, precond, betas, x, chain, rng, lambda beta: R.HierChain(hier, beta, prec),
                             std_range=(0.5, 2.0), form="whole")


# ---- whole runs ------------------------------------------------------------------------------------------------------------------------
def _run(P, target, prec, seed, n_rounds, explorer):
    return G.run_rounds(P, target, prec, seed, n_rounds, explorer, n_chains=16,
                        record=["round_trip", "online", "traces", "log_sum_ratio", "index_process"])


def _target_minus_reference(hier, X, prec):
    """(target - reference)(x) of every state of X [..., d] (plain sums: this feeds an error estimate, not a parity check)"""
    mu, lt, xg = X[..., 0], X[..., 1], X[..., 2:]
    th = hier.theta(X)
    z = (hier.y - th) * hier.isig
    lp = -(mu * hier.imu) ** 2 / 2.0 - R.LOG2PI / 2.0 - hier.lmu + hier.c_tau - np.log1p((np.exp(lt) * hier.its) ** 2) + lt
    lp = lp + (-(z * z + R.LOG2PI) / 2.0 - hier.lsig).sum(-1)
    if hier.param == R.CENTERED:
        u = (xg - mu[..., None]) * np.exp(-lt)[..., None]
        lp = lp + (-(u * u + R.LOG2PI) / 2.0).sum(-1) - hier.J * lt
    else:
        lp = lp + (-(xg * xg + R.LOG2PI) / 2.0).sum(-1)
    return lp + 0.5 * prec * (X * X).sum(-1)


def _stepping_stone_se(tr, betas, hier, prec):
    return G.stepping_stone_se(_target_minus_reference(hier, tr[:, :, :hier.d], prec), betas)


@pytest.fixture(scope="module")
def schools_truth():
    """the quadrature, computed once: (posterior means, posterior sds, log evidence)"""
    hier = R.Hier(SCHOOLS_Y, SCHOOLS_SIGMA, 5.0, 5.0)
    return hier.posterior_means(), hier.posterior_sds(), hier.log_evidence()


@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("param", ["centered", "noncentered"])
def test_eight_schools_run_against_the_quadrature(P, schools_truth, param, seed):
    """Eight schools, p = 1/9, 16 chains, 10 rounds, AutoMALA.  The target chain's means of mu, log tau and theta_j (reconstructed per sample
    in the non-centred form) over the last round's 1024 scans within 5 batch-means standard errors (B = 16) of the quadrature, and
    stepping_stone - evidence_offset within 5 standard errors (_stepping_stone_se) of the quadrature's log evidence, -31.3113.  Five standard
    errors: a false failure has probability below 1e-3 over all comparisons even with se estimated from 8-16 batches (t tails), the argument
    of tests/test_gpu_glm.py.  So that wide error bars cannot pass, every standard error of a mean must also be below a quarter of the
    quadrature's posterior sd of its quantity (an effective sample size of at least 16)."""
    want, sd, log_z = schools_truth
    prec, d = 1.0 / 9.0, 10
    t = P.HierarchicalNormalMeans(SCHOOLS_Y, SCHOOLS_SIGMA, mu_sd=5.0, tau_scale=5.0, parameterization=param)
    pt, grids = _run(P, t, prec, seed, 10, P.AutoMALA())
    hier = R.Hier(SCHOOLS_Y, SCHOOLS_SIGMA, 5.0, 5.0, param)
    tr_all = pt.reduced_recorders.traces                          # [scan][chain][d + 1]
    assert tr_all.shape[0] == 1024
    x = tr_all[:, -1, :d]                                         # the target chain
    q = np.concatenate([x[:, :2], hier.theta(x)], axis=1)
    se = G.batches(q, 16).mean(axis=1).std(axis=0, ddof=1) / 4.0
    z = np.abs(q.mean(axis=0) - want) / se
    se_ss = _stepping_stone_se(tr_all, grids, hier, prec)
    est = P.stepping_stone(pt) - t.evidence_offset(prec)
    print("eight schools %s seed %d: max |z| %.2f, max se / sd %.3f, log evidence %.4f (exact %.4f, se %.4f, |z| %.2f)"
          % (param, seed, z.max(), (se / sd).max(), est, log_z, se_ss, abs(est - log_z) / se_ss))
    assert np.all(z < 5.0), (z, q.mean(axis=0), want, se)
    assert np.all(se < 0.25 * sd), se / sd
    assert abs(est - log_z) < 5 * se_ss, (est, log_z, se_ss)
    assert P.n_round_trips(pt) > 0


def _inputs(P, seed=1, explorer=None, n_rounds=5, checkpoint=False, param="noncentered"):
    y, s = _data(9, seed=23)
    return P.Inputs(target=P.HierarchicalNormalMeans(y, s, mu_sd=2.0, tau_scale=1.5, parameterization=param),
                    reference=P.ScaledPrecisionNormalLogPotential(0.5, 11), n_chains=12, n_rounds=n_rounds,
                    seed=seed, explorer=explorer or P.SliceSampler(), checkpoint=checkpoint,
                    record=[P.round_trip, P.traces, P.log_sum_ratio, P.index_process, P.swap_acceptance_pr, P.energy_ac1], show_report=False)


def test_two_runs_are_equal_bit_for_bit(P):
    G.assert_two_runs_equal(P, lambda: _inputs(P, seed=3, explorer=P.AutoMALA(), param="centered"))


def test_compose_slice_automala_runs(P):
    pt = G.assert_compose_runs(P, _inputs(P, seed=2, explorer=P.Compose(P.SliceSampler(), P.AutoMALA())), "k_explore_hier")
    assert P.n_round_trips(pt) > 0


@pytest.mark.parametrize("explorer", ["slice", "automala"])
def test_sharded_equals_single_engine(P, explorer):
    mk = lambda: G.with_recorders(P, _inputs(P, seed=4, n_rounds=4, explorer=P.SliceSampler() if explorer == "slice" else P.AutoMALA()), "online")
    G.assert_sharded_equals_single(P, mk, n_shards=2)


def test_checkpoint_resume_equals_uninterrupted(P, tmp_path):
    G.assert_checkpoint_resume(P, lambda **kw: _inputs(P, seed=5, explorer=P.MALA(step_size=0.2), **kw), tmp_path)


def test_new_data_replaces_the_old(P):
    """set_target_hier again (other estimates, the other parameterisation, other hyper-parameters): the swap statistics are refreshed at once,
    and the log densities of the next step are the new data's"""
    J, N, prec = 7, 8, 0.5
    d = J + 2
    y1, s1 = _data(J, seed=31)
    pt = _pt(P, y1, s1, "c", prec, N, P.SliceSampler(n_passes=1), record=[P.traces], extended_traces=True)
    betas, _, _, _ = G.random_states(pt, N, d, seed=3, scale=0.5)
    y2, s2 = _data(J, seed=32)
    pt.replicas.set_target_hier(P._lib.HIER_NONCENTERED, y2, s2, 3.0, 0.8)
    tr = G.log_densities(pt, N, d)
    new, old = R.Hier(y2, s2, 3.0, 0.8, "noncentered"), R.Hier(y1, s1, 2.0, 1.5, "centered")
    G.assert_log_density_at_every_beta(tr, betas, d, lambda beta: R.HierChain(new, beta, prec).path_lp, LP_RTOL, abs_tol=1e-11)
    G.assert_log_density_is_not(tr, betas, d, lambda beta: R.HierChain(old, beta, prec).path_lp)
