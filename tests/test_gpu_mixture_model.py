"""The mixture-model-posterior family on the device (k_explore_mixture_model, pigeons.jl_amd/csrc/pte_mixture_model.hpp) against its NumPy
restatement (tests/mixture_model_ref.py): the log density at every chain's beta, one SliceSampler and one MALA transition of every replica
from random states, the evidence of a small data set against prior Monte Carlo, label switching on two well-separated clusters,
determinism, Compose, the chain-sharded engine, checkpoint / resume and replacing the data.

The shared checks and their tolerances (RTOL, LP_RTOL, and why) are in tests/family_gpu.py."""
import math

import numpy as np
import pytest

import family_gpu as G
import mixture_model_ref as R
from family_gpu import LP_RTOL, P  # noqa: F401  (P: the module's fixture)

pytestmark = pytest.mark.gpu

Y8 = [-1.6, -1.3, -1.0, -0.9, 0.8, 1.1, 1.3, 1.7]


def _data(n, seed=1):
    """standardised draws from a two-component mixture"""
    g = np.random.default_rng(seed)
    y = np.where(g.uniform(size=n) < 0.4, g.normal(-1.0, 0.4, n), g.normal(0.8, 0.7, n))
    return (y - y.mean()) / (y.std() if n > 1 else 1.0)


def test_state_calls_need_the_data_and_the_setter_validates(P):
    L = P._lib
    eng = P.Engine(n_chains=4, target=L.TARGET_MIXTURE_MODEL, dim=6, explorer=L.EXPLORER_SLICE, target_params=[1.0])
    for call in (lambda: eng.explore(1), lambda: eng.swap(1), lambda: eng.run_scans(1, 2), lambda: eng.states()):
        with pytest.raises(P.PteError, match="call pte_set_target_mixture_model first"):
            call()
    y = _data(10)
    cases = [
        (np.zeros(65537), r"1\.\.65536 observations"),
        (np.zeros(0), r"1\.\.65536 observations"),
        (np.where(np.arange(10) == 2, np.inf, y), r"y\[2\] must be finite"),
        (np.where(np.arange(10) >= 7, np.nan, y), r"y\[7\] must be finite"),
    ]
    for arg, msg in cases:
        with pytest.raises(P.PteError, match=msg):
            eng.set_target_mixture_model(arg)
    with pytest.raises(P.PteError, match="null argument"):
        eng._chk(eng.L.pte_set_target_mixture_model(eng.h, 10, None))
    with pytest.raises(P.PteError, match=r"1\.\.65536 observations"):           # the n range is checked before the pointer
        eng._chk(eng.L.pte_set_target_mixture_model(eng.h, 0, None))
    other = P.Engine(n_chains=4, target=L.TARGET_FUNNEL, dim=6, explorer=L.EXPLORER_SLICE, target_params=[1.0])
    with pytest.raises(P.PteError, match="this engine's target is 2, not PTE_TARGET_MIXTURE_MODEL"):
        other._chk(other.L.pte_set_target_mixture_model(other.h, 0, None))       # the engine's target is checked first
    eng.set_target_mixture_model(y)
    eng.explore(1)
    assert eng.states()[0].shape == (4, 6) and eng.kernel_name() == "k_explore_mixture_model" and eng.scan_loop_name() == ""
    for ex in (L.EXPLORER_AUTOMALA, L.EXPLORER_MALA):
        e2 = P.Engine(n_chains=4, target=L.TARGET_MIXTURE_MODEL, dim=9, explorer=ex, target_params=[1.0])
        assert e2.kernel_name() == "k_explore_mixture_model" and e2.scan_loop_name() == ""


@pytest.mark.parametrize("n,K", [(1, 1), (70, 2), (300, 3), (4096, 8), (65536, 4)])
def test_log_density_at_every_beta(P, n, K):
    """the device's log density (extended traces of one explore step) against the restatement at the state the step left, every chain's
    beta: one observation, ragged n, every bucket of components, the largest n"""
    y = _data(n, seed=n + K)
    d, N, prec = 3 * K, 12, 0.5
    pt = P.PT(P.Inputs(target=P.MixtureModelPosterior(y, K), reference=P.ScaledPrecisionNormalLogPotential(prec, d),
                       n_chains=N, n_rounds=2, explorer=P.SliceSampler(n_passes=1), record=[P.traces], extended_traces=True, show_report=False))
    betas, _, _, _ = G.random_states(pt, N, d, seed=d, scale=0.5)
    tr = G.log_densities(pt, N, d)
    model = R.MixtureModel(y, K, prec)
    G.assert_log_density_at_every_beta(tr, betas, d, lambda beta: R.MixtureModelChain(model, beta, prec).path_lp, LP_RTOL, abs_tol=1e-11)


@pytest.mark.parametrize("n,K", [(50, 1), (70, 2), (130, 3), (200, 8)])
def test_one_slice_transition_parity(P, n, K):
    y = _data(n, seed=7 * n + K)
    d, N, prec = 3 * K, 10, 0.5
    pt = P.PT(P.Inputs(target=P.MixtureModelPosterior(y, K), reference=P.ScaledPrecisionNormalLogPotential(prec, d), n_chains=N,
                       n_rounds=2, explorer=P.SliceSampler(), show_report=False))
    betas, x, chain, rng = G.random_states(pt, N, d, seed=n, scale=1.0)
    model = R.MixtureModel(y, K, prec)
    G.assert_slice_transition(pt.replicas, betas, x, chain, rng, lambda beta: R.MixtureModelChain(model, beta, prec).path_lp)


@pytest.mark.parametrize("n,K,precond", [(40, 2, "mix"), (64, 3, "diagonal"), (100, 1, "identity"), (90, 8, "mix"), (200, 4, "diagonal")])
def test_one_mala_transition_parity(P, n, K, precond):
    y = _data(n, seed=3 * n + K)
    d, N, step, prec = 3 * K, 10, 0.05, 1.0
    ex = G.mala_explorer(P, step, precond)
    pt = P.PT(P.Inputs(target=P.MixtureModelPosterior(y, K), reference=P.ScaledPrecisionNormalLogPotential(prec, d), n_chains=N,
                       n_rounds=2, explorer=ex, show_report=False))
    betas, x, chain, rng = G.random_states(pt, N, d, seed=d, scale=0.5)
    model = R.MixtureModel(y, K, prec)
    G.assert_mala_transition(pt.replicas, ex, precond, betas, x, chain, rng, lambda beta: R.MixtureModelChain(model, beta, prec),
                             std_range=(0.5, 2.0), form="whole")


# ---- whole runs ------------------------------------------------------------------------------------------------------------------------
def _run(P, target, prec, seed, n_rounds, explorer, n_chains=16):
    return G.run_rounds(P, target, prec, seed, n_rounds, explorer, n_chains=n_chains,
                        record=["round_trip", "traces", "log_sum_ratio", "index_process"])


def _stepping_stone_se(tr, betas, model):
    """G.stepping_stone_se on this family's target - reference = log likelihood + the constants"""
    return G.stepping_stone_se(model.log_likelihood(tr[:, :, :model.d]) + model.c_prior, betas)


@pytest.fixture(scope="module")
def evidence_mc():
    """log p(y) of the eight observations under K = 2, p = 1 by prior Monte Carlo: -14.417 +- 0.0044 (4e6 draws, default_rng(1))"""
    est, se = R.prior_monte_carlo_log_evidence(Y8, 2, 1.0, 4000000, 1)
    assert se <= 0.01
    return est, se


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_evidence_against_prior_monte_carlo(P, seed, evidence_mc):
    """n = 8, K = 2, p = 1, 16 chains, AutoMALA, 10 rounds: stepping_stone + (d/2) log(2 pi / p) within 4 sqrt(se_PT^2 + se_MC^2) of the
    prior-Monte-Carlo log evidence; se_PT by batch means (_stepping_stone_se).  Measured: -14.467 +- 0.037, -14.428 +- 0.042,
    -14.432 +- 0.043 against -14.417 +- 0.0044, 191-197 round trips."""
    mc, se_mc = evidence_mc
    model = R.MixtureModel(Y8, 2, 1.0)
    pt, grids = _run(P, P.MixtureModelPosterior(Y8, 2), 1.0, seed, 10, P.AutoMALA())
    se_pt = _stepping_stone_se(pt.reduced_recorders.traces, grids, model)
    est = P.stepping_stone(pt) - model.evidence_offset()
    print("evidence seed %d: PT %.4f +- %.4f, prior MC %.4f +- %.4f, round trips %d" % (seed, est, se_pt, mc, se_mc, P.n_round_trips(pt)))
    assert abs(est - mc) <= 4 * math.sqrt(se_pt ** 2 + se_mc ** 2), (est, mc, se_pt, se_mc)
    assert P.n_round_trips(pt) > 0


def test_label_switching_on_two_separated_clusters(P):
    """n = 200, half near -1 and half near +1 at sd 0.2, K = 2, p = 0.25: the two labellings are separated by a barrier no local move
    crosses, and by symmetry the target chain spends exactly half its scans with mu_1 < mu_2.  32 chains, SliceSampler, 12 rounds: the
    fraction over the last round's 4096 scans within 4 batch-means standard errors (B = 16) of 1/2, and that error at most 0.1 -- a chain
    stuck in one labelling has fraction 0 or 1 and fails the first, one that switched a few times only fails the second.  Measured
    (DESIGN 4.11): fraction 0.4678, standard error 0.0245, 232 round trips."""
    g = np.random.default_rng(5)
    y = np.concatenate([g.normal(-1.0, 0.2, 100), g.normal(1.0, 0.2, 100)])
    pt, _ = _run(P, P.MixtureModelPosterior(y, 2), 0.25, 1, 12, P.SliceSampler(), n_chains=32)
    tr = pt.reduced_recorders.traces[:, -1, :6]                    # the target chain
    ind = (tr[:, 0] < tr[:, 1]).astype(float)
    frac = ind.mean()
    se = float(G.batches(ind, 16).mean(axis=1).std(ddof=1) / 4.0)
    print("label switching: fraction %.4f, se %.4f, scans %d, round trips %d" % (frac, se, ind.size, P.n_round_trips(pt)))
    assert se <= 0.1, (frac, se)
    assert abs(frac - 0.5) <= 4 * se, (frac, se)
    # the target chain sits in the two-cluster fit: the means near -1 and +1 in either order
    lo, hi = np.minimum(tr[:, 0], tr[:, 1]), np.maximum(tr[:, 0], tr[:, 1])
    assert abs(np.median(lo) + 1.0) < 0.1 and abs(np.median(hi) - 1.0) < 0.1


def _inputs(P, seed=1, explorer=None, n_rounds=5, checkpoint=False):
    return P.Inputs(target=P.MixtureModelPosterior(_data(80, seed=23), 2), reference=P.ScaledPrecisionNormalLogPotential(0.5, 6), n_chains=12,
                    n_rounds=n_rounds, seed=seed, explorer=explorer or P.SliceSampler(), checkpoint=checkpoint,
                    record=[P.round_trip, P.traces, P.log_sum_ratio, P.index_process, P.swap_acceptance_pr, P.energy_ac1], show_report=False)


def test_two_runs_are_equal_bit_for_bit(P):
    G.assert_two_runs_equal(P, lambda: _inputs(P, seed=3, explorer=P.AutoMALA()))


def test_compose_slice_automala_runs(P):
    G.assert_compose_runs(P, _inputs(P, seed=2, explorer=P.Compose(P.SliceSampler(), P.AutoMALA())), "k_explore_mixture_model")


@pytest.mark.parametrize("explorer", ["slice", "automala"])
def test_sharded_equals_single_engine(P, explorer):
    mk = lambda: G.with_recorders(P, _inputs(P, seed=4, n_rounds=4, explorer=P.SliceSampler() if explorer == "slice" else P.AutoMALA()), "online")
    G.assert_sharded_equals_single(P, mk, n_shards=2)


def test_checkpoint_resume_equals_uninterrupted(P, tmp_path):
    G.assert_checkpoint_resume(P, lambda **kw: _inputs(P, seed=5, explorer=P.MALA(step_size=0.1), **kw), tmp_path)


def test_new_data_replaces_the_old(P):
    """set_target_mixture_model again (another n on the same engine): the swap statistics are refreshed at once, and the log densities of
    the next step are the new data's"""
    K, N, prec = 3, 8, 0.5
    d = 3 * K
    y1 = _data(90, seed=31)
    pt = P.PT(P.Inputs(target=P.MixtureModelPosterior(y1, K), reference=P.ScaledPrecisionNormalLogPotential(prec, d),
                       n_chains=N, n_rounds=2, explorer=P.SliceSampler(n_passes=1), record=[P.traces], extended_traces=True, show_report=False))
    betas, _, _, _ = G.random_states(pt, N, d, seed=3, scale=0.5)
    y2 = 1.5 * _data(200, seed=32)
    pt.replicas.set_target_mixture_model(y2)
    tr = G.log_densities(pt, N, d)
    new, old = R.MixtureModel(y2, K, prec), R.MixtureModel(y1, K, prec)
    G.assert_log_density_at_every_beta(tr, betas, d, lambda beta: R.MixtureModelChain(new, beta, prec).path_lp, LP_RTOL, abs_tol=1e-11)
    G.assert_log_density_is_not(tr, betas, d, lambda beta: R.MixtureModelChain(old, beta, prec).path_lp)
