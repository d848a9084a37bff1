"""The latent-AR(1) state-space family on the device (k_explore_ar1, pigeons.jl_amd/csrc/pte_ar1.hpp) against its NumPy restatement
(tests/ar1_ref.py): the log density at every chain's beta, one SliceSampler and one MALA transition of every replica from random states,
whole runs of the normal observation model against the quadrature's posterior means and evidence, and on the stochastic-volatility model
determinism, Compose, the chain-sharded engine, checkpoint / resume and replacing the data.

The shared checks and their tolerances (RTOL, LP_RTOL, and why) are in tests/family_gpu.py; what differs from libm by an ulp here is the
device's tanh / exp / log / log1p."""
import numpy as np
import pytest

import ar1_ref as R
import family_gpu as G
from family_gpu import LP_RTOL, P  # noqa: F401  (P: the module's fixture)

pytestmark = pytest.mark.gpu

TRUTH_Y = (0.3, 0.9, 1.4, 0.8, 0.2, -0.5, -1.1, -0.6, 0.1, 0.7, 1.2, 0.9)
TRUTH_KW = dict(obs_sd=0.5, mu_sd=2.0, phi_loc=0.0, phi_scale=1.0, sigma_scale=1.0)
LIK = {"sv": "stochastic_volatility", "n": "normal_identity"}
PRIORS = dict(obs_sd=0.7, mu_sd=2.0, phi_loc=0.3, phi_scale=0.8, sigma_scale=1.5)
MALA_STEP = {7: 0.2, 64: 0.1, 65: 0.1}          # by d: the restatement's own MALA accepts some proposals and rejects others at these


def _data(T, lik, seed=1):
    """a latent AR(1) path (phi = 0.8, sigma = 0.5, mu = 0.2) observed through the model"""
    g = np.random.default_rng(seed)
    h = np.empty(T)
    h[0] = 0.2 + g.normal(0.0, 0.5 / 0.6)
    for t in range(1, T):
        h[t] = 0.2 + 0.8 * (h[t - 1] - 0.2) + 0.5 * g.normal()
    if LIK.get(lik, lik) == "normal_identity":
        return h + 0.7 * g.normal(0.0, 1.0, T)
    return np.exp(h / 2.0) * g.normal(0.0, 1.0, T)


def _pt(P, y, lik, prec, N, explorer, priors=PRIORS, **kw):
    t = P.LatentAR1(y, likelihood=LIK.get(lik, lik), **priors)
    return P.PT(P.Inputs(target=t, reference=P.ScaledPrecisionNormalLogPotential(prec, t.dim), n_chains=N, n_rounds=2, explorer=explorer,
                         show_report=False, **kw))


def test_state_calls_need_the_data_and_the_setter_validates(P):
    L = P._lib
    eng = P.Engine(n_chains=4, target=L.TARGET_LATENT_AR1, dim=6, explorer=L.EXPLORER_SLICE, target_params=[1.0])
    for call in (lambda: eng.explore(1), lambda: eng.swap(1), lambda: eng.run_scans(1, 2), lambda: eng.states()):
        with pytest.raises(P.PteError, match=r"the latent-AR\(1\) target has no data yet; call pte_set_target_ar1 first"):
            call()
    y = np.array([1.0, -2.0, 0.5])
    ok = (1.0, 5.0, 0.0, 1.0, 1.0)                  # obs_sd, mu_sd, phi_loc, phi_scale, sigma_scale
    cases = [
        ((2, y) + ok, r"likelihood must be PTE_AR1_STOCHASTIC_VOLATILITY \(0\) or PTE_AR1_NORMAL_IDENTITY \(1\) \(got 2\)"),
        ((0, y[:2]) + ok, r"n_obs must be dim - 3 = 3 \(got 2\)"),
        ((1, np.zeros(4)) + ok, r"n_obs must be dim - 3 = 3 \(got 4\)"),
        ((0, np.where(np.arange(3) == 1, np.nan, y)) + ok, r"y\[1\] must be finite \(got nan\)"),
        ((1, np.where(np.arange(3) == 2, np.inf, y)) + ok, r"y\[2\] must be finite \(got inf\)"),
        ((1, y, 0.0, 5.0, 0.0, 1.0, 1.0), r"obs_sd must be positive and finite \(got 0\)"),
        ((1, y, np.nan, 5.0, 0.0, 1.0, 1.0), r"obs_sd must be positive and finite \(got nan\)"),
        ((0, y, 1.0, 0.0, 0.0, 1.0, 1.0), r"mu_sd must be positive and finite \(got 0\)"),
        ((0, y, 1.0, np.inf, 0.0, 1.0, 1.0), r"mu_sd must be positive and finite \(got inf\)"),
        ((0, y, 1.0, 5.0, 0.0, -1.0, 1.0), r"phi_scale must be positive and finite \(got -1\)"),
        ((0, y, 1.0, 5.0, 0.0, 1.0, np.nan), r"sigma_scale must be positive and finite \(got nan\)"),
        ((0, y, 1.0, 5.0, 0.0, 1.0, 0.0), r"sigma_scale must be positive and finite \(got 0\)"),
        ((0, y, 1.0, 5.0, np.inf, 1.0, 1.0), r"phi_loc must be finite \(got inf\)"),
        ((0, y, 1.0, 0.0, np.nan, 1.0, 1.0), r"mu_sd must be positive and finite \(got 0\)"),          # the first failure in the order of pte.h
    ]
    for args, msg in cases:
        with pytest.raises(P.PteError, match=msg):
            eng.set_target_ar1(*args)
    with pytest.raises(P.PteError, match="null argument"):
        eng._chk(eng.L.pte_set_target_ar1(eng.h, 0, 3, None, 1.0, 5.0, 0.0, 1.0, 1.0))
    with pytest.raises(P.PteError, match="has no data yet"):          # a refused call left the engine as it was
        eng.explore(1)
    funnel = P.Engine(n_chains=4, target=L.TARGET_FUNNEL, dim=6, explorer=L.EXPLORER_SLICE, target_params=[1.0])
    with pytest.raises(P.PteError, match="pte_set_target_ar1: this engine's target is 2, not PTE_TARGET_LATENT_AR1"):
        funnel.set_target_ar1(0, y, *ok)
    eng.set_target_ar1(0, y, 0.0, 5.0, 0.0, 1.0, 1.0)                  # obs_sd is not read by the stochastic-volatility model
    eng.explore(1)
    assert eng.states()[0].shape == (4, 6) and eng.kernel_name() == "k_explore_ar1" and eng.scan_loop_name() == ""
    with pytest.raises(P.PteError, match=r"y\[0\] must be finite"):   # ... nor does a refused call replace data that is there
        eng.set_target_ar1(0, np.array([np.nan, 0.0, 0.0]), *ok)
    eng.explore(2)
    assert np.all(np.isfinite(eng.states()[0]))


@pytest.mark.parametrize("lik", ["sv", "n"])
@pytest.mark.parametrize("d", [4, 5, 64, 65, 67, 132, 512])
def test_log_density_at_every_beta(P, d, lik):
    """the device's log density (extended traces of one explore step) against the restatement at the state the step left, every chain's
    beta: d = 4 (T = 1: no transition between observations); 5; 64 (one whole block); 65 (coordinate 64's predecessor is lane 63 of block 0);
    67; 132 (four blocks, ragged: the data re-read from L2); 512 (eight whole blocks)"""
    T = d - 3
    y = _data(T, lik, seed=d)
    N, prec = 8, 0.5
    pt = _pt(P, y, lik, prec, N, P.SliceSampler(n_passes=1), record=[P.traces], extended_traces=True)
    betas, _, _, _ = G.random_states(pt, N, d, seed=d, scale=1.5)
    tr = G.log_densities(pt, N, d)
    ar1 = R.Ar1(y, LIK[lik], **PRIORS)
    G.assert_log_density_at_every_beta(tr, betas, d, lambda beta: R.Ar1Chain(ar1, beta, prec).path_lp, LP_RTOL, abs_tol=1e-11)


@pytest.mark.parametrize("d,lik,w,p", [(6, "sv", 10.0, 20), (6, "n", 10.0, 20), (11, "sv", 10.0, 20), (11, "n", 10.0, 20),
                                       (69, "sv", 10.0, 20), (69, "n", 10.0, 20), (11, "sv", 0.25, 3), (11, "n", 0.25, 3)])
def test_one_slice_transition_parity(P, d, lik, w, p):
    """(w = 0.25, p = 3: the doubling stops at its cap, the slice is wider than the interval)"""
    T = d - 3
    y = _data(T, lik, seed=7 * d)
    N, prec = 10, 0.5
    pt = _pt(P, y, lik, prec, N, P.SliceSampler(w=w, p=p))
    betas, x, chain, rng = G.random_states(pt, N, d, seed=d, scale=1.0)
    ar1 = R.Ar1(y, LIK[lik], **PRIORS)
    G.assert_slice_transition(pt.replicas, betas, x, chain, rng, lambda beta: R.Ar1Chain(ar1, beta, prec).path_lp, w=w, p=p)


@pytest.mark.parametrize("d,lik,precond", [(7, "sv", "mix"), (7, "n", "identity"), (7, "sv", "diagonal"),
                                           (64, "sv", "diagonal"), (64, "n", "mix"), (64, "n", "identity"),
                                           (65, "sv", "identity"), (65, "n", "diagonal"), (65, "sv", "mix")])
def test_one_mala_transition_parity(P, d, lik, precond):
    """(d = 64: the whole-block instantiation; d = 65: the successor's residual of coordinate 63 comes from lane 0 of block 1)"""
    T = d - 3
    y = _data(T, lik, seed=3 * d)
    N, step, prec = 10, MALA_STEP[d], 1.0                 # (at this step the chains accept some proposals and reject others)
    ex = G.mala_explorer(P, step, precond)
    pt = _pt(P, y, lik, prec, N, ex)
    betas, x, chain, rng = G.random_states(pt, N, d, seed=d, scale=0.5)
    ar1 = R.Ar1(y, LIK[lik], **PRIORS)
    G.assert_mala_transition(pt.replicas, ex, precond, betas, x, chain, rng, lambda beta: R.Ar1Chain(ar1, beta, prec),
                             std_range=(0.5, 2.0), form="whole")


# ---- whole runs ------------------------------------------------------------------------------------------------------------------------
def _run(P, target, prec, seed, n_rounds, explorer):
    return G.run_rounds(P, target, prec, seed, n_rounds, explorer, n_chains=16,
                        record=["round_trip", "online", "traces", "log_sum_ratio", "index_process"])


def _target_minus_reference(ar1, X, prec):
    """(target - reference)(x) of every state of X [..., d] (plain sums: this feeds an error estimate, not a parity check)"""
    flat = X.reshape(-1, X.shape[-1])
    lp = np.array([ar1.lp_plain(x) for x in flat]).reshape(X.shape[:-1])
    return lp + 0.5 * prec * (X * X).sum(-1)


def _stepping_stone_se(tr, betas, ar1, prec):
    return G.stepping_stone_se(_target_minus_reference(ar1, tr[:, :, :ar1.d], prec), betas)


@pytest.fixture(scope="module")
def truth():
    """the quadrature, computed once: (log evidence, posterior means, posterior sds)"""
    return R.Ar1(TRUTH_Y, "normal_identity", **TRUTH_KW)._quadrature()


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_normal_model_run_against_the_quadrature(P, truth, seed):
    """The normal observation model on the 12 observations of DESIGN 4.15, p = 1, 16 chains, 10 rounds, SliceSampler's defaults.  The target
    chain's 15 means over the last round's 1024 scans within 5 batch-means standard errors (B = 16) of the quadrature, and stepping_stone -
    evidence_offset within 5 standard errors (_stepping_stone_se) of the quadrature's log evidence, -15.91679.  So that wide error bars cannot
    pass, every standard error of a mean must also be below a quarter of the quadrature's posterior sd of its quantity."""
    log_z, want, sd = truth
    assert abs(log_z - (-15.91679)) < 1e-5
    prec, d = 1.0, 15
    t = P.LatentAR1(TRUTH_Y, likelihood="normal_identity", **TRUTH_KW)
    pt, grids = _run(P, t, prec, seed, 10, P.SliceSampler())
    ar1 = R.Ar1(TRUTH_Y, "normal_identity", **TRUTH_KW)
    tr_all = pt.reduced_recorders.traces                          # [scan][chain][d + 1]
    assert tr_all.shape[0] == 1024
    q = tr_all[:, -1, :d]                                         # the target chain
    se = G.batches(q, 16).mean(axis=1).std(axis=0, ddof=1) / 4.0
    z = np.abs(q.mean(axis=0) - want) / se
    se_ss = _stepping_stone_se(tr_all, grids, ar1, prec)
    est = P.stepping_stone(pt) - t.evidence_offset(prec)
    print("latent AR(1), normal model, seed %d: max |z| %.2f, max se / sd %.3f, log evidence %.4f (exact %.4f, se %.4f, |z| %.2f), round trips %d"
          % (seed, z.max(), (se / sd).max(), est, log_z, se_ss, abs(est - log_z) / se_ss, P.n_round_trips(pt)))
    assert np.all(z < 5.0), (z, q.mean(axis=0), want, se)
    assert np.all(se < 0.25 * sd), se / sd
    assert abs(est - (-15.91679)) < 5 * se_ss, (est, log_z, se_ss)
    assert P.n_round_trips(pt) > 0


# ---- the stochastic-volatility model: no exact truth ----------------------------------------------------------------------------------------
def _inputs(P, seed=1, explorer=None, n_rounds=5, checkpoint=False):
    y = _data(12, "sv", seed=23)
    return P.Inputs(target=P.LatentAR1(y, likelihood="stochastic_volatility", **PRIORS),
                    reference=P.ScaledPrecisionNormalLogPotential(0.5, 15), n_chains=8, n_rounds=n_rounds,
                    seed=seed, explorer=explorer or P.SliceSampler(), checkpoint=checkpoint,
                    record=[P.round_trip, P.traces, P.log_sum_ratio, P.index_process, P.swap_acceptance_pr, P.energy_ac1], show_report=False)


def test_two_runs_are_equal_bit_for_bit(P):
    G.assert_two_runs_equal(P, lambda: _inputs(P, seed=3, explorer=P.AutoMALA()))


def test_compose_slice_automala_runs(P):
    G.assert_compose_runs(P, _inputs(P, seed=2, explorer=P.Compose(P.SliceSampler(), P.AutoMALA())), "k_explore_ar1")


@pytest.mark.parametrize("n_shards", [2, 4])
@pytest.mark.parametrize("explorer", ["slice", "automala"])
def test_sharded_equals_single_engine(P, explorer, n_shards):
    mk = lambda: G.with_recorders(P, _inputs(P, seed=4, n_rounds=4, explorer=P.SliceSampler() if explorer == "slice" else P.AutoMALA()), "online")
    G.assert_sharded_equals_single(P, mk, n_shards=n_shards)


def test_checkpoint_resume_equals_uninterrupted(P, tmp_path):
    G.assert_checkpoint_resume(P, lambda **kw: _inputs(P, seed=5, explorer=P.MALA(step_size=0.2), **kw), tmp_path)


def test_new_data_replaces_the_old(P):
    """set_target_ar1 again (other observations, the other observation model, other priors): the swap statistics are refreshed at once, and
    the log densities of the next step are the new data's"""
    T, N, prec = 12, 8, 0.5
    d = T + 3
    y1 = _data(T, "sv", seed=31)
    pt = _pt(P, y1, "sv", prec, N, P.SliceSampler(n_passes=1), record=[P.traces], extended_traces=True)
    betas, _, _, _ = G.random_states(pt, N, d, seed=3, scale=0.5)
    y2 = _data(T, "n", seed=32)
    pt.replicas.set_target_ar1(P._lib.AR1_NORMAL_IDENTITY, y2, 0.4, 3.0, -0.2, 1.1, 0.8)
    tr = G.log_densities(pt, N, d)
    new = R.Ar1(y2, "normal_identity", obs_sd=0.4, mu_sd=3.0, phi_loc=-0.2, phi_scale=1.1, sigma_scale=0.8)
    old = R.Ar1(y1, "stochastic_volatility", **PRIORS)
    G.assert_log_density_at_every_beta(tr, betas, d, lambda beta: R.Ar1Chain(new, beta, prec).path_lp, LP_RTOL, abs_tol=1e-11)
    G.assert_log_density_is_not(tr, betas, d, lambda beta: R.Ar1Chain(old, beta, prec).path_lp)
