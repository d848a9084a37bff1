"""The dense-precision Gaussian family on the device (k_explore_dense, k_explore_dense_slice, pigeons.jl_amd/csrc/pte_dense.hpp) against its
NumPy restatement (tests/dense_ref.py), which restates the FULL evaluation only -- the slice kernel's cached form is held to it: the setter,
the log density at every chain's beta, one SliceSampler and one MALA transition of every replica from random states, whole runs against the
closed-form law of every chain, determinism, Compose, the chain-sharded engine and checkpoint / resume.

The shared checks and their tolerances (RTOL, LP_RTOL, and why) are in tests/family_gpu.py; log densities get 1e-11 absolute with the
relative figure.  The test matrices are Q = U diag(lambda) U' with log-spaced lambda and cond <= 100, for which the restatement's own
summation-order error is a few 1e-16 relative: the tolerance tests the kernel, not the inputs."""
import math

import numpy as np
import pytest

import dense_ref as R
import family_gpu as G
from family_gpu import LP_RTOL, P  # noqa: F401  (P: the module's fixture)

pytestmark = pytest.mark.gpu


def _target(d, seed, cond=100.0):
    """(mean, Q): the mean N(0, 1), the spectrum log-spaced over cond"""
    return np.random.default_rng(1000 + seed).normal(0.0, 1.0, d), R.spectrum_matrix(d, cond, seed)


def _pt(P, mean, Q, prec, N, explorer, **kw):
    t = P.DenseNormal(mean, Q)
    return P.PT(P.Inputs(target=t, reference=P.ScaledPrecisionNormalLogPotential(prec, t.dim), n_chains=N, n_rounds=2, explorer=explorer,
                         show_report=False, **kw))


def test_state_calls_need_the_data_and_the_setter_validates(P):
    L = P._lib
    d = 5
    eng = P.Engine(n_chains=4, target=L.TARGET_DENSE_NORMAL, dim=d, explorer=L.EXPLORER_SLICE, target_params=[1.0])
    for call in (lambda: eng.explore(1), lambda: eng.swap(1), lambda: eng.run_scans(1, 2), lambda: eng.states()):
        with pytest.raises(P.PteError, match="the dense-normal target has no mean and precision yet; call pte_set_target_dense first"):
            call()
    m, Q = _target(d, 3)

    def at(a, idx, v):
        b = np.array(a, dtype=np.float64)
        b[idx] = v
        return b
    asym = at(Q, (1, 3), np.nextafter(Q[1, 3], np.inf))              # one ulp off its mirror image
    indef = Q - 1.5 * np.linalg.eigvalsh(Q)[0] * np.eye(d)           # the smallest eigenvalue becomes negative
    piv = next(j for j in range(d) if np.linalg.det(indef[:j + 1, :j + 1]) <= 0.0)
    cases = [
        ((m[:4], Q[:4, :4]), r"dim must be the engine's dim = 5 \(got 4\)"),
        ((np.zeros(6), np.eye(6)), r"dim must be the engine's dim = 5 \(got 6\)"),
        ((at(m, 2, np.nan), Q), r"mean\[2\] must be finite \(got nan\)"),
        ((m, at(Q, (3, 1), np.inf)), r"precision\[3\]\[1\] must be finite \(got inf\)"),
        ((m, at(at(Q, (4, 0), np.nan), (0, 2), 7.0)), r"precision\[4\]\[0\] must be finite"),       # non-finite is found before asymmetric
        ((m, asym), r"precision must be symmetric bit for bit: precision\[1\]\[3\] = \S+, precision\[3\]\[1\] = "),
        ((m, at(at(Q, (0, 2), 7.0), (2, 4), 7.0)), r"symmetric bit for bit: precision\[0\]\[2\]"),   # the first offending pair
        ((m, indef), r"precision is not positive definite: the Cholesky pivot %d is -?\d" % piv),
        ((m, -Q), r"not positive definite: the Cholesky pivot 0 is -"),
        ((m, np.zeros((d, d))), r"not positive definite: the Cholesky pivot 0 is 0"),
        ((m, at(asym, (4, 4), -1.0)), r"symmetric bit for bit: precision\[1\]\[3\]"),                # asymmetric is found before indefinite
    ]
    for args, msg in cases:
        with pytest.raises(P.PteError, match=msg):
            eng.set_target_dense(*args)
    for mean_p, prec_p in ((None, P.engine._dp(Q)), (P.engine._dp(m), None)):
        with pytest.raises(P.PteError, match="pte_set_target_dense: null argument"):
            eng._chk(eng.L.pte_set_target_dense(eng.h, d, mean_p, prec_p))
    with pytest.raises(P.PteError, match="has no mean and precision yet"):          # a refused call left the engine as it was
        eng.explore(1)
    funnel = P.Engine(n_chains=4, target=L.TARGET_FUNNEL, dim=d, explorer=L.EXPLORER_SLICE, target_params=[1.0])
    with pytest.raises(P.PteError, match="pte_set_target_dense: this engine's target is 2, not PTE_TARGET_DENSE_NORMAL"):
        funnel.set_target_dense(m, Q)
    with pytest.raises(P.PteError, match="null argument"):                           # a null argument is found before the wrong target
        funnel._chk(funnel.L.pte_set_target_dense(funnel.h, d, None, None))
    eng.set_target_dense(m, Q)
    eng.explore(1)
    assert eng.states()[0].shape == (4, d) and eng.kernel_name() == "k_explore_dense_slice" and eng.scan_loop_name() == ""
    for ex, name in ((L.EXPLORER_AUTOMALA, "k_explore_dense"), (L.EXPLORER_MALA, "k_explore_dense")):
        assert P.Engine(n_chains=4, target=L.TARGET_DENSE_NORMAL, dim=d, explorer=ex, target_params=[1.0]).kernel_name() == name
    both = P.Engine(n_chains=4, target=L.TARGET_DENSE_NORMAL, dim=d, explorer=L.EXPLORER_AUTOMALA, explorer2=L.EXPLORER_SLICE, target_params=[1.0])
    assert both.kernel_name() == "k_explore_dense"                   # a Compose: the first explorer's kernel


def test_a_refused_call_changes_nothing_and_new_data_replaces_the_old(P):
    """after a successful call a refused one leaves data and statistics alone; a second successful call replaces the data: the swap statistics
    are refreshed at once and the log densities of the next step follow the new matrix, away from the old one by more than 1e-6"""
    d, N, prec = 7, 8, 0.5
    m1, Q1 = _target(d, 31)
    pt = _pt(P, m1, Q1, prec, N, P.SliceSampler(n_passes=1), record=[P.traces], extended_traces=True)
    betas, _, _, _ = G.random_states(pt, N, d, seed=3, scale=0.5)
    with pytest.raises(P.PteError, match="not positive definite"):
        pt.replicas.set_target_dense(m1, -Q1)
    with pytest.raises(P.PteError, match="symmetric bit for bit"):
        pt.replicas.set_target_dense(m1, np.triu(Q1))
    tr = G.log_densities(pt, N, d)
    old = R.Dense(m1, Q1)
    G.assert_log_density_at_every_beta(tr, betas, d, lambda beta: R.DenseChain(old, beta, prec).path_lp, LP_RTOL, abs_tol=1e-11)
    m2, Q2 = _target(d, 32, cond=20.0)
    pt = _pt(P, m1, Q1, prec, N, P.SliceSampler(n_passes=1), record=[P.traces], extended_traces=True)
    betas, _, _, _ = G.random_states(pt, N, d, seed=3, scale=0.5)
    pt.replicas.set_target_dense(m2, Q2)
    tr = G.log_densities(pt, N, d)
    new = R.Dense(m2, Q2)
    G.assert_log_density_at_every_beta(tr, betas, d, lambda beta: R.DenseChain(new, beta, prec).path_lp, LP_RTOL, abs_tol=1e-11)
    for c in range(N):
        if betas[c] > 0:
            was = R.DenseChain(old, betas[c], prec).path_lp(tr[c, :d])
            assert abs(tr[c, d] - was) > 1e-6 and not math.isclose(tr[c, d], was, rel_tol=1e-6)


@pytest.mark.parametrize("d", [1, 2, 64, 65, 132, 512])
def test_log_density_at_every_beta(P, d):
    """the device's log density (extended traces of one SliceSampler pass) against the restatement at the state the pass left, every chain's
    beta: d = 1 a single coordinate; 2 the smallest coupled case; 64 a whole block; 65 the k loop and the broadcast cross into block 1;
    132 four blocks, ragged; 512 eight whole blocks.  The epilogue recomputes in full, so this also checks that nothing cached leaks out."""
    mean, Q = _target(d, d)
    N, prec = 8, 0.5
    pt = _pt(P, mean, Q, prec, N, P.SliceSampler(n_passes=1), record=[P.traces], extended_traces=True)
    betas, x0, _, _ = G.random_states(pt, N, d, seed=d, scale=1.5)
    tr = G.log_densities(pt, N, d)
    dense = R.Dense(mean, Q)
    G.assert_log_density_at_every_beta(tr, betas, d, lambda beta: R.DenseChain(dense, beta, prec).path_lp, LP_RTOL, abs_tol=1e-11)
    moved = sum(int(not any(np.array_equal(tr[c, :d], x0[i]) for i in range(N))) for c in range(N))
    assert moved == N                                             # every chain's state is the pass's, not the one that was set


@pytest.mark.parametrize("d,w,p,n_passes", [(2, 10.0, 20, 1), (11, 10.0, 20, 1), (69, 10.0, 20, 1), (11, 0.25, 3, 1), (65, 10.0, 20, 3)])
def test_one_slice_transition_parity(P, d, w, p, n_passes):
    """the cached-slice kernel against the oracle's slice sampler on the FULL restated density (w = 0.25, p = 3: the doubling stops at its
    cap, the slice is wider than the interval; n_passes = 3 at d = 65: the cached u, A and S drift over 195 coordinates)"""
    mean, Q = _target(d, 7 * d)
    N, prec = 10, 0.5
    pt = _pt(P, mean, Q, prec, N, P.SliceSampler(w=w, p=p, n_passes=n_passes))
    betas, x, chain, rng = G.random_states(pt, N, d, seed=d, scale=1.0)
    dense = R.Dense(mean, Q)
    G.assert_slice_transition(pt.replicas, betas, x, chain, rng, lambda beta: R.DenseChain(dense, beta, prec).path_lp,
                              w=w, p=p, n_passes=n_passes)


MALA_STEP = {7: 0.5, 64: 0.4, 65: 0.4}        # chosen on the restatement (below the stability limit 2 / sqrt(lambda_max) = 0.63): it accepts about three proposals in four


@pytest.mark.parametrize("precond", ["identity", "diagonal", "mix"])
@pytest.mark.parametrize("d", [7, 64, 65])
def test_one_mala_transition_parity(P, d, precond):
    """(d = 64: the whole-block instantiation; 65: two blocks, ragged).  The restatement runs refresh by refresh, so the test sees that it
    accepts some proposals and rejects others."""
    mean, Q = _target(d, 3 * d)
    N, step, prec = 10, MALA_STEP[d], 1.0
    ex = G.mala_explorer(P, step, precond)
    pt = _pt(P, 0.3 * mean, Q, prec, N, ex)
    betas, x, chain, rng = G.random_states(pt, N, d, seed=d, scale=0.5)
    dense = R.Dense(0.3 * mean, Q)
    G.assert_mala_transition(pt.replicas, ex, precond, betas, x, chain, rng, lambda beta: R.DenseChain(dense, beta, prec),
                             std_range=(0.7, 1.4), form="by_refresh", label="MALA d = %d, %s" % (d, precond))


# ---- whole runs ------------------------------------------------------------------------------------------------------------------------
EXACT_D = np.array([0.5, 0.8, 1.1, 1.4, 1.7, 2.0])
EXACT_COV = EXACT_D[:, None] * (0.6 * np.ones((6, 6)) + 0.4 * np.eye(6)) * EXACT_D[None, :]       # cond about 68
EXACT_MEAN = np.array([2.0, -1.0, 0.5, 3.0, -2.5, 1.0])


def _run(P, target, prec, seed, n_rounds, explorer):
    return G.run_rounds(P, target, prec, seed, n_rounds, explorer, n_chains=10,
                        record=["round_trip", "online", "traces", "log_sum_ratio", "index_process"])


def _stepping_stone_se(tr, betas, dense, prec):
    """G.stepping_stone_se on this family's target - reference (plain sums: this feeds an error estimate, not a parity check)"""
    X = tr[:, :, :dense.d]
    Z = X - dense.mean
    return G.stepping_stone_se(dense.c - 0.5 * np.einsum("tci,ij,tcj->tc", Z, dense.Q, Z) + 0.5 * prec * (X * X).sum(-1), betas)


@pytest.mark.parametrize("seed", [1, 2])
@pytest.mark.parametrize("explorer", ["slice", "automala"])
def test_run_against_the_closed_forms(P, explorer, seed):
    """d = 6, covariance D (0.6 11' + 0.4 I) D (cond about 68), mean (2, -1, 0.5, 3, -2.5, 1), p = 0.25, 10 chains, 10 rounds.  Over the
    last round's 1024 scans (extended traces): EVERY chain's mean vector within 5 batch-means standard errors (B = 16) of the exact mean of
    the Gaussian chain beta is (precision (1 - beta) p I + beta Q); for the target chain the six second moments E x_i^2 and the cross
    moments E x_0 x_1, E x_2 x_5 likewise; stepping_stone - evidence_offset within 5 standard errors (_stepping_stone_se) of 0, the log
    evidence of the normalised target.  Five standard errors: the argument of tests/test_gpu_hier.py.  So that wide error bars cannot pass,
    every standard error of a target-chain moment must be below a quarter of that moment's exact standard deviation (Var x^2 = 2 s^4 +
    4 m^2 s^2; Var xy = mx^2 sy^2 + my^2 sx^2 + 2 mx my sxy + sx^2 sy^2 + sxy^2 for a Gaussian pair)."""
    prec, d = 0.25, 6
    Qm = np.linalg.inv(EXACT_COV)
    t = P.DenseNormal(EXACT_MEAN, Qm)
    pt, grids = _run(P, t, prec, seed, 10, P.SliceSampler() if explorer == "slice" else P.AutoMALA())
    dense = R.Dense(t.mean, t.precision)
    tr_all = pt.reduced_recorders.traces                          # [scan][chain][d + 1]
    assert tr_all.shape == (1024, 10, d + 1)
    zmax = 0.0
    for c in range(10):                                           # every chain's mean vector
        want, _ = R.DenseChain(dense, grids[c], prec).chain_moments()
        xc = tr_all[:, c, :d]
        se = G.batches(xc, 16).mean(axis=1).std(axis=0, ddof=1) / 4.0
        z = np.abs(xc.mean(axis=0) - want) / se
        zmax = max(zmax, z.max())
        assert np.all(z < 5.0), (c, grids[c], z, xc.mean(axis=0), want, se)
    assert grids[-1] == 1.0
    m, cov = t.chain_moments(1.0, prec)
    np.testing.assert_allclose(cov, EXACT_COV, rtol=1e-9)
    x = tr_all[:, -1, :d]                                         # the target chain
    pairs = [(i, i) for i in range(d)] + [(0, 1), (2, 5)]
    q = np.stack([x[:, i] for i in range(d)] + [x[:, i] * x[:, j] for i, j in pairs], axis=1)
    want = np.array(list(m) + [cov[i, j] + m[i] * m[j] for i, j in pairs])
    var = [cov[i, i] for i in range(d)] + [m[i] ** 2 * cov[j, j] + m[j] ** 2 * cov[i, i] + 2 * m[i] * m[j] * cov[i, j] + cov[i, i] * cov[j, j] + cov[i, j] ** 2
                                         for i, j in pairs]
    sd = np.sqrt(np.array(var))
    se = G.batches(q, 16).mean(axis=1).std(axis=0, ddof=1) / 4.0
    z = np.abs(q.mean(axis=0) - want) / se
    se_ss = _stepping_stone_se(tr_all, grids, dense, prec)
    est = P.stepping_stone(pt) - t.evidence_offset(prec)
    print("dense normal %s seed %d: max |z| of the chains' means %.2f, of the target chain's moments %.2f, max se / sd %.3f, "
          "log evidence %.4f (exact 0, se %.4f, |z| %.2f)" % (explorer, seed, zmax, z.max(), (se / sd).max(), est, se_ss, abs(est) / se_ss))
    assert np.all(z < 5.0), (z, q.mean(axis=0), want, se)
    assert np.all(se < 0.25 * sd), se / sd
    assert abs(est) < 5 * se_ss, (est, se_ss)
    assert P.n_round_trips(pt) > 0


def _inputs(P, seed=1, explorer=None, n_rounds=5, checkpoint=False):
    mean, Q = _target(11, 23)
    return P.Inputs(target=P.DenseNormal(mean, Q), reference=P.ScaledPrecisionNormalLogPotential(0.5, 11), n_chains=12, n_rounds=n_rounds,
                    seed=seed, explorer=explorer or P.SliceSampler(), checkpoint=checkpoint,
                    record=[P.round_trip, P.traces, P.log_sum_ratio, P.index_process, P.swap_acceptance_pr, P.energy_ac1], show_report=False)


@pytest.mark.parametrize("explorer", ["slice", "automala"])
def test_two_runs_are_equal_bit_for_bit(P, explorer):
    G.assert_two_runs_equal(P, lambda: _inputs(P, seed=3, explorer=P.SliceSampler() if explorer == "slice" else P.AutoMALA()))


def test_compose_slice_automala_runs(P):
    G.assert_compose_runs(P, _inputs(P, seed=2, explorer=P.Compose(P.SliceSampler(), P.AutoMALA())), "k_explore_dense_slice")
    # (no round-trip count here: 12 chains need 22 scans for one and the last of the 5 rounds has 32; test_run_against_the_closed_forms asks it of 10 rounds)


@pytest.mark.parametrize("explorer", ["slice", "automala"])
def test_sharded_equals_single_engine(P, explorer):
    mk = lambda: G.with_recorders(P, _inputs(P, seed=4, n_rounds=4, explorer=P.SliceSampler() if explorer == "slice" else P.AutoMALA()), "online")
    G.assert_sharded_equals_single(P, mk, n_shards=2)


@pytest.mark.parametrize("explorer", ["slice", "mala"])
def test_checkpoint_resume_equals_uninterrupted(P, tmp_path, explorer):
    """(the slice kernel's swap statistics are recomputed in full from the stored state, so a resumed run sees the same bits)"""
    ex = lambda: P.SliceSampler() if explorer == "slice" else P.MALA(step_size=0.2)
    G.assert_checkpoint_resume(P, lambda **kw: _inputs(P, seed=5, explorer=ex(), **kw), tmp_path)
