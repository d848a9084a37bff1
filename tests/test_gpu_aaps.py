"""AAPS on the device (k_explore_aaps, pigeons.jl_amd/csrc/pte_aaps.hpp) against its NumPy restatement (tests/aaps_ref.py): one transition of
every replica from random states, invariance of the target, whole runs, determinism, the recorders and the chain-sharded engine.

RNG words are compared exactly; states and recorders to 1e-9 relative -- the device sums over its fixed tree and its exp / log differ from
libm by an ulp (the bar of the Langevin parity tests)."""
import math

import numpy as np
import pytest

import aaps_ref as A
import oracle as O

pytestmark = pytest.mark.gpu

RTOL = 1e-9


@pytest.fixture(scope="module")
def P():
    import pigeons_amd
    return pigeons_amd


PRECONDS = {"identity": (0, lambda P: P.IdentityPreconditioner()), "diagonal": (1, lambda P: P.DiagonalPreconditioner()),
            "mix": (2, lambda P: P.MixDiagonalPreconditioner())}


def _one_step(P, target, N, d, precond="mix", step=0.4, K=4, vref=False, seed=3):
    """set every replica to a random state (chains permuted, one of them the reference), explore once, compare with aaps_ref"""
    mode, mk = PRECONDS[precond]
    funnel = target == "funnel"
    inp = P.Inputs(target=P.Funnel(d) if funnel else P.toy_mvn_target(d),
                   reference=P.ScaledPrecisionNormalLogPotential(1.0 / 9.0, d) if funnel else None,
                   n_chains=N, n_rounds=2, explorer=P.AAPS(step_size=step, K=K, preconditioner=mk(P)), seed=seed, show_report=False)
    pt = P.PT(inp)
    eng = pt.replicas
    assert eng.kernel_name() == "k_explore_aaps" and eng.scan_loop_name() == ""
    g = np.random.default_rng(seed)
    betas = np.concatenate([[0.0], np.sort(g.uniform(0.0, 1.0, N - 2)) ** 2, [1.0]]) if N > 1 else np.array([1.0])
    eng.set_schedule(betas)
    x = g.standard_normal((N, d)) * (0.5 if funnel else 0.4)
    chain = g.permutation(N).astype(np.int64)
    _, _, rng = eng.states()
    eng.set_states(x, chain, rng)
    std = g.uniform(0.5, 2.0, d)
    eng.set_explorer_adaptation(step, std)
    vm = vs = None
    if vref:
        vm, vs = g.normal(0.0, 0.3, d), g.uniform(0.7, 1.5, d)
        eng.set_variational_reference(vm, vs, np.ones(N, dtype=np.int32))
    eng.explore(1)
    x1, c1, r1 = eng.states()
    eng.reduce()
    am, an, ss, sn = eng.explorer_stats()
    assert np.array_equal(c1, chain)
    n_moved = 0
    for i in range(N):
        c = int(chain[i])
        if c == 0 and N > 1:                                  # the reference chain: sample_iid!
            continue
        r = O.OracleRng(state=(int(rng[i, 0]), int(rng[i, 1])))
        M = A.build_preconditioner(r, d, mode, 1.0 / 3.0, 1.0 / 3.0, std)
        ch = A.FunnelChain(betas[c], 1.0 / 9.0, vm, vs) if funnel else A.mvn_chain(1.0, 10.0, betas[c])
        res = A.transition(x[i], r, ch, step, K, M)
        assert int(r1[i, 0]) == r.state[0] and int(r1[i, 1]) == r.state[1], (i, c)
        np.testing.assert_allclose(x1[i], res["x"], rtol=RTOL, atol=1e-12, err_msg="replica %d chain %d" % (i, c))
        assert an[c] == 1 and sn[c] == 1 and ss[c] == res["steps"], (i, c, ss[c], res["steps"])
        np.testing.assert_allclose(am[c], res["acc"], rtol=RTOL, atol=1e-12)
        n_moved += int(not np.array_equal(res["x"], x[i]))
    assert n_moved > 0
    return pt


@pytest.mark.parametrize("d", [1, 7, 64, 100, 256, 512])
def test_one_step_parity_mvn(P, d):
    _one_step(P, "mvn", 16 if d <= 256 else 8, d)


@pytest.mark.parametrize("d", [2, 8, 128])
@pytest.mark.parametrize("vref", [False, True])
def test_one_step_parity_funnel(P, d, vref):
    _one_step(P, "funnel", 12, d, step=0.3, vref=vref)


@pytest.mark.parametrize("precond", ["identity", "diagonal", "mix"])
@pytest.mark.parametrize("target", ["mvn", "funnel"])
def test_one_step_parity_preconditioners(P, precond, target):
    for seed in (1, 2):
        _one_step(P, target, 10, 20, precond=precond, step=0.5, K=2, seed=seed)


def test_one_step_parity_K(P):
    for K in (0, 1, 9):
        _one_step(P, "mvn", 8, 33, K=K, step=0.6, precond="identity")


def test_invariance_on_the_device(P):
    """N = 1024 chains of toy_mvn(64) set to exact draws at their own beta; three explore calls without swaps keep them N(0, 1 / precision)"""
    from scipy import stats
    N, d = 1024, 64
    pt = P.PT(P.Inputs(target=P.toy_mvn_target(d), n_chains=N, n_rounds=2, explorer=P.AAPS(step_size=0.3, K=3), seed=5, show_report=False))
    eng = pt.replicas
    betas = np.linspace(0.0, 1.0, N)
    eng.set_schedule(betas)
    prec = 1.0 + 9.0 * betas
    g = np.random.default_rng(11)
    chain = g.permutation(N).astype(np.int64)
    x = g.standard_normal((N, d)) / np.sqrt(prec[chain])[:, None]
    _, _, rng = eng.states()
    eng.set_states(x, chain, rng)
    for s in (1, 2, 3):
        eng.explore(s)
    x1, c1, _ = eng.states()
    keep = c1 != 0
    Z = x1[keep] * np.sqrt(prec[c1[keep]])[:, None]
    assert np.mean(np.any(x1[keep] != x[keep], axis=1)) > 0.9
    n = Z.size
    assert abs(Z.mean()) * math.sqrt(n) < 4.0, Z.mean()
    assert abs(Z.var() - 1.0) / math.sqrt(2.0 / n) < 4.0, Z.var()
    for j in (0, d // 2, d - 1):
        assert stats.kstest(Z[:, j], "norm").pvalue > 1e-3, j


def test_whole_run_mvn(P):
    d = 64
    pt = P.pigeons(target=P.toy_mvn_target(d), explorer=P.AAPS(), n_chains=16, n_rounds=8, seed=2,
                   record=[P.round_trip, P.online, P.log_sum_ratio, P.explorer_acceptance_pr, P.explorer_n_steps], show_report=False)
    m, v, n = pt.reduced_recorders.online
    assert n > 0
    assert abs(float(np.mean(m))) < 0.03, np.mean(m)                 # measured 0.003
    assert abs(float(np.mean(v)) - 0.1) < 0.01, np.mean(v)           # 1 / precision = 0.1; measured 0.098
    exact = P.analytic_lognormalization(pt.inputs.target)
    assert abs(P.stepping_stone(pt) - exact) < 1.0, (P.stepping_stone(pt), exact)     # measured -73.91 against -73.68
    am, an = pt.reduced_recorders.explorer_acceptance_pr
    ss, sn = pt.reduced_recorders.explorer_n_steps
    assert np.all(an[1:] > 0) and np.all(sn[1:] == an[1:]) and np.all(ss[1:] >= 2 * sn[1:])
    assert np.all((am[1:] >= 0.0) & (am[1:] <= 1.0)) and am[-1] > 0.1


def test_whole_run_funnel(P):
    """Funnel(8): round trips, and the funnel coordinate's variance near 9 (two seeds: measured 6.0 and 10.1; AutoMALA at the same settings
    5.1 and 9.3 -- the neck is slow to explore at this length)"""
    d = 8
    vs = []
    for seed in (1, 2):
        pt = P.pigeons(target=P.Funnel(d), reference=P.ScaledPrecisionNormalLogPotential(1.0 / 9.0, d), explorer=P.AAPS(step_size=0.5),
                       n_chains=16, n_rounds=12, seed=seed, record=[P.round_trip, P.online, P.log_sum_ratio], show_report=False)
        m, v, n = pt.reduced_recorders.online
        assert n > 0 and P.n_round_trips(pt) > 0
        assert 4.5 < v[0] < 16.0, (seed, v[0])
        vs.append(v[0])
    assert 6.0 < np.mean(vs) < 12.0, vs


def test_determinism_and_the_two_forms(P):
    mk = lambda: P.PT(P.Inputs(target=P.toy_mvn_target(30), n_chains=8, n_rounds=3, explorer=P.AAPS(step_size=0.5), seed=4,
                               record=[P.round_trip, P.index_process], show_report=False))
    a, b = mk(), mk()
    a.replicas.run_scans(1, 6)
    for s in range(1, 7):
        b.replicas.explore(s)
        b.replicas.swap(s)
    xa, ca, ra = a.replicas.states()
    xb, cb, rb = b.replicas.states()
    assert np.array_equal(xa, xb) and np.array_equal(ca, cb) and np.array_equal(ra, rb)
    c = mk()
    c.replicas.run_scans(1, 6)
    xc, cc, rc = c.replicas.states()
    assert np.array_equal(xa, xc) and np.array_equal(ca, cc) and np.array_equal(ra, rc)


@pytest.mark.parametrize("target", ["mvn", "funnel"])
def test_recorders(P, target):
    d = 12
    rec = [P.round_trip, P.index_process, P.log_sum_ratio, P.swap_acceptance_pr, P.traces, P.energy_ac1, P.online]
    kw = dict(target=P.Funnel(d), reference=P.ScaledPrecisionNormalLogPotential(1.0 / 9.0, d)) if target == "funnel" else dict(target=P.toy_mvn_target(d))
    for ext, refred in ((False, False), (True, True)):
        pt = P.PT(P.Inputs(n_chains=6, n_rounds=3, explorer=P.AAPS(step_size=0.4), record=rec, extended_traces=ext, show_report=False, **kw),
                  reference_reduction=refred)
        for _ in range(3):
            assert P.next_round(pt)
            red = P.run_one_round(pt)
            P.adapt(pt, red)
        assert red.index_process.shape == (6, 8)
        tr = red.traces
        assert tr.shape == ((8, 6, d + 1) if ext else (8, d + 1)) and np.all(np.isfinite(tr))
        cor, n, _ = red.energy_ac1
        assert np.all(n[1:] > 0) and np.all(np.isfinite(cor[1:]))
        m, _ = red.swap_acceptance_pr
        assert np.all(np.isfinite(m)) and np.isfinite(P.stepping_stone(pt))


def test_sharded_equals_single_engine(P):
    rec = [P.round_trip, P.index_process, P.log_sum_ratio, P.energy_ac1, P.traces]
    mk = lambda: P.Inputs(target=P.toy_mvn_target(20), n_chains=8, n_rounds=4, explorer=P.AAPS(step_size=0.5, K=3), record=rec, show_report=False)
    one, many = P.PT(mk()), P.PT(mk(), n_shards=4, device_messages=True)
    for _ in range(4):
        assert P.next_round(one) and P.next_round(many)
        ra = P.run_one_round(one); P.adapt(one, ra)
        rb = P.run_one_round(many); P.adapt(many, rb)
        assert np.array_equal(ra.index_process, rb.index_process) and np.array_equal(ra.traces, rb.traces)
        for a, b in zip(ra.energy_ac1 + ra.explorer_acceptance_pr + ra.explorer_n_steps, rb.energy_ac1 + rb.explorer_acceptance_pr + rb.explorer_n_steps):
            assert np.array_equal(a, b, equal_nan=True)
    xa, ca, ga = one.replicas.states(); xb, cb, gb = many.shards.states()
    assert np.array_equal(xa, xb) and np.array_equal(ca, cb) and np.array_equal(ga, gb)


def test_positive_density_error(P):
    pt = P.PT(P.Inputs(target=P.toy_mvn_target(4), n_chains=4, n_rounds=2, explorer=P.AAPS(), show_report=False))
    eng = pt.replicas
    x, chain, rng = eng.states()
    x[chain == 3] = np.inf
    eng.set_states(x, chain, rng)
    with pytest.raises(P.PteError, match="AAPS can only be called on a configuration of positive density"):
        eng.explore(1)
