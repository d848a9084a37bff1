"""AAPS without a GPU: the specification (tests/aaps_ref.py) leaves the target invariant, its range draw is the oracle's, pte_create refuses
what the device does not run -- before any device work -- and the Python surface maps AAPS() onto pte_config."""
import ctypes as C

import numpy as np
import pytest

import aaps_ref as A
import family_cpu as F
import oracle as O
from family_cpu import P  # noqa: F401  (P: the module's fixture)


def _one_transition_sample(prec, eps, K, n=4000, uniform_weights=False, seed=7):
    chain = A.MvnChain(prec)
    sd = 1.0 / np.sqrt(prec)
    X = np.random.default_rng(seed).standard_normal((n, 3)) * sd        # exact draws from the target
    out = np.empty_like(X)
    for i in range(n):
        res = A.transition(X[i], O.OracleRng(seed=1000 + i), chain, eps, K, np.ones(3), uniform_weights=uniform_weights)
        out[i] = res["x"]
    return X, out / sd


def _invariant(Z):
    from scipy import stats
    n = Z.shape[0]
    for j in range(Z.shape[1]):
        z = Z[:, j]
        assert abs(z.mean()) * np.sqrt(n) < 4.0, (j, z.mean())
        assert abs(z.var() - 1.0) / np.sqrt(2.0 / n) < 4.0, (j, z.var())
        assert stats.kstest(z, "norm").pvalue > 1e-3, j


# (precision, step size, K): eps * sqrt(precision) = 0.5 (small energy error) ... 1.9 (close to the leapfrog's stability edge: the energy error
# dominates the weights)
@pytest.mark.parametrize("prec,eps,K", [(1.0, 0.5, 2), (4.0, 0.95, 3), (1.0, 1.9, 2), (0.25, 3.0, 5)])
def test_specification_leaves_the_target_invariant(prec, eps, K):
    X, Z = _one_transition_sample(prec, eps, K)
    assert np.mean(np.any(Z != X * np.sqrt(prec), axis=1)) > 0.5       # it moves
    _invariant(Z)


def test_uniform_weights_break_the_invariance():
    """the sensitivity of the test above: choosing among the candidates uniformly instead of proportionally to pi~ is detected"""
    _, Z = _one_transition_sample(1.0, 1.9, 2, uniform_weights=True)
    with pytest.raises(AssertionError):
        _invariant(Z)


def test_range_draw_is_the_oracles():
    for K in (0, 1, 5, 64):
        a, b = O.OracleRng(seed=11), O.OracleRng(seed=11)
        for _ in range(200):
            assert a.rand_range(0, K) == b.L.po_rand_range(C.byref(b.r), 0, K)
        a2 = O.OracleRng(seed=3)
        res = A.transition(np.zeros(2) + 0.1, a2, A.MvnChain(1.0), 0.3, K, np.ones(2))
        b2 = O.OracleRng(seed=3)
        b2.randn(); b2.randn()
        assert res["Kf"] == b2.rand_range(0, K) and 0 <= res["Kf"] <= K


def test_transition_records():
    """acceptance = 1 - exp(w0 - L), in [0, 1); a stay after a failure records 0; steps count both stopping points"""
    r = O.OracleRng(seed=5)
    res = A.transition(np.array([0.3, -0.2]), r, A.MvnChain(1.0), 0.4, 3, np.ones(2))
    assert not res["failed"] and 0.0 <= res["acc"] < 1.0 and res["steps"] >= 2
    res = A.transition(np.array([0.3, -0.2]), O.OracleRng(seed=5), A.MvnChain(1.0), 0.4, 3, np.ones(2), max_leapfrogs=3)
    assert res["failed"] and res["acc"] == 0.0 and res["steps"] == 3 and np.array_equal(res["x"], [0.3, -0.2])
    # an unstable integrator (eps * sqrt(prec) > 2) blows up to a non-finite point: the state stays
    res = A.transition(np.array([0.3, -0.2]), O.OracleRng(seed=5), A.MvnChain(100.0), 1.0, 3, np.ones(2))
    assert res["failed"] and res["acc"] == 0.0 and np.array_equal(res["x"], [0.3, -0.2])
    with pytest.raises(A.AapsDensityError, match="positive density"):
        A.transition(np.array([np.inf, 0.0]), O.OracleRng(seed=5), A.MvnChain(1.0), 0.4, 3, np.ones(2))


def test_default_config_has_K_5(P):
    from pigeons_amd import _lib
    cfg = _lib.PteConfig()
    assert _lib.load().pte_default_config(C.byref(cfg)) == 0
    assert cfg.aaps_K == 5 and _lib.EXPLORER_AAPS == 6
    assert C.sizeof(_lib.PteConfig) == cfg.struct_size


_MVN = dict(target=0, dim=8, explorer=6)


@pytest.mark.parametrize("kw,msg", [
    (dict(target=3, dim=64), "AAPS is implemented on the scaled-precision MVN and funnel paths only"),       # Ising
    (dict(target=1, dim=1), "AAPS is implemented on the scaled-precision MVN and funnel paths only"),        # TestSwapper
    (dict(dim=0), "AAPS keeps the replica in the registers of one wave, dim must be in 1..512"),
    (dict(dim=513), "AAPS keeps the replica in the registers of one wave, dim must be in 1..512"),
    (dict(target=2, dim=1024), "AAPS keeps the replica in the registers of one wave, dim must be in 1..512"),
    (dict(aaps_K=-1), r"AAPS needs aaps_K in 0\.\.64"),
    (dict(aaps_K=65), r"AAPS needs aaps_K in 0\.\.64"),
    (dict(am_step_size=0.0), "AAPS needs a positive finite step size"),
    (dict(am_step_size=-1.0), "AAPS needs a positive finite step size"),
    (dict(am_step_size=float("inf")), "AAPS needs a positive finite step size"),
    (dict(am_step_size=float("nan")), "AAPS needs a positive finite step size"),
    (dict(explorer2=2), "AAPS is not available as half of a Compose"),
    (dict(explorer=3, explorer2=6), "AAPS is not available as half of a Compose"),
    (dict(debug_kernel=1), "AAPS has one kernel; debug_kernel must be 0"),
    (dict(debug_kernel=0x1000), "AAPS has one kernel; debug_kernel must be 0"),
])
def test_pte_create_refusals(P, kw, msg):
    F.assert_create_refused(P, dict(_MVN, n_chains=4), kw, msg)


def test_accepted_config_reaches_the_device_check(P):
    """a valid AAPS configuration passes validation: without a GPU it fails only where pte_create looks for the device"""
    F.no_device()
    for target, dim in ((0, 1), (0, 512), (2, 2), (2, 512)):
        F.assert_reaches_the_device_check(P, n_chains=4, target=target, dim=dim, explorer=6, aaps_K=64)


def _captured_config(P, explorer, target=None):
    seen = {}

    class Stub:
        def __init__(self, **kw):
            seen.update(kw)

    P.PT(P.Inputs(target=target or P.toy_mvn_target(4), n_chains=4, n_rounds=2, explorer=explorer, show_report=False), engine_factory=Stub)
    return seen


def test_config_mapping(P):
    from pigeons_amd import _lib
    kw = _captured_config(P, P.AAPS())
    assert kw["explorer"] == _lib.EXPLORER_AAPS == 6 and kw["aaps_K"] == 5
    assert kw["am_step_size"] == 1.0 and kw["am_preconditioner"] == 2 and kw["am_p0"] == 1.0 / 3.0 and kw["am_p1"] == 1.0 / 3.0
    assert "explorer2" not in kw
    kw = _captured_config(P, P.AAPS(step_size=0.25, K=9, preconditioner=P.DiagonalPreconditioner()))
    assert kw["explorer"] == 6 and kw["aaps_K"] == 9 and kw["am_step_size"] == 0.25 and kw["am_preconditioner"] == 1
    kw = _captured_config(P, P.AAPS(preconditioner=P.IdentityPreconditioner()))
    assert kw["am_preconditioner"] == 0
    a = P.AAPS()
    assert (a.step_size, a.K, a.estimated_target_std_deviations) == (1.0, 5, None)
    assert isinstance(a.preconditioner, P.MixDiagonalPreconditioner)


@pytest.mark.parametrize("pair", ["first", "second"])
def test_compose_with_aaps_raises(P, pair):
    ex = P.Compose(P.AAPS(), P.SliceSampler()) if pair == "first" else P.Compose(P.AutoMALA(), P.AAPS())
    with pytest.raises(NotImplementedError, match="AAPS"):
        _captured_config(P, ex)


def test_adapt_explorer_keeps_the_step_size_and_sets_the_std(P):
    """adapt_explorer: AAPS as MALA -- the step size stays, the preconditioner's std deviations come from the online variance"""
    calls = []

    class Stub:
        def __init__(self, **kw):
            pass

        def set_explorer_adaptation(self, step, std):
            calls.append((step, None if std is None else np.array(std)))

    pt = P.PT(P.Inputs(target=P.toy_mvn_target(3), n_chains=4, n_rounds=2, explorer=P.AAPS(step_size=0.7, K=2), show_report=False),
              engine_factory=Stub)
    red = P.pt.ReducedRecorders(am_factors=(np.zeros(4), np.zeros(4, dtype=np.int64)), online=(np.zeros(3), np.array([4.0, 1.0, 0.25]), 10))
    P.pt.adapt_explorer(pt, red)
    ex = pt.shared.explorer
    assert isinstance(ex, P.AAPS) and ex.step_size == 0.7 and ex.K == 2
    np.testing.assert_array_equal(ex.estimated_target_std_deviations, [2.0, 1.0, 0.5])
    assert calls[-1][0] == 0.7 and np.array_equal(calls[-1][1], [2.0, 1.0, 0.5])
