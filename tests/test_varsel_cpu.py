"""The variable-selection family without a GPU: pte_create accepts it (a valid configuration reaches the device check) and refuses -- before
any device work -- what the device does not run; the Python and Julia surfaces map SpikeSlabRegression onto pte_config and
pte_set_target_varsel; the NumPy restatement (tests/varsel_ref.py) agrees with the textbook density, its cached-predictor call-back with
its full evaluation, and its enumeration of the 2^d models with brute-force numerical integration."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import family_cpu as F
import oracle as O
import varsel_ref as R
from family_cpu import ROOT, P  # noqa: F401  (P: the module's fixture)


def test_enum_and_export_mirrors(P):
    import __graft_entry__ as g
    from pigeons_amd import _lib
    assert _lib.TARGET_VARIABLE_SELECTION == 7
    assert "pte_set_target_varsel" in _lib.EXPORTS
    assert hasattr(_lib.load(), "pte_set_target_varsel")
    hdr = F.HEADER
    assert "PTE_TARGET_VARIABLE_SELECTION = 7" in hdr and "int pte_set_target_varsel(pte_engine *h, const double *X" in hdr
    jl = F.JULIA
    assert "const TARGET_VARIABLE_SELECTION = Int32(7)\n" in jl
    assert "struct DeviceSpikeSlabRegression" in jl and "device_family(t::DeviceSpikeSlabRegression, inputs)" in jl
    assert ":pte_set_target_varsel" in jl
    assert "SpikeSlabRegression" in P.__dict__
    assert ("pte_varsel.hip", []) in g.UNITS
    params = open(os.path.join(ROOT, "pigeons.jl_amd", "csrc", "pte_automala_params.hpp")).read()
    assert "X(varsel)" in params                       # pte_set_rng_policy reaches the unit's copy of the policy word (the Bool draw reads it)


@pytest.mark.parametrize("dim", [2, 8, 64, 130, 512])
def test_accepted_config_reaches_the_device_check(P, dim):
    """fails on the code before the family existed ("target 7 has no device log-potential"): a valid configuration now passes validation"""
    F.no_device()
    from pigeons_amd import _lib
    F.assert_reaches_the_device_check(P, n_chains=4, target=7, dim=dim, explorer=2, target_params=[1.0])
    for dk in (0x1000, 0x2000):                         # the scan-loop flags (PTE_KERNEL_FLAG_BITS) are allowed
        if dk & _lib.KERNEL_FLAG_BITS:
            F.assert_reaches_the_device_check(P, n_chains=4, target=7, dim=dim, explorer=2, debug_kernel=dk)


_VS = dict(target=7, dim=8, explorer=2, n_chains=4)


@pytest.mark.parametrize("kw,msg", [
    (dict(explorer=3), "variable-selection path is explored by SliceSampler only"),                  # AutoMALA
    (dict(explorer=5), "variable-selection path is explored by SliceSampler only"),                  # MALA
    (dict(explorer=1), "variable-selection path is explored by SliceSampler only"),                  # ToyExplorer
    (dict(explorer=4), "variable-selection path is explored by SliceSampler only"),                  # IsingMetropolis
    (dict(explorer=0), "variable-selection path is explored by SliceSampler only"),                  # none
    (dict(explorer=2, explorer2=3), "variable-selection path is explored by SliceSampler only"),     # Compose(SliceSampler, AutoMALA)
    (dict(explorer=5, explorer2=2), "variable-selection path is explored by SliceSampler only"),     # Compose(MALA, SliceSampler)
    (dict(explorer=2, explorer2=2), "variable-selection path is explored by SliceSampler only"),
    (dict(explorer=6), "AAPS is implemented on the scaled-precision MVN and funnel paths only"),      # AAPS keeps its refusal
    (dict(dim=7), r"dim = 2 d must be even \(got 7\)"),
    (dict(dim=1), r"dim = 2 d must be even \(got 1\)"),
    (dict(dim=0), r"d = dim / 2 must be in 1\.\.256"),
    (dict(dim=514), r"d = dim / 2 must be in 1\.\.256"),
    (dict(dim=4096), r"d = dim / 2 must be in 1\.\.256"),
    (dict(debug_kernel=1), "debug_kernel 1 is not available on the variable-selection path"),
    (dict(debug_kernel=8), "debug_kernel 8 is not available on the variable-selection path"),
    (dict(n_chains_variational=4), "two-leg tempering"),
])
def test_pte_create_refusals(P, kw, msg):
    F.assert_create_refused(P, _VS, kw, msg)


def test_the_setters_refusals_are_in_the_library():
    """pte_set_target_varsel needs an engine, so a machine without a device cannot reach these; their text is pinned here and they are
    raised on the device in tests/test_gpu_varsel.py"""
    src = open(os.path.join(ROOT, "pigeons.jl_amd", "csrc", "pte.hip")).read()
    for msg in ("pte_set_target_varsel: inclusion_prob must be in (0, 1)", "pte_set_target_varsel: X[%lld][%lld] must be finite",
                "pte_set_target_varsel: y[%lld] must be finite", "pte_set_target_varsel: the device holds 1..4096 observations",
                "pte_set_target_varsel: n_obs * d must be <= 131072", "pte_set_target_varsel: this engine holds dim / 2 = %lld columns",
                "only the interpolated (funnel) path has a replaceable reference"):
        assert msg in src, msg


def _data(n=20, d=3, lik="bernoulli_logit", seed=1):
    g = np.random.default_rng(seed)
    X = g.normal(0.0, 1.0, (n, d))
    y = (g.uniform(size=n) < 0.4).astype(float) if lik == "bernoulli_logit" else g.normal(0.0, 2.0, n)
    return X, y


def _captured(P, target, **kw):
    return F.captured(P, target, ref_dim=target.n_columns, **kw)             # the reference has d coordinates, not 2 d


def test_python_mapping(P):
    from pigeons_amd import _lib
    X, y = _data(20, 3, "normal_identity")
    t = P.SpikeSlabRegression(X, y, likelihood="normal_identity", noise_sd=0.7, inclusion_prob=0.3)
    kw = _captured(P, t)
    assert kw["target"] == _lib.TARGET_VARIABLE_SELECTION and kw["dim"] == 6 and list(kw["target_params"]) == [0.5]
    assert kw["explorer"] == _lib.EXPLORER_SLICE and "explorer2" not in kw          # default explorer: SliceSampler (target.jl:20)
    (lik, Xs, ys, sd, pi), = kw["set_target_varsel"]                                # set after create, once per engine
    assert lik == _lib.GLM_NORMAL_IDENTITY and sd == 0.7 and pi == 0.3
    np.testing.assert_array_equal(Xs, X); np.testing.assert_array_equal(ys, y)
    kw = _captured(P, P.SpikeSlabRegression(*_data(20, 3)), explorer=P.SliceSampler(n_passes=2))
    assert kw["slice_n_passes"] == 2 and kw["set_target_varsel"][0][0] == _lib.GLM_BERNOULLI_LOGIT and kw["set_target_varsel"][0][4] == 0.5
    for ex in (P.AutoMALA(), P.MALA(), P.AAPS(), P.Compose(P.SliceSampler(), P.AutoMALA()), P.Compose(P.SliceSampler(), P.SliceSampler())):
        with pytest.raises(NotImplementedError, match="explored by SliceSampler only"):
            _captured(P, t, explorer=ex)
    F.assert_reference_refusals(P, t, wrong_dim=6, ref_dim=t.n_columns)             # (a reference of 2 d coordinates is the wrong one)


def test_every_shard_gets_the_data(P):
    X, y = _data(10, 3)
    F.assert_every_shard_gets_the_data(P, P.SpikeSlabRegression(X, y), P.ScaledPrecisionNormalLogPotential(1.0, 3), N=4, d=6,
                                       setter="set_target_varsel")


@pytest.mark.parametrize("args,kw,msg", [
    ((np.zeros((3, 2)), np.zeros(3)), dict(likelihood="poisson_log"), "likelihood must be"),
    ((np.zeros(3), np.zeros(3)), {}, "X must be an n x d array"),
    ((np.zeros((4097, 1)), np.zeros(4097)), {}, r"1\.\.4096 observations"),
    ((np.zeros((2, 257)), np.zeros(2)), {}, r"d must be in 1\.\.256"),
    ((np.zeros((1025, 256)), np.zeros(1025)), {}, "n \\* d must be <= 131072"),
    ((np.zeros((3, 2)), np.zeros(4)), {}, "y must be a vector of the n = 3 observations"),
    (([[0.0, np.nan], [0.0, 0.0]], [0.0, 1.0]), {}, "X must be finite"),
    ((np.zeros((2, 2)), [0.0, np.inf]), dict(likelihood="normal_identity"), "y must be finite"),
    ((np.zeros((2, 2)), [0.0, 0.5]), {}, r"y in \{0, 1\}"),
    ((np.zeros((2, 2)), [0.0, 0.5]), dict(likelihood="normal_identity", noise_sd=0.0), "noise_sd must be positive and finite"),
    ((np.zeros((2, 2)), [0.0, 1.0]), dict(inclusion_prob=0.0), r"inclusion_prob must be in \(0, 1\)"),
    ((np.zeros((2, 2)), [0.0, 1.0]), dict(inclusion_prob=1.0), r"inclusion_prob must be in \(0, 1\)"),
    ((np.zeros((2, 2)), [0.0, 1.0]), dict(inclusion_prob=-0.1), r"inclusion_prob must be in \(0, 1\)"),
    ((np.zeros((2, 2)), [0.0, 1.0]), dict(inclusion_prob=np.nan), r"inclusion_prob must be in \(0, 1\)"),
])
def test_python_validation(P, args, kw, msg):
    with pytest.raises(ValueError, match=msg):
        P.SpikeSlabRegression(*args, **kw)


def test_spike_slab_surface(P):
    t = P.SpikeSlabRegression([[1.0, 2.0], [3.0, 4.0], [5.0, 6.0]], [0, 1, 1])
    assert t.n_obs == 3 and t.n_columns == 2 and t.dim == 4 and t.likelihood == "bernoulli_logit" and t.inclusion_prob == 0.5
    assert P.SpikeSlabRegression(np.ones((4096, 32)), np.zeros(4096)).n_obs == 4096           # the limits themselves are accepted
    assert P.SpikeSlabRegression(np.ones((512, 256)), np.zeros(512), likelihood="normal_identity", noise_sd=2.0).dim == 512
    assert math.isclose(t.evidence_offset(0.5), -math.log(2 * math.pi / 0.5) - 2 * math.log(2.0), rel_tol=1e-15)
    assert math.isclose(t.evidence_offset(0.5), R.VarSel(t.X, t.y, "bernoulli_logit", 1.0, 0.5).evidence_offset(), rel_tol=1e-15)
    assert "evidence_offset" in P.SpikeSlabRegression.__doc__ and "d log 2" in P.SpikeSlabRegression.__doc__


def test_set_target_varsel_is_bound(P):
    from pigeons_amd import _lib
    F.assert_null_engine_refused(_lib.load().pte_set_target_varsel, (None, None, None, 2, 1, 0, 1.0, 0.5),
                                 {3: C.c_int64, 4: C.c_int64, 5: C.c_int32, 6: C.c_double, 7: C.c_double})


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lik", ["bernoulli_logit", "normal_identity"])
def test_restatement_against_the_textbook_density(lik):
    n, d, p, sd, pi = 100, 4, 0.7, 1.3, 0.3
    X, y = _data(n, d, lik, seed=5)
    vs = R.VarSel(X, y, lik, sd, p, pi)
    g = np.random.default_rng(6)
    theta, gamma = g.normal(0.0, 1.0, d), np.array([1.0, 0.0, 1.0, 1.0])
    eta = X @ (gamma * theta)
    if lik == "bernoulli_logit":
        ll = np.sum(y * np.log(1 / (1 + np.exp(-eta))) + (1 - y) * np.log(1 / (1 + np.exp(eta))))
    else:
        ll = np.sum(-0.5 * np.log(2 * np.pi * sd ** 2) - (y - eta) ** 2 / (2 * sd ** 2))
    prior = np.sum(-0.5 * np.log(2 * np.pi / p) - 0.5 * p * theta ** 2) + 3 * math.log(pi) + math.log(1 - pi)
    assert math.isclose(vs.lp(np.concatenate([theta, gamma])), prior + ll, rel_tol=1e-12)


@pytest.mark.parametrize("lik,beta", [("bernoulli_logit", 0.4), ("normal_identity", 1.0), ("normal_identity", 0.0)])
def test_cached_predictor_follows_the_full_evaluation(lik, beta):
    """one SliceSampler step of the oracle on the cached-predictor call-back: every value it returns is the full evaluation's up to the
    rounding of the incremental eta, the walk ends where the call-back's committed state says, and the Bool coordinates stay Bool"""
    n, d, p = 70, 5, 0.6
    X, y = _data(n, d, lik, seed=9)
    vs = R.VarSel(X, y, lik, 0.9, p, 0.35)
    ch = R.VarSelChain(vs, beta, p)
    worst = [0.0]

    def lp(state):
        a, b = ch.path_lp(state), R.VarSelChain(vs, beta, p).lp_full(state)
        worst[0] = max(worst[0], abs(a - b) / max(1.0, abs(b)))
        return a
    kinds = np.array([O.COORD_FLOAT64] * d + [O.COORD_BOOL] * d, dtype=np.int32)
    g = np.random.default_rng(3)
    state = np.concatenate([g.normal(0.0, 1.0, d), (g.uniform(size=d) < 0.5).astype(float)])
    start = state.copy()
    s = O.MixedSliceSampler(lp, kinds)
    s.step(O.OracleRng(seed=11), state)
    assert worst[0] < 1e-12 and s.n_evals > 6 * d
    assert set(np.unique(state[d:])) <= {0.0, 1.0} and not np.array_equal(state[:d], start[:d])
    done = np.arange(2 * d) != ch.cur                 # every coordinate but the last one visited has been committed
    np.testing.assert_array_equal(ch.state[done], state[done])
    assert s.stats.steps_n == 2 * d * 3               # the Float64 coordinates record two counts per visit, the Bool ones nothing


def test_enumeration_against_numerical_integration():
    """d = 2: inclusion probabilities, E[b_j] and the evidence from the 4 models in closed form against the integral of exp(target) over
    theta on a grid, for each gamma (an excluded theta integrates over its prior alone)"""
    n, p, sd, pi = 15, 0.8, 0.9, 0.3
    X, y = _data(n, 2, "normal_identity", seed=11)
    vs = R.VarSel(X, y, "normal_identity", sd, p, pi)
    incl, b, log_ev = vs.exact()
    a = np.linspace(-12.0, 12.0, 1201)
    A, B = np.meshgrid(a, a, indexing="ij")
    T = np.stack([A.ravel(), B.ravel()], axis=1)
    h2 = (a[1] - a[0]) ** 2
    Z, Zb = {}, {}
    for g in ((0, 0), (0, 1), (1, 0), (1, 1)):
        gv = np.array(g, dtype=np.float64)
        eta = (T * gv) @ X.T
        logf = (-np.log(2 * np.pi / p) - 0.5 * p * (T ** 2).sum(1)) + gv.sum() * math.log(pi) + (2 - gv.sum()) * math.log(1 - pi) \
            + np.sum(-0.5 * np.log(2 * np.pi * sd ** 2) - (y - eta) ** 2 / (2 * sd ** 2), axis=1)
        f = np.exp(logf)
        Z[g] = f.sum() * h2
        Zb[g] = (f[:, None] * T * gv).sum(0) * h2
        k = 400 * 1201 + 700                          # the restatement's target density is the same integrand
        assert math.isclose(vs.lp(np.concatenate([T[k], gv])), logf[k], rel_tol=1e-12)
    tot = sum(Z.values())
    assert math.isclose(log_ev, math.log(tot), rel_tol=0, abs_tol=1e-8)
    np.testing.assert_allclose(incl, [(Z[1, 0] + Z[1, 1]) / tot, (Z[0, 1] + Z[1, 1]) / tot], rtol=1e-8)
    np.testing.assert_allclose(b, sum(Zb.values()) / tot, rtol=1e-7, atol=1e-10)
    assert abs(incl[0] - pi) > 1e-3 or abs(incl[1] - pi) > 1e-3
