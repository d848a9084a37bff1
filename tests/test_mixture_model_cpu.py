"""The mixture-model-posterior family without a GPU: pte_create accepts it (a valid configuration reaches the device check) and refuses --
before any device work -- what the device does not run; the Python and Julia surfaces map MixtureModelPosterior onto pte_config and
pte_set_target_mixture_model; the NumPy restatement (tests/mixture_model_ref.py) has the right gradient, agrees with the textbook density, is
symmetric under relabelling, keeps its -inf / NaN rules, and prior Monte Carlo gives the evidence the GPU test compares with."""
import ctypes as C
import itertools
import math

import numpy as np
import pytest

import family_cpu as F
import mixture_model_ref as R
from family_cpu import P  # noqa: F401  (P: the module's fixture)

Y8 = [-1.6, -1.3, -1.0, -0.9, 0.8, 1.1, 1.3, 1.7]


def test_enum_and_export_mirrors(P):
    from pigeons_amd import _lib
    assert _lib.TARGET_MIXTURE_MODEL == 6
    assert "pte_set_target_mixture_model" in _lib.EXPORTS
    assert hasattr(_lib.load(), "pte_set_target_mixture_model")
    hdr = F.HEADER
    assert "PTE_TARGET_MIXTURE_MODEL        = 6" in hdr
    assert "int pte_set_target_mixture_model(pte_engine *h, int64_t n_obs, const double *y" in hdr
    jl = F.JULIA
    assert "const TARGET_MIXTURE_MODEL = Int32(6)\n" in jl
    assert "struct DeviceMixtureModelPosterior" in jl and "device_family(t::DeviceMixtureModelPosterior, inputs)" in jl
    assert ":pte_set_target_mixture_model" in jl
    assert "MixtureModelPosterior" in P.__dict__
    import __graft_entry__ as g
    assert ("pte_mixture_model.hip", []) in g.UNITS


@pytest.mark.parametrize("explorer,explorer2,dim", [(2, 0, 3), (3, 0, 6), (5, 0, 9), (2, 3, 24), (3, 2, 12), (5, 2, 15), (2, 0, 18), (3, 0, 21)])
def test_accepted_config_reaches_the_device_check(P, explorer, explorer2, dim):
    """fails on the code before the family existed ("target 6 has no device log-potential"): a valid configuration now passes validation"""
    F.no_device()
    from pigeons_amd import _lib
    F.assert_reaches_the_device_check(P, n_chains=4, target=6, dim=dim, explorer=explorer, explorer2=explorer2, target_params=[1.0])
    for dk in (0x1000, 0x2000):                         # the scan-loop flags (PTE_KERNEL_FLAG_BITS) are allowed
        if dk & _lib.KERNEL_FLAG_BITS:
            F.assert_reaches_the_device_check(P, n_chains=4, target=6, dim=dim, explorer=explorer, explorer2=explorer2, debug_kernel=dk)


_MM = dict(target=6, dim=6, explorer=2, n_chains=4)
_DIM = r"mixture-model path holds theta = \[mu, s, alpha\] of 1\.\.8 components, dim must be in \{3, 6, \.\.\., 24\}"


@pytest.mark.parametrize("kw,msg", [
    (dict(dim=0), _DIM), (dict(dim=1), _DIM), (dict(dim=4), _DIM), (dict(dim=25), _DIM), (dict(dim=27), _DIM), (dict(dim=-3), _DIM),
    (dict(dim=513, explorer=3), _DIM),
    (dict(explorer=1), "mixture-model path is implemented for SliceSampler / AutoMALA / MALA"),       # ToyExplorer
    (dict(explorer=4), "mixture-model path is implemented for SliceSampler / AutoMALA / MALA"),       # IsingMetropolis
    (dict(explorer=0), "mixture-model path is implemented for SliceSampler / AutoMALA / MALA"),       # none
    (dict(explorer=2, explorer2=1), "mixture-model path is implemented for SliceSampler / AutoMALA / MALA"),
    (dict(explorer=6), "AAPS is implemented on the scaled-precision MVN and funnel paths only"),       # AAPS keeps its refusal
    (dict(debug_kernel=1), "debug_kernel 1 is not available on the mixture-model path"),
    (dict(debug_kernel=8), "debug_kernel 8 is not available on the mixture-model path"),
    (dict(n_chains_variational=4), "two-leg tempering .* is not available on the mixture-model path"),
])
def test_pte_create_refusals(P, kw, msg):
    F.assert_create_refused(P, _MM, kw, msg)


def test_python_mapping(P):
    from pigeons_amd import _lib
    t = P.MixtureModelPosterior(Y8, 2)
    kw = F.captured(P, t)
    assert kw["target"] == _lib.TARGET_MIXTURE_MODEL and kw["dim"] == 6 and list(kw["target_params"]) == [0.5]
    assert kw["explorer"] == _lib.EXPLORER_SLICE                      # default explorer: SliceSampler (target.jl:20)
    (ys,), = kw["set_target_mixture_model"]                           # set after create, once per engine
    np.testing.assert_array_equal(ys, np.array(Y8))
    kw = F.captured(P, P.MixtureModelPosterior(Y8, 3), explorer=P.AutoMALA())
    assert kw["explorer"] == _lib.EXPLORER_AUTOMALA and kw["dim"] == 9
    kw = F.captured(P, t, explorer=P.Compose(P.SliceSampler(), P.MALA()))
    assert kw["explorer"] == _lib.EXPLORER_SLICE and kw["explorer2"] == _lib.EXPLORER_MALA
    F.assert_reference_refusals(P, t, wrong_dim=5)


def test_every_shard_gets_the_data(P):
    F.assert_every_shard_gets_the_data(P, P.MixtureModelPosterior(Y8, 2), P.ScaledPrecisionNormalLogPotential(1.0, 6), N=4, d=6,
                                       setter="set_target_mixture_model")


@pytest.mark.parametrize("args,msg", [
    ((Y8, 0), r"1\.\.8 components"),
    ((Y8, 9), r"1\.\.8 components"),
    ((Y8, 2.5), r"1\.\.8 components"),
    ((np.zeros((4, 2)), 2), "y must be a vector"),
    ((3.0, 2), "y must be a vector"),
    ((np.zeros(0), 2), r"1\.\.65536 observations"),
    ((np.zeros(65537), 2), r"1\.\.65536 observations"),
    (([0.0, 1.0, np.nan], 2), r"y\[2\] must be finite"),
    (([np.inf, 1.0, 0.0], 2), r"y\[0\] must be finite"),
])
def test_python_validation(P, args, msg):
    with pytest.raises(ValueError, match=msg):
        P.MixtureModelPosterior(*args)


def test_mixture_model_posterior_surface(P):
    t = P.MixtureModelPosterior(Y8, 2)
    assert t.n_obs == 8 and t.dim == 6 and t.n_components == 2 and t.y.dtype == np.float64
    assert P.MixtureModelPosterior(np.zeros(65536), 8).dim == 24                       # the limits themselves are accepted
    assert P.MixtureModelPosterior([0.5], 1).dim == 3
    doc = P.MixtureModelPosterior.__doc__
    assert "stepping_stone(pt) + (d/2) log(2 pi / p)" in doc and "softmax(alpha)" in doc


def test_set_target_mixture_model_is_bound(P):
    from pigeons_amd import _lib
    F.assert_null_engine_refused(_lib.load().pte_set_target_mixture_model, (None, 2, None), {1: C.c_int64}, n_args=3)


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------
def _y(n, seed):
    g = np.random.default_rng(seed)
    return np.where(g.uniform(size=n) < 0.4, g.normal(-1.0, 0.4, n), g.normal(0.8, 0.7, n))


@pytest.mark.parametrize("n,K", [(1, 1), (70, 2), (130, 3), (200, 8)])
def test_gradient_against_central_differences(n, K):
    model = R.MixtureModel(_y(n, n + K), K, 0.6)
    g = np.random.default_rng(n * 10 + K)
    for beta in (1.0, 0.3):
        ch = R.MixtureModelChain(model, beta, 0.6)
        for _ in range(3):
            x = g.normal(0.0, 0.7, 3 * K)
            _, grad = ch.lp_grad(x)
            h = 1e-5
            num = np.array([(ch.lp_grad(x + h * e)[0] - ch.lp_grad(x - h * e)[0]) / (2 * h) for e in np.eye(3 * K)])
            np.testing.assert_allclose(grad, num, rtol=1e-6, atol=1e-6)
            assert math.isclose(ch.path_lp(x), ch.lp_grad(x)[0], rel_tol=1e-14, abs_tol=1e-14)


def _textbook(y, theta, K, p):
    """log of N(theta; 0, I / p) prod_i sum_k w_k N(y_i; mu_k, sigma_k^2), formed directly"""
    mu, sd, w = theta[:K], np.exp(theta[K:2 * K]), np.exp(theta[2 * K:]) / np.exp(theta[2 * K:]).sum()
    dens = (w / (sd * math.sqrt(2 * math.pi)) * np.exp(-0.5 * ((y[:, None] - mu) / sd) ** 2)).sum(1)
    return np.sum(-0.5 * np.log(2 * np.pi / p) - 0.5 * p * theta ** 2) + np.log(dens).sum()


@pytest.mark.parametrize("n,K", [(100, 1), (100, 3), (333, 8)])
def test_restatement_against_the_textbook_density(n, K):
    """the prior N(0, I / p) normalised, the likelihood by its textbook formula (the ragged last block of observations contributes nothing)"""
    p = 0.7
    y = _y(n, 5)
    model = R.MixtureModel(y, K, p)
    theta = np.random.default_rng(6).normal(0.0, 0.5, 3 * K)
    assert math.isclose(model.lp(theta), _textbook(y, theta, K, p), rel_tol=1e-12)
    assert math.isclose(model.lp(theta), model.lp_grad(theta)[0], rel_tol=0, abs_tol=0)
    assert math.isclose(model.log_likelihood(theta) + (-0.5 * p * (theta ** 2).sum() + model.c_prior), model.lp(theta), rel_tol=1e-12)


@pytest.mark.parametrize("K", [2, 3, 4])
def test_relabelling_leaves_the_density_unchanged(K):
    y = _y(150, 9)
    model = R.MixtureModel(y, K, 0.5)
    theta = np.random.default_rng(K).normal(0.0, 0.8, 3 * K)
    lp0, g0 = model.lp_grad(theta)
    for perm in itertools.permutations(range(K)):
        idx = np.concatenate([np.array(perm), K + np.array(perm), 2 * K + np.array(perm)])
        lp1, g1 = model.lp_grad(theta[idx])
        assert math.isclose(lp1, lp0, rel_tol=1e-13), (perm, lp1, lp0)
        np.testing.assert_allclose(g1, g0[idx], rtol=1e-9, atol=1e-9)


def test_minus_infinity_and_nan_rules_at_an_extreme_scale():
    """s_k = -800: e_k = exp(800) overflows.  An observation equal to mu_k gives z = 0 x inf = NaN, which counts as a_ik = -inf; with every
    component at -inf, l_i = -inf and every r_ik = 0.  One finite component keeps l_i finite and takes all the responsibility."""
    y = np.array([0.25, -1.0, 2.0])
    one = R.MixtureModel(y, 1, 1.0)
    th = np.array([0.25, -800.0, 0.0])
    l, r, z = one.terms(th)
    assert np.isnan(z[0, 0]) and l[0] == -np.inf and np.all(l == -np.inf) and np.all(r == 0.0)
    assert one.lp(th) == -np.inf and one.lp_grad(th)[0] == -np.inf
    two = R.MixtureModel(y, 2, 1.0)
    th = np.array([0.25, 0.5, -800.0, 0.0, 0.0, 0.0])
    l, r, _ = two.terms(th)
    assert np.all(np.isfinite(l)) and np.all(r[:, 0] == 0.0) and np.all(r[:, 1] == 1.0)
    assert math.isfinite(two.lp(th))
    want = np.log(0.5) - 0.5 * (y - 0.5) ** 2
    np.testing.assert_allclose(l, want, rtol=1e-15)
    # s_k = +800: e_k = 0, z = 0, a_ik = log w_k - 800: finite, no special case
    assert math.isfinite(one.lp(np.array([0.0, 800.0, 0.0])))


def test_padded_observations_contribute_nothing():
    """n = 65 (one observation in the second block of 64) against n = 64 plus that observation's own term"""
    y = _y(65, 3)
    th = np.random.default_rng(1).normal(0.0, 0.5, 6)
    a, b = R.MixtureModel(y, 2, 1.0), R.MixtureModel(y[:64], 2, 1.0)
    la, _, _ = a.terms(th)
    assert math.isclose(a.lp(th) - a.c_obs, (b.lp(th) - b.c_obs) + la[64], rel_tol=1e-13)


def test_prior_monte_carlo_evidence():
    """K = 2, p = 1 on the eight observations of the GPU evidence test: log p(y) = -14.417 +- 0.0044 from 4e6 prior draws (default_rng(1));
    recomputed here with 1e6 draws, whose own standard error must be at most 0.01, and the two must agree within 4 combined errors"""
    est, se = R.prior_monte_carlo_log_evidence(Y8, 2, 1.0, 1000000, 1)
    assert se <= 0.01, se
    assert abs(est - (-14.417)) <= 4 * math.sqrt(se ** 2 + 0.0044 ** 2), (est, se)
    model = R.MixtureModel(Y8, 2, 1.0)
    assert math.isclose(model.evidence_offset(), -3.0 * math.log(2 * math.pi), rel_tol=1e-15)
