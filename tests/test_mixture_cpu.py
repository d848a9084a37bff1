"""The Gaussian-mixture family without a GPU: pte_create accepts it (a valid configuration reaches the device check) and refuses -- before
any device work -- what the device does not run; the Python and Julia surfaces map GaussianMixture onto pte_config and pte_set_target_mixture;
the NumPy restatement (tests/mixture_ref.py) has the right gradient, is normalised, and gives the path's known log normalising constant."""
import ctypes as C
import math

import numpy as np
import pytest

import family_cpu as F
import mixture_ref as R
from family_cpu import P  # noqa: F401  (P: the module's fixture)


def test_enum_and_export_mirrors(P):
    from pigeons_amd import _lib
    assert _lib.TARGET_GAUSSIAN_MIXTURE == 4
    assert "pte_set_target_mixture" in _lib.EXPORTS
    assert hasattr(_lib.load(), "pte_set_target_mixture")
    hdr = F.HEADER
    assert "PTE_TARGET_GAUSSIAN_MIXTURE     = 4" in hdr and "int pte_set_target_mixture(" in hdr
    jl = F.JULIA
    assert "TARGET_GAUSSIAN_MIXTURE = Int32(0), Int32(1), Int32(2), Int32(3), Int32(4)" in jl
    assert "struct DeviceGaussianMixture" in jl and "device_family(t::DeviceGaussianMixture, inputs)" in jl
    assert ":pte_set_target_mixture" in jl
    assert "GaussianMixture" in P.__dict__


@pytest.mark.parametrize("explorer,explorer2,dim", [(2, 0, 1), (3, 0, 8), (5, 0, 100), (2, 3, 512), (3, 2, 64), (5, 2, 7)])
def test_accepted_config_reaches_the_device_check(P, explorer, explorer2, dim):
    """fails on the code before the family existed ("target 4 has no device log-potential"): a valid configuration now passes validation"""
    F.no_device()
    F.assert_reaches_the_device_check(P, n_chains=4, target=4, dim=dim, explorer=explorer, explorer2=explorer2, target_params=[1.0])
    for dk in (0x1000, 0x2000):                         # the scan-loop flags (PTE_KERNEL_FLAG_BITS) are allowed
        from pigeons_amd import _lib
        if dk & _lib.KERNEL_FLAG_BITS:
            F.assert_reaches_the_device_check(P, n_chains=4, target=4, dim=dim, explorer=explorer, explorer2=explorer2, debug_kernel=dk)


_MIX = dict(target=4, dim=8, explorer=2, n_chains=4)


@pytest.mark.parametrize("kw,msg", [
    (dict(dim=0), r"Gaussian-mixture path keeps the replica in the registers of one wave, dim must be in 1\.\.512"),
    (dict(dim=513), r"Gaussian-mixture path keeps the replica in the registers of one wave, dim must be in 1\.\.512"),
    (dict(dim=1024, explorer=3), r"dim must be in 1\.\.512"),
    (dict(explorer=1), "Gaussian-mixture path is implemented for SliceSampler / AutoMALA / MALA"),       # ToyExplorer
    (dict(explorer=4), "Gaussian-mixture path is implemented for SliceSampler / AutoMALA / MALA"),       # IsingMetropolis
    (dict(explorer=0), "Gaussian-mixture path is implemented for SliceSampler / AutoMALA / MALA"),       # none
    (dict(explorer=2, explorer2=1), "Gaussian-mixture path is implemented for SliceSampler / AutoMALA / MALA"),
    (dict(explorer=6), "AAPS is implemented on the scaled-precision MVN and funnel paths only"),          # AAPS keeps its refusal
    (dict(debug_kernel=1), "debug_kernel 1 is not available on the Gaussian-mixture path"),
    (dict(debug_kernel=8), "debug_kernel 8 is not available on the Gaussian-mixture path"),
    (dict(n_chains_variational=4), "two-leg tempering"),
])
def test_pte_create_refusals(P, kw, msg):
    F.assert_create_refused(P, _MIX, kw, msg)


def _mix(d=3, K=2):
    g = np.random.default_rng(1)
    return P_GM(np.arange(1.0, K + 1.0), g.normal(0, 2, (K, d)), g.uniform(0.5, 1.5, (K, d)))


def P_GM(w, m, s):
    import pigeons_amd
    return pigeons_amd.GaussianMixture(w, m, s)


def test_python_mapping(P):
    from pigeons_amd import _lib
    t = _mix(d=3, K=2)
    kw = F.captured(P, t)
    assert kw["target"] == _lib.TARGET_GAUSSIAN_MIXTURE and kw["dim"] == 3 and list(kw["target_params"]) == [0.5]
    assert kw["explorer"] == _lib.EXPLORER_SLICE                      # default explorer: SliceSampler (target.jl:20)
    (w, m, s), = kw["set_target_mixture"]                            # set after create, once per engine
    np.testing.assert_array_equal(w, t.weights); np.testing.assert_array_equal(m, t.means); np.testing.assert_array_equal(s, t.std_devs)
    kw = F.captured(P, t, explorer=P.AutoMALA())
    assert kw["explorer"] == _lib.EXPLORER_AUTOMALA
    kw = F.captured(P, t, explorer=P.Compose(P.SliceSampler(), P.MALA()))
    assert kw["explorer"] == _lib.EXPLORER_SLICE and kw["explorer2"] == _lib.EXPLORER_MALA
    F.assert_reference_refusals(P, t, wrong_dim=4)


def test_every_shard_gets_the_mixture(P):
    F.assert_every_shard_gets_the_data(P, _mix(d=3, K=3), P.ScaledPrecisionNormalLogPotential(1.0, 3), N=4, d=3, setter="set_target_mixture")


@pytest.mark.parametrize("args,msg", [
    (([], np.zeros((0, 2)), np.zeros((0, 2))), "1..8 components"),
    ((np.ones(9), np.zeros((9, 2)), np.ones((9, 2))), "1..8 components"),
    (([1.0, 2.0], np.zeros((2, 2)), np.ones((3, 2))), "K x dim"),
    (([1.0, 2.0], np.zeros(2), np.ones(2)), "K x dim"),
    (([1.0, 0.0], np.zeros((2, 2)), np.ones((2, 2))), "weights must be positive and finite"),
    (([1.0, -1.0], np.zeros((2, 2)), np.ones((2, 2))), "weights must be positive and finite"),
    (([1.0, np.inf], np.zeros((2, 2)), np.ones((2, 2))), "weights must be positive and finite"),
    (([1.0, np.nan], np.zeros((2, 2)), np.ones((2, 2))), "weights must be positive and finite"),
    (([1.0, 1.0], np.zeros((2, 2)), [[1.0, 0.0], [1.0, 1.0]]), "std_devs must be positive and finite"),
    (([1.0, 1.0], np.zeros((2, 2)), [[1.0, np.inf], [1.0, 1.0]]), "std_devs must be positive and finite"),
    (([1.0, 1.0], [[0.0, np.nan], [0.0, 0.0]], np.ones((2, 2))), "means must be finite"),
    (([1.0, 1.0], [[0.0, -np.inf], [0.0, 0.0]], np.ones((2, 2))), "means must be finite"),
])
def test_python_validation(P, args, msg):
    with pytest.raises(ValueError, match=msg):
        P.GaussianMixture(*args)


def test_gaussian_mixture_surface(P):
    t = P.GaussianMixture([1, 3], [[0.0, 1.0, 2.0], [3.0, 4.0, 5.0]], [[1, 1, 1], [2, 2, 2]])
    assert t.n_components == 2 and t.dim == 3 and t.weights.dtype == np.float64
    assert "MixtureModel" in P.GaussianMixture.__doc__ and "Diagonal" in P.GaussianMixture.__doc__
    ref = P.ScaledPrecisionNormalLogPotential(2.5, 3)
    assert P.analytic_lognormalization(t, ref) == R.analytic_lognormalization(3, 2.5)
    assert math.isclose(P.analytic_lognormalization(t, ref), -1.5 * math.log(2.0 * math.pi / 2.5), rel_tol=1e-15)
    with pytest.raises(ValueError, match="reference"):
        P.analytic_lognormalization(t)


def test_set_target_mixture_is_bound(P):
    from pigeons_amd import _lib
    F.assert_null_engine_refused(_lib.load().pte_set_target_mixture, (None, 2, None, None, None), {1: C.c_int64})


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------
def _ref_mix(K=3, d=5, seed=3):
    g = np.random.default_rng(seed)
    return R.Mixture(g.uniform(0.2, 2.0, K), g.normal(0.0, 2.0, (K, d)), g.uniform(0.4, 1.6, (K, d)))


def test_tree_sum_is_the_fixed_tree():
    v = np.random.default_rng(0).standard_normal(13)
    a = np.zeros(16); a[:13] = v
    l1 = a[0::2] + a[1::2]; l2 = l1[0::2] + l1[1::2]; l3 = l2[0::2] + l2[1::2]
    assert R.tree_sum(v) == l3[0] + l3[1]
    assert R.tree_sum([2.5]) == 2.5


@pytest.mark.parametrize("K,d", [(1, 1), (2, 4), (3, 5), (8, 9)])
def test_gradient_against_central_differences(K, d):
    mix = _ref_mix(K, d)
    g = np.random.default_rng(K * 10 + d)
    for beta in (1.0, 0.3):
        ch = R.MixtureChain(mix, beta, 0.7)
        for _ in range(3):
            x = g.normal(0.0, 2.0, d)
            _, grad = ch.lp_grad(x)
            h = 1e-5
            num = np.array([(ch.lp_grad(x + h * e)[0] - ch.lp_grad(x - h * e)[0]) / (2 * h) for e in np.eye(d)])
            np.testing.assert_allclose(grad, num, rtol=1e-6, atol=1e-7)
            # the plain callable and the AD form agree away from the short-circuits
            assert math.isclose(ch.path_lp(x), ch.lp_grad(x)[0], rel_tol=1e-14, abs_tol=1e-14)


def test_normalisation_by_quadrature():
    """K = 3 in one dimension: the density integrates to 1, and its log is the mixture's by the textbook formula"""
    w, mu, sd = np.array([0.2, 1.0, 3.0]), np.array([[-4.0], [0.5], [3.0]]), np.array([[0.5], [1.5], [0.8]])
    mix = R.Mixture(w, mu, sd)
    xs = np.linspace(-14.0, 14.0, 28001)
    dens = np.array([math.exp(mix.lp([x])) for x in xs])
    integral = np.trapezoid(dens, xs) if hasattr(np, "trapezoid") else np.trapz(dens, xs)
    assert abs(integral - 1.0) < 1e-9
    for x in (-4.0, 0.0, 2.2, 7.0):
        want = math.log(sum(w[k] / w.sum() * math.exp(-0.5 * ((x - mu[k, 0]) / sd[k, 0]) ** 2) / (sd[k, 0] * math.sqrt(2 * math.pi)) for k in range(3)))
        assert math.isclose(mix.lp([x]), want, rel_tol=1e-13)


def test_analytic_lognormalization_of_the_path():
    """Z0 = integral of exp(-prec x^2 / 2) = sqrt(2 pi / prec) per coordinate, Z1 = 1: log Z1 / Z0 by quadrature in d = 1, and in d = 3 by
    the product of the reference's integrals"""
    prec = 0.3
    xs = np.linspace(-40.0, 40.0, 80001)
    z0 = np.trapezoid(np.exp(-0.5 * prec * xs ** 2), xs) if hasattr(np, "trapezoid") else np.trapz(np.exp(-0.5 * prec * xs ** 2), xs)
    assert math.isclose(R.analytic_lognormalization(1, prec), -math.log(z0), rel_tol=1e-9)
    assert math.isclose(R.analytic_lognormalization(3, prec), -3 * math.log(z0), rel_tol=1e-9)
    ch0 = R.MixtureChain(_ref_mix(2, 3), 0.0, prec)
    x = np.array([0.3, -1.0, 2.0])
    assert ch0.path_lp(x) == -0.5 * prec * R.tree_sum(x * x)


def test_mala_restatement_leaves_a_gaussian_invariant():
    """K = 1: every interpolated density is Gaussian; one MALA transition from exact draws keeps the draws' distribution"""
    from scipy import stats
    import oracle as O
    mix = R.Mixture([1.0], [[0.5, -1.0]], [[0.8, 1.3]])
    beta, prec = 0.6, 1.0
    ch = R.MixtureChain(mix, beta, prec)
    # precision of the interpolated Gaussian per coordinate, and its mean
    p = (1 - beta) * prec + beta / mix.sd[0] ** 2
    m = beta * mix.mu[0] / mix.sd[0] ** 2 / p
    n = 3000
    X = np.random.default_rng(4).standard_normal((n, 2)) / np.sqrt(p) + m
    Z = np.empty_like(X)
    for i in range(n):
        Z[i] = R.mala_transition(X[i], O.OracleRng(seed=500 + i), ch, 0.9, 1, np.ones(2))["x"]
    U = (Z - m) * np.sqrt(p)
    assert np.mean(np.any(Z != X, axis=1)) > 0.3
    for j in range(2):
        assert abs(U[:, j].mean()) * math.sqrt(n) < 4.0 and abs(U[:, j].var() - 1.0) / math.sqrt(2.0 / n) < 4.0
        assert stats.kstest(U[:, j], "norm").pvalue > 1e-3
