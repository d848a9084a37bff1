"""The dense-precision Gaussian family without a GPU: pte_create accepts it (a valid configuration reaches the device check) and refuses --
before any device work -- what the device does not run; the Python and Julia surfaces map DenseNormal onto pte_config and
pte_set_target_dense; the NumPy restatement (tests/dense_ref.py) has the right gradient, constant and chain moments, and a conjugate
linear-regression posterior written as a DenseNormal is the regression's density up to its evidence."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import dense_ref as R
import family_cpu as F
from family_cpu import P  # noqa: F401  (P: the module's fixture)


def test_enum_and_export_mirrors(P):
    from pigeons_amd import _lib
    import __graft_entry__ as g
    assert _lib.TARGET_DENSE_NORMAL == 11
    assert "pte_set_target_dense" in _lib.EXPORTS
    assert hasattr(_lib.load(), "pte_set_target_dense")
    hdr = F.HEADER
    assert "PTE_TARGET_DENSE_NORMAL = 11" in hdr
    assert "int pte_set_target_dense(pte_engine *h, int64_t dim, const double *mean /*[dim]*/, const double *precision /*[dim][dim]*/);" in hdr
    jl = F.JULIA
    assert "const TARGET_DENSE_NORMAL = Int32(11)\n" in jl
    assert "struct DeviceDenseNormal" in jl and "device_family(t::DeviceDenseNormal, inputs)" in jl
    assert ":pte_set_target_dense" in jl
    assert "DenseNormal" in P.__dict__
    # the kernels live in an existing translation unit: no ninth one, no RNG-policy setter of their own
    assert len(g.UNITS) == 8
    params = open(os.path.join(g.CSRC, "pte_automala_params.hpp")).read()
    assert "TGT_DENSE = 11" in params and "X(dense)" not in params
    assert '#include "pte_dense.hpp"' in open(os.path.join(g.CSRC, "pte_glm.hip")).read()
    assert "PTE_DEFINE_RNG_POLICY_SETTER" not in open(os.path.join(g.CSRC, "pte_dense.hpp")).read()


@pytest.mark.parametrize("dim", [1, 64, 65, 512])
@pytest.mark.parametrize("explorer,explorer2", [(2, 0), (3, 0), (5, 0), (2, 3)])
def test_accepted_config_reaches_the_device_check(P, explorer, explorer2, dim):
    """fails on the code before the family existed ("target 11 has no device log-potential"): a valid configuration now passes validation"""
    F.no_device()
    F.assert_reaches_the_device_check(P, n_chains=4, target=11, dim=dim, explorer=explorer, explorer2=explorer2, target_params=[1.0])


_DENSE = dict(target=11, dim=15, explorer=2, n_chains=4)


@pytest.mark.parametrize("kw,msg", [
    (dict(explorer=0), "dense-normal path is implemented for SliceSampler / AutoMALA / MALA"),       # none
    (dict(explorer=1), "dense-normal path is implemented for SliceSampler / AutoMALA / MALA"),       # ToyExplorer
    (dict(explorer=4), "dense-normal path is implemented for SliceSampler / AutoMALA / MALA"),       # IsingMetropolis
    (dict(explorer=2, explorer2=1), "dense-normal path is implemented for SliceSampler / AutoMALA / MALA"),
    (dict(explorer=6), r"AAPS is implemented on the scaled-precision MVN and funnel paths only \(got target 11\)"),
    (dict(explorer=2, explorer2=6), "AAPS is not available as half of a Compose on the device"),
    (dict(dim=0), r"dense-normal path keeps the replica in the registers of one wave, dim must be in 1\.\.512 \(got 0\)"),
    (dict(dim=513), r"dense-normal path keeps the replica in the registers of one wave, dim must be in 1\.\.512 \(got 513\)"),
    (dict(debug_kernel=1), r"debug_kernel 1 is not available on the dense-normal path"),
    (dict(debug_kernel=8), r"debug_kernel 8 is not available on the dense-normal path"),
    (dict(n_chains_variational=4), r"two-leg tempering \(n_chains_variational > 0\) is not available on the dense-normal path"),
    # a doubly-wrong configuration gets the earlier message
    (dict(explorer=1, dim=513), "dense-normal path is implemented for SliceSampler / AutoMALA / MALA"),
    (dict(dim=513, debug_kernel=1), r"dim must be in 1\.\.512 \(got 513\)"),
    (dict(debug_kernel=1, n_chains_variational=4), r"debug_kernel 1 is not available on the dense-normal path"),
])
def test_pte_create_refusals(P, kw, msg):
    F.assert_create_refused(P, _DENSE, kw, msg)


def test_python_mapping(P):
    from pigeons_amd import _lib
    Q = R.spectrum_matrix(7, 50.0, 1)
    m = np.arange(7.0)
    t = P.DenseNormal(m, Q)
    kw = F.captured(P, t)
    assert kw["target"] == _lib.TARGET_DENSE_NORMAL and kw["dim"] == 7 and list(kw["target_params"]) == [0.5]
    assert kw["explorer"] == _lib.EXPLORER_SLICE                      # default explorer: SliceSampler (target.jl:20)
    (ms, Qs), = kw["set_target_dense"]                                # set after create, once per engine
    np.testing.assert_array_equal(ms, m); np.testing.assert_array_equal(Qs, Q)
    kw = F.captured(P, t, explorer=P.AutoMALA())
    assert kw["explorer"] == _lib.EXPLORER_AUTOMALA
    kw = F.captured(P, t, explorer=P.Compose(P.SliceSampler(), P.MALA()))
    assert kw["explorer"] == _lib.EXPLORER_SLICE and kw["explorer2"] == _lib.EXPLORER_MALA
    F.assert_reference_refusals(P, t, wrong_dim=8)


def test_every_shard_gets_the_data(P):
    F.assert_every_shard_gets_the_data(P, P.DenseNormal(np.zeros(5), np.eye(5)), P.ScaledPrecisionNormalLogPotential(1.0, 5),
                                       N=4, d=5, setter="set_target_dense")


_I2 = np.eye(2)


@pytest.mark.parametrize("args,kw,msg", [
    (([0.0, 0.0],), {}, "exactly one of precision and covariance"),
    (([0.0, 0.0], _I2), dict(covariance=_I2), "exactly one of precision and covariance"),
    (([], np.zeros((0, 0))), {}, r"mean must be a vector of 1\.\.512 entries"),
    ((np.zeros(513), np.eye(513)), {}, r"mean must be a vector of 1\.\.512 entries"),
    ((np.zeros((2, 2)), _I2), {}, r"mean must be a vector of 1\.\.512 entries"),
    (([0.0, np.nan], _I2), {}, r"mean\[1\] must be finite"),
    (([0.0, 0.0], np.eye(3)), {}, r"precision must be 2 x 2"),
    (([0.0, 0.0], np.ones(4)), {}, r"precision must be 2 x 2"),
    (([0.0, 0.0],), dict(covariance=np.eye(3)), r"covariance must be 2 x 2"),
    (([0.0, 0.0], [[1.0, np.inf], [0.0, 1.0]]), {}, r"precision\[0\]\[1\] must be finite"),
    (([0.0, 0.0],), dict(covariance=[[1.0, 0.0], [np.nan, 1.0]]), r"covariance\[1\]\[0\] must be finite"),
    (([0.0, 0.0], [[1.0, 2.0], [2.0, 1.0]]), {}, "precision must be positive definite"),
    (([0.0, 0.0], [[1.0, 0.0], [0.0, 0.0]]), {}, "precision must be positive definite"),
    (([0.0, 0.0],), dict(covariance=[[1.0, 0.0], [0.0, -1.0]]), "covariance must be positive definite"),
])
def test_python_validation(P, args, kw, msg):
    with pytest.raises(ValueError, match=msg):
        P.DenseNormal(*args, **kw)


def test_dense_normal_surface(P):
    Q = np.array([[2.0, 0.5], [0.7, 1.0]])
    t = P.DenseNormal([1.0, -1.0], Q)
    assert t.dim == 2 and t.mean.dtype == np.float64 and repr(t) == "DenseNormal(dim=2)"
    np.testing.assert_array_equal(t.precision, (Q + Q.T) / 2.0)      # symmetrised, bit for bit symmetric
    assert np.array_equal(t.precision, t.precision.T)
    c = P.DenseNormal([1.0, -1.0], covariance=np.linalg.inv(t.precision))
    np.testing.assert_allclose(c.precision, t.precision, rtol=1e-13)
    assert np.array_equal(c.precision, c.precision.T)
    assert P.DenseNormal(np.zeros(512), np.eye(512)).dim == 512      # the limits are accepted
    assert P.DenseNormal([0.5], [[2.0]]).dim == 1
    assert math.isclose(t.evidence_offset(0.25), -1.0 * math.log(2.0 * math.pi / 0.25), rel_tol=1e-15)
    assert math.isclose(t.evidence_offset(0.25), R.Dense(t.mean, t.precision).evidence_offset(0.25), rel_tol=1e-15)
    for beta in (0.0, 0.3, 1.0):
        m, cov = t.chain_moments(beta, 0.25)
        mr, cr = R.DenseChain(R.Dense(t.mean, t.precision), beta, 0.25).chain_moments()
        np.testing.assert_allclose(m, mr, rtol=1e-13, atol=1e-15); np.testing.assert_allclose(cov, cr, rtol=1e-13)
    from pigeons_amd.pt import default_explorer
    assert isinstance(default_explorer(t), P.SliceSampler)


def test_set_target_dense_is_bound(P):
    from pigeons_amd import _lib
    F.assert_null_engine_refused(_lib.load().pte_set_target_dense, (None, 2, None, None), {1: C.c_int64}, n_args=4)


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------
def test_gradient_against_central_differences():
    """18 random states (d = 1, 5, 70: one block and a ragged second one), the target alone and on the path"""
    g = np.random.default_rng(7)
    n = 0
    for d in (1, 5, 70):
        dense = R.Dense(g.normal(0.0, 1.0, d), R.spectrum_matrix(d, 100.0, d))
        for k in range(6):
            x = g.normal(0.0, 0.7, d)
            ch = R.DenseChain(dense, (1.0, 0.3)[k % 2], 0.6)
            lp, grad = ch.lp_grad(x)
            h = 1e-5
            num = np.array([(ch.lp_grad(x + h * e)[0] - ch.lp_grad(x - h * e)[0]) / (2 * h) for e in np.eye(d)])
            np.testing.assert_allclose(grad, num, rtol=1e-6, atol=1e-6)
            assert math.isclose(ch.path_lp(x), lp, rel_tol=1e-14, abs_tol=1e-14)
            assert ch.logdensity_and_gradient(x)[0] == lp
            n += 1
    assert n == 18


@pytest.mark.parametrize("d", [1, 2, 6, 65, 512])
def test_constant_against_slogdet_and_the_textbook_density(d):
    g = np.random.default_rng(d)
    Q = R.spectrum_matrix(d, 100.0, 3 * d)
    dense = R.Dense(g.normal(0.0, 1.0, d), Q)
    sign, logdet = np.linalg.slogdet(Q)
    assert sign == 1.0
    assert math.isclose(dense.c, 0.5 * logdet - 0.5 * d * math.log(2.0 * math.pi), rel_tol=1e-12, abs_tol=1e-11)
    x = g.normal(0.0, 1.0, d)
    z = x - dense.mean
    assert math.isclose(dense.lp(x), dense.c - 0.5 * float(z @ Q @ z), rel_tol=1e-12, abs_tol=1e-12)
    with pytest.raises(ValueError, match="pivot 0"):
        R.Dense._cholesky(-Q)


def test_chain_moments_against_brute_force():
    """chain beta has density exp((1 - beta)(-p/2 |x|^2) + beta l2(x)): precision P = (1 - beta) p I + beta Q -- the gradient of the chain's
    log density vanishes at the mean and its Hessian (finite differences of the restated gradient) is -P"""
    g = np.random.default_rng(11)
    d, p = 6, 0.25
    dense = R.Dense(g.normal(0.0, 2.0, d), R.spectrum_matrix(d, 68.0, 5))
    for beta in (0.0, 0.2, 0.7, 1.0):
        ch = R.DenseChain(dense, beta, p)
        mean, cov = ch.chain_moments()
        _, grad = ch.lp_grad(mean)
        np.testing.assert_allclose(grad, 0.0, atol=1e-12)
        H = np.array([(ch.lp_grad(mean + 0.5 * e)[1] - ch.lp_grad(mean - 0.5 * e)[1]) for e in np.eye(d)])       # exact for a quadratic
        np.testing.assert_allclose(np.linalg.inv(-H), cov, rtol=1e-10, atol=1e-13)
    m0, c0 = R.DenseChain(dense, 0.0, p).chain_moments()
    np.testing.assert_allclose(m0, 0.0, atol=0); np.testing.assert_allclose(c0, np.eye(d) / p, rtol=1e-15, atol=0)
    m1, c1 = R.DenseChain(dense, 1.0, p).chain_moments()
    np.testing.assert_allclose(m1, dense.mean, rtol=1e-12); np.testing.assert_allclose(c1, np.linalg.inv(dense.Q), rtol=1e-12, atol=1e-15)


def test_a_conjugate_regression_posterior_is_a_dense_normal():
    """BayesianGLM(normal_identity): prior x likelihood (tests/glm_ref.py) = evidence x N(posterior mean, posterior precision^-1), so the
    two densities differ by one constant -- the regression's log evidence -- over random points"""
    import glm_ref as G
    g = np.random.default_rng(5)
    n, d, prec, sd = 40, 9, 0.7, 1.3
    X = g.normal(0.0, 1.0, (n, d))
    y = X @ g.normal(0.0, 1.0, d) + sd * g.normal(0.0, 1.0, n)
    glm = G.Glm(X, y, "normal_identity", sd, prec)
    mean, cov = glm.posterior()
    A = prec * np.eye(d) + X.T @ X / sd ** 2
    dense = R.Dense(mean, (A + A.T) / 2.0)
    diff = np.array([glm.lp(t) - dense.lp(t) for t in g.normal(0.0, 1.5, (12, d))])
    np.testing.assert_allclose(diff, diff[0], rtol=0, atol=1e-9)
    assert math.isclose(diff[0], glm.log_evidence(), rel_tol=0, abs_tol=1e-9)
