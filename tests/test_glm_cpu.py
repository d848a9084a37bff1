"""The Bayesian-GLM family without a GPU: pte_create accepts it (a valid configuration reaches the device check) and refuses -- before any
device work -- what the device does not run; the Python and Julia surfaces map BayesianGLM onto pte_config and pte_set_target_glm; the NumPy
restatement (tests/glm_ref.py) has the right gradient, and the normal-identity evidence in closed form agrees with quadrature."""
import ctypes as C
import math

import numpy as np
import pytest

import family_cpu as F
import glm_ref as R
from family_cpu import P  # noqa: F401  (P: the module's fixture)


def test_enum_and_export_mirrors(P):
    from pigeons_amd import _lib
    assert _lib.TARGET_BAYESIAN_GLM == 5
    assert (_lib.GLM_BERNOULLI_LOGIT, _lib.GLM_NORMAL_IDENTITY) == (0, 1)
    assert "pte_set_target_glm" in _lib.EXPORTS
    assert hasattr(_lib.load(), "pte_set_target_glm")
    hdr = F.HEADER
    assert "PTE_TARGET_BAYESIAN_GLM         = 5" in hdr and "int pte_set_target_glm(" in hdr
    assert "PTE_GLM_BERNOULLI_LOGIT = 0" in hdr and "PTE_GLM_NORMAL_IDENTITY = 1" in hdr
    jl = F.JULIA
    assert "const TARGET_BAYESIAN_GLM = Int32(5)\n" in jl
    assert "const GLM_BERNOULLI_LOGIT, GLM_NORMAL_IDENTITY = Int32(0), Int32(1)" in jl
    assert "struct DeviceBayesianGLM" in jl and "device_family(t::DeviceBayesianGLM, inputs)" in jl
    assert ":pte_set_target_glm" in jl
    assert "BayesianGLM" in P.__dict__


@pytest.mark.parametrize("explorer,explorer2,dim", [(2, 0, 1), (3, 0, 8), (5, 0, 100), (2, 3, 512), (3, 2, 64), (5, 2, 7)])
def test_accepted_config_reaches_the_device_check(P, explorer, explorer2, dim):
    """fails on the code before the family existed ("target 5 has no device log-potential"): a valid configuration now passes validation"""
    F.no_device()
    from pigeons_amd import _lib
    F.assert_reaches_the_device_check(P, n_chains=4, target=5, dim=dim, explorer=explorer, explorer2=explorer2, target_params=[1.0])
    for dk in (0x1000, 0x2000):                         # the scan-loop flags (PTE_KERNEL_FLAG_BITS) are allowed
        if dk & _lib.KERNEL_FLAG_BITS:
            F.assert_reaches_the_device_check(P, n_chains=4, target=5, dim=dim, explorer=explorer, explorer2=explorer2, debug_kernel=dk)


_GLM = dict(target=5, dim=8, explorer=2, n_chains=4)


@pytest.mark.parametrize("kw,msg", [
    (dict(dim=0), r"Bayesian-GLM path keeps the replica in the registers of one wave, dim must be in 1\.\.512"),
    (dict(dim=513), r"Bayesian-GLM path keeps the replica in the registers of one wave, dim must be in 1\.\.512"),
    (dict(dim=1024, explorer=3), r"dim must be in 1\.\.512"),
    (dict(explorer=1), "Bayesian-GLM path is implemented for SliceSampler / AutoMALA / MALA"),       # ToyExplorer
    (dict(explorer=4), "Bayesian-GLM path is implemented for SliceSampler / AutoMALA / MALA"),       # IsingMetropolis
    (dict(explorer=0), "Bayesian-GLM path is implemented for SliceSampler / AutoMALA / MALA"),       # none
    (dict(explorer=2, explorer2=1), "Bayesian-GLM path is implemented for SliceSampler / AutoMALA / MALA"),
    (dict(explorer=6), "AAPS is implemented on the scaled-precision MVN and funnel paths only"),      # AAPS keeps its refusal
    (dict(debug_kernel=1), "debug_kernel 1 is not available on the Bayesian-GLM path"),
    (dict(debug_kernel=8), "debug_kernel 8 is not available on the Bayesian-GLM path"),
    (dict(n_chains_variational=4), "two-leg tempering"),
])
def test_pte_create_refusals(P, kw, msg):
    F.assert_create_refused(P, _GLM, kw, msg)


def _data(n=20, d=3, lik="bernoulli_logit", seed=1):
    g = np.random.default_rng(seed)
    X = g.normal(0.0, 1.0, (n, d))
    y = (g.uniform(size=n) < 0.4).astype(float) if lik == "bernoulli_logit" else g.normal(0.0, 2.0, n)
    return X, y


def test_python_mapping(P):
    from pigeons_amd import _lib
    X, y = _data(20, 3, "normal_identity")
    t = P.BayesianGLM(X, y, likelihood="normal_identity", noise_sd=0.7)
    kw = F.captured(P, t)
    assert kw["target"] == _lib.TARGET_BAYESIAN_GLM and kw["dim"] == 3 and list(kw["target_params"]) == [0.5]
    assert kw["explorer"] == _lib.EXPLORER_SLICE                      # default explorer: SliceSampler (target.jl:20)
    (lik, Xs, ys, sd), = kw["set_target_glm"]                        # set after create, once per engine
    assert lik == _lib.GLM_NORMAL_IDENTITY and sd == 0.7
    np.testing.assert_array_equal(Xs, X); np.testing.assert_array_equal(ys, y)
    X, y = _data(20, 3)
    kw = F.captured(P, P.BayesianGLM(X, y), explorer=P.AutoMALA())
    assert kw["explorer"] == _lib.EXPLORER_AUTOMALA and kw["set_target_glm"][0][0] == _lib.GLM_BERNOULLI_LOGIT
    kw = F.captured(P, t, explorer=P.Compose(P.SliceSampler(), P.MALA()))
    assert kw["explorer"] == _lib.EXPLORER_SLICE and kw["explorer2"] == _lib.EXPLORER_MALA
    F.assert_reference_refusals(P, t, wrong_dim=4)


def test_every_shard_gets_the_data(P):
    X, y = _data(10, 3)
    F.assert_every_shard_gets_the_data(P, P.BayesianGLM(X, y), P.ScaledPrecisionNormalLogPotential(1.0, 3), N=4, d=3, setter="set_target_glm")


@pytest.mark.parametrize("args,kw,msg", [
    ((np.zeros((3, 2)), np.zeros(3)), dict(likelihood="poisson_log"), "likelihood must be"),
    ((np.zeros(3), np.zeros(3)), {}, "X must be an n x d array"),
    ((np.zeros((0, 2)), np.zeros(0)), {}, "X must be an n x d array"),
    ((np.zeros((3, 0)), np.zeros(3)), {}, "X must be an n x d array"),
    ((np.zeros((4097, 1)), np.zeros(4097)), {}, r"1\.\.4096 observations"),
    ((np.zeros((2, 513)), np.zeros(2)), {}, r"d must be in 1\.\.512"),
    ((np.zeros((257, 512)), np.zeros(257)), {}, "n \\* d must be <= 131072"),
    ((np.zeros((3, 2)), np.zeros(4)), {}, "y must be a vector of the n = 3 observations"),
    ((np.zeros((3, 2)), np.zeros((3, 1))), {}, "y must be a vector"),
    (([[0.0, np.nan], [0.0, 0.0]], [0.0, 1.0]), {}, "X must be finite"),
    (([[0.0, np.inf], [0.0, 0.0]], [0.0, 1.0]), {}, "X must be finite"),
    ((np.zeros((2, 2)), [0.0, np.nan]), dict(likelihood="normal_identity"), "y must be finite"),
    ((np.zeros((2, 2)), [0.0, 0.5]), {}, r"y in \{0, 1\}"),
    ((np.zeros((2, 2)), [0.0, -1.0]), dict(likelihood="bernoulli_logit"), r"y in \{0, 1\}"),
    ((np.zeros((2, 2)), [0.0, 0.5]), dict(likelihood="normal_identity", noise_sd=0.0), "noise_sd must be positive and finite"),
    ((np.zeros((2, 2)), [0.0, 0.5]), dict(likelihood="normal_identity", noise_sd=-1.0), "noise_sd must be positive and finite"),
    ((np.zeros((2, 2)), [0.0, 0.5]), dict(likelihood="normal_identity", noise_sd=np.inf), "noise_sd must be positive and finite"),
])
def test_python_validation(P, args, kw, msg):
    with pytest.raises(ValueError, match=msg):
        P.BayesianGLM(*args, **kw)


def test_bayesian_glm_surface(P):
    t = P.BayesianGLM([[1.0, 2.0], [3.0, 4.0], [5.0, 6.0]], [0, 1, 1])
    assert t.n_obs == 3 and t.dim == 2 and t.likelihood == "bernoulli_logit" and t.X.dtype == np.float64
    assert P.BayesianGLM(np.ones((4096, 32)), np.zeros(4096)).n_obs == 4096            # the limits themselves are accepted
    assert P.BayesianGLM(np.ones((256, 512)), np.zeros(256), likelihood="normal_identity", noise_sd=2.0).dim == 512
    doc = P.BayesianGLM.__doc__
    assert "stepping_stone(pt) + (d/2) log(2 pi / p)" in doc and "bernoulli_logit" in doc and "normal_identity" in doc


def test_set_target_glm_is_bound(P):
    from pigeons_amd import _lib
    F.assert_null_engine_refused(_lib.load().pte_set_target_glm, (None, 0, 2, None, None, 1.0), {1: C.c_int32, 2: C.c_int64, 5: C.c_double})


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lik", ["bernoulli_logit", "normal_identity"])
@pytest.mark.parametrize("n,d", [(1, 1), (70, 3), (130, 9)])
def test_gradient_against_central_differences(lik, n, d):
    X, y = _data(n, d, lik, seed=n + d)
    glm = R.Glm(X, y, lik, 0.8, 0.6)
    g = np.random.default_rng(n * 10 + d)
    for beta in (1.0, 0.3):
        ch = R.GlmChain(glm, beta, 0.6)
        for _ in range(3):
            x = g.normal(0.0, 1.0, d)
            _, grad = ch.lp_grad(x)
            h = 1e-5
            num = np.array([(ch.lp_grad(x + h * e)[0] - ch.lp_grad(x - h * e)[0]) / (2 * h) for e in np.eye(d)])
            np.testing.assert_allclose(grad, num, rtol=1e-6, atol=1e-6)
            assert math.isclose(ch.path_lp(x), ch.lp_grad(x)[0], rel_tol=1e-14, abs_tol=1e-14)


@pytest.mark.parametrize("lik", ["bernoulli_logit", "normal_identity"])
def test_restatement_against_the_textbook_density(lik):
    """the prior N(0, I / p) normalised, the likelihood by its textbook formula (the ragged last block of observations contributes nothing)"""
    n, d, p, sd = 100, 4, 0.7, 1.3
    X, y = _data(n, d, lik, seed=5)
    glm = R.Glm(X, y, lik, sd, p)
    theta = np.random.default_rng(6).normal(0.0, 1.0, d)
    eta = X @ theta
    if lik == "bernoulli_logit":
        ll = np.sum(y * np.log(1 / (1 + np.exp(-eta))) + (1 - y) * np.log(1 / (1 + np.exp(eta))))
    else:
        ll = np.sum(-0.5 * np.log(2 * np.pi * sd ** 2) - (y - eta) ** 2 / (2 * sd ** 2))
    prior = np.sum(-0.5 * np.log(2 * np.pi / p) - 0.5 * p * theta ** 2)
    assert math.isclose(glm.lp(theta), prior + ll, rel_tol=1e-12)
    assert glm.terms(np.zeros(1))[0][0] == (-math.log(2.0) if lik == "bernoulli_logit" else -(y[0] ** 2) * glm.w2)


def test_normal_evidence_closed_form_against_quadrature():
    """d = 2: y ~ N(0, sigma^2 I + X X^T / p) against the integral of prior x likelihood on a grid; and the evidence convention of
    stepping_stone (log Z1 / Z0 = log p(y) - (d/2) log(2 pi / p))"""
    n, p, sd = 15, 0.8, 0.9
    X, y = _data(n, 2, "normal_identity", seed=11)
    glm = R.Glm(X, y, "normal_identity", sd, p)
    m, cov = glm.posterior()
    s = np.sqrt(np.diag(cov))
    a = np.linspace(m[0] - 12 * s[0], m[0] + 12 * s[0], 801)
    b = np.linspace(m[1] - 12 * s[1], m[1] + 12 * s[1], 801)
    A, B = np.meshgrid(a, b, indexing="ij")
    T = np.stack([A.ravel(), B.ravel()], axis=1)
    eta = T @ X.T
    logf = (-np.log(2 * np.pi / p) - 0.5 * p * (T ** 2).sum(1)) + np.sum(-0.5 * np.log(2 * np.pi * sd ** 2) - (y - eta) ** 2 / (2 * sd ** 2), axis=1)
    mx = logf.max()
    Z = np.exp(logf - mx).reshape(A.shape).sum() * (a[1] - a[0]) * (b[1] - b[0])
    assert math.isclose(glm.log_evidence(), mx + math.log(Z), rel_tol=0, abs_tol=1e-8)
    # the restatement's target density is the same integrand
    for k in (0, 12345, 400 * 801 + 400):
        assert math.isclose(glm.lp(T[k]), logf[k], rel_tol=1e-12, abs_tol=1e-12)
    assert math.isclose(glm.evidence_offset(), -math.log(2 * math.pi / p), rel_tol=1e-15)
