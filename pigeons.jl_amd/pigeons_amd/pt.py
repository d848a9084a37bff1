"""pigeons() / Inputs / PT: the reference's top-level surface (src/api.jl:8-19,
src/pt/Inputs.jl:9-131, src/pt/PT.jl:6-51, src/pt/pigeons.jl:12-55,152-162,
src/pt/Iterators.jl:9-49) driving the MI355X engine for the explore-then-swap loop.

Everything inside `while next_scan!` runs on the GPU (one C-ABI call per round);
what the reference runs a logarithmic number of times (adapt, report) stays host-side.
"""
import math
import time
from dataclasses import dataclass, field
from typing import Any, List, Optional

import numpy as np

from . import _lib
from .engine import Engine
from . import tempering as T


# ---- targets (src/targets/toy_mvn_target.jl, src/paths/ScaledPrecisionNormalPath.jl) ---------
@dataclass
class ScaledPrecisionNormalPath:
    precision0: float = 1.0
    precision1: float = 10.0
    dim: int = 1

    def precision(self, beta):
        return (1.0 - beta) * self.precision0 + beta * self.precision1


def toy_mvn_target(dim):
    """src/targets/toy_mvn_target.jl:8"""
    return ScaledPrecisionNormalPath(1.0, 10.0, dim)


def analytic_lognormalization(path, reference=None):
    """src/paths/ScaledPrecisionNormalPath.jl:66-71.  GaussianMixture (with its reference ScaledPrecisionNormalLogPotential(prec, dim), which
    is unnormalised): log Z1 / Z0 = -(dim / 2) log(2 pi / prec)."""
    if isinstance(path, GaussianMixture):
        if not isinstance(reference, ScaledPrecisionNormalLogPotential):
            raise ValueError("GaussianMixture: pass reference=ScaledPrecisionNormalLogPotential(prec, dim)")
        return -(path.dim / 2.0) * math.log(2.0 * math.pi / reference.precision)
    return 0.5 * path.dim * (math.log(path.precision0) - math.log(path.precision1))


def analytic_cumulativebarrier(path):
    """src/paths/ScaledPrecisionNormalPath.jl:56-64"""
    from scipy.special import beta as beta_fn
    b = beta_fn(path.dim / 2.0, path.dim / 2.0)

    def cumulativebarrier(beta):
        sigma0 = 1.0 / math.sqrt(path.precision0)
        sigmab = 1.0 / math.sqrt(path.precision(beta))
        return 2 ** (2.0 - path.dim) / b * math.log(sigma0 / sigmab)
    return cumulativebarrier


@dataclass
class ScaledPrecisionNormalLogPotential:
    """src/paths/ScaledPrecisionNormalPath.jl:14-20 (used as a `reference`)"""
    precision: float = 1.0
    dim: int = 1


@dataclass
class Funnel:
    """Neal's funnel as a LogDensityProblems target (reference test/supporting/dimensional-analysis.jl:33-48):
    z[1] ~ Normal(0, 3), z[i] ~ Normal(0, exp(z[1]/2)); initialization = zeros(dim).  Tempered through the
    default InterpolatingPath(reference, target) (src/targets/target.jl:72-75)."""
    dim: int = 2


class GaussianMixture:
    """A normalised mixture of K <= 8 Gaussians with diagonal covariance, the device's multimodal target.  The Julia form is
        DistributionLogPotential(MixtureModel([MvNormal(means[k], Diagonal(std_devs[k] .^ 2)) for k in 1:K], weights))
    weights: K positive numbers (normalised here as by MixtureModel); means, std_devs: K x dim.  Tempered through the default
    InterpolatingPath(reference, target) (src/targets/target.jl:72-75) with reference=ScaledPrecisionNormalLogPotential(prec, dim);
    initialization = zeros(dim); default explorer SliceSampler (target.jl:20)."""

    def __init__(self, weights, means, std_devs):
        w = np.array(weights, dtype=np.float64).ravel()
        m = np.array(means, dtype=np.float64)
        s = np.array(std_devs, dtype=np.float64)
        if w.size < 1 or w.size > 8:
            raise ValueError("GaussianMixture: the device holds 1..8 components (got %d)" % w.size)
        if m.ndim != 2 or m.shape[0] != w.size or s.shape != m.shape or m.shape[1] < 1:
            raise ValueError("GaussianMixture: means and std_devs must both be K x dim arrays with K = len(weights)")
        if not np.all(np.isfinite(w)) or np.any(w <= 0):
            raise ValueError("GaussianMixture: weights must be positive and finite")
        if not np.all(np.isfinite(s)) or np.any(s <= 0):
            raise ValueError("GaussianMixture: std_devs must be positive and finite")
        if not np.all(np.isfinite(m)):
            raise ValueError("GaussianMixture: means must be finite")
        self.weights, self.means, self.std_devs = w, m, s

    @property
    def n_components(self):
        return self.weights.size

    @property
    def dim(self):
        return self.means.shape[1]

    def __repr__(self):
        return "GaussianMixture(K=%d, dim=%d)" % (self.n_components, self.dim)


class BayesianGLM:
    """The posterior of a Bayesian generalised linear model, the device's data-reading target: prior N(0, I / p) on the
    coefficients theta (d of them) times the likelihood of n observations y_i given eta_i = X[i] . theta,
        likelihood="bernoulli_logit"   y_i in {0, 1}, log p(y_i | eta_i) = y_i eta_i - softplus(eta_i)     (logistic regression)
        likelihood="normal_identity"   log p(y_i | eta_i) = log N(y_i; eta_i, noise_sd^2)                   (linear regression, known noise)
    X: n x d, y: n (1 <= n <= 4096, 1 <= d <= 512, n d <= 131072).  Tempered through the default InterpolatingPath(reference, target)
    (src/targets/target.jl:72-75) from reference=ScaledPrecisionNormalLogPotential(p, d) -- the prior, unnormalised -- to prior x likelihood
    with the prior normalised; initialization = zeros(d); default explorer SliceSampler (target.jl:20).

    Evidence: stepping_stone(pt) estimates log Z1 / Z0 = log p(y) - (d/2) log(2 pi / p), so the log evidence (marginal likelihood) is
    stepping_stone(pt) + (d/2) log(2 pi / p)."""

    LIKELIHOODS = {"bernoulli_logit": 0, "normal_identity": 1}

    def __init__(self, X, y, likelihood="bernoulli_logit", noise_sd=1.0):
        if likelihood not in self.LIKELIHOODS:
            raise ValueError("BayesianGLM: likelihood must be 'bernoulli_logit' or 'normal_identity' (got %r)" % (likelihood,))
        X = np.array(X, dtype=np.float64)
        y = np.array(y, dtype=np.float64)
        if X.ndim != 2 or X.shape[0] < 1 or X.shape[1] < 1:
            raise ValueError("BayesianGLM: X must be an n x d array")
        n, d = X.shape
        if n > 4096:
            raise ValueError("BayesianGLM: the device holds 1..4096 observations (got %d)" % n)
        if d > 512:
            raise ValueError("BayesianGLM: the device keeps theta in one wave's registers, d must be in 1..512 (got %d)" % d)
        if n * d > 131072:
            raise ValueError("BayesianGLM: n * d must be <= 131072 (got %d * %d)" % (n, d))
        if y.ndim != 1 or y.size != n:
            raise ValueError("BayesianGLM: y must be a vector of the n = %d observations" % n)
        if not np.all(np.isfinite(X)):
            raise ValueError("BayesianGLM: X must be finite")
        if not np.all(np.isfinite(y)):
            raise ValueError("BayesianGLM: y must be finite")
        if likelihood == "bernoulli_logit" and not np.all((y == 0.0) | (y == 1.0)):
            raise ValueError("BayesianGLM: the Bernoulli-logit likelihood needs y in {0, 1}")
        noise_sd = float(noise_sd)
        if likelihood == "normal_identity" and not (noise_sd > 0 and math.isfinite(noise_sd)):
            raise ValueError("BayesianGLM: noise_sd must be positive and finite (got %r)" % (noise_sd,))
        self.X, self.y, self.likelihood, self.noise_sd = X, y, likelihood, noise_sd

    @property
    def n_obs(self):
        return self.X.shape[0]

    @property
    def dim(self):
        return self.X.shape[1]

    @property
    def likelihood_code(self):
        return self.LIKELIHOODS[self.likelihood]

    def __repr__(self):
        return "BayesianGLM(%s, n=%d, dim=%d)" % (self.likelihood, self.n_obs, self.dim)


class MixtureModelPosterior:
    """The posterior of a finite mixture model given data, the device's label-switching target: n real observations y_i from
    a mixture of K = n_components normals (1 <= K <= 8, 1 <= n <= 65536), with the state
        theta = [mu_1..mu_K, s_1..s_K, alpha_1..alpha_K]        (d = 3 K)
    component k having mean mu_k, standard deviation exp(s_k) and weight softmax(alpha)_k, and the prior N(0, I / p) on theta (standardise
    y).  Every relabelling of the components has the same posterior density: K! symmetric modes.  Tempered through the default
    InterpolatingPath(reference, target) (src/targets/target.jl:72-75) from reference=ScaledPrecisionNormalLogPotential(p, d) -- the prior,
    unnormalised -- to prior x likelihood with the prior normalised; initialization = zeros(d); default explorer SliceSampler (target.jl:20).

    Evidence: stepping_stone(pt) estimates log Z1 / Z0 = log p(y) - (d/2) log(2 pi / p), so the log evidence (marginal likelihood) is
    stepping_stone(pt) + (d/2) log(2 pi / p)."""

    def __init__(self, y, n_components):
        y = np.array(y, dtype=np.float64)
        if isinstance(n_components, bool) or int(n_components) != n_components or not 1 <= int(n_components) <= 8:
            raise ValueError("MixtureModelPosterior: the device holds 1..8 components (got %r)" % (n_components,))
        if y.ndim != 1:
            raise ValueError("MixtureModelPosterior: y must be a vector of real observations")
        if y.size < 1 or y.size > 65536:
            raise ValueError("MixtureModelPosterior: the device holds 1..65536 observations (got %d)" % y.size)
        if not np.all(np.isfinite(y)):
            raise ValueError("MixtureModelPosterior: y[%d] must be finite" % int(np.flatnonzero(~np.isfinite(y))[0]))
        self.y, self.n_components = y, int(n_components)

    @property
    def n_obs(self):
        return self.y.size

    @property
    def dim(self):
        return 3 * self.n_components

    def __repr__(self):
        return "MixtureModelPosterior(n=%d, K=%d)" % (self.n_obs, self.n_components)


class HierarchicalNormalMeans:
    """The posterior of a hierarchical normal-means model, the device's funnel-with-data target ("eight schools"): J groups with
    estimates y_j and known standard errors sigma_j,
        y_j ~ N(theta_j, sigma_j^2),  theta_j ~ N(mu, tau^2),  mu ~ N(0, mu_sd^2),  tau ~ HalfCauchy(0, tau_scale)
    with the state x = [mu, log tau, x_2 .. x_{J+1}] (dim = J + 2, 1 <= J <= 510) and
        parameterization="centered"      x_{2+j} = theta_j
        parameterization="noncentered"   x_{2+j} = eta_j ~ N(0, 1), theta_j = mu + tau eta_j
    The density is normalised in x (it includes the Jacobian of log tau).  Tempered through the default InterpolatingPath(reference, target)
    (src/targets/target.jl:72-75) from reference=ScaledPrecisionNormalLogPotential(p, dim), unnormalised; initialization = zeros(dim);
    default explorer SliceSampler (target.jl:20).

    Evidence: stepping_stone(pt) estimates log Z1 / Z0 = log p(y) - (d/2) log(2 pi / p) in either parameterization, so the log evidence
    (marginal likelihood) is stepping_stone(pt) - evidence_offset(p): see evidence_offset."""

    PARAMETERIZATIONS = {"centered": 0, "noncentered": 1}

    def __init__(self, y, sigma, mu_sd=5.0, tau_scale=5.0, parameterization="centered"):
        if parameterization not in self.PARAMETERIZATIONS:
            raise ValueError("HierarchicalNormalMeans: parameterization must be 'centered' or 'noncentered' (got %r)" % (parameterization,))
        y = np.array(y, dtype=np.float64)
        sigma = np.array(sigma, dtype=np.float64)
        if y.ndim != 1 or not 1 <= y.size <= 510:
            raise ValueError("HierarchicalNormalMeans: y must be a vector of 1..510 group estimates (got shape %s)" % (y.shape,))
        if sigma.shape != y.shape:
            raise ValueError("HierarchicalNormalMeans: sigma must hold one standard error per group, %d of them (got shape %s)" % (y.size, sigma.shape))
        if not np.all(np.isfinite(y)):
            raise ValueError("HierarchicalNormalMeans: y[%d] must be finite" % int(np.flatnonzero(~np.isfinite(y))[0]))
        bad = ~(np.isfinite(sigma) & (sigma > 0))
        if np.any(bad):
            raise ValueError("HierarchicalNormalMeans: sigma[%d] must be positive and finite" % int(np.flatnonzero(bad)[0]))
        mu_sd, tau_scale = float(mu_sd), float(tau_scale)
        if not (mu_sd > 0 and math.isfinite(mu_sd)):
            raise ValueError("HierarchicalNormalMeans: mu_sd must be positive and finite (got %r)" % (mu_sd,))
        if not (tau_scale > 0 and math.isfinite(tau_scale)):
            raise ValueError("HierarchicalNormalMeans: tau_scale must be positive and finite (got %r)" % (tau_scale,))
        self.y, self.sigma, self.mu_sd, self.tau_scale, self.parameterization = y, sigma, mu_sd, tau_scale, parameterization

    @property
    def n_groups(self):
        return self.y.size

    @property
    def dim(self):
        return self.y.size + 2

    @property
    def parameterization_code(self):
        return self.PARAMETERIZATIONS[self.parameterization]

    def evidence_offset(self, precision):
        """what stepping_stone(pt) is off the log evidence by: stepping_stone(pt) = log p(y) + evidence_offset(p), with
        evidence_offset(p) = -(d/2) log(2 pi / p), d = dim and p the reference's precision"""
        return -(self.dim / 2.0) * math.log(2.0 * math.pi / float(precision))

    def __repr__(self):
        return "HierarchicalNormalMeans(%s, J=%d, dim=%d)" % (self.parameterization, self.n_groups, self.dim)


class LatentAR1:
    """The posterior of a latent AR(1) state-space model, the device's family with coordinates coupled to their neighbours: T
    observations y_t of a latent state h,
        h_0 ~ N(mu, sigma^2 / (1 - phi^2)),  h_t | h_{t-1} ~ N(mu + phi (h_{t-1} - mu), sigma^2),
        mu ~ N(0, mu_sd^2),  a = atanh(phi) ~ N(phi_loc, phi_scale^2),  sigma ~ HalfCauchy(0, sigma_scale)
    observed through
        likelihood="stochastic_volatility"   y_t ~ N(0, exp(h_t))
        likelihood="normal_identity"         y_t ~ N(h_t, obs_sd^2)   (linear-Gaussian given phi and sigma: exact evidence by quadrature)
    with the state x = [mu, a, log sigma, h_0 .. h_{T-1}] (dim = T + 3, 1 <= T <= 509).  The density is normalised in x (it includes the Jacobian
    of log sigma).  Tempered through the default InterpolatingPath(reference, target) (src/targets/target.jl:72-75) from
    reference=ScaledPrecisionNormalLogPotential(p, dim), unnormalised; initialization = zeros(dim); default explorer SliceSampler (target.jl:20).

    Evidence: stepping_stone(pt) estimates log Z1 / Z0 = log p(y) - (d/2) log(2 pi / p), so the log evidence (marginal likelihood) is
    stepping_stone(pt) - evidence_offset(p): see evidence_offset."""

    LIKELIHOODS = {"stochastic_volatility": 0, "normal_identity": 1}

    def __init__(self, y, likelihood="stochastic_volatility", obs_sd=1.0, mu_sd=5.0, phi_loc=0.0, phi_scale=1.0, sigma_scale=1.0):
        if likelihood not in self.LIKELIHOODS:
            raise ValueError("LatentAR1: likelihood must be 'stochastic_volatility' or 'normal_identity' (got %r)" % (likelihood,))
        y = np.array(y, dtype=np.float64)
        if y.ndim != 1 or not 1 <= y.size <= 509:
            raise ValueError("LatentAR1: y must be a vector of 1..509 observations (got shape %s)" % (y.shape,))
        if not np.all(np.isfinite(y)):
            raise ValueError("LatentAR1: y[%d] must be finite" % int(np.flatnonzero(~np.isfinite(y))[0]))
        obs_sd, mu_sd, phi_loc, phi_scale, sigma_scale = float(obs_sd), float(mu_sd), float(phi_loc), float(phi_scale), float(sigma_scale)
        for name, v in (("obs_sd", obs_sd), ("mu_sd", mu_sd), ("phi_scale", phi_scale), ("sigma_scale", sigma_scale)):
            if not (v > 0 and math.isfinite(v)):
                raise ValueError("LatentAR1: %s must be positive and finite (got %r)" % (name, v))
        if not math.isfinite(phi_loc):
            raise ValueError("LatentAR1: phi_loc must be finite (got %r)" % (phi_loc,))
        self.y, self.likelihood = y, likelihood
        self.obs_sd, self.mu_sd, self.phi_loc, self.phi_scale, self.sigma_scale = obs_sd, mu_sd, phi_loc, phi_scale, sigma_scale

    @property
    def n_obs(self):
        return self.y.size

    @property
    def dim(self):
        return self.y.size + 3

    @property
    def likelihood_code(self):
        return self.LIKELIHOODS[self.likelihood]

    def evidence_offset(self, precision):
        """what stepping_stone(pt) is off the log evidence by: stepping_stone(pt) = log p(y) + evidence_offset(p), with
        evidence_offset(p) = -(d/2) log(2 pi / p), d = dim and p the reference's precision"""
        return -(self.dim / 2.0) * math.log(2.0 * math.pi / float(precision))

    def __repr__(self):
        return "LatentAR1(%s, T=%d, dim=%d)" % (self.likelihood, self.n_obs, self.dim)


class DenseNormal:
    """The multivariate normal N(mean, precision^-1) with a dense precision matrix, the device's first family whose log potential costs
    O(d^2): an ill-conditioned Gaussian, a conjugate regression posterior, a Laplace approximation.  Exactly one of
    `precision` and `covariance` is given (dim x dim, 1 <= dim <= 512); it is symmetrised with (Q + Q') / 2 and must be positive definite.
    The density is normalised.  Tempered through the default InterpolatingPath(reference, target) (src/targets/target.jl:72-75) from
    reference=ScaledPrecisionNormalLogPotential(p, dim), unnormalised; initialization = zeros(dim); default explorer SliceSampler (target.jl:20),
    which on this family evaluates a proposal in O(1) and reads one matrix row per coordinate.

    Everything about the path is exact: chain beta is Gaussian (chain_moments), and the log evidence of the normalised target is 0, so
    stepping_stone(pt) - evidence_offset(p) estimates 0."""

    def __init__(self, mean, precision=None, *, covariance=None):
        if (precision is None) == (covariance is None):
            raise ValueError("DenseNormal: give exactly one of precision and covariance")
        mean = np.array(mean, dtype=np.float64)
        if mean.ndim != 1 or not 1 <= mean.size <= 512:
            raise ValueError("DenseNormal: mean must be a vector of 1..512 entries (got shape %s)" % (mean.shape,))
        if not np.all(np.isfinite(mean)):
            raise ValueError("DenseNormal: mean[%d] must be finite" % int(np.flatnonzero(~np.isfinite(mean))[0]))
        name = "precision" if covariance is None else "covariance"
        M = np.array(precision if covariance is None else covariance, dtype=np.float64)
        if M.ndim != 2 or M.shape != (mean.size, mean.size):
            raise ValueError("DenseNormal: %s must be %d x %d, the mean's length (got shape %s)" % (name, mean.size, mean.size, M.shape))
        if not np.all(np.isfinite(M)):
            i, j = np.argwhere(~np.isfinite(M))[0]
            raise ValueError("DenseNormal: %s[%d][%d] must be finite" % (name, i, j))
        M = (M + M.T) / 2.0
        try:
            np.linalg.cholesky(M)
        except np.linalg.LinAlgError:
            raise ValueError("DenseNormal: %s must be positive definite" % name) from None
        if covariance is not None:
            M = np.linalg.inv(M)
            M = (M + M.T) / 2.0
            try:
                np.linalg.cholesky(M)
            except np.linalg.LinAlgError:
                raise ValueError("DenseNormal: covariance is too ill-conditioned to invert to a positive-definite precision") from None
        self.mean, self.precision = mean, np.ascontiguousarray(M)

    @property
    def dim(self):
        return self.mean.size

    def evidence_offset(self, precision):
        """what stepping_stone(pt) is off the log evidence by: stepping_stone(pt) = log evidence + evidence_offset(p) with
        evidence_offset(p) = -(d/2) log(2 pi / p), d = dim and p the reference's precision; the log evidence of this normalised target is 0"""
        return -(self.dim / 2.0) * math.log(2.0 * math.pi / float(precision))

    def chain_moments(self, beta, ref_precision):
        """(mean, covariance) of chain beta of the path, exactly: its precision is P = (1 - beta) p I + beta Q and its mean P^-1 beta Q m"""
        beta, p = float(beta), float(ref_precision)
        P = (1.0 - beta) * p * np.eye(self.dim) + beta * self.precision
        cov = np.linalg.inv(P)
        cov = (cov + cov.T) / 2.0
        return cov @ (beta * (self.precision @ self.mean)), cov

    def __repr__(self):
        return "DenseNormal(dim=%d)" % self.dim


class SpikeSlabRegression:
    """Bayesian variable selection, a spike-and-slab regression: the data of BayesianGLM (X: n x d, y: n, the same two
    likelihoods) with an inclusion indicator per column.  The state is
        [theta_0..theta_{d-1}, gamma_0..gamma_{d-1}]            (dim = 2 d; theta Float64, gamma Bool stored as 0.0 / 1.0)
    the linear predictor eta_i = sum_j X[i][j] gamma_j theta_j, the prior N(0, I / p) on theta and Bernoulli(inclusion_prob) on every gamma_j
    (1 <= d <= 256, 1 <= n <= 4096, n d <= 131072).  Tempered from reference=ScaledPrecisionNormalLogPotential(p, d) on theta -- the
    prior, unnormalised -- times the uniform distribution on gamma, to prior x likelihood; initialization = zeros(2 d).  The explorer is
    SliceSampler (target.jl:20) and nothing else: its Float64 method on the thetas, its Bool method on the gammas.

    Evidence: stepping_stone(pt) estimates log p(y) - (d/2) log(2 pi / p) - d log 2 (the reference has mass (2 pi / p)^(d/2) 2^d), so the
    log evidence is stepping_stone(pt) - evidence_offset(p): see evidence_offset."""

    LIKELIHOODS = BayesianGLM.LIKELIHOODS

    def __init__(self, X, y, likelihood="bernoulli_logit", noise_sd=1.0, inclusion_prob=0.5):
        glm = BayesianGLM(X, y, likelihood=likelihood, noise_sd=noise_sd)          # the GLM family's validation of the data
        n, d = glm.X.shape
        if d > 256:
            raise ValueError("SpikeSlabRegression: the device keeps [theta, gamma] in one wave's registers, d must be in 1..256 (got %d)" % d)
        inclusion_prob = float(inclusion_prob)
        if not 0.0 < inclusion_prob < 1.0:
            raise ValueError("SpikeSlabRegression: inclusion_prob must be in (0, 1) (got %r)" % (inclusion_prob,))
        self.X, self.y, self.likelihood, self.noise_sd, self.inclusion_prob = glm.X, glm.y, likelihood, glm.noise_sd, inclusion_prob

    @property
    def n_obs(self):
        return self.X.shape[0]

    @property
    def n_columns(self):
        return self.X.shape[1]

    @property
    def dim(self):
        return 2 * self.X.shape[1]

    @property
    def likelihood_code(self):
        return self.LIKELIHOODS[self.likelihood]

    def evidence_offset(self, precision):
        """what stepping_stone(pt) is off the log evidence by: stepping_stone(pt) = log p(y) + evidence_offset(p), with
        evidence_offset(p) = -(d/2) log(2 pi / p) - d log 2 and p the reference's precision"""
        d = self.n_columns
        return -(d / 2.0) * math.log(2.0 * math.pi / float(precision)) - d * math.log(2.0)

    def __repr__(self):
        return "SpikeSlabRegression(%s, n=%d, d=%d, inclusion_prob=%g)" % (self.likelihood, self.n_obs, self.n_columns, self.inclusion_prob)


class PoissonChangePoint:
    """Multiple change-point detection on count data: n counts y_i, K = n_changepoints change points, K + 1 segments with a
    Poisson rate each.  The state is
        [r_0..r_K, tau_1..tau_K]            (dim = 2 K + 1; the log rates Float64, the change points Integer stored as integral doubles)
    every tau_k in 0..n and the taus unordered: with s_1 <= ... <= s_K the sorted taus, s_0 = 0 and s_{K+1} = n, segment j covers observations
    [s_j, s_{j+1}) with y_i ~ Poisson(exp(r_j)); the prior is N(0, I / p) on r and uniform on the (n + 1)^K placements
    (1 <= K <= 63, 1 <= n <= 65536, every y_i an integer in 0..2^20).  Tempered from reference=ScaledPrecisionNormalLogPotential(p, K + 1)
    on r -- the prior, unnormalised -- times the uniform distribution on tau, to prior x likelihood; initialization = zeros(2 K + 1).  The
    explorer is SliceSampler (target.jl:20) and nothing else: its Float64 method on the rates, its Integer method on the change points, so
    its width w must be integral.

    Evidence: stepping_stone(pt) estimates log p(y) - ((K+1)/2) log(2 pi / p) - K log(n + 1) (the reference has mass
    (2 pi / p)^((K+1)/2) (n + 1)^K), so the log evidence is stepping_stone(pt) - evidence_offset(p): see evidence_offset."""

    def __init__(self, y, n_changepoints):
        y = np.ascontiguousarray(y, dtype=np.float64)
        if y.ndim != 1 or not 1 <= y.size <= 65536:
            raise ValueError("PoissonChangePoint: y must be a vector of 1..65536 observations (got shape %s)" % (y.shape,))
        if not np.all(np.isfinite(y)) or np.any(y != np.floor(y)) or np.any(y < 0) or np.any(y > 2 ** 20):
            raise ValueError("PoissonChangePoint: every y must be an integer count in 0..2^20")
        K = int(n_changepoints)
        if K != n_changepoints or not 1 <= K <= 63:
            raise ValueError("PoissonChangePoint: the device gives every segment a lane of one wave, n_changepoints must be in 1..63 (got %r)"
                             % (n_changepoints,))
        self.y, self.n_changepoints = y, K

    @property
    def n_obs(self):
        return self.y.size

    @property
    def n_rates(self):
        return self.n_changepoints + 1

    @property
    def dim(self):
        return 2 * self.n_changepoints + 1

    def evidence_offset(self, precision):
        """what stepping_stone(pt) is off the log evidence by: stepping_stone(pt) = log p(y) + evidence_offset(p), with
        evidence_offset(p) = -((K+1)/2) log(2 pi / p) - K log(n + 1) and p the reference's precision"""
        K = self.n_changepoints
        return -((K + 1) / 2.0) * math.log(2.0 * math.pi / float(precision)) - K * math.log(self.n_obs + 1.0)

    def __repr__(self):
        return "PoissonChangePoint(n=%d, K=%d)" % (self.n_obs, self.n_changepoints)


@dataclass
class GaussianReference:
    """src/variational/GaussianReference.jl:4-17: mean-field Gaussian variational reference, refitted every round from
    the target chains' online mean / standard deviation once `first_tuning_round` is reached."""
    mean: Any = None
    standard_deviation: Any = None
    first_tuning_round: int = 6


@dataclass
class InterpolatingPath:
    """src/paths/InterpolatingPath.jl: (1 - beta) ref + beta target; what update_path_variational builds
    (src/variational/variational.jl:36-41)."""
    ref: Any = None
    target: Any = None


@dataclass
class IsingLogPotential:
    """2-D Ising model, p(state) ∝ exp(beta * sum of neighbour products) (reference examples/ising.jl:6-9,74).
    The reference distribution is IsingLogPotential(0.0, base_length) (ising.jl:77); states are
    base_length x base_length spin matrices, exposed here as 0/1 vectors in row-major order."""
    beta: float = 1.0
    base_length: int = 5


class SpinGlassLogPotential:
    """The +-J Edwards-Anderson spin glass on the L x L periodic lattice: p(state) ∝ exp(beta * S), S = sum_ij s_ij (bonds_right_ij s_i,j+1 +
    bonds_down_ij s_i+1,j) -- IsingLogPotential with every neighbour product multiplied by a quenched bond in {+1, -1} (at L = 2 the two bonds
    between the same pair of sites are distinct terms).  The reference is beta = 0; states are 0/1 vectors in row-major order, explored by
    IsingMetropolis.  Bonds are +-1 only: real-valued or diluted couplings are not available on the device."""

    def __init__(self, beta, bonds_right, bonds_down):
        planes = []
        for name, b in (("bonds_right", bonds_right), ("bonds_down", bonds_down)):
            a = np.asarray(b)
            if a.ndim != 2 or a.shape[0] != a.shape[1] or a.shape[0] < 2:
                raise ValueError("SpinGlassLogPotential: %s must be L x L with L >= 2 (got shape %s)" % (name, a.shape))
            if a.size > 65536:
                raise ValueError("SpinGlassLogPotential: the device holds lattices of at most 65536 sites (got %s = %d x %d)" % (name, a.shape[0], a.shape[1]))
            planes.append(a)
        if planes[0].shape != planes[1].shape:
            raise ValueError("SpinGlassLogPotential: bonds_right and bonds_down must have the same shape (got %s and %s)" % (planes[0].shape, planes[1].shape))
        for name, a in zip(("bonds_right", "bonds_down"), planes):
            bad = np.argwhere(~((a == 1) | (a == -1)))
            if len(bad):
                i, j = (int(v) for v in bad[0])
                raise ValueError("SpinGlassLogPotential: %s[%d][%d] must be +1 or -1 (got %r): ±J is the supported disorder, "
                                 "real-valued or diluted couplings are out of scope" % (name, i, j, a[i, j].item()))
        self.beta = float(beta)
        self.bonds_right = np.ascontiguousarray(planes[0], dtype=np.int8)
        self.bonds_down = np.ascontiguousarray(planes[1], dtype=np.int8)

    @classmethod
    def edwards_anderson(cls, beta, base_length, seed=1):
        """both planes drawn +-1 with probability 1/2 each from np.random.default_rng(seed): bonds_right first, then bonds_down"""
        rng = np.random.default_rng(seed)
        L = int(base_length)
        right = (2 * rng.integers(0, 2, size=(L, L)) - 1).astype(np.int8)
        down = (2 * rng.integers(0, 2, size=(L, L)) - 1).astype(np.int8)
        return cls(beta, right, down)

    @property
    def base_length(self):
        return int(self.bonds_right.shape[0])

    @property
    def dim(self):
        return self.base_length ** 2

    def __repr__(self):
        return "SpinGlassLogPotential(beta=%r, base_length=%d)" % (self.beta, self.base_length)


class SpinGlass3DLogPotential:
    """The +-J Edwards-Anderson spin glass on the L x L x L periodic lattice, L even and in 2..32 (the project's own
    specification): p(state) ∝ exp(beta * S), S = sum s_zyx (bonds_x_zyx s_z,y,x+1 + bonds_y_zyx s_z,y+1,x + bonds_z_zyx s_z+1,y,x) (at L = 2
    the two bonds between the same pair of sites are distinct terms).  The planes are [L][L][L] in the order [z][y][x]; the reference is
    beta = 0; states are 0/1 vectors in that (C) order, explored by CheckerboardMetropolis.  Bonds are +-1 only."""

    def __init__(self, beta, bonds_x, bonds_y, bonds_z):
        names = ("bonds_x", "bonds_y", "bonds_z")
        planes = []
        for name, b in zip(names, (bonds_x, bonds_y, bonds_z)):
            a = np.asarray(b)
            if a.ndim != 3 or a.shape[0] != a.shape[1] or a.shape[0] != a.shape[2] or a.shape[0] < 2:
                raise ValueError("SpinGlass3DLogPotential: %s must be L x L x L with L >= 2 (got shape %s)" % (name, a.shape))
            if a.shape[0] % 2 != 0:
                raise ValueError("SpinGlass3DLogPotential: base_length must be even (got %s of shape %s): on an odd periodic lattice two sites of "
                                 "one colour would be neighbours" % (name, a.shape))
            if a.shape[0] > 32:
                raise ValueError("SpinGlass3DLogPotential: base_length must be at most 32 (got %s of shape %s): the device holds a row of the "
                                 "lattice in one 32-bit word" % (name, a.shape))
            planes.append(a)
        if planes[0].shape != planes[1].shape or planes[0].shape != planes[2].shape:
            raise ValueError("SpinGlass3DLogPotential: bonds_x, bonds_y and bonds_z must have the same shape (got %s, %s and %s)"
                             % tuple(a.shape for a in planes))
        for name, a in zip(names, planes):
            bad = np.argwhere(~((a == 1) | (a == -1)))
            if len(bad):
                z, y, x = (int(v) for v in bad[0])
                raise ValueError("SpinGlass3DLogPotential: %s[%d][%d][%d] must be +1 or -1 (got %r): ±J is the supported disorder, "
                                 "real-valued or diluted couplings are out of scope" % (name, z, y, x, a[z, y, x].item()))
        self.beta = float(beta)
        self.bonds_x, self.bonds_y, self.bonds_z = (np.ascontiguousarray(a, dtype=np.int8) for a in planes)

    @classmethod
    def edwards_anderson(cls, beta, base_length, seed=1):
        """the three planes drawn +-1 with probability 1/2 each from np.random.default_rng(seed): bonds_x first, then bonds_y, then bonds_z"""
        rng = np.random.default_rng(seed)
        L = cls._checked_length(base_length)
        return cls(beta, *[(2 * rng.integers(0, 2, size=(L, L, L)) - 1).astype(np.int8) for _ in range(3)])

    @classmethod
    def ferromagnet(cls, beta, base_length):
        """every bond +1: the 3-D Ising model"""
        L = cls._checked_length(base_length)
        return cls(beta, *[np.ones((L, L, L), dtype=np.int8) for _ in range(3)])

    @staticmethod
    def _checked_length(base_length):
        L = int(base_length)
        if L < 2 or L % 2 != 0 or L > 32:
            raise ValueError("SpinGlass3DLogPotential: base_length must be even and in 2..32 (got %d)" % L)
        return L

    @property
    def base_length(self):
        return int(self.bonds_x.shape[0])

    @property
    def dim(self):
        return self.base_length ** 3

    def __repr__(self):
        return "SpinGlass3DLogPotential(beta=%r, base_length=%d)" % (self.beta, self.base_length)


@dataclass
class IsingMetropolis:
    """examples/ising.jl:91-93"""
    n_steps: int = 3


@dataclass
class CheckerboardMetropolis:
    """The two-colour (red / black) Metropolis sweep of IsingLogPotential and SpinGlassLogPotential (the project's own
    specification): n_steps sweeps of two half-sweeps each, all sites of a colour decided at once.  base_length must be even."""
    n_steps: int = 3


@dataclass
class TestSwapper:
    """src/swap/pair_swapper.jl:100-149"""
    constant_swap_accept_pr: float = 1.0
    __test__ = False


# ---- explorers (src/explorers/*.jl) ------------------------------------------------------------
@dataclass
class SliceSampler:
    """src/explorers/SliceSampler.jl:8-20"""
    w: float = 10.0
    p: int = 20
    n_passes: int = 3
    max_iter: int = 1024


@dataclass
class ToyExplorer:
    """src/explorers/ToyExplorer.jl:5"""


@dataclass
class IdentityPreconditioner:
    """src/explorers/Preconditioner.jl:14"""


@dataclass
class DiagonalPreconditioner:
    """src/explorers/Preconditioner.jl:22"""


@dataclass
class MixDiagonalPreconditioner:
    """src/explorers/Preconditioner.jl:43-52 (default proportions 1//3, 1//3)"""
    p0: float = 1.0 / 3.0
    p1: float = 1.0 / 3.0


@dataclass
class AutoMALA:
    """src/explorers/AutoMALA.jl:29-68"""
    base_n_refresh: int = 3
    exponent_n_refresh: float = 0.35
    step_size: float = 1.0
    preconditioner: Any = field(default_factory=MixDiagonalPreconditioner)
    estimated_target_std_deviations: Any = None


@dataclass
class MALA:
    """src/explorers/MALA.jl:19-61 (the step size is NOT adapted; the preconditioner is)"""
    base_n_refresh: int = 3
    exponent_n_refresh: float = 0.35
    step_size: float = 1.0
    preconditioner: Any = field(default_factory=MixDiagonalPreconditioner)
    estimated_target_std_deviations: Any = None


@dataclass
class AAPS:
    """src/explorers/AAPS.jl: the apogee-to-apogee path sampler (Sherlock, Urbas & Ludkin, JCGS 2023).  One transition per explore!;
    K segments besides the current one; the step size is NOT adapted, the preconditioner is (as MALA's)."""
    step_size: float = 1.0
    K: int = 5
    preconditioner: Any = field(default_factory=MixDiagonalPreconditioner)
    estimated_target_std_deviations: Any = None


@dataclass
class Compose:
    """src/explorers/Compose.jl:5-8: deterministic composition, e.g. Compose(SliceSampler(), AutoMALA())"""
    first: Any = None
    second: Any = None


def default_explorer(target):
    if isinstance(target, ScaledPrecisionNormalPath):
        return ToyExplorer()           # src/targets/toy_mvn_target.jl:13
    if isinstance(target, TestSwapper):
        return None                    # src/swap/pair_swapper.jl:139
    if isinstance(target, (IsingLogPotential, SpinGlassLogPotential)):
        return IsingMetropolis()       # examples/ising.jl:94
    if isinstance(target, SpinGlass3DLogPotential):
        return CheckerboardMetropolis()    # the family's one explorer
    return SliceSampler()              # src/targets/target.jl:20


# ---- recorder builders (src/recorders/recorder.jl) ----------------------------------------------
def log_sum_ratio(): return "log_sum_ratio"
def swap_acceptance_pr(): return "swap_acceptance_pr"
def round_trip(): return "round_trip"
def index_process(): return "index_process"
def online(): return "online"
def traces(): return "traces"
def energy_ac1(): return "energy_ac1"
def timing_extrema(): return "timing_extrema"
def allocation_extrema(): return "allocation_extrema"
def explorer_acceptance_pr(): return "explorer_acceptance_pr"
def explorer_n_steps(): return "explorer_n_steps"


def record_default():
    """src/pt/Inputs.jl:107-111"""
    return [log_sum_ratio, timing_extrema, allocation_extrema]


def record_online():
    """src/pt/Inputs.jl:116-123"""
    return [log_sum_ratio, timing_extrema, allocation_extrema, round_trip, energy_ac1, online]


@dataclass
class Inputs:
    """src/pt/Inputs.jl:9-102 (fields the hot path reads)."""
    target: Any = None
    seed: int = 1
    n_rounds: int = 10
    n_chains: int = 10
    n_chains_variational: int = 0
    reference: Any = None
    variational: Any = None
    checkpoint: bool = False
    record: List = field(default_factory=record_default)
    checked_round: int = 0
    multithreaded: bool = False
    explorer: Any = None
    extractor: Any = None
    show_report: bool = True
    extended_traces: bool = False
    device: int = 0                 # HIP device ordinal (not in the reference)


@dataclass
class Iterators:
    """src/pt/Iterators.jl:9-25"""
    round: int = 0
    scan: int = 0


def n_scans_in_round(iterators):
    return 2 ** iterators.round


@dataclass
class ReducedRecorders:
    """The reduced `recorders` NamedTuple of one round (src/recorders/recorders.jl:88-120)."""
    swap_acceptance_pr: Any = None      # (mean[N-1], n[N-1]) keyed (c, c+1)
    log_sum_ratio: Any = None           # (up[N-1], up_n, dn[N-1], dn_n)
    round_trip: Any = None              # (n_tempered_restarts, n_round_trips)
    index_process: Any = None           # int64 [replica][scan]
    explorer_acceptance_pr: Any = None  # (mean[N], n[N]) keyed by chain
    explorer_n_steps: Any = None        # (sum[N], n[N])
    am_factors: Any = None              # (mean[N], n[N])       src/explorers/AutoMALA.jl:277
    reversibility_rate: Any = None      # (mean[N], n[N])       src/explorers/AutoMALA.jl:294
    online: Any = None                  # (mean[d], var[d], n)
    online_log_density: Any = None      # (mean, var): entry d+1 of the online sample [state; log density]
    energy_ac1: Any = None              # (cor[N], n[N], moments[N,5]) keyed by chain      recorder.jl:113
    traces: Any = None                  # float64 [scan][d+1], target chain               recorder.jl:27
    timing_extrema: Any = None          # {"round": seconds}


@dataclass
class NonReversiblePT:
    """src/tempering/NonReversiblePT.jl:7-50"""
    path: Any
    schedule: T.Schedule
    communication_barriers: Optional[T.CommunicationBarriers] = None


@dataclass
class StabilizedPT:
    """src/tempering/StabilizedPT.jl:8-51 with inputs.variational == nothing (both legs keep the fixed reference).
    Global chain order (1-based i): i <= n_var -> variational leg chain i; i > n_var -> fixed leg chain
    n_fixed - (i - n_var) + 1 (create_replica_indexer, :86-104)."""
    fixed_leg: NonReversiblePT
    variational_leg: NonReversiblePT

    @property
    def n_fixed(self): return len(self.fixed_leg.schedule.grids)

    @property
    def n_var(self): return len(self.variational_leg.schedule.grids)

    @property
    def path(self): return self.fixed_leg.path

    @property
    def schedule(self):
        """per-chain grid in global chain order (concatenate_log_potentials, :67-69)"""
        return T.Schedule(np.concatenate([self.variational_leg.schedule.grids, self.fixed_leg.schedule.grids[::-1]]), check=False)

    @property
    def communication_barriers(self): return self.fixed_leg.communication_barriers      # global_barrier(::StabilizedPT), :115

    def is_reference(self, chain): return chain == 1 or chain == self.n_fixed + self.n_var           # VariationalDEO.jl:20
    def is_target(self, chain): return chain == self.n_var or chain == self.n_var + 1                # VariationalDEO.jl:21
    def leg_of(self, chain): return "variational" if chain <= self.n_var else "fixed"                 # indexer.i2t


@dataclass
class Shared:
    """src/pt/Shared.jl:12-48"""
    iterators: Iterators
    tempering: NonReversiblePT
    explorer: Any
    reports: list


class PT:
    """src/pt/PT.jl:6-51.  `replicas` is the device engine.

    Sharding (not in the reference's PT; replaces its MPI `EntangledReplicas`):
      n_shards=G           G chain-shards driven from this process (LoopbackShards; single-GPU tests;
                           device_messages=True: the device-resident exchange kernels of the RCCL path)
                           transport="group": the library's own pte_group_run_scans
      rank=r, world=G      this process owns shard r of G.  HIP engines: RcclShard -- the boundary exchange is RCCL
                           send/recv inside libpte (pte_comm_init; comm_id = the 128-byte id if the caller already
                           distributed it, else it is broadcast over torch.distributed).  transport="host" (and
                           engines without comm_init: the CPU tests' oracle shards): DistShard, host-driven over gloo.
    debug_kernel           pte_config.debug_kernel (0 = the default kernel)
    reference_reduction    PTE_RECORD_REFERENCE_REDUCTION: swap_acceptance_pr / log_sum_ratio from per-replica Mean / LogSum fits merged over
                           the replica-index tree (src/recorders/recorders.jl:88-130, src/mpi_utils/Entangler.jl:188-251) instead of the
                           device's chain-keyed sums -- the adapted schedule then equals the oracle's bit for bit (chain-shards replay their own pairs).
    """

    def __init__(self, inputs: Inputs, n_shards=1, rank=0, world=1, dist_device=None, engine_factory=None, device_messages=False,
                 transport=None, comm_id=None, debug_kernel=0, reference_reduction=False):
        self.inputs = inputs
        target = inputs.target
        explorer = inputs.explorer if inputs.explorer is not None else default_explorer(target)
        N = inputs.n_chains
        n_var = int(getattr(inputs, "n_chains_variational", 0) or 0)
        if n_var > 0 and N > 0:                         # create_tempering, src/tempering/tempering.jl:64-70
            tempering = StabilizedPT(NonReversiblePT(target, T.equally_spaced_schedule(N)),
                                     NonReversiblePT(target, T.equally_spaced_schedule(n_var)))
        else:
            tempering = NonReversiblePT(target, T.equally_spaced_schedule(N))
        self.shared = Shared(Iterators(), tempering, explorer, [])
        self.reduced_recorders = ReducedRecorders()
        names = {b() for b in inputs.record}
        flags = 0
        if "round_trip" in names:
            flags |= _lib.RECORD_ROUND_TRIP
        if "index_process" in names:
            flags |= _lib.RECORD_INDEX_PROCESS
        if "online" in names:
            flags |= _lib.RECORD_ONLINE
        if inputs.variational is not None:
            if not isinstance(inputs.variational, GaussianReference) or not isinstance(target, Funnel):
                raise NotImplementedError("the device engine has GaussianReference on the interpolated (funnel) path only")
            flags |= _lib.RECORD_ONLINE                 # variational_recorder_builders: _transformed_online
        if "traces" in names:
            flags |= _lib.RECORD_TRACES
            if getattr(inputs, "extended_traces", False):
                flags |= _lib.RECORD_TRACES_EXTENDED
        if "energy_ac1" in names:
            flags |= _lib.RECORD_ENERGY_AC1
        if reference_reduction:
            flags |= _lib.RECORD_REFERENCE_REDUCTION | _lib.RECORD_INDEX_PROCESS
        kw = dict(device=inputs.device, n_chains=N, n_chains_variational=n_var, seed=inputs.seed, record_flags=flags,
                  max_scans_per_round=2 ** inputs.n_rounds)
        if isinstance(explorer, CheckerboardMetropolis) and isinstance(target, (IsingLogPotential, SpinGlassLogPotential)) and target.base_length % 2 != 0:
            raise ValueError("CheckerboardMetropolis needs an even base_length (got %d): on an odd periodic lattice two sites of one colour "
                             "would be neighbours" % target.base_length)
        if isinstance(target, ScaledPrecisionNormalPath):
            kw.update(target=_lib.TARGET_MVN_SCALED_PRECISION, dim=target.dim,
                      target_params=[target.precision0, target.precision1])
        elif isinstance(target, TestSwapper):
            kw.update(target=_lib.TARGET_TEST_SWAPPER, dim=1, target_params=[target.constant_swap_accept_pr])
        elif isinstance(target, IsingLogPotential):
            kw.update(target=_lib.TARGET_ISING, dim=target.base_length ** 2, target_params=[target.beta])
        elif isinstance(target, SpinGlassLogPotential):
            if not isinstance(explorer, (IsingMetropolis, CheckerboardMetropolis)):
                raise NotImplementedError("the device spin-glass path is explored by IsingMetropolis only (got %r)" % (explorer,))
            kw.update(target=_lib.TARGET_SPIN_GLASS, dim=target.dim, target_params=[target.beta])
        elif isinstance(target, SpinGlass3DLogPotential):
            if not isinstance(explorer, CheckerboardMetropolis):
                raise NotImplementedError("the device 3-D spin-glass path is explored by CheckerboardMetropolis only (got %r)" % (explorer,))
            kw.update(target=_lib.TARGET_SPIN_GLASS_3D, dim=target.dim, target_params=[target.beta])
        elif isinstance(target, Funnel):
            ref = inputs.reference
            if not isinstance(ref, ScaledPrecisionNormalLogPotential) or ref.dim != target.dim:
                raise NotImplementedError("the device funnel path needs reference=ScaledPrecisionNormalLogPotential(prec, dim)")
            kw.update(target=_lib.TARGET_FUNNEL, dim=target.dim, target_params=[ref.precision])
        elif isinstance(target, GaussianMixture):
            ref = inputs.reference
            if not isinstance(ref, ScaledPrecisionNormalLogPotential) or ref.dim != target.dim:
                raise NotImplementedError("the device Gaussian-mixture path needs reference=ScaledPrecisionNormalLogPotential(prec, dim)")
            kw.update(target=_lib.TARGET_GAUSSIAN_MIXTURE, dim=target.dim, target_params=[ref.precision])
        elif isinstance(target, BayesianGLM):
            ref = inputs.reference
            if not isinstance(ref, ScaledPrecisionNormalLogPotential) or ref.dim != target.dim:
                raise NotImplementedError("the device Bayesian-GLM path needs reference=ScaledPrecisionNormalLogPotential(prec, dim) -- the prior")
            kw.update(target=_lib.TARGET_BAYESIAN_GLM, dim=target.dim, target_params=[ref.precision])
        elif isinstance(target, MixtureModelPosterior):
            ref = inputs.reference
            if not isinstance(ref, ScaledPrecisionNormalLogPotential) or ref.dim != target.dim:
                raise NotImplementedError("the device mixture-model path needs reference=ScaledPrecisionNormalLogPotential(prec, dim) -- the prior")
            kw.update(target=_lib.TARGET_MIXTURE_MODEL, dim=target.dim, target_params=[ref.precision])
        elif isinstance(target, HierarchicalNormalMeans):
            ref = inputs.reference
            if not isinstance(ref, ScaledPrecisionNormalLogPotential) or ref.dim != target.dim:
                raise NotImplementedError("the device hierarchical-normal path needs reference=ScaledPrecisionNormalLogPotential(prec, dim)")
            kw.update(target=_lib.TARGET_HIERARCHICAL_NORMAL, dim=target.dim, target_params=[ref.precision])
        elif isinstance(target, LatentAR1):
            ref = inputs.reference
            if not isinstance(ref, ScaledPrecisionNormalLogPotential) or ref.dim != target.dim:
                raise NotImplementedError("the device latent-AR(1) path needs reference=ScaledPrecisionNormalLogPotential(prec, dim)")
            kw.update(target=_lib.TARGET_LATENT_AR1, dim=target.dim, target_params=[ref.precision])
        elif isinstance(target, DenseNormal):
            ref = inputs.reference
            if not isinstance(ref, ScaledPrecisionNormalLogPotential) or ref.dim != target.dim:
                raise NotImplementedError("the device dense-normal path needs reference=ScaledPrecisionNormalLogPotential(prec, dim)")
            kw.update(target=_lib.TARGET_DENSE_NORMAL, dim=target.dim, target_params=[ref.precision])
        elif isinstance(target, SpikeSlabRegression):
            ref = inputs.reference
            if not isinstance(ref, ScaledPrecisionNormalLogPotential) or ref.dim != target.n_columns:
                raise NotImplementedError("the device variable-selection path needs reference=ScaledPrecisionNormalLogPotential(prec, d) "
                                          "-- the prior of the d coefficients")
            if not isinstance(explorer, SliceSampler):
                raise NotImplementedError("the device variable-selection path is explored by SliceSampler only (got %r)" % (explorer,))
            kw.update(target=_lib.TARGET_VARIABLE_SELECTION, dim=target.dim, target_params=[ref.precision])
        elif isinstance(target, PoissonChangePoint):
            ref = inputs.reference
            if not isinstance(ref, ScaledPrecisionNormalLogPotential) or ref.dim != target.n_rates:
                raise NotImplementedError("the device change-point path needs reference=ScaledPrecisionNormalLogPotential(prec, K + 1) "
                                          "-- the prior of the K + 1 log rates")
            if not isinstance(explorer, SliceSampler):
                raise NotImplementedError("the device change-point path is explored by SliceSampler only (got %r)" % (explorer,))
            kw.update(target=_lib.TARGET_CHANGE_POINT, dim=target.dim, target_params=[ref.precision])
        else:
            raise NotImplementedError(
                "target %r has no device log-potential; use the reference CPU path (Pigeons.jl)" % (target,))
        def explorer_kw(ex):
            if ex is None:
                return dict(explorer=_lib.EXPLORER_NONE)
            if isinstance(ex, ToyExplorer):
                return dict(explorer=_lib.EXPLORER_TOY)
            if isinstance(ex, SliceSampler):
                return dict(explorer=_lib.EXPLORER_SLICE, slice_w=ex.w, slice_p=ex.p, slice_n_passes=ex.n_passes,
                            slice_max_iter=ex.max_iter)
            if isinstance(ex, IsingMetropolis):
                return dict(explorer=_lib.EXPLORER_ISING_METROPOLIS, slice_n_passes=ex.n_steps)
            if isinstance(ex, CheckerboardMetropolis):
                return dict(explorer=_lib.EXPLORER_CHECKERBOARD_METROPOLIS, slice_n_passes=ex.n_steps)
            if isinstance(ex, AAPS):
                pc = ex.preconditioner
                kind = 0 if isinstance(pc, IdentityPreconditioner) else 1 if isinstance(pc, DiagonalPreconditioner) else 2
                return dict(explorer=_lib.EXPLORER_AAPS, am_step_size=ex.step_size, aaps_K=ex.K, am_preconditioner=kind,
                            am_p0=getattr(pc, "p0", 0.0), am_p1=getattr(pc, "p1", 0.0))
            if isinstance(ex, (AutoMALA, MALA)):
                pc = ex.preconditioner
                kind = 0 if isinstance(pc, IdentityPreconditioner) else 1 if isinstance(pc, DiagonalPreconditioner) else 2
                return dict(explorer=_lib.EXPLORER_AUTOMALA if isinstance(ex, AutoMALA) else _lib.EXPLORER_MALA,
                            am_base_n_refresh=ex.base_n_refresh, am_exponent_n_refresh=ex.exponent_n_refresh,
                            am_step_size=ex.step_size, am_preconditioner=kind, am_p0=getattr(pc, "p0", 0.0),
                            am_p1=getattr(pc, "p1", 0.0))
            raise NotImplementedError("explorer %r is not available on the device" % (ex,))
        if isinstance(explorer, Compose):
            if isinstance(explorer.first, Compose) or isinstance(explorer.second, Compose):
                raise NotImplementedError("nested Compose is not available on the device")
            if isinstance(explorer.first, AAPS) or isinstance(explorer.second, AAPS):
                raise NotImplementedError("AAPS is not available as half of a Compose on the device")
            k1, k2 = explorer_kw(explorer.first), explorer_kw(explorer.second)
            shared_keys = (set(k1) & set(k2)) - {"explorer"}
            if any(k1[k] != k2[k] for k in shared_keys):
                raise NotImplementedError("Compose of two samplers of the same family needs identical parameters on the device")
            kw.update(k1); kw.update({k: v for k, v in k2.items() if k != "explorer"}); kw.update(explorer2=k2["explorer"])
        else:
            kw.update(explorer_kw(explorer))
        make = engine_factory or Engine
        if debug_kernel:
            kw.update(debug_kernel=debug_kernel)
            if (debug_kernel & ~(_lib.KERNEL_FLAG_BITS | _lib.KERNEL_TEST_BITS)) not in (0, _lib.KERNEL_SLICE_SEQUENTIAL, _lib.KERNEL_ISING_BYTES) or (debug_kernel & _lib.KERNEL_TEST_BITS):
                kw.update(test_build=True)              # the dominated generations live in libpte_test.so only
        self.shards = None
        if n_shards > 1:
            from .sharded import LoopbackShards
            self.shards = LoopbackShards([make(rank=g, world_size=n_shards, **kw) for g in range(n_shards)], device_messages=device_messages,
                                         transport=transport)
            self.replicas = self.shards.engines[0]
        elif world > 1:
            from .sharded import DistShard, RcclShard
            self.replicas = make(rank=rank, world_size=world, **kw)
            if transport != "host" and hasattr(self.replicas, "comm_init"):
                self.shards = RcclShard(self.replicas, rank, world, id_bytes=comm_id)
            else:
                self.shards = DistShard(self.replicas, rank, world, device=dist_device)
        else:
            self.replicas = make(**kw)
        if isinstance(target, GaussianMixture):          # every engine (rank) holds the components
            for eng in (self.shards.engines if hasattr(self.shards, "engines") else [self.replicas]):
                eng.set_target_mixture(target.weights, target.means, target.std_devs)
        if isinstance(target, BayesianGLM):              # every engine (rank) holds the data
            for eng in (self.shards.engines if hasattr(self.shards, "engines") else [self.replicas]):
                eng.set_target_glm(target.likelihood_code, target.X, target.y, target.noise_sd)
        if isinstance(target, MixtureModelPosterior):    # every engine (rank) holds the observations
            for eng in (self.shards.engines if hasattr(self.shards, "engines") else [self.replicas]):
                eng.set_target_mixture_model(target.y)
        if isinstance(target, HierarchicalNormalMeans):  # every engine (rank) holds the data
            for eng in (self.shards.engines if hasattr(self.shards, "engines") else [self.replicas]):
                eng.set_target_hier(target.parameterization_code, target.y, target.sigma, target.mu_sd, target.tau_scale)
        if isinstance(target, LatentAR1):                # every engine (rank) holds the data
            for eng in (self.shards.engines if hasattr(self.shards, "engines") else [self.replicas]):
                eng.set_target_ar1(target.likelihood_code, target.y, target.obs_sd, target.mu_sd, target.phi_loc, target.phi_scale, target.sigma_scale)
        if isinstance(target, DenseNormal):              # every engine (rank) holds the data
            for eng in (self.shards.engines if hasattr(self.shards, "engines") else [self.replicas]):
                eng.set_target_dense(target.mean, target.precision)
        if isinstance(target, SpinGlassLogPotential):    # every engine (rank) holds the bonds
            for eng in (self.shards.engines if hasattr(self.shards, "engines") else [self.replicas]):
                eng.set_target_spin_glass(target.bonds_right, target.bonds_down)
        if isinstance(target, SpinGlass3DLogPotential):  # every engine (rank) holds the bonds
            for eng in (self.shards.engines if hasattr(self.shards, "engines") else [self.replicas]):
                eng.set_target_spin_glass_3d(target.bonds_x, target.bonds_y, target.bonds_z)
        if isinstance(target, SpikeSlabRegression):      # every engine (rank) holds the data
            for eng in (self.shards.engines if hasattr(self.shards, "engines") else [self.replicas]):
                eng.set_target_varsel(target.likelihood_code, target.X, target.y, target.noise_sd, target.inclusion_prob)
        if isinstance(target, PoissonChangePoint):       # every engine (rank) holds the data
            for eng in (self.shards.engines if hasattr(self.shards, "engines") else [self.replicas]):
                eng.set_target_changepoint(target.y)


def next_round(pt):
    """src/pt/Iterators.jl:27-35"""
    it = pt.shared.iterators
    if it.round + 1 <= pt.inputs.n_rounds:
        it.round += 1
        return True
    return False


def run_one_round(pt):
    """src/pt/pigeons.jl:46-55: the scan loop runs fused on the device."""
    it = pt.shared.iterators
    eng = pt.shards if pt.shards is not None else pt.replicas
    n = n_scans_in_round(it)
    t0 = time.perf_counter()
    eng.run_scans(1, n)                  # explore!; communicate! for scan = 1..2^round (synchronous)
    elapsed = time.perf_counter() - t0
    it.scan = 0
    return reduce_recorders(pt, elapsed)


def reduce_recorders(pt, elapsed=None):
    """src/recorders/recorders.jl:88-120"""
    if pt.shards is not None:
        r = pt.shards.reduce()
        r.timing_extrema = {"round": elapsed}
        return r
    eng = pt.replicas
    eng.reduce()
    am, an, ss, sn = eng.explorer_stats()
    fm, fn, rm, rn = eng.automala_stats()
    r = ReducedRecorders(
        am_factors=(fm, fn), reversibility_rate=(rm, rn),
        swap_acceptance_pr=eng.swap_acceptance(),
        log_sum_ratio=eng.log_sum_ratio(),
        round_trip=eng.round_trip(),
        index_process=eng.index_process(),
        explorer_acceptance_pr=(am, an),
        explorer_n_steps=(ss, sn),
        online=eng.online(),
        online_log_density=eng.online_log_density(),
        energy_ac1=eng.energy_ac1(),
        traces=eng.traces(),
        timing_extrema={"round": elapsed},
    )
    return r


def adapt(pt, reduced):
    """src/pt/pigeons.jl:152-162 with adapt_tempering (src/tempering/NonReversiblePT.jl:52-66)."""
    temp = pt.shared.tempering
    pt.reduced_recorders = reduced
    adapt_explorer(pt, reduced)
    update_variational(pt, reduced)
    if isinstance(pt.inputs.target, TestSwapper) or len(temp.schedule.grids) == 1:
        return pt
    mean, n = reduced.swap_acceptance_pr
    rej = T.rejections(mean, n)
    if isinstance(temp, StabilizedPT):
        # adapt_tempering(::StabilizedPT) (StabilizedPT.jl:53-65): each leg from its own pairs; the fixed leg reads
        # (N-1,N), (N-2,N-1), ... from its reference towards the target
        nv, nf, Ntot = temp.n_var, temp.n_fixed, temp.n_var + temp.n_fixed
        legs = []
        for leg, r in ((temp.variational_leg, rej[:nv - 1]), (temp.fixed_leg, rej[Ntot - 2 - np.arange(nf - 1)] if nf > 1 else rej[:0])):
            old = leg.schedule.grids
            if len(old) == 1:
                legs.append(leg); continue
            legs.append(NonReversiblePT(leg.path, T.Schedule(T.optimal_schedule(r, old, len(old))), T.CommunicationBarriers(r, old)))
        pt.shared.tempering = StabilizedPT(fixed_leg=legs[1], variational_leg=legs[0])
        pt.replicas.set_schedule(pt.shared.tempering.schedule.grids)
        return pt
    old = temp.schedule.grids
    new_sched = T.Schedule(T.optimal_schedule(rej, old, len(old)))
    barriers = T.CommunicationBarriers(rej, old)
    pt.shared.tempering = NonReversiblePT(temp.path, new_sched, barriers)
    (pt.shards if pt.shards is not None else pt.replicas).set_schedule(new_sched.grids)   # discretize on the device
    return pt


def update_variational(pt, reduced):
    """update_path_if_needed (src/variational/variational.jl:28-41): from first_tuning_round on, refit the
    GaussianReference to the target chains' online statistics and put it at the reference end of the variational leg
    (of the only leg when there is one)."""
    var = pt.inputs.variational
    if not isinstance(var, GaussianReference) or pt.shared.iterators.round < var.first_tuning_round:
        return
    mean, variance, _n = reduced.online
    ref = GaussianReference(np.array(mean, dtype=np.float64), np.sqrt(np.asarray(variance, dtype=np.float64)), var.first_tuning_round)
    pt.inputs.variational = ref
    temp = pt.shared.tempering
    N = pt.replicas.N
    if isinstance(temp, StabilizedPT):
        temp.variational_leg.path = InterpolatingPath(ref, pt.inputs.target)
        uses = np.array([1 if c < temp.n_var else 0 for c in range(N)], dtype=np.int32)
    else:
        temp.path = InterpolatingPath(ref, pt.inputs.target)
        uses = np.ones(N, dtype=np.int32)
    pt.replicas.set_variational_reference(ref.mean, ref.standard_deviation, uses)


def adapt_explorer(pt, reduced):
    """adapt_explorer (src/explorers/AutoMALA.jl:70-79, MALA.jl:63-69, Compose.jl:10-14, Preconditioner.jl:54-55); AAPS as MALA."""
    def adapt_one(ex):
        if isinstance(ex, Compose):
            return Compose(adapt_one(ex.first), adapt_one(ex.second))
        if not isinstance(ex, (AutoMALA, MALA, AAPS)) or reduced.am_factors is None:
            return ex
        std = None
        if not isinstance(ex.preconditioner, IdentityPreconditioner):
            std = np.sqrt(np.asarray(reduced.online[1], dtype=np.float64))
        new_step = ex.step_size
        if isinstance(ex, AutoMALA):
            fm, fn = reduced.am_factors
            present = np.asarray(fn) > 0
            if present.any():
                acc = 0.0                                # (a plain left-to-right sum, as the oracle's: np.mean sums in eight interleaved partial sums)
                for v in np.asarray(fm, dtype=np.float64)[present]:
                    acc += float(v)
                new_step = ex.step_size * (acc / float(int(present.sum())))
        adapted.append((new_step, std))
        if isinstance(ex, AAPS):
            return AAPS(ex.step_size, ex.K, ex.preconditioner, std)
        return type(ex)(ex.base_n_refresh, ex.exponent_n_refresh, new_step, ex.preconditioner, std)
    adapted = []
    pt.shared.explorer = adapt_one(pt.shared.explorer)
    if not adapted:
        return
    new_step, std = adapted[-1]
    eng = pt.shards if pt.shards is not None else pt.replicas
    if hasattr(eng, "engines"):
        for e in eng.engines:
            e.set_explorer_adaptation(new_step, std)
    else:
        pt.replicas.set_explorer_adaptation(new_step, std)


def stepping_stone_pair(pt):
    up, un, dn, dnn = pt.reduced_recorders.log_sum_ratio
    temp = pt.shared.tempering
    if isinstance(temp, StabilizedPT):                 # only the variational leg's keys (stepping_stone.jl:53-65)
        k = temp.n_var - 1
        up, un, dn, dnn = up[:k], un[:k], dn[:k], dnn[:k]
    return T.stepping_stone_pair(up, un, dn, dnn)


def stepping_stone(pt):
    return T.stepping_stone(stepping_stone_pair(pt))


def energy_ac1s(pt, skip_reference=False):
    """src/recorders/recorder.jl:156-173: autocorrelation of the log density before / after an exploration
    step, one entry per chain."""
    cor = np.asarray(pt.reduced_recorders.energy_ac1[0])
    if not skip_reference or len(cor) <= 1:
        return cor
    return cor[1:-1] if isinstance(pt.shared.tempering, StabilizedPT) else cor[1:]     # is_reference: chain 1 (and N with two legs)


def sample_names(pt):
    """src/pt/state.jl:60-63,91"""
    d = pt.replicas.d
    return ["param_%d" % (i + 1) for i in range(d)] + ["log_density"]


def sample_array(pt):
    """src/pt/process_sample.jl:19-32: [iteration, variable, target chain] of the last round's traces."""
    tr = pt.reduced_recorders.traces
    if tr is None or tr.size == 0:
        raise ValueError("no traces recorded: pass record=[traces]")
    if tr.ndim == 3:                                   # extended_traces: [scan][chain][var] -> [scan, var, chain]
        return np.transpose(tr, (0, 2, 1)).copy()
    return tr[:, :, None].copy()


def get_sample(pt, chain=None, scan=None):
    """src/pt/process_sample.jl get_sample(pt, chain[, scan]) for the target chain (1-based scan)."""
    tr = pt.reduced_recorders.traces
    if tr.ndim == 3:                                   # extended_traces
        tr = tr[:, (pt.inputs.n_chains if chain is None else chain) - 1, :]
    elif chain is not None and chain != pt.inputs.n_chains:
        raise ValueError("traces were recorded for the target chain only: pass extended_traces=True")
    return tr if scan is None else tr[scan - 1]


def mean(pt):
    """Statistics.mean(pt) (src/recorders/OnlineStateRecorder.jl:16): online mean of [state; log density]."""
    r = pt.reduced_recorders
    return np.concatenate([r.online[0], [r.online_log_density[0]]])


def var(pt):
    """Statistics.var(pt) (src/recorders/OnlineStateRecorder.jl:21)."""
    r = pt.reduced_recorders
    return np.concatenate([r.online[1], [r.online_log_density[1]]])


def n_round_trips(pt):
    return pt.reduced_recorders.round_trip[1]


def n_tempered_restarts(pt):
    return pt.reduced_recorders.round_trip[0]


def global_barrier(pt):
    return pt.shared.tempering.communication_barriers.globalbarrier


def global_barrier_variational(pt):
    """src/tempering/StabilizedPT.jl:117"""
    return pt.shared.tempering.variational_leg.communication_barriers.globalbarrier


def target_chains(pt):
    """src/pt/process_sample.jl:41-44 (1-based chain indices)"""
    temp = pt.shared.tempering
    n = pt.replicas.N
    return [i for i in range(1, n + 1) if (temp.is_target(i) if isinstance(temp, StabilizedPT) else i == n)]


def last_round_max_time(pt):
    """src/recorders/recorder.jl:137"""
    return pt.reduced_recorders.timing_extrema["round"]


def report(pt):
    """One line of the reference's report table (all_reports(), src/pt/report.jl:8-26); an item whose recorder is
    missing is skipped, as there."""
    it = pt.shared.iterators
    red = pt.reduced_recorders
    row = {"scans": n_scans_in_round(it)}
    if red.round_trip is not None:
        row["restarts"] = red.round_trip[0]
    n_total = pt.replicas.N
    if not isinstance(pt.inputs.target, TestSwapper) and n_total > 1:
        m, n = red.swap_acceptance_pr
        row["Λ"] = global_barrier(pt)
        if isinstance(pt.shared.tempering, StabilizedPT) and pt.shared.tempering.variational_leg.communication_barriers is not None:
            row["Λ_var"] = global_barrier_variational(pt)
        row.update({"time(s)": last_round_max_time(pt), "log(Z₁/Z₀)": stepping_stone(pt),
                    "min(α)": float(np.min(m)), "mean(α)": float(np.mean(m))})
        names = {b() for b in pt.inputs.record}
        if "energy_ac1" in names and red.energy_ac1 is not None:
            rho = np.abs(energy_ac1s(pt, True)); rho = rho[np.isfinite(rho)]
            if rho.size:
                row["max|ρ|"], row["mean|ρ|"] = float(rho.max()), float(rho.mean())
        am, an = red.explorer_acceptance_pr if red.explorer_acceptance_pr is not None else (None, None)
        if am is not None and np.any(np.asarray(an) > 0):
            a = np.asarray(am)[np.asarray(an) > 0]
            row["min(αₑ)"], row["mean(αₑ)"] = float(a.min()), float(a.mean())
        if red.reversibility_rate is not None and np.any(np.asarray(red.reversibility_rate[1]) > 0):
            rr = np.asarray(red.reversibility_rate[0])[np.asarray(red.reversibility_rate[1]) > 0]
            row["min(RR)"], row["mean(RR)"] = float(rr.min()), float(rr.mean())
    else:
        row["time(s)"] = last_round_max_time(pt)
    if red.round_trip is not None:
        row["round trips"] = red.round_trip[1]
    pt.shared.reports.append(row)
    if pt.inputs.show_report:
        print("  ".join("%s=%s" % (k, ("%.4g" % v) if isinstance(v, float) else v) for k, v in row.items()))


def pigeons(pt_or_none=None, **kwargs):
    """pigeons(; target, seed, n_rounds, n_chains, explorer, record, ...) -> PT  (src/api.jl:8-19)."""
    exec_folder = kwargs.pop("exec_folder", None)
    pt = pt_or_none if pt_or_none is not None else PT(Inputs(**kwargs))
    if exec_folder is not None:
        pt.exec_folder = exec_folder
    elif pt.inputs.checkpoint and getattr(pt, "exec_folder", None) is None:
        from .checkpoint import next_exec_folder           # the reference always has an exec folder when checkpoint = true
        pt.exec_folder = next_exec_folder()                # (results/all/<time stamp>, src/pt/pigeons.jl:20, checkpoint.jl:110-113)
    while next_round(pt):
        reduced = run_one_round(pt)
        pt = adapt(pt, reduced)
        report(pt)
        if pt.inputs.checkpoint and getattr(pt, "exec_folder", None):     # src/pt/pigeons.jl:20, checkpoint.jl:110-113
            from .checkpoint import write_checkpoint
            write_checkpoint(pt)
    return pt
