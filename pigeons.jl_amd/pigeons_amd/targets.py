"""The target families of the device engine and what each tells the host about itself, under the names of the Julia glue:
    device_family(self, inputs, explorer)   dict(target=, dim=, target_params=) for Engine, or the refusal of what the device has not
    upload(self, engine)                    the family's data to one engine, through its Engine.set_target_* method (families without data: none)
    default_explorer(self)                  the explorer of a run that names none
With them the references, GaussianReference, InterpolatingPath and the analytic results of the toy path."""
import math
from dataclasses import dataclass
from typing import Any

import numpy as np

from . import _lib
from .explorers import CheckerboardMetropolis, IsingMetropolis, SliceSampler, ToyExplorer


# ---- targets (src/targets/toy_mvn_target.jl, src/paths/ScaledPrecisionNormalPath.jl) ---------
@dataclass
class ScaledPrecisionNormalPath:
    precision0: float = 1.0
    precision1: float = 10.0
    dim: int = 1

    def precision(self, beta):
        return (1.0 - beta) * self.precision0 + beta * self.precision1

    def device_family(self, inputs, explorer): return dict(target=_lib.TARGET_MVN_SCALED_PRECISION, dim=self.dim, target_params=[self.precision0, self.precision1])
    def default_explorer(self): return ToyExplorer()           # src/targets/toy_mvn_target.jl:13


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


def _interpolated(target, code, inputs, phrase, suffix="dim)", ref_dim=None):
    """device_family of a target tempered from reference=ScaledPrecisionNormalLogPotential(prec, dim), whose prec is the family's one parameter;
    any other reference is refused in the family's words: `phrase` names its path, `suffix` is what its message says after "(prec, " """
    ref = inputs.reference
    if not isinstance(ref, ScaledPrecisionNormalLogPotential) or ref.dim != (target.dim if ref_dim is None else ref_dim):
        raise NotImplementedError("the device %s path needs reference=ScaledPrecisionNormalLogPotential(prec, %s" % (phrase, suffix))
    return dict(target=code, dim=target.dim, target_params=[ref.precision])


def _slice_sampler_only(explorer, phrase):
    if not isinstance(explorer, SliceSampler):
        raise NotImplementedError("the device %s path is explored by SliceSampler only (got %r)" % (phrase, explorer))


def _even_for_checkerboard(target, explorer):
    if isinstance(explorer, CheckerboardMetropolis) and target.base_length % 2 != 0:
        raise ValueError("CheckerboardMetropolis needs an even base_length (got %d): on an odd periodic lattice two sites of one colour "
                         "would be neighbours" % target.base_length)


@dataclass
class Funnel:
    """Neal's funnel as a LogDensityProblems target (reference test/supporting/dimensional-analysis.jl:33-48):
    z[1] ~ Normal(0, 3), z[i] ~ Normal(0, exp(z[1]/2)); initialization = zeros(dim).  Tempered through the
    default InterpolatingPath(reference, target) (src/targets/target.jl:72-75)."""
    dim: int = 2
    takes_gaussian_reference = True    # the one path with GaussianReference on the device (inputs.variational)

    def device_family(self, inputs, explorer): return _interpolated(self, _lib.TARGET_FUNNEL, inputs, "funnel")


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

    def device_family(self, inputs, explorer): return _interpolated(self, _lib.TARGET_GAUSSIAN_MIXTURE, inputs, "Gaussian-mixture")
    def upload(self, engine): engine.set_target_mixture(self.weights, self.means, self.std_devs)

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

    def device_family(self, inputs, explorer): return _interpolated(self, _lib.TARGET_BAYESIAN_GLM, inputs, "Bayesian-GLM", "dim) -- the prior")
    def upload(self, engine): engine.set_target_glm(self.likelihood_code, self.X, self.y, self.noise_sd)

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

    def device_family(self, inputs, explorer): return _interpolated(self, _lib.TARGET_MIXTURE_MODEL, inputs, "mixture-model", "dim) -- the prior")
    def upload(self, engine): engine.set_target_mixture_model(self.y)

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

    def device_family(self, inputs, explorer): return _interpolated(self, _lib.TARGET_HIERARCHICAL_NORMAL, inputs, "hierarchical-normal")
    def upload(self, engine): engine.set_target_hier(self.parameterization_code, self.y, self.sigma, self.mu_sd, self.tau_scale)

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

    def device_family(self, inputs, explorer): return _interpolated(self, _lib.TARGET_LATENT_AR1, inputs, "latent-AR(1)")
    def upload(self, engine): engine.set_target_ar1(self.likelihood_code, self.y, self.obs_sd, self.mu_sd, self.phi_loc, self.phi_scale, self.sigma_scale)

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

    def device_family(self, inputs, explorer): return _interpolated(self, _lib.TARGET_DENSE_NORMAL, inputs, "dense-normal")
    def upload(self, engine): engine.set_target_dense(self.mean, self.precision)

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

    def device_family(self, inputs, explorer):
        family = _interpolated(self, _lib.TARGET_VARIABLE_SELECTION, inputs, "variable-selection", "d) -- the prior of the d coefficients", self.n_columns)
        _slice_sampler_only(explorer, "variable-selection")
        return family

    def upload(self, engine): engine.set_target_varsel(self.likelihood_code, self.X, self.y, self.noise_sd, self.inclusion_prob)

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

    def device_family(self, inputs, explorer):
        family = _interpolated(self, _lib.TARGET_CHANGE_POINT, inputs, "change-point", "K + 1) -- the prior of the K + 1 log rates", self.n_rates)
        _slice_sampler_only(explorer, "change-point")
        return family

    def upload(self, engine): engine.set_target_changepoint(self.y)

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

    def device_family(self, inputs, explorer):
        _even_for_checkerboard(self, explorer)
        return dict(target=_lib.TARGET_ISING, dim=self.base_length ** 2, target_params=[self.beta])

    def default_explorer(self): return IsingMetropolis()       # examples/ising.jl:94


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

    def device_family(self, inputs, explorer):
        _even_for_checkerboard(self, explorer)
        if not isinstance(explorer, (IsingMetropolis, CheckerboardMetropolis)):
            raise NotImplementedError("the device spin-glass path is explored by IsingMetropolis only (got %r)" % (explorer,))
        return dict(target=_lib.TARGET_SPIN_GLASS, dim=self.dim, target_params=[self.beta])

    def upload(self, engine): engine.set_target_spin_glass(self.bonds_right, self.bonds_down)
    def default_explorer(self): return IsingMetropolis()       # examples/ising.jl:94

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

    def device_family(self, inputs, explorer):
        if not isinstance(explorer, CheckerboardMetropolis):
            raise NotImplementedError("the device 3-D spin-glass path is explored by CheckerboardMetropolis only (got %r)" % (explorer,))
        return dict(target=_lib.TARGET_SPIN_GLASS_3D, dim=self.dim, target_params=[self.beta])

    def upload(self, engine): engine.set_target_spin_glass_3d(self.bonds_x, self.bonds_y, self.bonds_z)
    def default_explorer(self): return CheckerboardMetropolis()    # the family's one explorer

    def __repr__(self):
        return "SpinGlass3DLogPotential(beta=%r, base_length=%d)" % (self.beta, self.base_length)


@dataclass
class TestSwapper:
    """src/swap/pair_swapper.jl:100-149"""
    constant_swap_accept_pr: float = 1.0
    __test__ = False

    def device_family(self, inputs, explorer): return dict(target=_lib.TARGET_TEST_SWAPPER, dim=1, target_params=[self.constant_swap_accept_pr])
    def default_explorer(self): return None                    # src/swap/pair_swapper.jl:139


def default_explorer(target):
    """the target's own default; a target that names none gets the reference's (src/targets/target.jl:20)"""
    return target.default_explorer() if hasattr(target, "default_explorer") else SliceSampler()
