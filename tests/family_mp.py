"""The path log density (1 - beta) ref(x) + beta target(x) of the nine target families on the interpolated path, evaluated with mpmath at 60
digits from each model's definition (include/pte.h): a density is a sum of named log densities of named distributions, in
no particular order, with none of the kernels' rearrangements -- no maxima taken out of a log-sum-exp (mpmath's exponent range has no
underflow), no sign split of the softplus, no cached predictor, no sorted bounds, no exp(-2 |a|) forms.  The restatements tests/<family>_ref.py
follow the kernels' operations in the kernels' order and cannot see a wrong formula; this file can.

One function per family: the constructor arguments of the <family>_ref class, then beta, ref_prec and the state x; it returns an mpf.  The
reference is ScaledPrecisionNormal(ref_prec), unnormalised: ref(x) = -(ref_prec / 2) sum x_i^2 over the Float64 coordinates (the variable-
selection indicators and the change points have the uniform reference, a constant that is left out as the engine leaves it out).  beta = 0
and beta = 1 return the end point itself, as InterpolatedLogPotential does.  Every input is a double and is taken exactly."""
import numpy as np
from mpmath import mp, mpf

mp.dps = 60


def _v(a):
    """a vector of doubles, taken exactly; entries that are mpf already stay (mp.diff moves one coordinate off its double)"""
    return [t if isinstance(t, mpf) else mpf(float(t)) for t in (a.ravel().tolist() if isinstance(a, np.ndarray) else list(a))]


_LOGS, _ARRAYS = {}, {}


def _log(s):
    """mp.log, remembered per argument and working precision: the same few scales come back for every observation"""
    key = (s, mp.prec)
    if key not in _LOGS:
        if len(_LOGS) > 100000:
            _LOGS.clear()
        _LOGS[key] = mp.log(s)
    return _LOGS[key]


def _m(a):
    """a constant matrix of doubles as rows of mpf, converted once per array"""
    if id(a) not in _ARRAYS:
        _ARRAYS[id(a)] = (a, [[mpf(float(t)) for t in row] for row in np.asarray(a, dtype=np.float64)])
    return _ARRAYS[id(a)][1]


def _normal(x, m, s):
    """log N(x; m, s^2)"""
    z = (x - m) / s
    return -z * z / 2 - _log(s) - _log(2 * mp.pi) / 2


def _half_cauchy(t, scale):
    """log HalfCauchy(t; 0, scale), t > 0"""
    return mp.log(2) - mp.log(mp.pi) - mp.log(scale) - mp.log(1 + (t / scale) ** 2)


def _path(beta, ref, target):
    """target: a callable, so that the reference end never evaluates it"""
    b = mpf(float(beta))
    if b == 0:
        return ref
    if b == 1:
        return target()
    return (1 - b) * ref + b * target()


def _ref(ref_prec, x):
    return -mpf(float(ref_prec)) / 2 * mp.fsum(t * t for t in x)


def funnel(dim, beta, ref_prec, x):
    """Neal's funnel: x_0 ~ N(0, 3^2), x_i ~ N(0, exp(x_0 / 2)^2)"""
    x = _v(x)
    assert len(x) == dim
    return _path(beta, _ref(ref_prec, x),
                 lambda: _normal(x[0], 0, mpf(3)) + mp.fsum(_normal(t, 0, mp.exp(x[0] / 2)) for t in x[1:]))


def mixture(weights, means, std_devs, beta, ref_prec, x):
    """sum_k w_k / (sum w) prod_i N(x_i; means[k][i], std_devs[k][i]^2)"""
    x = _v(x)
    w = _v(weights)
    mu, sd = _m(means), _m(std_devs)

    def target():
        comp = [mp.log(w[k] / mp.fsum(w)) + mp.fsum(_normal(x[i], mu[k][i], sd[k][i]) for i in range(len(x))) for k in range(len(w))]
        return mp.log(mp.fsum(mp.exp(c) for c in comp))
    return _path(beta, _ref(ref_prec, x), target)


def _glm_loglik(likelihood, eta, y, noise_sd):
    if likelihood in ("bernoulli_logit", 0):                     # y eta - log(1 + e^eta)
        return mp.fsum(yi * e - mp.log(1 + mp.exp(e)) for yi, e in zip(y, eta))
    return mp.fsum(_normal(yi, e, mpf(float(noise_sd))) for yi, e in zip(y, eta))


def glm(X, y, likelihood, noise_sd, prec, beta, ref_prec, x):
    """theta ~ N(0, I / prec), y_i | eta_i = X[i] . theta Bernoulli-logit or N(eta_i, noise_sd^2)"""
    x, y = _v(x), _v(y)
    X = _m(X)
    p = mpf(float(prec))

    def target():
        eta = [mp.fdot(zip(X[i], x)) for i in range(len(y))]
        return mp.fsum(_normal(t, 0, 1 / mp.sqrt(p)) for t in x) + _glm_loglik(likelihood, eta, y, noise_sd)
    return _path(beta, _ref(ref_prec, x), target)


def varsel(X, y, likelihood, noise_sd, prec, inclusion_prob, beta, ref_prec, x):
    """x = [theta, gamma]: theta ~ N(0, I / prec), gamma_j ~ Bernoulli(inclusion_prob), eta = X (gamma * theta), the likelihoods of glm"""
    x, y = _v(x), _v(y)
    X = _m(X)
    d = len(X[0])
    assert len(x) == 2 * d
    theta, gamma = x[:d], x[d:]
    assert all(g in (0, 1) for g in gamma)
    p, pi = mpf(float(prec)), mpf(float(inclusion_prob))

    def target():
        eta = [mp.fdot((X[i][j], theta[j]) for j in range(d) if gamma[j] == 1) for i in range(len(y))]
        return (mp.fsum(_normal(t, 0, 1 / mp.sqrt(p)) for t in theta) + mp.fsum(mp.log(pi) if g == 1 else mp.log(1 - pi) for g in gamma)
                + _glm_loglik(likelihood, eta, y, noise_sd))
    return _path(beta, _ref(ref_prec, theta), target)


def mixture_model(y, n_components, prec, beta, ref_prec, x):
    """x = [mu, s, alpha] ~ N(0, I / prec); y_i ~ sum_k softmax(alpha)_k N(mu_k, exp(s_k)^2)"""
    x, y = _v(x), _v(y)
    K = int(n_components)
    assert len(x) == 3 * K
    mu, s, al = x[:K], x[K:2 * K], x[2 * K:]
    p = mpf(float(prec))

    def target():
        tot = mp.fsum(mp.exp(a) for a in al)
        return (mp.fsum(_normal(t, 0, 1 / mp.sqrt(p)) for t in x)
                + mp.fsum(mp.log(mp.fsum(mp.exp(al[k]) / tot * mp.exp(_normal(yi, mu[k], mp.exp(s[k]))) for k in range(K))) for yi in y))
    return _path(beta, _ref(ref_prec, x), target)


def changepoint(y, n_changepoints, prec, beta, ref_prec, x):
    """x = [r_0 .. r_K, tau_1 .. tau_K]: r ~ N(0, I / prec), every tau uniform on 0 .. n; observation i (from 0) lies in segment
    j = #{k : tau_k <= i} and is Poisson(exp(r_j))"""
    x, y = _v(x), _v(y)
    K, n = int(n_changepoints), len(y)
    assert len(x) == 2 * K + 1
    r, tau = x[:K + 1], x[K + 1:]
    assert all(t == mp.floor(t) and 0 <= t <= n for t in tau)
    p = mpf(float(prec))

    def target():
        lp = mp.fsum(_normal(t, 0, 1 / mp.sqrt(p)) for t in r) - K * mp.log(n + 1)
        for i, yi in enumerate(y):
            rj = r[sum(1 for t in tau if t <= i)]
            lp += yi * rj - mp.exp(rj) - mp.loggamma(yi + 1)
        return lp
    return _path(beta, _ref(ref_prec, r), target)


def hier(y, sigma, mu_sd, tau_scale, parameterization, beta, ref_prec, x):
    """x = [mu, log tau, x_2 ..]: mu ~ N(0, mu_sd^2), tau ~ HalfCauchy(0, tau_scale) (times tau, the Jacobian of log tau),
    theta_j ~ N(mu, tau^2), y_j ~ N(theta_j, sigma_j^2); centred: x_{2+j} = theta_j; non-centred: x_{2+j} = eta_j ~ N(0, 1), theta_j = mu + tau eta_j"""
    x, y, sg = _v(x), _v(y), _v(sigma)
    assert len(x) == len(y) + 2

    def target():
        mu, lt = x[0], x[1]
        tau = mp.exp(lt)
        lp = _normal(mu, 0, mpf(float(mu_sd))) + _half_cauchy(tau, mpf(float(tau_scale))) + lt
        for j in range(len(y)):
            if parameterization in ("noncentered", 1):
                lp += _normal(x[2 + j], 0, 1) + _normal(y[j], mu + tau * x[2 + j], sg[j])
            else:
                lp += _normal(x[2 + j], mu, tau) + _normal(y[j], x[2 + j], sg[j])
        return lp
    return _path(beta, _ref(ref_prec, x), target)


def ar1(y, likelihood, obs_sd, mu_sd, phi_loc, phi_scale, sigma_scale, beta, ref_prec, x):
    """x = [mu, a, ls, h_0 ..]: mu ~ N(0, mu_sd^2), a ~ N(phi_loc, phi_scale^2), sigma = exp(ls) ~ HalfCauchy(0, sigma_scale) (times sigma),
    h_0 ~ N(mu, sigma^2 / (1 - phi^2)), h_t ~ N(mu + phi (h_{t-1} - mu), sigma^2), phi = tanh(a), 1 - phi^2 = sech(a)^2;
    y_t ~ N(0, exp(h_t)) (stochastic volatility) or N(h_t, obs_sd^2)"""
    x, y = _v(x), _v(y)
    assert len(x) == len(y) + 3

    def target():
        mu, a, ls = x[0], x[1], x[2]
        h = x[3:]
        phi, sg = mp.tanh(a), mp.exp(ls)
        lp = (_normal(mu, 0, mpf(float(mu_sd))) + _normal(a, mpf(float(phi_loc)), mpf(float(phi_scale)))
              + _half_cauchy(sg, mpf(float(sigma_scale))) + ls)
        lp += _normal(h[0], mu, sg / mp.sech(a))
        for t in range(1, len(h)):
            lp += _normal(h[t], mu + phi * (h[t - 1] - mu), sg)
        for t in range(len(h)):
            if likelihood in ("normal_identity", 1):
                lp += _normal(y[t], h[t], mpf(float(obs_sd)))
            else:
                lp += _normal(y[t], 0, mp.exp(h[t] / 2))
        return lp
    return _path(beta, _ref(ref_prec, x), target)


_LOGDET = {}


def dense(mean, precision, beta, ref_prec, x):
    """N(mean, precision^-1): log det(Q) / 2 - (d / 2) log 2 pi - (x - m)' Q (x - m) / 2, the determinant from an LU factorisation at 60 digits"""
    x, m = _v(x), _v(mean)
    Q = np.ascontiguousarray(precision, dtype=np.float64)
    d = len(x)

    def target():
        key = Q.tobytes()
        if key not in _LOGDET:
            _LOGDET[key] = mp.log(mp.det(mp.matrix([[mpf(Q[i, j]) for j in range(d)] for i in range(d)])))
        z = [x[i] - m[i] for i in range(d)]
        Qm = _m(precision)
        quad = mp.fdot((z[i], mp.fdot(zip(Qm[i], z))) for i in range(d))
        return _LOGDET[key] / 2 - mpf(d) / 2 * mp.log(2 * mp.pi) - quad / 2
    return _path(beta, _ref(ref_prec, x), target)
