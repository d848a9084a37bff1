"""A NumPy restatement of the mixture-model-posterior family as the device computes it (this project's specification).  The test
files use it as their reference.

The state is theta = [mu_1..mu_K, s_1..s_K, alpha_1..alpha_K]; component k has mean mu_k, standard deviation exp(s_k) and weight
softmax(alpha)_k.  The orders are the kernels': sums over components run in component order, the per-observation terms are summed by lane
(lane l: observations l, l + 64, ... in increasing i) and the 64 lane sums go over the fixed tree of DESIGN 3.  exp / log are libm's, the
device's differ by an ulp: densities agree to ~1e-14 relative, states after a transition to ~1e-12."""
import math

import numpy as np

from path_ref import PathChain, tree_sum


def lane_tree_sum(t):
    """sum_i t_i as the kernels take it: lane l sums its observations in increasing i, then the fixed tree over the 64 lane sums"""
    lanes = np.zeros(64)
    for m0 in range(0, t.size, 64):
        blk = t[m0:m0 + 64]
        lanes[:blk.size] = lanes[:blk.size] + blk
    return tree_sum(lanes)


class MixtureModel:
    """the target prior x likelihood with the host constants of pte_set_target_mixture_model; prec = the prior's (and the reference's)
    precision p"""

    def __init__(self, y, n_components, prec):
        self.y = np.asarray(y, dtype=np.float64).ravel()
        self.n, self.K, self.d = self.y.size, int(n_components), 3 * int(n_components)
        self.prec = float(prec)
        self.c_prior = -(self.d / 2.0) * math.log(2.0 * math.pi / self.prec)
        self.c_obs = -(self.n / 2.0) * math.log(2.0 * math.pi)

    def per_evaluation(self, theta):
        """(mu, e_k = exp(-s_k), b_k = log w_k - s_k, w_k)"""
        K = self.K
        mu, s, al = theta[:K], theta[K:2 * K], theta[2 * K:]
        with np.errstate(all="ignore"):
            m = al[0]
            for k in range(1, K):
                m = al[k] if al[k] > m else m
            se = 0.0
            for k in range(K):
                se += np.exp(al[k] - m)
            A = m + np.log(se)
            return mu, np.exp(-s), (al - A) - s, np.exp(al - A)

    def terms(self, theta):
        """(l_i [n], r_ik [n][K], z_ik [n][K]) of every observation"""
        K, y = self.K, self.y
        mu, e, b, _ = self.per_evaluation(theta)
        with np.errstate(all="ignore"):
            z = (y[:, None] - mu[None, :]) * e[None, :]
            a = b[None, :] - (z * z) / 2.0
            a = np.where(np.isnan(a), -np.inf, a)
            mi = a[:, 0].copy()
            for k in range(1, K):
                mi = np.where(a[:, k] > mi, a[:, k], mi)
            dead = mi == -np.inf
            u = np.exp(a - mi[:, None])
            su = np.zeros(self.n)
            for k in range(K):
                su = su + u[:, k]
            l = np.where(dead, -np.inf, mi + np.log(su))
            r = np.where(dead[:, None], 0.0, u / su[:, None])
        return l, r, z

    def lp(self, theta):
        theta = np.asarray(theta, dtype=np.float64)
        l, _, _ = self.terms(theta)
        S = tree_sum(theta * theta)
        with np.errstate(all="ignore"):
            return ((((-0.5 * self.prec) * S) + self.c_prior) + lane_tree_sum(l)) + self.c_obs

    def lp_grad(self, theta):
        theta = np.asarray(theta, dtype=np.float64)
        K = self.K
        l, r, z = self.terms(theta)
        _, e, _, w = self.per_evaluation(theta)
        S = tree_sum(theta * theta)
        with np.errstate(all="ignore"):
            lp = ((((-0.5 * self.prec) * S) + self.c_prior) + lane_tree_sum(l)) + self.c_obs
            gl = np.zeros(self.d)
            for k in range(K):
                gl[k] = e[k] * lane_tree_sum(r[:, k] * z[:, k])
                gl[K + k] = lane_tree_sum(r[:, k] * (z[:, k] * z[:, k] - 1.0))
                gl[2 * K + k] = lane_tree_sum(r[:, k]) - float(self.n) * w[k]
            return lp, ((-self.prec) * theta) + gl

    def evidence_offset(self):
        """stepping_stone estimates log Z1 / Z0 = log p(y) - (d/2) log(2 pi / p): the reference is the unnormalised prior"""
        return -(self.d / 2.0) * math.log(2.0 * math.pi / self.prec)

    def log_likelihood(self, thetas):
        """sum_i l_i for a batch of states [..., d] by the textbook formula (plain sums): what Monte Carlo estimates average"""
        K, y = self.K, self.y
        T = np.asarray(thetas, dtype=np.float64)
        mu, s, al = T[..., None, :K], T[..., None, K:2 * K], T[..., None, 2 * K:]
        lw = al - (al.max(-1, keepdims=True) + np.log(np.exp(al - al.max(-1, keepdims=True)).sum(-1, keepdims=True)))
        a = lw - s - 0.5 * ((y[:, None] - mu) * np.exp(-s)) ** 2
        m = a.max(-1, keepdims=True)
        return (m[..., 0] + np.log(np.exp(a - m).sum(-1))).sum(-1) + self.c_obs


MixtureModelChain = PathChain          # (model, beta, ref_prec): the chain of the interpolated path, tests/path_ref.py


def prior_monte_carlo_log_evidence(y, n_components, prec, n_draws, seed, chunk=200000):
    """log p(y) = log E_prior[prod_i p(y_i | theta)] by plain Monte Carlo over theta ~ N(0, I / prec), with its standard error (delta
    method on the mean of the likelihoods) -> (estimate, standard error)"""
    model = MixtureModel(y, n_components, prec)
    g = np.random.default_rng(seed)
    ll = np.concatenate([model.log_likelihood(g.normal(0.0, 1.0 / math.sqrt(prec), (min(chunk, n_draws - a), model.d)))
                         for a in range(0, n_draws, chunk)])
    m = ll.max()
    w = np.exp(ll - m)
    mean = w.mean()
    return m + math.log(mean), float(w.std(ddof=1) / math.sqrt(w.size) / mean)
