"""A NumPy restatement of the Bayesian-GLM family as the device computes it (this project's specification).  The test files use
it as their reference.

The orders are the kernels': eta_i sequential in j, the log-likelihood terms summed by lane (lane l: observations l, l + 64, ... in
increasing i) and the 64 lane sums over the fixed tree of DESIGN 3, sum_i X_ij r_i sequential in i.  The kernels fuse each of those
multiply-adds (one rounding); here the product and the sum are formed in extended precision and rounded once more, which agrees with the
fused result up to rare double-rounding ties.  exp / log1p are libm's, the device's differ by an ulp: densities agree to ~1e-14 relative,
states after a transition to ~1e-12."""
import math

import numpy as np

from path_ref import PathChain, tree_sum

LOG2PI = 1.8378770664093453
BERNOULLI_LOGIT, NORMAL_IDENTITY = 0, 1


def fma(a, b, c):
    """a * b + c elementwise, rounded as the kernels' fused multiply-adds (see the module's docstring)"""
    L = np.longdouble
    return (np.asarray(a, dtype=np.float64).astype(L) * L(b) + np.asarray(c, dtype=np.float64).astype(L)).astype(np.float64)


class Glm:
    """the target prior x likelihood with the host constants of pte_set_target_glm; prec = the prior's (and the reference's) precision"""

    def __init__(self, X, y, likelihood, noise_sd, prec):
        self.X = np.asarray(X, dtype=np.float64)
        self.y = np.asarray(y, dtype=np.float64).ravel()
        self.n, self.d = self.X.shape
        self.lik = {"bernoulli_logit": BERNOULLI_LOGIT, "normal_identity": NORMAL_IDENTITY}.get(likelihood, likelihood)
        self.prec, self.sd = float(prec), float(noise_sd)
        self.c_prior = -(self.d / 2.0) * math.log(2.0 * math.pi / self.prec)
        self.c_obs = -self.n * (math.log(self.sd) + 0.5 * LOG2PI) if self.lik == NORMAL_IDENTITY else 0.0
        self.w1 = 1.0 / (self.sd * self.sd)
        self.w2 = 1.0 / (2.0 * (self.sd * self.sd))

    def eta(self, theta):
        e = np.zeros(self.n)
        for j in range(self.d):
            e = fma(self.X[:, j], theta[j], e)
        return e

    def terms(self, eta):
        """(l_i, r_i = dl_i / deta_i) of every observation"""
        y = self.y
        with np.errstate(all="ignore"):
            if self.lik == BERNOULLI_LOGIT:
                t = np.exp(-np.abs(eta))
                return y * eta - (np.maximum(eta, 0.0) + np.log1p(t)), y - np.where(eta >= 0.0, 1.0, t) / (1.0 + t)
            res = y - eta
            return -(res * res) * self.w2, res * self.w1

    def loglik_sum(self, l):
        """sum_i l_i: lane l sums its observations in increasing i, then the fixed tree over the 64 lane sums"""
        lanes = np.zeros(64)
        for m0 in range(0, self.n, 64):
            blk = l[m0:m0 + 64]
            lanes[:blk.size] = lanes[:blk.size] + blk
        return tree_sum(lanes)

    def lp(self, theta):
        theta = np.asarray(theta, dtype=np.float64)
        l, _ = self.terms(self.eta(theta))
        S = tree_sum(theta * theta)
        return ((((-0.5 * self.prec) * S) + self.c_prior) + self.loglik_sum(l)) + self.c_obs

    def lp_grad(self, theta):
        theta = np.asarray(theta, dtype=np.float64)
        l, r = self.terms(self.eta(theta))
        S = tree_sum(theta * theta)
        lp = ((((-0.5 * self.prec) * S) + self.c_prior) + self.loglik_sum(l)) + self.c_obs
        acc = np.zeros(self.d)
        for i in range(self.n):
            acc = fma(self.X[i], r[i], acc)
        return lp, ((-self.prec) * theta) + acc

    # ---- closed forms (normal-identity likelihood) -----------------------------------------------------------------------------------
    def posterior(self):
        """exact posterior mean and covariance: precision p I + X^T X / sigma^2, mean A^-1 X^T y / sigma^2"""
        assert self.lik == NORMAL_IDENTITY
        A = self.prec * np.eye(self.d) + self.X.T @ self.X / self.sd ** 2
        cov = np.linalg.inv(A)
        return cov @ (self.X.T @ self.y) / self.sd ** 2, cov

    def log_evidence(self):
        """log p(y), y ~ N(0, sigma^2 I + X X^T / p)"""
        assert self.lik == NORMAL_IDENTITY
        C = self.sd ** 2 * np.eye(self.n) + self.X @ self.X.T / self.prec
        _, logdet = np.linalg.slogdet(C)
        return -0.5 * (self.n * LOG2PI + logdet + self.y @ np.linalg.solve(C, self.y))

    def evidence_offset(self):
        """stepping_stone estimates log Z1 / Z0 = log p(y) - (d/2) log(2 pi / p): the reference is the unnormalised prior"""
        return -(self.d / 2.0) * math.log(2.0 * math.pi / self.prec)


GlmChain = PathChain          # (glm, beta, ref_prec): the chain of the interpolated path, tests/path_ref.py
