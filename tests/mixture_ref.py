"""A NumPy restatement of the Gaussian-mixture family as the device computes it (this project's specification).  The test files
use it as their reference.

Sums over coordinates follow the fixed tree of DESIGN 3 (balanced, natural order, zero-padded to a power of two), as the kernels' do;
sums over components run in component order.  exp / log are libm's, the device's differ by an ulp: densities agree to ~1e-15 relative,
states after a transition to ~1e-12."""
import math

import numpy as np

from path_ref import PathChain, tree_sum          # noqa: F401  (tree_sum: imported from here by the other restatements)

LOG2PI = 1.8378770664093453


class Mixture:
    """the target: a normalised mixture of K diagonal Gaussians, with the host constants of pte_set_target_mixture"""

    def __init__(self, weights, means, std_devs):
        self.w = np.asarray(weights, dtype=np.float64).ravel()
        self.mu = np.asarray(means, dtype=np.float64)
        self.sd = np.asarray(std_devs, dtype=np.float64)
        self.K, self.d = self.mu.shape
        lw = [math.log(x) for x in self.w]
        lmax = max(lw)
        se = 0.0
        for x in lw:
            se += math.exp(x - lmax)
        lse = lmax + math.log(se)
        self.c = np.zeros(self.K)
        for k in range(self.K):
            sl = 0.0
            for i in range(self.d):
                sl += math.log(self.sd[k, i])
            self.c[k] = (lw[k] - lse) - sl - (self.d / 2.0) * LOG2PI
        self.inv = 1.0 / self.sd

    def _a(self, x):
        with np.errstate(all="ignore"):
            return np.array([self.c[k] - tree_sum(((x - self.mu[k]) * self.inv[k]) ** 2) / 2.0 for k in range(self.K)])

    def lp(self, x):
        a = self._a(np.asarray(x, dtype=np.float64))
        m = a[0]
        for k in range(1, self.K):
            m = a[k] if a[k] > m else m
        s = 0.0
        for k in range(self.K):
            s += math.exp(a[k] - m)
        return m + math.log(s)

    def lp_grad(self, x):
        x = np.asarray(x, dtype=np.float64)
        lp = self.lp(x)
        a = self._a(x)
        g = None
        with np.errstate(all="ignore"):
            for k in range(self.K):
                r = math.exp(a[k] - lp)
                gk = -((x - self.mu[k]) * (self.inv[k] * self.inv[k]))
                g = r * gk if g is None else g + r * gk
        return lp, g


MixtureChain = PathChain          # (mix, beta, ref_prec): the chain of the interpolated path, tests/path_ref.py


def analytic_lognormalization(d, ref_prec):
    """log Z1 / Z0 of the path: the mixture is normalised, the reference exp(-prec |x|^2 / 2) integrates to (2 pi / prec)^(d/2)"""
    return -(d / 2.0) * math.log(2.0 * math.pi / ref_prec)


def mala_transition(x0, rng, chain, step_size, n_refresh, M):
    """explore! with MALA (MALA.jl:74-97) as automala_body runs it: n_refresh refreshes of momentum, one leapfrog, MH.  The preconditioner M
    is drawn already (aaps_ref.build_preconditioner).  -> dict(x, acc_sum, acc_n, steps)"""
    x = np.asarray(x0, dtype=np.float64).copy()
    d = x.size
    lp0, g0 = chain.lp_grad(x)
    g0 = g0 / M
    acc_sum, steps = 0.0, 0
    half = step_size / 2
    for _ in range(n_refresh):
        p = np.array([rng.randn() for _ in range(d)])
        init_joint = lp0 - 0.5 * tree_sum(p * p)
        if not math.isfinite(init_joint):
            raise ValueError("MALA can only be called on a configuration of positive density")
        xs = x.copy()
        with np.errstate(all="ignore"):
            p = p + half * g0                                   # am_leap_frog
            x = x + step_size * (p / M)
            lpn, g = chain.lp_grad(x)
            g = g / M
            ken = 0.5 * tree_sum(p * p)
            if math.isfinite(lpn - ken):
                p = p + half * g
                ken = 0.5 * tree_sum(p * p)
            ex = float(np.exp((lpn - ken) - init_joint))
        prob = ex if ex < 1.0 else (ex if math.isnan(ex) else 1.0)
        acc_sum += prob
        if not (rng.rand() < prob):
            x = xs
        else:
            lp0, g0 = lpn, g
        steps += 1
    return dict(x=x, acc_sum=acc_sum, acc_n=n_refresh, steps=steps)
