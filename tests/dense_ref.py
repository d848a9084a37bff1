"""A NumPy restatement of the dense-precision Gaussian family as the device computes a FULL evaluation (this project's
specification), and the exact law of every chain of its path.  The test files use it as their reference.

The target is N(m, Q^-1), normalised: l2(x) = c - (x - m)' Q (x - m) / 2 with c = log det(Q) / 2 - (d/2) log 2 pi from a Cholesky
factorisation, sum_i log L_ii in index order.  One evaluation: z = x - m; u_i = sum_k Q[k][i] z_k accumulated for k = 0 .. d-1 in that order
from 0.0 (the device fuses each multiply-add; NumPy rounds the product first -- for the well-conditioned test matrices the two differ by
a few 1e-16 relative); A = the fixed-tree sum of z_i u_i; the gradient is -u.  The device's SliceSampler kernel does NOT evaluate
this way -- it keeps u and A and updates them per coordinate -- and is held to this restatement, not to a copy of itself."""
import math

import numpy as np

from path_ref import PathChain, tree_sum

LOG2PI = 1.8378770664093453


class Dense:
    """the target with the host constants of pte_set_target_dense"""

    def __init__(self, mean, precision):
        self.mean = np.asarray(mean, dtype=np.float64).ravel()
        self.Q = np.ascontiguousarray(precision, dtype=np.float64)
        self.d = self.mean.size
        assert self.Q.shape == (self.d, self.d) and np.array_equal(self.Q, self.Q.T)
        L = self._cholesky(self.Q)
        s = 0.0
        for i in range(self.d):
            s += math.log(L[i, i])
        self.c = s - 0.5 * self.d * math.log(2.0 * math.pi)

    @staticmethod
    def _cholesky(Q):
        """column by column, as the host does: the first non-positive pivot raises"""
        d = Q.shape[0]
        L = np.zeros((d, d))
        for j in range(d):
            piv = Q[j, j] - float(np.dot(L[j, :j], L[j, :j]))
            if not piv > 0.0:
                raise ValueError("not positive definite: pivot %d is %g" % (j, piv))
            L[j, j] = math.sqrt(piv)
            if j + 1 < d:
                L[j + 1:, j] = (Q[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
        return L

    def zu(self, x):
        z = np.asarray(x, dtype=np.float64) - self.mean
        u = np.cumsum(self.Q * z[:, None], axis=0)[-1]       # sum_k Q[k][i] z_k, k = 0 .. d-1 in that order (cumsum adds sequentially)
        return z, u

    def lp(self, x):
        z, u = self.zu(x)
        return self.c - 0.5 * tree_sum(z * u)

    def lp_grad(self, x):
        z, u = self.zu(x)
        return self.c - 0.5 * tree_sum(z * u), -u

    def evidence_offset(self, prec):
        """stepping_stone estimates log Z1 / Z0 = 0 - (d/2) log(2 pi / p): the reference is unnormalised, the target normalised"""
        return -(self.d / 2.0) * math.log(2.0 * math.pi / prec)


class DenseChain(PathChain):
    """(dense, beta, prec): the chain of the interpolated path (tests/path_ref.py) with the exact law of the chain beside it"""

    logdensity_and_gradient = PathChain.lp_grad

    def chain_moments(self):
        """(mean, covariance) of this chain, exactly: precision P = (1 - beta) p I + beta Q, mean P^-1 beta Q m"""
        d = self.model.d
        P = self.omb * self.ref_prec * np.eye(d) + self.beta * self.model.Q
        cov = np.linalg.inv(P)
        cov = (cov + cov.T) / 2.0
        return cov @ (self.beta * (self.model.Q @ self.model.mean)), cov


def spectrum_matrix(d, cond, seed):
    """Q = U diag(lambda) U', symmetrised bit for bit: U a random orthogonal matrix, lambda log-spaced from 1 / sqrt(cond) to sqrt(cond)"""
    g = np.random.default_rng(seed)
    U, _ = np.linalg.qr(g.normal(size=(d, d)))
    lam = np.exp(np.linspace(-0.5 * math.log(cond), 0.5 * math.log(cond), d)) if d > 1 else np.array([1.3])
    Q = (U * lam) @ U.T
    return (Q + Q.T) / 2.0
