"""A NumPy restatement of the hierarchical normal-means family as the device computes it (this project's specification), and
its exact ground truth by quadrature.  The test files use it as their reference.

The model: J groups with estimates y_j and known standard errors sigma_j, y_j ~ N(theta_j, sigma_j^2), theta_j ~ N(mu, tau^2),
mu ~ N(0, mu_sd^2), tau ~ HalfCauchy(0, tau_scale).  The state is x = [mu, lt = log tau, x_2 .. x_{J+1}], d = J + 2, with x_{2+j} = theta_j
(centred) or eta_j, theta_j = mu + tau eta_j (non-centred).  The density is normalised in x (it includes the Jacobian of lt) and is ONE sum
over the fixed tree of DESIGN 3 with the leaves in state order; the gradients of mu and lt are two more sums over the same tree.  The
operations and their order are the kernels' (no fused multiply-adds); exp / log1p are libm's, the device's differ by an ulp."""
import math

import numpy as np

from path_ref import PathChain, tree_sum

LOG2PI = 1.8378770664093453
CENTERED, NONCENTERED = 0, 1


class Hier:
    """the target with the host constants of pte_set_target_hier"""

    def __init__(self, y, sigma, mu_sd=5.0, tau_scale=5.0, parameterization="centered"):
        self.y = np.asarray(y, dtype=np.float64).ravel()
        self.sigma = np.asarray(sigma, dtype=np.float64).ravel()
        self.J = self.y.size
        self.d = self.J + 2
        self.param = {"centered": CENTERED, "noncentered": NONCENTERED}.get(parameterization, parameterization)
        self.mu_sd, self.tau_scale = float(mu_sd), float(tau_scale)
        self.isig = np.array([1.0 / s for s in self.sigma])
        self.lsig = np.array([math.log(s) for s in self.sigma])
        self.imu, self.lmu = 1.0 / self.mu_sd, math.log(self.mu_sd)
        self.c_tau = math.log(2.0) - math.log(math.pi) - math.log(self.tau_scale)
        self.its = 1.0 / self.tau_scale

    # ---- the density and its gradient as the kernels evaluate them ------------------------------------------------------------------------
    def leaves(self, x, grad=True):
        """(density leaves [d], elementwise gradient [d] with 0 at mu and lt, leaves of d/dmu [d], leaves of d/dlt [d]); grad=False: the
        density leaves alone"""
        x = np.asarray(x, dtype=np.float64)
        with np.errstate(all="ignore"):
            mu, lt = np.float64(x[0]), np.float64(x[1])
            tau = np.exp(lt)
            ts = tau * self.its
            r = ts * ts
            xg = x[2:]
            if self.param == NONCENTERED:
                th = mu + tau * xg
                z = (self.y - th) * self.isig
                zi = z * self.isig
                zt = zi * tau
                lf = (-(z * z + LOG2PI) / 2.0 - self.lsig) + (-(xg * xg + LOG2PI) / 2.0)
                if grad:
                    gj, gm, gt = zt - xg, zi, zt * xg
            else:
                itau = np.exp(-lt)
                z = (self.y - xg) * self.isig
                u = (xg - mu) * itau
                ui = u * itau
                lf = (-(z * z + LOG2PI) / 2.0 - self.lsig) + (-(u * u + LOG2PI) / 2.0 - lt)
                if grad:
                    gj, gm, gt = z * self.isig - ui, ui, u * u - 1.0
            m = mu * self.imu
            l0 = -(m * m + LOG2PI) / 2.0 - self.lmu
            l1 = (self.c_tau - np.log1p(r)) + lt
            t = np.concatenate([[l0, l1], lf])
            if not grad:
                return t, None, None, None
            g = np.concatenate([[0.0, 0.0], gj])
            tm = np.concatenate([[-m * self.imu, 0.0], gm])
            tt = np.concatenate([[0.0, 1.0 - (2.0 * r) / (1.0 + r)], gt])
        return t, g, tm, tt

    def lp(self, x):
        with np.errstate(all="ignore"):
            return tree_sum(self.leaves(x, grad=False)[0])

    def lp_grad(self, x):
        with np.errstate(all="ignore"):
            t, g, tm, tt = self.leaves(x)
            g = g.copy()
            g[0], g[1] = tree_sum(tm), tree_sum(tt)
            return tree_sum(t), g

    def theta(self, x):
        """the group means of a state (or of an array of states [..., d])"""
        x = np.asarray(x, dtype=np.float64)
        if self.param == CENTERED:
            return x[..., 2:]
        return x[..., 0:1] + np.exp(x[..., 1:2]) * x[..., 2:]

    # ---- ground truth: the group means and mu integrate out analytically, a trapezoid rule over lt is left --------------------------------
    def _grid(self, n=40001, lo=-25.0, hi=12.0):
        lt = np.linspace(lo, hi, n)
        tau2 = np.exp(2.0 * lt)[:, None]
        V = self.sigma[None, :] ** 2 + tau2
        A = (1.0 / V).sum(1) + 1.0 / self.mu_sd ** 2
        B = (self.y[None, :] / V).sum(1)
        ll = (-0.5 * np.log(2.0 * math.pi * V).sum(1) - 0.5 * (self.y[None, :] ** 2 / V).sum(1)
              - 0.5 * np.log(self.mu_sd ** 2 * A) + B * B / (2.0 * A))
        lw = ll + (self.c_tau - np.log1p(np.exp(2.0 * lt) * self.its ** 2)) + lt          # x HalfCauchy(tau) tau
        w = np.full(n, lt[1] - lt[0])
        w[0] *= 0.5; w[-1] *= 0.5
        return lt, tau2, V, A, B, lw, w

    def log_evidence(self, n=40001):
        """log p(y)"""
        _, _, _, _, _, lw, w = self._grid(n)
        m = lw.max()
        return float(m + math.log(np.sum(w * np.exp(lw - m))))

    def _moments(self, n=40001):
        lt, tau2, V, A, B, lw, w = self._grid(n)
        p = w * np.exp(lw - lw.max())
        p /= p.sum()
        s2 = self.sigma[None, :] ** 2
        mu_c = B / A                                                   # E[mu | tau], Var[mu | tau] = 1 / A
        wj = s2 / V                                                    # theta_j | mu, tau ~ N((y_j tau^2 + mu sigma_j^2) / V_j, sigma_j^2 tau^2 / V_j)
        mj = (self.y[None, :] * tau2 + mu_c[:, None] * s2) / V
        vj = s2 * tau2 / V + wj * wj / A[:, None]
        mean = np.concatenate([[p @ mu_c, p @ lt], p @ mj])
        second = np.concatenate([[p @ (1.0 / A + mu_c * mu_c), p @ (lt * lt)], p @ (vj + mj * mj)])
        return mean, np.sqrt(second - mean * mean)

    def posterior_means(self, n=40001):
        """[E mu, E log tau, E theta_1 .. E theta_J]"""
        return self._moments(n)[0]

    def posterior_sds(self, n=40001):
        """posterior standard deviations of [mu, log tau, theta_1 .. theta_J]"""
        return self._moments(n)[1]

    def evidence_offset(self, prec):
        """stepping_stone estimates log Z1 / Z0 = log p(y) - (d/2) log(2 pi / p): the reference is unnormalised, the target normalised in x in
        either parameterisation (the change of variables has Jacobian tau^J, which the normalised eta prior absorbs)"""
        return -(self.d / 2.0) * math.log(2.0 * math.pi / prec)


HierChain = PathChain          # (hier, beta, ref_prec): the chain of the interpolated path, tests/path_ref.py
