"""A NumPy restatement of the latent-AR(1) state-space family as the device computes it (this project's specification), and the
exact ground truth of its normal observation model by quadrature.  The test files use it as their reference.

The model: T observations y_t of a latent state h, h_0 ~ N(mu, sigma^2 / om), h_t | h_{t-1} ~ N(mu + phi (h_{t-1} - mu), sigma^2), phi = tanh(a),
sigma = exp(ls), om = 1 - phi^2; mu ~ N(0, mu_sd^2), a ~ N(phi_loc, phi_scale^2), sigma ~ HalfCauchy(0, sigma_scale); y_t ~ N(0, exp(h_t))
(stochastic volatility) or y_t ~ N(h_t, obs_sd^2) (normal).  The state is x = [mu, a, ls, h_0 .. h_{T-1}], d = T + 3.  The density is
normalised in x (it includes the Jacobian of ls) and is ONE sum over the fixed tree of DESIGN 3 with the leaves in state order; the gradients
of mu, a and ls are three more sums over the same tree.  The operations and their order are the kernels' (no fused multiply-adds); tanh / exp /
log / log1p are libm's, the device's differ by an ulp.  om, its root, its log and 1 - phi come from exp(-2 |a|), as in the kernel: 1 - tanh(a)^2
cancels (tests/test_family_edges_cpu.py holds these leaves to a 60-digit evaluation of the model up to |a| = 25)."""
import math

import numpy as np

from path_ref import PathChain, tree_sum

LOG2PI = 1.8378770664093453
LOG2 = 0.6931471805599453
STOCHASTIC_VOLATILITY, NORMAL_IDENTITY = 0, 1


class Ar1:
    """the target with the host constants of pte_set_target_ar1"""

    def __init__(self, y, likelihood="stochastic_volatility", obs_sd=1.0, mu_sd=5.0, phi_loc=0.0, phi_scale=1.0, sigma_scale=1.0):
        self.y = np.asarray(y, dtype=np.float64).ravel()
        self.y2 = self.y * self.y
        self.T = self.y.size
        self.d = self.T + 3
        self.lik = {"stochastic_volatility": STOCHASTIC_VOLATILITY, "normal_identity": NORMAL_IDENTITY}.get(likelihood, likelihood)
        self.obs_sd, self.mu_sd, self.phi_loc = float(obs_sd), float(mu_sd), float(phi_loc)
        self.phi_scale, self.sigma_scale = float(phi_scale), float(sigma_scale)
        self.imu, self.lmu = 1.0 / self.mu_sd, math.log(self.mu_sd)
        self.ips, self.lps = 1.0 / self.phi_scale, math.log(self.phi_scale)
        self.c_sigma = math.log(2.0) - math.log(math.pi) - math.log(self.sigma_scale)
        self.iss = 1.0 / self.sigma_scale
        self.iobs, self.lobs = 1.0 / self.obs_sd, math.log(self.obs_sd)

    # ---- the density and its gradient as the kernels evaluate them ------------------------------------------------------------------------
    def leaves(self, x, grad=True):
        """(density leaves [d], elementwise gradient [d] with 0 at mu, a and ls, leaves of d/dmu, d/da, d/dls [d] each); grad=False: the
        density leaves alone"""
        x = np.asarray(x, dtype=np.float64)
        with np.errstate(all="ignore"):
            mu, a, ls = np.float64(x[0]), np.float64(x[1]), np.float64(x[2])
            phi = np.tanh(a)
            ta = np.abs(a)                                               # om = sech^2(a) and 1 - phi from exp(-2 |a|): 1 - tanh^2 cancels
            e2 = np.exp(-2.0 * ta)
            q2 = 1.0 + e2
            sqom = (2.0 * np.exp(-ta)) / q2
            om = sqom * sqom
            lom = 2.0 * ((LOG2 - ta) - np.log1p(e2))
            omp = (2.0 * e2) / q2 if a > 0.0 else 2.0 / q2               # 1 - phi
            isg, sg = np.exp(-ls), np.exp(ls)
            ts = sg * self.iss
            r = ts * ts
            c0, pis, cm, ca = isg * sqom, phi * isg, omp * isg, isg * om
            h = x[3:]
            first = np.arange(self.T) == 0
            hm = h - mu
            pv = np.concatenate([[0.0], hm[:-1]])                         # h_{t-1} - mu (h_0 reads none)
            u = np.where(first, (hm * isg) * sqom, (hm - phi * pv) * isg)
            tr = -(u * u + LOG2PI) / 2.0 - ls
            tr[0] = tr[0] + lom / 2.0
            if self.lik == NORMAL_IDENTITY:
                z = (self.y - h) * self.iobs
                ob = -(z * z + LOG2PI) / 2.0 - self.lobs
                obd = z * self.iobs
            else:
                ye = self.y2 * np.exp(-h)
                ob = -((ye + h) + LOG2PI) / 2.0
                obd = (ye - 1.0) / 2.0
            m = mu * self.imu
            za = (a - self.phi_loc) * self.ips
            l0 = -(m * m + LOG2PI) / 2.0 - self.lmu
            l1 = -(za * za + LOG2PI) / 2.0 - self.lps
            l2 = (self.c_sigma - np.log1p(r)) + ls
            t = np.concatenate([[l0, l1, l2], tr + ob])
            if not grad:
                return t, None, None, None, None
            ut = np.where(first, 0.0, u)                                 # the residuals that read a predecessor
            us = np.concatenate([ut[1:], [0.0]])                          # u_{t+1} (the last state has no successor)
            ow = np.where(first, u * c0, u * isg)
            g = np.concatenate([[0.0, 0.0, 0.0], (us * pis - ow) + obd])
            tm = np.concatenate([[-m * self.imu, 0.0, 0.0], np.where(first, u * c0, u * cm)])
            ta = np.concatenate([[0.0, -za * self.ips, 0.0], np.where(first, (u * u - 1.0) * phi, (u * pv) * ca)])
            tl = np.concatenate([[0.0, 0.0, 1.0 - (2.0 * r) / (1.0 + r)], u * u - 1.0])
        return t, g, tm, ta, tl

    def lp(self, x):
        with np.errstate(all="ignore"):
            return tree_sum(self.leaves(x, grad=False)[0])

    def lp_plain(self, x):
        """the same leaves added by np.sum: what the tree sum is checked against, and what the long CPU chains evaluate"""
        with np.errstate(all="ignore"):
            return float(np.sum(self.leaves(x, grad=False)[0]))

    def lp_grad(self, x):
        with np.errstate(all="ignore"):
            t, g, tm, ta, tl = self.leaves(x)
            g = g.copy()
            g[0], g[1], g[2] = tree_sum(tm), tree_sum(ta), tree_sum(tl)
            return tree_sum(t), g

    def evidence_offset(self, prec):
        """stepping_stone estimates log Z1 / Z0 = log p(y) - (d/2) log(2 pi / p): the reference is unnormalised, the target normalised in x"""
        return -(self.d / 2.0) * math.log(2.0 * math.pi / prec)

    # ---- ground truth of the normal model: given (a, ls) it is linear-Gaussian, a trapezoid rule over (a, ls) is left ---------------------
    def _quadrature(self, na=321, nl=401, a_lo=-8.0, a_hi=8.0, l_lo=-14.0, l_hi=6.0):
        """Given (a, ls): y ~ N(0, Sigma), Sigma = C + obs_sd^2 I + mu_sd^2 11', C_ij = sigma^2 phi^|i-j| / om.  -> (log evidence, posterior
        means [d], posterior sds [d]) of [mu, a, ls, h]: the conditional Gaussian moments E[mu | .] = mu_sd^2 1' Sigma^-1 y,
        E[h | .] = (C + mu_sd^2 11') Sigma^-1 y (and their conditional variances) averaged under the weights of the grid"""
        if self.lik != NORMAL_IDENTITY:
            raise ValueError("the quadrature is that of the normal observation model")
        T, y = self.T, self.y
        av, lv = np.linspace(a_lo, a_hi, na), np.linspace(l_lo, l_hi, nl)
        wa = np.full(na, av[1] - av[0]); wa[0] *= 0.5; wa[-1] *= 0.5
        wl = np.full(nl, lv[1] - lv[0]); wl[0] *= 0.5; wl[-1] *= 0.5
        lag = np.abs(np.arange(T)[:, None] - np.arange(T)[None, :])
        one = np.ones(T)
        D = self.obs_sd ** 2 * np.eye(T) + self.mu_sd ** 2 * np.outer(one, one)
        s2 = np.exp(2.0 * lv)
        lp_l = (self.c_sigma - np.log1p(s2 * self.iss ** 2)) + lv                      # HalfCauchy(sigma) sigma
        logw = np.empty((na, nl))
        m1 = np.empty((na, nl, T + 1)); m2 = np.empty((na, nl, T + 1))                # conditional first and second moments of [mu, h]
        for i, a in enumerate(av):
            phi = math.tanh(a)
            om = 1.0 - phi * phi
            Cn = (phi ** lag / om)[None] * s2[:, None, None]                            # [nl][T][T]
            Sig = Cn + D[None]
            L = np.linalg.cholesky(Sig)
            logdet = 2.0 * np.log(np.einsum("kii->ki", L)).sum(1)
            sy = np.linalg.solve(Sig, np.broadcast_to(y[None, :, None], (nl, T, 1)))[..., 0]
            za = (a - self.phi_loc) * self.ips
            logw[i] = (-0.5 * (logdet + T * LOG2PI) - 0.5 * (sy @ y)) + (-(za * za + LOG2PI) / 2.0 - self.lps) + lp_l
            Pm = np.concatenate([np.broadcast_to(self.mu_sd ** 2 * one[None, None, :], (nl, 1, T)), Cn + self.mu_sd ** 2], axis=1)   # Cov([mu, h], y)
            mean = np.einsum("kij,kj->ki", Pm, sy)
            prior_var = np.concatenate([np.full((nl, 1), self.mu_sd ** 2), np.einsum("kii->ki", Cn) + self.mu_sd ** 2], axis=1)
            var = prior_var - np.einsum("kij,kij->ki", Pm, np.swapaxes(np.linalg.solve(Sig, np.swapaxes(Pm, 1, 2)), 1, 2))
            m1[i] = mean; m2[i] = var + mean * mean
        mx = logw.max()
        W = np.exp(logw - mx) * wa[:, None] * wl[None, :]
        Z = W.sum()
        p = W / Z
        e_a, e_l = (p.sum(1) * av).sum(), (p.sum(0) * lv).sum()
        e_a2, e_l2 = (p.sum(1) * av * av).sum(), (p.sum(0) * lv * lv).sum()
        e1, e2 = np.einsum("il,ilk->k", p, m1), np.einsum("il,ilk->k", p, m2)
        mean = np.concatenate([[e1[0], e_a, e_l], e1[1:]])
        second = np.concatenate([[e2[0], e_a2, e_l2], e2[1:]])
        return float(mx + math.log(Z)), mean, np.sqrt(second - mean * mean)

    def log_evidence(self, na=321, nl=401):
        """log p(y)"""
        return self._quadrature(na, nl)[0]

    def posterior_means(self, na=321, nl=401):
        """[E mu, E a, E ls, E h_0 .. E h_{T-1}]"""
        return self._quadrature(na, nl)[1]

    def posterior_sds(self, na=321, nl=401):
        return self._quadrature(na, nl)[2]


Ar1Chain = PathChain          # (ar1, beta, ref_prec): the chain of the interpolated path, tests/path_ref.py
