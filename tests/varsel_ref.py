"""A NumPy restatement of the variable-selection family as the device computes it (this project's specification), built on the
GLM restatement (tests/glm_ref.py: terms, fma, the lane sums) and the fixed tree.  The test files use it as their reference.

The state is [theta_0..theta_{d-1}, gamma_0..gamma_{d-1}] (gamma 0.0 / 1.0), b_j = gamma_j theta_j, eta = X b, and
    target = ((((-(p/2) S) + c_prior) + G) + sum_i l_i(eta_i)) + c_obs,   S = tree_sum(theta^2),   G = m log pi + (d - m) log(1 - pi).
VarSel.lp forms eta in full (sequential in j, one fused multiply-add per term): what k_refresh_varsel_stats, the explorer's prologue and its
epilogue do.  VarSelChain.path_lp is the call-back SliceSampler evaluates, with the explorer's cached predictor: it tracks the committed
state, its eta and the one coordinate being updated (column c, effective coefficient b_old), forms a proposal's predictor as
fma(X_c, b_new, fma(X_c, -b_old, eta)) -- eta itself when b_new == b_old -- and commits a coordinate's final value, the same way, when the
sampler moves on to the next one.

Closed forms for the normal-identity likelihood enumerate the 2^d models: y | gamma ~ N(0, sigma^2 I + X_gamma X_gamma^T / p)."""
import itertools
import math

import numpy as np

from glm_ref import Glm, fma, LOG2PI, NORMAL_IDENTITY
from mixture_ref import tree_sum


class VarSel:
    """the target with the host constants of pte_set_target_varsel; prec = the prior's (and the reference's) precision"""

    def __init__(self, X, y, likelihood, noise_sd, prec, inclusion_prob=0.5):
        self.glm = Glm(X, y, likelihood, noise_sd, prec)           # c_prior, c_obs, w2 with d = the number of columns
        self.X, self.y, self.n, self.d = self.glm.X, self.glm.y, self.glm.n, self.glm.d
        self.prec, self.pi = float(prec), float(inclusion_prob)
        self.log_pi, self.log_1mpi = math.log(self.pi), math.log(1.0 - self.pi)

    def split(self, state):
        state = np.asarray(state, dtype=np.float64)
        return state[:self.d], state[self.d:]

    def eta(self, state):
        theta, gamma = self.split(state)
        e = np.zeros(self.n)
        for j in range(self.d):
            e = fma(self.X[:, j], gamma[j] * theta[j], e)
        return e

    def loglik_sum(self, eta):
        return self.glm.loglik_sum(self.glm.terms(eta)[0])

    def combine(self, S, m, ls):
        G = m * self.log_pi + (float(self.d) - m) * self.log_1mpi
        return (((((-0.5 * self.prec) * S) + self.glm.c_prior) + G) + ls) + self.glm.c_obs

    def lp(self, state):
        theta, gamma = self.split(state)
        with np.errstate(all="ignore"):
            return self.combine(tree_sum(theta * theta), float(np.sum(gamma)), self.loglik_sum(self.eta(state)))

    def evidence_offset(self):
        """stepping_stone estimates log p(y) + this: the reference, exp(-(p/2) S) on theta and uniform on gamma, has mass (2 pi / p)^(d/2) 2^d"""
        return -(self.d / 2.0) * math.log(2.0 * math.pi / self.prec) - self.d * math.log(2.0)

    # ---- closed forms (normal-identity likelihood): the 2^d models enumerated --------------------------------------------------------
    def models(self):
        """[(gamma, log p(y | gamma) + log p(gamma), E[theta | y, gamma] on the included columns)]"""
        assert self.glm.lik == NORMAL_IDENTITY
        sd2 = self.glm.sd ** 2
        out = []
        for bits in itertools.product((0, 1), repeat=self.d):
            g = np.array(bits, dtype=np.float64)
            Xg = self.X[:, g > 0]
            C = sd2 * np.eye(self.n) + Xg @ Xg.T / self.prec
            _, logdet = np.linalg.slogdet(C)
            lml = -0.5 * (self.n * LOG2PI + logdet + self.y @ np.linalg.solve(C, self.y))
            k = int(g.sum())
            mean = np.zeros(self.d)
            if k:
                A = self.prec * np.eye(k) + Xg.T @ Xg / sd2
                mean[g > 0] = np.linalg.solve(A, Xg.T @ self.y) / sd2
            out.append((g, lml + k * self.log_pi + (self.d - k) * self.log_1mpi, mean))
        return out

    def exact(self):
        """(posterior inclusion probabilities, posterior means of b_j = gamma_j theta_j, log evidence)"""
        ms = self.models()
        lw = np.array([w for _, w, _ in ms])
        mx = lw.max()
        log_ev = mx + math.log(np.exp(lw - mx).sum())
        pr = np.exp(lw - log_ev)
        incl = sum(p * g for p, (g, _, _) in zip(pr, ms))
        b = sum(p * mean for p, (_, _, mean) in zip(pr, ms))
        return incl, b, log_ev


class VarSelChain:
    """one chain of the path (1 - beta) ref + beta target, ref = -(ref_prec / 2) S.  lp_full: from the state alone.  path_lp: the call-back of
    one SliceSampler step (oracle.MixedSliceSampler with kinds = [FLOAT64] * d + [BOOL] * d), the cached-predictor arithmetic of the kernel;
    a new VarSelChain per step."""

    def __init__(self, vs, beta, ref_prec):
        self.vs, self.beta, self.omb, self.ref_prec = vs, beta, 1.0 - beta, ref_prec
        self.state = None               # the committed state, its eta and sums
        self.cur = None                 # the coordinate being updated

    def _path(self, S, m, ls):
        ref = (-0.5 * self.ref_prec) * S
        if self.beta == 0.0:
            return ref
        l2 = self.vs.combine(S, m, ls)
        if self.beta == 1.0:
            return l2
        return self.omb * ref + self.beta * l2

    def lp_full(self, state):
        theta, gamma = self.vs.split(state)
        with np.errstate(all="ignore"):
            return self._path(tree_sum(theta * theta), float(np.sum(gamma)), self.vs.loglik_sum(self.vs.eta(state)))

    def _proposal(self, c, v):
        """(eta, S, m, ls) of the committed state with coordinate c at v"""
        vs, d = self.vs, self.vs.d
        j = c % d
        old = self.state[c]
        other = self.state[j + d] if c < d else self.state[j]
        b_old, b_new = (other * old, other * v) if c < d else (old * other, v * other)
        theta = self.state[:d].copy()
        m = self.m
        if c < d:
            theta[j] = v
        else:
            m = (self.m - old) + v
        if b_new == b_old:
            eta, ls = self.eta, self.ls
        else:
            eta = fma(vs.X[:, j], b_new, fma(vs.X[:, j], -b_old, self.eta))
            ls = vs.loglik_sum(eta)
        return eta, tree_sum(theta * theta), m, ls

    def path_lp(self, state):
        state = np.array(state, dtype=np.float64)
        with np.errstate(all="ignore"):
            if self.state is None:
                self.state = state.copy()
                self.eta = self.vs.eta(state)
                theta, gamma = self.vs.split(state)
                self.S, self.m, self.ls = tree_sum(theta * theta), float(np.sum(gamma)), self.vs.loglik_sum(self.eta)
                return self._path(self.S, self.m, self.ls)
            others = [int(i) for i in np.flatnonzero(state != self.state) if i != self.cur]
            if others:                  # the sampler has moved on: coordinate cur ends at state[cur]
                assert len(others) == 1, others
                if self.cur is not None:
                    self.eta, self.S, self.m, self.ls = self._proposal(self.cur, state[self.cur])
                    self.state[self.cur] = state[self.cur]
                self.cur = others[0]
            if self.cur is None:
                return self._path(self.S, self.m, self.ls)
            _, S, m, ls = self._proposal(self.cur, state[self.cur])
            return self._path(S, m, ls)
