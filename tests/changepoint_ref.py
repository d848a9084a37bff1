"""A NumPy restatement of the Poisson change-point family as the device computes it (this project's specification), built on
the fixed tree (tests/mixture_ref.py).  The test files use it as their reference.

The state is [r_0..r_K, tau_1..tau_K]: K + 1 log rates, then K change points, integral doubles in 0..n, unordered.  With s_1 <= ... <= s_K
the sorted taus, s_0 = 0 and s_{K+1} = n, segment j covers observations [s_j, s_{j+1}) and
    t_j = (Y_j * r_j) - (len_j * exp(r_j)),  0 when len_j == 0,     Y_j = C[s_{j+1}] - C[s_j],   len_j = s_{j+1} - s_j
    target = ((((-(p/2) S) + c_prior) + c_tau) + tree_sum(t)) + c_obs,   S = tree_sum(r^2)
and -inf when a tau is outside 0..n.  The kernel's two evaluation forms compute these bits both, so one restatement serves them.

exact() enumerates the (n + 1)^K placements and integrates every segment's rate out by quadrature."""
import ctypes
import ctypes.util
import itertools
import math

import numpy as np

from mixture_ref import tree_sum

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.lgamma.restype = ctypes.c_double
_libm.lgamma.argtypes = [ctypes.c_double]


def lgamma(x):
    """the host libm's lgamma, the one pte_set_target_changepoint calls (math.lgamma is CPython's own and may differ in the last bit)"""
    return _libm.lgamma(float(x))


class ChangePoint:
    """the target with the host constants of pte_set_target_changepoint; prec = the prior's (and the reference's) precision"""

    def __init__(self, y, n_changepoints, prec):
        self.y = np.asarray(y, dtype=np.float64)
        self.n, self.K, self.prec = self.y.size, int(n_changepoints), float(prec)
        self.C = np.concatenate([[0.0], np.cumsum(self.y)])             # exact: integers below 2^36
        self.c_prior = -((self.K + 1) / 2.0) * math.log(2.0 * math.pi / self.prec)
        self.c_tau = -float(self.K) * math.log(float(self.n + 1))
        c = 0.0
        for v in self.y:
            c = c - lgamma(v + 1.0)
        self.c_obs = c

    def split(self, state):
        state = np.asarray(state, dtype=np.float64)
        return state[:self.K + 1], state[self.K + 1:]

    def inside(self, state):
        tau = self.split(state)[1]
        return bool(np.all((tau >= 0.0) & (tau <= self.n)))

    def sums(self, state):
        """(S, sum of the segment terms) of a state inside the support"""
        r, tau = self.split(state)
        s = np.concatenate([[0], np.sort(tau).astype(np.int64), [self.n]])
        length = (s[1:] - s[:-1]).astype(np.float64)
        Y = self.C[s[1:]] - self.C[s[:-1]]
        with np.errstate(all="ignore"):
            t = np.where(length == 0.0, 0.0, (Y * r) - (length * np.exp(r)))
        return tree_sum(r * r), tree_sum(t)

    def combine(self, S, ls):
        return (((((-0.5 * self.prec) * S) + self.c_prior) + self.c_tau) + ls) + self.c_obs

    def lp(self, state):
        if not self.inside(state):
            return -math.inf
        return self.combine(*self.sums(state))

    def evidence_offset(self):
        """stepping_stone estimates log p(y) + this: the reference, exp(-(p/2) S) on r and uniform on tau, has mass
        (2 pi / p)^((K+1)/2) (n + 1)^K"""
        return -((self.K + 1) / 2.0) * math.log(2.0 * math.pi / self.prec) - self.K * math.log(self.n + 1.0)

    # ---- exact answers: the placements enumerated, every rate integrated out ---------------------------------------------------------------
    def _log_segment(self, a, b, cache, grid):
        """log of the integral of N(r; 0, 1 / p) exp(Y r - len exp(r)) dr over segment [a, b): the trapezoid rule on a grid that holds the
        integrand's mass (it decays like a Gaussian to the left and doubly exponentially to the right)"""
        if (a, b) not in cache:
            length, Y = float(b - a), self.C[b] - self.C[a]
            if length == 0.0:
                cache[a, b] = 0.0
            else:
                f = -0.5 * self.prec * grid ** 2 + Y * grid - length * np.exp(grid)
                m = f.max()
                cache[a, b] = m + math.log(np.exp(f - m).sum() * (grid[1] - grid[0])) - 0.5 * math.log(2.0 * math.pi / self.prec)
        return cache[a, b]

    def exact(self):
        """(log p(y), {sorted placement: posterior probability}) over the sorted placements s_1 <= ... <= s_K"""
        grid = np.linspace(-40.0, 20.0, 60001)
        cache, logw = {}, {}
        for taus in itertools.product(range(self.n + 1), repeat=self.K):
            s = tuple(sorted(taus))
            b = (0,) + s + (self.n,)
            lw = sum(self._log_segment(b[j], b[j + 1], cache, grid) for j in range(self.K + 1))
            logw[s] = np.logaddexp(logw[s], lw) if s in logw else lw
        keys = list(logw)
        v = np.array([logw[k] for k in keys])
        m = v.max()
        tot = m + math.log(np.exp(v - m).sum())
        log_ev = tot + self.c_tau + self.c_obs
        return log_ev, {k: math.exp(x - tot) for k, x in zip(keys, v)}


class ChangePointChain:
    """one chain of the path (1 - beta) ref + beta target, ref = -(ref_prec / 2) S; -inf outside the support at every beta.  path_lp is the
    call-back of oracle.MixedSliceSampler with kinds = [FLOAT64] * (K + 1) + [INTEGER] * K."""

    def __init__(self, cp, beta, ref_prec):
        self.cp, self.beta, self.omb, self.ref_prec = cp, beta, 1.0 - beta, ref_prec

    def path_lp(self, state):
        if not self.cp.inside(state):
            return -math.inf
        S, ls = self.cp.sums(state)
        ref = (-0.5 * self.ref_prec) * S
        if self.beta == 0.0:
            return ref
        l2 = self.cp.combine(S, ls)
        if self.beta == 1.0:
            return l2
        with np.errstate(all="ignore"):
            return self.omb * ref + self.beta * l2
