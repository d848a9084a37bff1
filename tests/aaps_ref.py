"""A NumPy restatement of one AAPS transition as the device runs it (this project's specification of the reference's
src/explorers/AAPS.jl, unpinned until tools/gen_golden.jl runs against a live Pigeons.jl).  The test files use it as their reference.

The draws come from tests/oracle.py::OracleRng (the replica's SplittableRandom with Julia's samplers), in this order: the mix-diagonal
preconditioner's one or two uniforms (am_build_preconditioner), d normals of the momentum, rand(rng, 0:K), then one uniform per candidate
in visit order.  Sums are NumPy's, not the device's fixed tree: states and recorders agree to ~1e-12, not bit for bit."""
import math

import numpy as np

import oracle as O

MAX_LEAPFROGS = 4096            # PTE_AAPS_MAX_LEAPFROGS (pigeons.jl_amd/csrc/pte_aaps_params.hpp)
LOG2PI = 1.8378770664093453


def logaddexp(a, b):
    return O.lib().po_logaddexp(a, b)


class MvnChain:
    """ScaledPrecisionNormalLogPotential at one chain: log density -prec/2 |x|^2, gradient -prec x (ScaledPrecisionNormalPath.jl:19-34)"""

    def __init__(self, precision):
        self.nhp, self.nprec = -0.5 * precision, -precision

    def lp_grad(self, x):
        with np.errstate(all="ignore"):
            return self.nhp * float(np.sum(x * x)), self.nprec * x


def mvn_chain(path_p0, path_p1, beta):
    return MvnChain((1.0 - beta) * path_p0 + beta * path_p1)


class FunnelChain:
    """InterpolatedAD of {ScaledPrecisionNormal(ref_prec) reference -- or a GaussianReference(mean, std) --, Neal's funnel} at beta,
    the arithmetic of AmTarget::logdensity_and_gradient_q (pte_automala.hpp)"""

    def __init__(self, beta, ref_prec, v_mean=None, v_std=None):
        self.beta, self.omb, self.ref_prec = beta, 1.0 - beta, ref_prec
        self.v = None
        if v_mean is not None:
            s2 = np.asarray(v_std, dtype=np.float64) ** 2
            self.v = (np.asarray(v_mean, dtype=np.float64), -0.5 * np.log(2.0 * math.pi * s2), 1.0 / (2.0 * s2), -1.0 / s2)

    def lp_grad(self, x):
        with np.errstate(all="ignore"):                      # IEEE results (inf, nan) where the device gets them: a failed step, not an error
            return self._lp_grad(x)

    def _lp_grad(self, x):
        y = x[0]
        sigma = np.exp(y / 2.0)
        logsigma = np.log(sigma)
        z = x[1:] / sigma
        l2 = float(np.sum(-(z * z + LOG2PI) / 2.0 - logsigma)) + (-((y / 3.0) * (y / 3.0) + LOG2PI) / 2.0 - math.log(3.0))
        g2 = np.empty_like(x)
        g2[1:] = -(z / sigma)
        g2[0] = float(np.sum((z * z - 1.0) / 2.0)) + (-(y / 9.0))
        if self.v is None:
            l1 = -0.5 * self.ref_prec * float(np.sum(x * x))
            g1 = -self.ref_prec * x
        else:
            m, c0, i2, gf = self.v
            dx = x - m
            l1 = float(np.sum(c0 - i2 * (dx * dx)))
            g1 = gf * dx
        return l1 * self.omb + l2 * self.beta, g1 * self.omb + g2 * self.beta


def build_preconditioner(rng, d, mode, p0, p1, target_std):
    """build_preconditioner! (Preconditioner.jl:57-77), the oracle's am_build_preconditioner"""
    if target_std is None or mode == 0:
        return np.ones(d)
    std = np.asarray(target_std, dtype=np.float64)
    inv = np.where(std == 0.0, 1.0, 1.0 / np.where(std == 0.0, 1.0, std))
    if mode == 1:
        return inv
    u = rng.rand()
    if u <= p0:
        return inv
    if u <= p0 + p1:
        return np.ones(d)
    mix = rng.rand()
    return np.where(std == 0.0, 1.0, mix + (1.0 - mix) / np.where(std == 0.0, 1.0, std))


class AapsDensityError(ValueError):
    pass


def transition(x0, rng, chain, step_size, K, M, max_leapfrogs=MAX_LEAPFROGS, uniform_weights=False):
    """One AAPS transition from x0 (the preconditioner M already drawn).  -> dict(x, acc, steps, Kf, failed).
    uniform_weights: choose among the candidates uniformly instead of proportionally to exp(w) -- wrong; the sensitivity check."""
    x0 = np.asarray(x0, dtype=np.float64)
    d = x0.size
    p0 = np.array([rng.randn() for _ in range(d)])
    Kf = rng.rand_range(0, K)
    Kb = K - Kf
    lp0, g0 = chain.lp_grad(x0)
    g0 = g0 / M
    w0 = lp0 - 0.5 * float(np.sum(p0 * p0))
    if not math.isfinite(w0):
        raise AapsDensityError("AAPS can only be called on a configuration of positive density")
    h0 = float(np.sum(p0 * g0))
    eps, half = step_size, step_size / 2
    st = dict(L=0.0 if uniform_weights else w0, sel=x0.copy(), steps=0, failed=False)

    def run(direction, stop_at):
        with np.errstate(all="ignore"):
            _run(direction, stop_at)

    def _run(direction, stop_at):
        x, p, g = x0.copy(), direction * p0, g0.copy()
        s_prev, seg = h0 >= 0.0, 0
        while True:
            if st["steps"] == max_leapfrogs:
                st["failed"] = True
                return
            st["steps"] += 1
            p = p + half * g                                  # am_leap_frog
            x = x + eps * (p / M)
            lp, gr = chain.lp_grad(x)
            g = gr / M
            if not math.isfinite(lp - 0.5 * float(np.sum(p * p))):
                st["failed"] = True
                return
            p = p + half * g
            pp = float(np.sum(p * p))
            w = lp - 0.5 * pp
            if not math.isfinite(pp) or not math.isfinite(w):
                st["failed"] = True
                return
            s = direction * float(np.sum(p * g)) >= 0.0
            if direction > 0:
                seg += 1 if (not s_prev and s) else 0
            else:
                seg -= 1 if (not s and s_prev) else 0
            if seg == stop_at:
                return
            wt = 0.0 if uniform_weights else w
            st["L"] = logaddexp(st["L"], wt)
            if rng.rand() < math.exp(wt - st["L"]):
                st["sel"] = x.copy()
            s_prev = s

    run(1.0, Kf + 1)
    if not st["failed"]:
        run(-1.0, -(Kb + 1))
    if st["failed"]:
        return dict(x=x0.copy(), acc=0.0, steps=st["steps"], Kf=Kf, failed=True)
    acc = 1.0 - math.exp((0.0 if uniform_weights else w0) - st["L"])
    return dict(x=st["sel"], acc=acc, steps=st["steps"], Kf=Kf, failed=False)
