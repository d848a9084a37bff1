"""The interpolated path of the data families as automala_body and the SliceSampler kernels compute it, restated once: one chain
(1 - beta) ScaledPrecisionNormal(ref_prec) + beta target over any model with `lp(x)` and `lp_grad(x) -> (lp, gradient)`, and the fixed
reduction tree its sums follow.  tests/{glm,hier,ar1,dense,mixture,mixture_model}_ref.py name it `<Family>Chain`; every GPU family test,
tests/family_blocks.py, tests/family_edges.py and tests/automala_ref.py hold the device to it.

The contract of the kernels that stands here and nowhere else: S = tree_sum(x * x); lp_grad accumulates `0.0 + l1 * omb + l2 * beta` in that
order and never short-circuits; path_lp returns the reference alone at beta = 0 and the target alone at beta = 1, and
`omb * l1 + beta * l2` between."""
import numpy as np


def tree_sum(v):
    """the fixed reduction tree of DESIGN 3 over the leaves v (natural order, zero-padded to a power of two)"""
    a = np.asarray(v, dtype=np.float64).ravel()
    P = 1
    while P < a.size:
        P <<= 1
    b = np.zeros(P)
    b[:a.size] = a
    while b.size > 1:
        b = b[0::2] + b[1::2]
    return float(b[0])


class PathChain:
    """one chain of the interpolated path (1 - beta) ScaledPrecisionNormal(ref_prec) + beta model: lp_grad is the AD form of
    AmTarget::logdensity_and_gradient_q (no short-circuits), path_lp the plain callable SliceSampler evaluates (InterpolatedLogPotential.jl:9-16)"""

    def __init__(self, model, beta, ref_prec):
        self.model, self.beta, self.omb, self.ref_prec = model, beta, 1.0 - beta, ref_prec

    def lp_grad(self, x):
        x = np.asarray(x, dtype=np.float64)
        with np.errstate(all="ignore"):
            S = tree_sum(x * x)
            l2, g2 = self.model.lp_grad(x)
            l1 = (-0.5 * self.ref_prec) * S
            return 0.0 + l1 * self.omb + l2 * self.beta, ((-self.ref_prec) * x) * self.omb + g2 * self.beta

    def path_lp(self, x):
        x = np.asarray(x, dtype=np.float64)
        with np.errstate(all="ignore"):
            S = tree_sum(x * x)
            if self.beta == 0.0:
                return (-0.5 * self.ref_prec) * S
            l2 = self.model.lp(x)
            if self.beta == 1.0:
                return l2
            return self.omb * ((-0.5 * self.ref_prec) * S) + self.beta * l2
