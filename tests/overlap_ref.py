"""The replica overlap, restated from its definition for the tests: spins +-1 on the periodic lattice, np.roll per axis.

    k  = #{sites i : s_i^a != s_i^b}
    kl = #{bonds (i, j) : s_i^a s_j^a != s_i^b s_j^b}, every site i owning the bond to its +direction neighbour j along every axis
         (at L = 2 the +direction and the -direction neighbour are the same site: the two bonds are two terms)

No XOR, no shift, no popcount: the device's form (pigeons.jl_amd/csrc/pte_overlap.hpp) is tested against this, not against itself."""
import numpy as np


def lattice_shape(d, cube):
    L = round(d ** (1.0 / 3.0)) if cube else round(d ** 0.5)
    shape = (L, L, L) if cube else (L, L)
    assert int(np.prod(shape)) == d, (d, cube)
    return shape


def spins(bits, shape):
    """the 0 / 1 state of the ABI (site (z, y, x) at (z L + y) L + x; 2-D: (i, j) at i L + j) as +-1 spins on the lattice"""
    return (2 * np.asarray(bits).astype(np.int64) - 1).reshape(shape)


def k_and_kl(a_bits, b_bits, shape):
    sa, sb = spins(a_bits, shape), spins(b_bits, shape)
    k = int(np.sum(sa != sb))
    kl = 0
    for axis in range(len(shape)):
        kl += int(np.sum(sa * np.roll(sa, -1, axis=axis) != sb * np.roll(sb, -1, axis=axis)))
    return k, kl


class Accumulators:
    """what the device keeps per chain, all integers"""

    def __init__(self, N, d):
        self.n = np.zeros(N, dtype=np.int64)
        self.hist = np.zeros((N, d + 1), dtype=np.int64)
        self.link_n = np.zeros(N, dtype=np.int64)
        self.link_sum = np.zeros(N, dtype=np.int64)
        self.link_sum2 = np.zeros(N, dtype=np.int64)

    def record(self, xa, chain_a, xb, chain_b, shape, link=True):
        """one record: x[slot] the 0 / 1 states and chain[slot] the chain of every slot, of run a and of run b; keyed by chain"""
        slot_b = {int(c): s for s, c in enumerate(chain_b)}
        for sa, c in enumerate(chain_a):
            c = int(c)
            k, kl = k_and_kl(xa[sa], xb[slot_b[c]], shape)
            self.n[c] += 1
            self.hist[c, k] += 1
            if link:
                self.link_n[c] += 1
                self.link_sum[c] += kl
                self.link_sum2[c] += kl * kl

    def assert_equal(self, rec):
        """rec: a pigeons_amd.OverlapRecord"""
        for name in ("n", "hist", "link_n", "link_sum", "link_sum2"):
            assert np.array_equal(getattr(rec, name), getattr(self, name)), name
