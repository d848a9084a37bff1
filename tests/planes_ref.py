"""The plane autocorrelation of the overlap field, restated from its definition for the tests: spins +-1 on the lattice,

    q_i        = s_i^a s_i^b
    Q_axis[p]  = the sum of q over the sites whose coordinate along the axis is p
    C_axis(r)  = sum_p Q_axis[p] Q_axis[(p + r) mod L]

Axis 0 is the fastest site index (x of site (z, y, x) at (z L + y) L + x; the column j of site (i, j) at i L + j), axis 1 the next, axis 2
the cube's z: axis a of the specification is numpy axis ndim - 1 - a of the reshaped lattice.

No XOR, no shift, no popcount: the device's form (pigeons.jl_amd/csrc/pte_overlap_planes.hpp) is tested against this, not against itself."""
import numpy as np

import overlap_ref as R


def plane_sums(a_bits, b_bits, shape):
    """Q [n_axes][L]"""
    q = R.spins(a_bits, shape) * R.spins(b_bits, shape)
    nd = len(shape)
    return np.array([q.sum(axis=tuple(ax for ax in range(nd) if ax != nd - 1 - a)) for a in range(nd)], dtype=np.int64)


def plane_corr(a_bits, b_bits, shape):
    """C [n_axes][L]"""
    Q = plane_sums(a_bits, b_bits, shape)
    L = shape[0]
    return np.array([[int(np.sum(Qa * np.roll(Qa, -r))) for r in range(L)] for Qa in Q], dtype=np.int64)


class Accumulators:
    """what the device keeps per chain, all integers"""

    def __init__(self, N, shape):
        self.shape = tuple(shape)
        self.plane_n = np.zeros(N, dtype=np.int64)
        self.plane_corr = np.zeros((N, len(shape), shape[0]), dtype=np.int64)

    def record(self, xa, chain_a, xb, chain_b):
        """one record: x[slot] the 0 / 1 states and chain[slot] the chain of every slot, of run a and of run b; keyed by chain"""
        slot_b = {int(c): s for s, c in enumerate(chain_b)}
        for sa, c in enumerate(chain_a):
            c = int(c)
            self.plane_n[c] += 1
            self.plane_corr[c] += plane_corr(xa[sa], xb[slot_b[c]], self.shape)

    def assert_equal(self, rec):
        """rec: a pigeons_amd.OverlapRecord"""
        assert rec.plane_n is not None and rec.plane_corr is not None
        assert np.array_equal(rec.plane_n, self.plane_n), "plane_n"
        assert np.asarray(rec.plane_corr).shape == self.plane_corr.shape
        assert np.array_equal(rec.plane_corr, self.plane_corr), "plane_corr"


def hist_identity(rec):
    """sum_r plane_corr[c][axis][r] == sum_k hist[c][k] (d - 2 k)^2 for every axis, in Python integers"""
    d = int(rec.dim)
    for c in range(len(rec.n)):
        want = sum(int(h) * (d - 2 * k) ** 2 for k, h in enumerate(rec.hist[c]) if h)
        for ax in range(np.asarray(rec.plane_corr).shape[1]):
            assert sum(int(v) for v in rec.plane_corr[c, ax]) == want, (c, ax)


def states_of_density(g, N, d, shape, trial):
    """(xa, xb) [N][d] 0 / 1 as float64: xa uniform, xb = xa with the sites of t flipped; t of density 0.5, 0.1, 0.9 (trial 0, 1, 2) or
    striped (3): whole planes of axis 0 and of the last axis differ alternately, with 2 % of noise -- the states in which the plane sums are
    large and the vertical counters of the kernel reach their high bits"""
    xa = g.integers(0, 2, size=(N, d))
    if trial < 3:
        t = g.random((N, d)) < (0.5, 0.1, 0.9)[trial]
    else:
        idx = np.indices(shape)
        stripes = ((idx[-1] % 2 == 0) | (idx[0] % 4 == 1)).reshape(-1)
        t = np.tile(stripes, (N, 1)) != (g.random((N, d)) < 0.02)
    return xa.astype(np.float64), np.where(t, 1 - xa, xa).astype(np.float64)
