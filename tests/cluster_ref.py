"""Houdayer's cluster move between the two copies of a lattice pair, restated from its definition for the tests: spins +-1 on
the periodic lattice, a stack flood fill over np.unravel_index neighbours, the seed site np.flatnonzero(t)[j], delta the difference of two
full energy sums.

    t      the sites at which the two copies differ, k their number
    draw   u = mix64(seed + (m N + c + 1) gamma) mod 2^64, j = ((u >> 32) k) >> 32
    C      the connected component of the j-th site of t (increasing site index) among the sites of t, nearest-neighbour links, periodic
    flip   both copies on C;  delta = S(a') - S(a) = -(S(b') - S(b))

No XOR, no shift, no popcount: the device's form (pigeons.jl_amd/csrc/pte_cluster.hpp) is tested against this, not against itself."""
import functools

import numpy as np

from overlap_ref import lattice_shape, spins  # noqa: F401  (lattice_shape: for the callers)

GAMMA = 0x9E3779B97F4A7C15
M64 = (1 << 64) - 1


def mix64(z):
    """the project's mix64 (pigeons.jl_amd/csrc/pte_device.hpp) in Python integers"""
    z &= M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def draw(seed, m, N, c):
    """the word chain c draws at the m-th launch since the move was set"""
    return mix64(seed + (m * N + c + 1) * GAMMA)


def seed_index(u, k):
    return ((u >> 32) * k) >> 32


def bonds_of(target):
    """the bond arrays of a lattice target per array axis, +-1 (every site owns the bond to its + neighbour along the axis); None: all +1"""
    if hasattr(target, "bonds_x"):
        return [np.asarray(target.bonds_z, dtype=np.int64), np.asarray(target.bonds_y, dtype=np.int64), np.asarray(target.bonds_x, dtype=np.int64)]
    if hasattr(target, "bonds_right"):
        return [np.asarray(target.bonds_down, dtype=np.int64), np.asarray(target.bonds_right, dtype=np.int64)]
    return None


def pair_sum(s, bonds):
    """S = sum over axes and sites of s_i J_i,axis s_(i + axis): at L = 2 the two bonds between the same pair of sites are two terms"""
    total = 0
    for axis in range(s.ndim):
        J = 1 if bonds is None else bonds[axis]
        total += int(np.sum(s * J * np.roll(s, -1, axis=axis)))
    return total


@functools.lru_cache(maxsize=None)
def neighbour_table(shape):
    """[d][2 ndim] flat indices of the nearest neighbours of every site, periodic (at L = 2 the + and - neighbour coincide): the
    coordinates by np.unravel_index, one step along one axis, back by np.ravel_multi_index"""
    idx = np.unravel_index(np.arange(int(np.prod(shape))), shape)
    cols = []
    for axis in range(len(shape)):
        for step in (-1, 1):
            nb = list(idx)
            nb[axis] = (nb[axis] + step) % shape[axis]
            cols.append(np.ravel_multi_index(nb, shape))
    return np.stack(cols, axis=1).tolist()


def neighbours(site, shape):
    return neighbour_table(tuple(shape))[site]


def component(t, shape, site):
    """the connected component of `site` among the true entries of the flat boolean array t: a stack flood fill"""
    assert t[site]
    inside = np.zeros(len(t), dtype=bool)
    inside[site] = True
    stack = [int(site)]
    while stack:
        s = stack.pop()
        for nb in neighbours(s, shape):
            if t[nb] and not inside[nb]:
                inside[nb] = True
                stack.append(nb)
    return inside


def move(a_bits, b_bits, shape, bonds, j=None, site=None):
    """one move on two 0 / 1 states, the seed site given by its rank j among the differing sites or directly
    -> None where the copies are equal, else (a', b', |C|, k, delta) with a', b' 0 / 1 arrays"""
    sa, sb = spins(a_bits, shape), spins(b_bits, shape)
    t = (sa != sb).ravel()
    k = int(np.sum(t))
    if k == 0:
        return None
    if site is None:
        site = int(np.flatnonzero(t)[j])
    inside = component(t, shape, site).reshape(shape)
    sa2, sb2 = np.where(inside, -sa, sa), np.where(inside, -sb, sb)
    delta = pair_sum(sa2, bonds) - pair_sum(sa, bonds)
    assert pair_sum(sb2, bonds) - pair_sum(sb, bonds) == -delta
    return ((sa2.ravel() + 1) // 2).astype(np.int64), ((sb2.ravel() + 1) // 2).astype(np.int64), int(np.sum(inside)), k, delta


class Accumulators:
    """what the device keeps per chain, all integers (passes_sum is the kernel's own and is not restated)"""
    NAMES = ("n", "empty", "size_sum", "k_sum", "abs_ds_sum")

    def __init__(self, N):
        for name in self.NAMES:
            setattr(self, name, np.zeros(N, dtype=np.int64))

    def assert_equal(self, rec):
        """rec: a pigeons_amd.ClusterRecord"""
        for name in self.NAMES:
            assert np.array_equal(getattr(rec, name), getattr(self, name)), (name, getattr(rec, name), getattr(self, name))


def launch(xa, chain_a, xb, chain_b, shape, bonds, betas, min_beta, seed, m, acc, S_a=None, S_b=None):
    """one launch of the move on both engines' states in place: x[slot] the 0 / 1 states, chain[slot] the chain of every slot; S_a / S_b
    [slot], where given, are updated by +-delta.  Chain c takes part iff betas[c] >= min_beta."""
    N = len(chain_a)
    slot_a = {int(c): s for s, c in enumerate(chain_a)}
    slot_b = {int(c): s for s, c in enumerate(chain_b)}
    for c in range(N):
        if not betas[c] >= min_beta:
            continue
        ia, ib = slot_a[c], slot_b[c]
        acc.n[c] += 1
        k = int(np.sum(xa[ia] != xb[ib]))
        if k == 0:
            acc.empty[c] += 1
            continue
        a2, b2, size, k2, delta = move(xa[ia], xb[ib], shape, bonds, j=seed_index(draw(seed, m, N, c), k))
        assert k2 == k
        xa[ia], xb[ib] = a2, b2
        acc.size_sum[c] += size
        acc.k_sum[c] += k
        acc.abs_ds_sum[c] += abs(delta)
        if S_a is not None:
            S_a[ia] += delta
        if S_b is not None:
            S_b[ib] -= delta
