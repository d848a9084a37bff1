"""NumPy / plain-Python restatement of the 3-D +-J spin-glass family under CheckerboardMetropolis.  TEST INFRASTRUCTURE ONLY.

Lattice L x L x L, periodic, L even; site (z, y, x) has index s = (z L + y) L + x and colour (x + y + z) % 2; spins are bits (1 = +1) in that
order.  Three bond planes [L][L][L] with entries +-1: JX[z][y][x] couples (z, y, x) with (z, y, x + 1), JY with (z, y + 1, x), JZ with
(z + 1, y, x).  S = sum s_zyx (JX s_x+1 + JY s_y+1 + JZ s_z+1); at L = 2 the two bonds between the same pair of sites are distinct terms.
ising_lp, the stream (mix64, draw numbers as consecutive rand() calls of tests/oracle.py's generator) and the shape of the rule are those of
tests/spinglass_ref.py and tests/checkerboard_ref.py, imported here; what is restated is the geometry: six neighbours, three thresholds."""
import math

import numpy as np

import oracle as O
from spinglass_ref import ising_lp                                                  # noqa: F401
from checkerboard_ref import mix64, uniform_of_draw, M64                            # noqa: F401


def pair_sum(bits, jx, jy, jz):
    """S of one lattice: bits [L][L][L] or [L^3] of 0 / 1, jx / jy / jz [L][L][L] of +-1"""
    jx, jy, jz = (np.asarray(j, dtype=np.int64) for j in (jx, jy, jz))
    L = jx.shape[0]
    s = 2 * np.asarray(bits, dtype=np.int64).reshape(L, L, L) - 1
    return int(np.sum(s * (jx * np.roll(s, -1, axis=2) + jy * np.roll(s, -1, axis=1) + jz * np.roll(s, -1, axis=0))))


def neighbour_table(L):
    """[d][6] flat indices of the -x, +x, -y, +y, -z, +z neighbours and [d][6] the flat index of the SITE whose bond couples them (the - directions
    go through the neighbour's bond), with [6] the plane (0 JX, 1 JY, 2 JZ) of each direction"""
    z, y, x = np.meshgrid(np.arange(L), np.arange(L), np.arange(L), indexing="ij")
    f = lambda zz, yy, xx: (((zz % L) * L + (yy % L)) * L + (xx % L)).ravel()
    s = f(z, y, x)
    nb = np.stack([f(z, y, x - 1), f(z, y, x + 1), f(z, y - 1, x), f(z, y + 1, x), f(z - 1, y, x), f(z + 1, y, x)], axis=1)
    bond_site = np.stack([nb[:, 0], s, nb[:, 2], s, nb[:, 4], s], axis=1)
    return nb, bond_site, np.array([0, 0, 1, 1, 2, 2])


class Lattice:
    """the bonds of one instance as flat arrays, with the neighbour table: what site_delta and the sweeps read"""

    def __init__(self, jx, jy, jz):
        self.L = int(np.asarray(jx).shape[0])
        assert self.L % 2 == 0 and np.asarray(jx).shape == np.asarray(jy).shape == np.asarray(jz).shape == (self.L,) * 3
        self.d = self.L ** 3
        self.nb, bond_site, plane = neighbour_table(self.L)
        J = np.stack([np.asarray(j, dtype=np.int64).ravel() for j in (jx, jy, jz)])
        self.Jn = J[plane[None, :], bond_site]                                     # [d][6]: the bond to each neighbour
        z, y, x = np.unravel_index(np.arange(self.d), (self.L,) * 3)
        self.colour = (x + y + z) % 2
        self.active = [np.flatnonzero(self.colour == c) for c in (0, 1)]            # raster order

    def deltas(self, bits, sites):
        """change of S when each of `sites` flips alone: -2 s sum_n J_sn s_n over the six neighbours"""
        s = 2 * np.asarray(bits, dtype=np.int64) - 1
        return -2 * s[sites] * np.sum(self.Jn[sites] * s[self.nb[sites]], axis=1)


def thresholds(beta, beta_target):
    """{4: r4, 8: r8, 12: r12}: once per explore step, independent of the current S"""
    return {k: math.exp(ising_lp(beta, beta_target, -float(k))) for k in (4, 8, 12)}


def flip_probability(delta, r):
    return 1.0 if delta >= 0 else min(1.0, r[-int(delta)])


def draw_number(L, h, z, y, x):
    """which draw of the stream at kernel entry site (z, y, x) owns in half-sweep h"""
    return h * (L ** 3 // 2) + (z * L + y) * (L // 2) + (x >> 1) + 1


def half_sweep(lat, bits, colour, r, S, rng):
    """one half-sweep in place on the int array `bits`: every site of `colour` decides from the lattice at entry (no two of them are
    neighbours on an even periodic lattice) and takes ONE rand() whatever its delta, in raster order.  Returns S."""
    sites = lat.active[colour]
    delta = lat.deltas(bits, sites)
    for s, dl in zip(sites, delta):
        u = rng.rand()                               # always one draw
        if dl >= 0 or not (u > r[-int(dl)]):
            bits[s] ^= 1
            S += int(dl)
    return S


def sweep(lat, bits, beta, beta_target, S, rng, n_steps):
    """CheckerboardMetropolis(n_steps) on one replica, in place.  rng: oracle.OracleRng.  Returns the new S."""
    r = thresholds(beta, beta_target)
    for h in range(2 * n_steps):
        S = half_sweep(lat, bits, h % 2, r, S, rng)
    return S


def refresh(lat, bits, jx, jy, jz, rng):
    """the reference chain: Bernoulli(1/2) per site in index order with the Ising family's draws and bool-bit policy; returns S"""
    for s in range(lat.d):
        bits[s] = int(rng.rand_bool())
    return pair_sum(bits, jx, jy, jz)


def explore(x, chain, rngs, betas, jx, jy, jz, beta_target, n_steps, S=None):
    """one explore step of every replica (slot): x [N][d] of 0 / 1, chain [N], rngs [N][2] (seed, gamma).
    -> (x', rngs', S' [N]); chain 0 is refreshed, the others sweep at betas[chain]"""
    lat = Lattice(jx, jy, jz)
    x = np.array(x, dtype=np.int64)
    rngs = np.array(rngs, dtype=np.uint64)
    N = x.shape[0]
    out_S = np.zeros(N, dtype=np.int64)
    for k in range(N):
        g = O.OracleRng(state=(int(rngs[k, 0]), int(rngs[k, 1])))
        b = x[k].copy()
        if chain[k] == 0:
            out_S[k] = refresh(lat, b, jx, jy, jz, g)
        else:
            S0 = pair_sum(b, jx, jy, jz) if S is None else int(S[k])
            out_S[k] = sweep(lat, b, float(betas[chain[k]]), beta_target, S0, g, n_steps)
        x[k] = b
        rngs[k] = g.state
    return x, rngs, out_S


def all_states():
    """the 256 states of the L = 2 lattice, state k = the bits of k"""
    return ((np.arange(256, dtype=np.int64)[:, None] >> np.arange(8)[None, :]) & 1).astype(np.int64)


def all_pair_sums(jx, jy, jz):
    return np.array([pair_sum(b, jx, jy, jz) for b in all_states()], dtype=np.int64)


def exact(beta, jx, jy, jz):
    """log sum_s exp(beta S(s)) - 8 log 2 by enumeration (L = 2): what stepping_stone estimates against the uniform reference"""
    S = all_pair_sums(jx, jy, jz).astype(np.float64)
    m = float(np.max(beta * S))
    return m + math.log(float(np.sum(np.exp(beta * S - m)))) - 8 * math.log(2.0)


def gauge(jx, jy, jz, g):
    """bonds g_i g_j J_ij for g [L][L][L] of +-1"""
    g = np.asarray(g, dtype=np.int64)
    return tuple((np.asarray(j) * g * np.roll(g, -1, axis=ax)).astype(np.int8) for j, ax in ((jx, 2), (jy, 1), (jz, 0)))


def edwards_anderson(L, seed):
    """SpinGlass3DLogPotential.edwards_anderson's draws: x, y, z from one generator"""
    g = np.random.default_rng(seed)
    return tuple((2 * g.integers(0, 2, size=(L, L, L)) - 1).astype(np.int8) for _ in range(3))


def bit_sliced_count(x):
    """the count of DESIGN 4.19 on six words x[0..5] (arrays of uint32): two full adders, then a 2-bit add -> the masks
    (none, one, two, three_or_more)"""
    x1, x2, x3, x4, x5, x6 = (np.asarray(v, dtype=np.uint32) for v in x)
    s1, c1 = x1 ^ x2 ^ x3, (x1 & x2) | (x3 & (x1 ^ x2))
    s2, c2 = x4 ^ x5 ^ x6, (x4 & x5) | (x6 & (x4 ^ x5))
    b0, k0 = s1 ^ s2, s1 & s2
    b1, b2 = c1 ^ c2 ^ k0, (c1 & c2) | (k0 & (c1 ^ c2))
    return ~(b0 | b1 | b2), b0 & ~(b1 | b2), b1 & ~(b0 | b2), b2 | (b1 & b0)
