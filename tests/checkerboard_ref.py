"""Plain-Python restatement of CheckerboardMetropolis.  TEST INFRASTRUCTURE ONLY.

The lattice, the bonds, the pair sum S, ising_lp and the refresh of the reference chain are those of tests/spinglass_ref.py (the Ising target is
all bonds +1).  Only the sweep of a tempered chain is new: site (i, j) has colour (i + j) % 2; one step is two half-sweeps, colour 0 then colour
1; half-sweep h = 0 .. 2 n_steps - 1 has colour h % 2.  Every active site consumes exactly ONE uniform, in raster order over the active sites
(consecutive rand() calls of tests/oracle.py's generator), and flips iff delta >= 0 or not (u > r_|delta|), r4 = exp(ising_lp(beta, bt, -4.0)),
r8 = exp(ising_lp(beta, bt, -8.0)).  S += delta for every flip, in integers."""
import math

import numpy as np

import oracle as O
from spinglass_ref import pair_sum, ising_lp, site_delta, refresh, all_states, all_pair_sums, exact, gauge    # noqa: F401


def thresholds(beta, beta_target):
    """(r4, r8): once per explore step, independent of the current S"""
    return math.exp(ising_lp(beta, beta_target, -4.0)), math.exp(ising_lp(beta, beta_target, -8.0))


def active_sites(L, colour):
    """the sites of one colour in raster order (flat indices)"""
    return [i * L + j for i in range(L) for j in range(L) if (i + j) % 2 == colour]


def flip_probability(delta, r4, r8):
    """probability that the rule flips a site whose flip changes S by delta (u uniform on [0, 1))"""
    return 1.0 if delta >= 0 else min(1.0, r4 if delta == -4 else r8)


def half_sweep(bits, jrf, jdf, L, colour, r4, r8, S, rng):
    """one half-sweep in place on the flat list `bits` (jrf, jdf: flat bond lists): every site of `colour` decides from the lattice as it was
    at entry (no two of them are neighbours on an even periodic lattice, so deciding them in turn is deciding them at once).  Returns S."""
    assert L % 2 == 0
    for s in active_sites(L, colour):
        delta = site_delta(bits, jrf, jdf, L, s)
        u = rng.rand()                               # always one draw
        if delta >= 0 or not (u > (r4 if delta == -4 else r8)):
            bits[s] ^= 1
            S += delta
    return S


def sweep(bits, jr, jd, beta, beta_target, S, rng, n_steps):
    """CheckerboardMetropolis(n_steps) on one replica, in place on the flat list `bits`.  rng: oracle.OracleRng.  Returns the new S."""
    L = int(np.asarray(jr).shape[0])
    jrf = [int(v) for v in np.asarray(jr).ravel()]
    jdf = [int(v) for v in np.asarray(jd).ravel()]
    r4, r8 = thresholds(beta, beta_target)
    for h in range(2 * n_steps):
        S = half_sweep(bits, jrf, jdf, L, h % 2, r4, r8, S, rng)
    return S


def explore(x, chain, rngs, betas, jr, jd, beta_target, n_steps, S=None):
    """one explore step of every replica (slot), the signature of spinglass_ref.explore: x [N][d] of 0 / 1, chain [N], rngs [N][2] (seed, gamma).
    -> (x', rngs', S' [N]); chain 0 is refreshed, the others sweep at betas[chain]"""
    x = np.array(x, dtype=np.int64)
    rngs = np.array(rngs, dtype=np.uint64)
    N = x.shape[0]
    out_S = np.zeros(N, dtype=np.int64)
    for r in range(N):
        g = O.OracleRng(state=(int(rngs[r, 0]), int(rngs[r, 1])))
        b = [int(v) for v in x[r]]
        if chain[r] == 0:
            out_S[r] = refresh(b, jr, jd, g)
        else:
            S0 = pair_sum(b, jr, jd) if S is None else int(S[r])
            out_S[r] = sweep(b, jr, jd, float(betas[chain[r]]), beta_target, S0, g, n_steps)
        x[r] = b
        rngs[r] = g.state
    return x, rngs, out_S


# ---- the draw of one site from the stream's definition (SplittableRandom: output k of a stream is mix64(seed + k gamma)) -------------------
M64 = (1 << 64) - 1


def mix64(z):
    z &= M64
    z = ((z ^ (z >> 30)) * 0xbf58476d1ce4e5b9) & M64
    z = ((z ^ (z >> 27)) * 0x94d049bb133111eb) & M64
    return z ^ (z >> 31)


def draw_number(L, h, i, j):
    """which draw of the stream at kernel entry site (i, j) owns in half-sweep h"""
    return h * (L * L // 2) + i * (L // 2) + (j >> 1) + 1


def uniform_of_draw(seed, gamma, n):
    """u52_to_unit(mix64(seed + n gamma)): the low 52 bits as a fraction (exact in doubles)"""
    return float(mix64(seed + n * gamma) & ((1 << 52) - 1)) * 2.0 ** -52
