"""NumPy / plain-Python restatement of the +-J spin-glass family.  TEST INFRASTRUCTURE ONLY.

Lattice L x L, periodic, spins s in {-1, +1} held as bits (1 = +1) in row-major order; two bond planes with entries +-1, JR[i][j] between
(i, j) and (i, j + 1), JD[i][j] between (i, j) and (i + 1, j).  Pair sum S = sum_ij s_ij (JR_ij s_i,j+1 + JD_ij s_i+1,j); at L = 2 the two
bonds between the same pair of sites are distinct terms.  Log potential of a chain at `beta`: the interpolation of 0.0 * S and beta_target * S
with ising_lp's arithmetic.  The explorer is the sequential raster sweep of IsingMetropolis; the draws come from tests/oracle.py's generator
(OracleRng over a (seed, gamma) stream), so the stream position after a sweep is comparable with the device's RNG words."""
import math

import numpy as np

import oracle as O


def pair_sum(bits, jr, jd):
    """S of one lattice: bits [L][L] or [L * L] of 0 / 1, jr / jd [L][L] of +-1"""
    jr, jd = np.asarray(jr, dtype=np.int64), np.asarray(jd, dtype=np.int64)
    L = jr.shape[0]
    s = 2 * np.asarray(bits, dtype=np.int64).reshape(L, L) - 1
    return int(np.sum(s * (jr * np.roll(s, -1, axis=1) + jd * np.roll(s, -1, axis=0))))


def ising_lp(beta, beta_target, S):
    """ising_lp of csrc/pte_ising.hpp, operation for operation (doubles, no contraction)"""
    S = float(S)
    ref, tgt = 0.0 * S, beta_target * S
    if beta == 0.0:
        return ref
    if beta == 1.0:
        return tgt
    return (1.0 - beta) * ref + beta * tgt


def site_delta(b, jr, jd, L, s):
    """change of S when site s flips: -2 s_s sum_n J_sn s_n (b, jr, jd: flat sequences)"""
    i, j = divmod(s, L)
    up, dn = ((i - 1) % L) * L + j, ((i + 1) % L) * L + j
    lf, rt = i * L + (j - 1) % L, i * L + (j + 1) % L
    nb = jd[up] * (2 * b[up] - 1) + jd[s] * (2 * b[dn] - 1) + jr[lf] * (2 * b[lf] - 1) + jr[s] * (2 * b[rt] - 1)
    return -2 * (2 * b[s] - 1) * nb


def flip_probability(b, s, jr, jd, L, beta, beta_target, delta_bonds=None):
    """probability that the single-site rule flips site s of lattice b (flat 0 / 1); delta_bonds = (jr, jd) replaces the bonds inside delta
    only (the detailed-balance test breaks the rule with it)"""
    djr, djd = delta_bonds if delta_bonds is not None else (jr, jd)
    delta = site_delta(b, djr, djd, L, s)
    if delta >= 0:
        return 1.0
    S = pair_sum(b, np.reshape(jr, (L, L)), np.reshape(jd, (L, L)))
    return min(1.0, math.exp(ising_lp(beta, beta_target, S + delta) - ising_lp(beta, beta_target, S)))


def sweep(bits, jr, jd, beta, beta_target, S, rng, n_steps, log=None):
    """IsingMetropolis(n_steps) on one replica, in place on the flat list `bits`: the draw order of k_explore_ising, statement for statement.
    rng: oracle.OracleRng (anything with rand()).  Returns the new S.  log: a list; every draw appends
    (k, step, site, delta, S_before, u, ratio, rejected), k = 1, 2, ... the draw's number since entry (tests/lattice_band.py)."""
    L = int(np.asarray(jr).shape[0])
    jrf = [int(v) for v in np.asarray(jr).ravel()]
    jdf = [int(v) for v in np.asarray(jd).ravel()]
    d = L * L
    k = 0
    for step in range(n_steps):
        for s in range(d):
            delta = site_delta(bits, jrf, jdf, L, s)
            if delta < 0:
                ratio = math.exp(ising_lp(beta, beta_target, S + delta) - ising_lp(beta, beta_target, S))
                if ratio < 1:
                    u = rng.rand()
                    k += 1
                    rejected = u > ratio
                    if log is not None:
                        log.append((k, step, s, delta, S, u, ratio, rejected))
                    if rejected:
                        continue
            bits[s] ^= 1
            S += delta
    return S


def refresh(bits, jr, jd, rng):
    """the reference chain: Bernoulli(1/2) per site in raster order with the Ising family's draws and bool-bit policy; returns S"""
    for s in range(len(bits)):
        bits[s] = int(rng.rand_bool())
    return pair_sum(bits, jr, jd)


def explore(x, chain, rngs, betas, jr, jd, beta_target, n_steps, S=None):
    """one explore step of every replica (slot): x [N][d] of 0 / 1, chain [N], rngs [N][2] (seed, gamma).
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


def all_states(L):
    """[2^(L^2)][L^2] of 0 / 1, state k = the bits of k"""
    d = L * L
    assert d <= 16
    return ((np.arange(1 << d, dtype=np.int64)[:, None] >> np.arange(d)[None, :]) & 1).astype(np.int64)


def all_pair_sums(jr, jd):
    jr, jd = np.asarray(jr, dtype=np.int64), np.asarray(jd, dtype=np.int64)
    L = jr.shape[0]
    s = (2 * all_states(L) - 1).reshape(-1, L, L)
    return np.sum(s * (jr[None] * np.roll(s, -1, axis=2) + jd[None] * np.roll(s, -1, axis=1)), axis=(1, 2))


def exact(beta, jr, jd):
    """log sum_s exp(beta S(s)) - L^2 log 2 by enumeration (L <= 4): what stepping_stone estimates against the uniform reference"""
    S = all_pair_sums(jr, jd).astype(np.float64)
    m = float(np.max(beta * S))
    L = np.asarray(jr).shape[0]
    return m + math.log(float(np.sum(np.exp(beta * S - m)))) - L * L * math.log(2.0)


def mattis(g):
    """the gauge transform of the ferromagnet by g [L][L] of +-1: J_ij = g_i g_j, no frustration"""
    g = np.asarray(g, dtype=np.int64)
    return (g * np.roll(g, -1, axis=1)).astype(np.int8), (g * np.roll(g, -1, axis=0)).astype(np.int8)


def gauge(jr, jd, g):
    """bonds g_i g_j J_ij"""
    mr, md = mattis(g)
    return (np.asarray(jr) * mr).astype(np.int8), (np.asarray(jd) * md).astype(np.int8)
