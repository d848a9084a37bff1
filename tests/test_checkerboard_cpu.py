"""CheckerboardMetropolis without a GPU: the restatement (tests/checkerboard_ref.py) leaves the enumerated target invariant one
colour at a time -- and would not if all sites were decided at once --, its single-site rule is in detailed balance, its draws sit where the
specification numbers them, it is gauge covariant; the enum, the export and the translation unit are mirrored where they must be, and
pte_create refuses -- before any device work -- what the explorer does not run, and accepts what it does."""
import math
import os

import numpy as np
import pytest

import family_cpu as F
import oracle as O
import checkerboard_ref as R
from family_cpu import P  # noqa: F401  (P: the module's fixture)


def _ea(L, seed):              # SpinGlassLogPotential.edwards_anderson's draws
    g = np.random.default_rng(seed)
    return (2 * g.integers(0, 2, size=(L, L)) - 1).astype(np.int8), (2 * g.integers(0, 2, size=(L, L)) - 1).astype(np.int8)


def _transition(L, jr, jd, sites, r4, r8):
    """the 2^d x 2^d matrix of 'every site of `sites` decides from the lattice at entry, independently': row = from, column = to"""
    jrf, jdf = [int(v) for v in np.ravel(jr)], [int(v) for v in np.ravel(jd)]
    states = R.all_states(L)
    n = len(states)
    T = np.zeros((n, n))
    for k in range(n):
        b = [int(v) for v in states[k]]
        p = [R.flip_probability(R.site_delta(b, jrf, jdf, L, s), r4, r8) for s in sites]
        for m in range(1 << len(sites)):
            k2, w = k, 1.0
            for q, s in enumerate(sites):
                if (m >> q) & 1:
                    k2 ^= 1 << s; w *= p[q]
                else:
                    w *= 1.0 - p[q]
            T[k, k2] += w
    return T


def test_each_half_sweep_leaves_the_target_invariant_and_an_all_sites_update_does_not():
    """L = 2 (16 states), a frustrated instance (max S = 6 < 8), beta = 0.7, beta_target = 0.9: pi P = pi to 1e-12 for the colour-0 and the
    colour-1 half-sweep (sums of 16 products of probabilities: rounding is ~1e-16); deciding all four sites at once is NOT a kernel for pi
    (residual 0.066), which is what the colours are for"""
    L, beta, bt = 2, 0.7, 0.9
    jr, jd = np.ones((2, 2), dtype=np.int8), np.array([[1, 1], [1, -1]], dtype=np.int8)
    S = R.all_pair_sums(jr, jd).astype(np.float64)
    assert S.max() == 6
    w = np.exp(np.array([R.ising_lp(beta, bt, s) for s in S]))
    pi = w / w.sum()
    r4, r8 = R.thresholds(beta, bt)
    res = []
    for sites in (R.active_sites(L, 0), R.active_sites(L, 1), list(range(L * L))):
        T = _transition(L, jr, jd, sites, r4, r8)
        assert np.allclose(T.sum(axis=1), 1.0, rtol=0, atol=1e-14)
        res.append(float(np.max(np.abs(pi @ T - pi))))
    print("residuals: colour 0 %.3g, colour 1 %.3g, all sites at once %.3g" % tuple(res))
    assert R.active_sites(L, 0) == [0, 3] and R.active_sites(L, 1) == [1, 2]
    assert res[0] < 1e-12 and res[1] < 1e-12
    assert res[2] > 1e-3


@pytest.mark.parametrize("beta", [0.3, 1.0])
def test_single_site_rule_is_in_detailed_balance(beta):
    """every site of every one of the 65536 states of edwards_anderson(1.0, 4, seed=2): pi(x) P(x -> x^s) = pi(x^s) P(x^s -> x) in logs, to
    rounding (each side is one product and one log of an exponential: 1e-12 relative to the largest log weight)"""
    L = 4
    jr, jd = _ea(L, 2)
    S = R.all_pair_sums(jr, jd)
    r4, r8 = R.thresholds(1.0, beta)
    logpi = beta * S.astype(np.float64)
    k = np.arange(1 << (L * L))
    logp = lambda delta: np.where(delta >= 0, 0.0, np.where(delta == -4, math.log(r4), math.log(r8)))
    jrf, jdf = [int(v) for v in jr.ravel()], [int(v) for v in jd.ravel()]
    states = R.all_states(L)
    g = np.random.default_rng(7)
    worst = 0.0
    for s in range(L * L):
        k2 = k ^ (1 << s)
        delta = S[k2] - S[k]
        assert set(np.unique(delta)) <= {-8, -4, 0, 4, 8}
        for kk in g.integers(0, len(k), 40):       # the rule's delta is the change of S (site_delta is what the sweep uses)
            assert R.site_delta([int(v) for v in states[kk]], jrf, jdf, L, s) == delta[kk]
        worst = max(worst, float(np.max(np.abs(logpi[k] + logp(delta) - logpi[k2] - logp(-delta)))))
    assert worst < 1e-12 * (1 + np.abs(logpi).max())


@pytest.mark.parametrize("L,n_steps", [(2, 3), (4, 1), (6, 2)])
def test_stream_position_and_draw_numbers(L, n_steps):
    """after sweep() the stream is n_steps d draws on; the uniform of site (i, j) in half-sweep h is draw h d / 2 + i L / 2 + (j >> 1) + 1 of the
    stream at entry: every decision of every half-sweep restated from mix64"""
    d = L * L
    jr, jd = _ea(L, 30 + L)
    jrf, jdf = [int(v) for v in jr.ravel()], [int(v) for v in jd.ravel()]
    g = np.random.default_rng(L)
    bits = [int(v) for v in g.integers(0, 2, d)]
    beta, bt = 0.45, 0.8
    rng = O.OracleRng(seed=123)
    seed, gamma = rng.state
    r4, r8 = R.thresholds(beta, bt)
    b = list(bits)
    S = R.pair_sum(b, jr, jd)
    n_rej = 0
    for h in range(2 * n_steps):
        want = list(b)
        for s in R.active_sites(L, h % 2):
            i, j = divmod(s, L)
            delta = R.site_delta(b, jrf, jdf, L, s)
            u = R.uniform_of_draw(seed, gamma, R.draw_number(L, h, i, j))
            if delta >= 0 or not (u > (r4 if delta == -4 else r8)):
                want[s] ^= 1
            else:
                n_rej += 1
        S = R.half_sweep(b, jrf, jdf, L, h % 2, r4, r8, S, rng)
        assert b == want, "half-sweep %d" % h
        assert S == R.pair_sum(b, jr, jd)
    assert n_rej > 0 and b != bits
    assert rng.state == ((seed + n_steps * d * gamma) & R.M64, gamma)
    rng2 = O.OracleRng(seed=123)
    b2 = list(bits)
    assert R.sweep(b2, jr, jd, beta, bt, R.pair_sum(bits, jr, jd), rng2, n_steps) == S and b2 == b and rng2.state == rng.state
    # the draws are consecutive rand() calls
    rng3 = O.OracleRng(seed=123)
    assert [rng3.rand() for _ in range(5)] == [R.uniform_of_draw(seed, gamma, n) for n in range(1, 6)]


@pytest.mark.parametrize("L,seed", [(2, 1), (4, 2), (6, 3)])
def test_gauge_covariance_of_the_restatement(L, seed):
    """bonds g_i g_j J_ij started from g . s give g . (trajectory) with the same stream position"""
    g = np.random.default_rng(seed)
    jr, jd = _ea(L, seed)
    gg = 2 * g.integers(0, 2, size=(L, L)) - 1
    jr2, jd2 = R.gauge(jr, jd, gg)
    gbits = ((gg.ravel() + 1) // 2).astype(np.int64)
    b1 = [int(v) for v in g.integers(0, 2, size=L * L)]
    b2 = [int(v) ^ int(1 - m) for v, m in zip(b1, gbits)]
    S1, S2 = R.pair_sum(b1, jr, jd), R.pair_sum(b2, jr2, jd2)
    assert S1 == S2
    r1, r2 = O.OracleRng(seed=77), O.OracleRng(seed=77)
    for _ in range(2):
        S1 = R.sweep(b1, jr, jd, 0.6, 0.9, S1, r1, 2)
        S2 = R.sweep(b2, jr2, jd2, 0.6, 0.9, S2, r2, 2)
        assert S1 == S2 and r1.state == r2.state
        assert b2 == [v ^ int(1 - m) for v, m in zip(b1, gbits)]
    assert r1.state != O.OracleRng(seed=77).state


def test_enum_export_and_unit_mirrors(P):
    from pigeons_amd import _lib
    import __graft_entry__ as g
    assert _lib.EXPLORER_CHECKERBOARD_METROPOLIS == 7
    hdr = F.HEADER
    assert "PTE_EXPLORER_CHECKERBOARD_METROPOLIS = 7" in hdr and "#define PTE_ABI_VERSION 2\n" in hdr
    jl = F.JULIA
    assert "const EXPLORER_CHECKERBOARD_METROPOLIS = Int32(7)" in jl
    assert "CheckerboardMetropolis" in P.__dict__ and P.CheckerboardMetropolis().n_steps == 3 and P.CheckerboardMetropolis(5).n_steps == 5
    assert isinstance(P.pt.default_explorer(P.IsingLogPotential(1.0, 4)), P.IsingMetropolis)         # unchanged
    # a translation unit of its own, in a list of its own, with pte_spinglass.hip's flags; the frozen lists did not grow
    assert g.CHECKERBOARD_UNITS == [("pte_checkerboard.hip", dict(g.LATTICE_UNITS)["pte_spinglass.hip"])]
    assert len(g.UNITS) == 8 and [u for u, _ in g.LATTICE_UNITS] == ["pte_spinglass.hip"]
    assert "X(checkerboard)" in open(os.path.join(g.CSRC, "pte_automala_params.hpp")).read()
    assert "PTE_DEFINE_RNG_POLICY_SETTER(checkerboard)" in open(os.path.join(g.CSRC, "pte_checkerboard.hpp")).read()
    assert os.path.exists(os.path.join(g.CSRC, "pte_checkerboard.hip")) and os.path.exists(os.path.join(g.CSRC, "pte_checkerboard_params.hpp"))


@pytest.mark.parametrize("target", [3, 12])
@pytest.mark.parametrize("dim", [4, 36, 1024, 65536])
def test_accepted_config_reaches_the_device_check(P, target, dim):
    """fails on the code before the explorer existed ("explored by IsingMetropolis only"): a valid configuration now passes validation"""
    F.no_device()
    for dk in (0, 102):
        F.assert_reaches_the_device_check(P, n_chains=4, target=target, dim=dim, explorer=7, target_params=[1.0], debug_kernel=dk)


@pytest.mark.parametrize("target", [3, 12])
@pytest.mark.parametrize("kw,msg", [
    (dict(dim=9), r"CheckerboardMetropolis needs an even base_length \(got 3\): on an odd periodic lattice two sites of one colour would be neighbours"),
    (dict(dim=25), r"CheckerboardMetropolis needs an even base_length \(got 5\): on an odd periodic lattice two sites of one colour would be neighbours"),
    (dict(explorer2=3), r"CheckerboardMetropolis is not available as half of a Compose on the device \(got explorers 7, 3\)"),
    (dict(explorer2=4), r"CheckerboardMetropolis is not available as half of a Compose on the device \(got explorers 7, 4\)"),
    (dict(explorer2=7), r"CheckerboardMetropolis is not available as half of a Compose on the device \(got explorers 7, 7\)"),
    (dict(debug_kernel=1), "debug_kernel 1 is not available for this explorer"),
    (dict(debug_kernel=101), "debug_kernel 101 is not available for this explorer"),
])
def test_pte_create_refusals(P, target, kw, msg):
    args = dict(n_chains=4, target=target, dim=16, explorer=7, target_params=[1.0])
    args.update(kw)
    with pytest.raises(P.PteError, match=msg):
        P.Engine(**args)
    if kw.get("debug_kernel") == 101:                # the scalar bit-packed generation is IsingMetropolis's, in the test build too
        with pytest.raises(P.PteError, match=msg):
            P.Engine(test_build=True, **args)


def test_the_explorer_elsewhere_is_refused_and_the_old_refusals_keep_their_text(P):
    for target in (0, 2, 11):
        with pytest.raises(P.PteError, match="^pte_create: CheckerboardMetropolis needs the Ising or the spin-glass target$"):
            P.Engine(n_chains=4, target=target, dim=16, explorer=7, target_params=[1.0, 10.0])
    for target, name in ((3, "Ising"), (12, "spin-glass")):
        for ex in (0, 1, 3):
            with pytest.raises(P.PteError, match="the %s path is explored by IsingMetropolis only" % name):
                P.Engine(n_chains=4, target=target, dim=16, explorer=ex, target_params=[1.0])


def test_python_refuses_an_odd_lattice_and_keeps_the_spin_glass_guard(P):
    for t in (P.IsingLogPotential(1.0, 5), P.SpinGlassLogPotential.edwards_anderson(1.0, 3, seed=1)):
        with pytest.raises(ValueError, match=r"CheckerboardMetropolis needs an even base_length \(got %d\): on an odd periodic lattice two sites of one "
                                             r"colour would be neighbours" % t.base_length):
            P.PT(P.Inputs(target=t, n_chains=4, n_rounds=2, explorer=P.CheckerboardMetropolis(), show_report=False))
    with pytest.raises(NotImplementedError, match="spin-glass path is explored by IsingMetropolis only"):
        P.PT(P.Inputs(target=P.SpinGlassLogPotential.edwards_anderson(1.0, 4, seed=1), n_chains=4, n_rounds=2, explorer=P.SliceSampler(), show_report=False))
