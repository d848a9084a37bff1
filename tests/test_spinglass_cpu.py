"""The +-J spin-glass family without a GPU: the NumPy restatement (tests/spinglass_ref.py) equals the oracle's Ising explore step when every
bond is +1, its single-site rule is in detailed balance with the enumerated target (and stops being so when a bond's sign is ignored), it is
gauge covariant; the Python surface validates its arguments and pte_create refuses -- before any device work -- what the device does not run."""
import math
import os

import numpy as np
import pytest

import family_cpu as F
import oracle as O
import spinglass_ref as R
from family_cpu import P  # noqa: F401  (P: the module's fixture)


def _ea(L, seed):
    g = np.random.default_rng(seed)
    return (2 * g.integers(0, 2, size=(L, L)) - 1).astype(np.int8), (2 * g.integers(0, 2, size=(L, L)) - 1).astype(np.int8)


@pytest.mark.parametrize("L", [3, 5, 8])
def test_all_ferro_restatement_equals_the_oracle_explore_step(L):
    N, beta_t, n_steps = 5, 0.7, 3
    d = L * L
    g = np.random.default_rng(10 + L)
    ref = O.OracleShard(target=O.TARGET_ISING, explorer=O.EXPLORER_ISING, dim=d, p0=beta_t, n_chains=N, seed=3, slice_n_passes=n_steps)
    betas = np.concatenate([[0.0], np.sort(g.uniform(0.0, 1.0, N - 2)), [1.0]])
    ref.set_schedule(betas)
    x = g.integers(0, 2, size=(N, d)).astype(np.float64)
    chain = g.permutation(N).astype(np.int64)
    _, _, rng = ref.states()
    ref.set_states(x, chain, rng)
    ones = np.ones((L, L), dtype=np.int8)
    ref.explore(1)
    xo, co, ro = ref.states()
    xr, rr, Sr = R.explore(x, chain, rng, betas, ones, ones, beta_t, n_steps)
    assert np.array_equal(co, chain)
    assert np.array_equal(xo, xr)                    # spins
    assert np.array_equal(ro, rr)                    # stream position
    for r in range(N):                               # pair sum: the one carried through the sweep is the lattice's
        s = 2 * xo[r].reshape(L, L) - 1
        ferro = int(np.sum(s * (np.roll(s, -1, 0) + np.roll(s, -1, 1))))
        assert Sr[r] == ferro == R.pair_sum(xo[r], ones, ones)
    assert not np.array_equal(xo, x) and not np.array_equal(ro, rng)


def _frustrated_3():
    jr, jd = _ea(3, 4)
    S = R.all_pair_sums(jr, jd)
    assert S.max() < 18                              # frustrated: no state satisfies all 18 bonds
    return jr, jd, S


@pytest.mark.parametrize("beta", [0.3, 1.0])
def test_single_site_rule_is_in_detailed_balance_and_a_dropped_bond_sign_breaks_it(beta):
    """exact probabilities, every site and state: pi(x) P(x -> x^s) = pi(x^s) P(x^s -> x) to rounding (both sides are products of at most two
    exponentials: 1e-12 relative)"""
    L = 3
    jr, jd, S = _frustrated_3()
    logpi = beta * S.astype(np.float64)
    states = R.all_states(L)
    jrf, jdf = [int(v) for v in jr.ravel()], [int(v) for v in jd.ravel()]
    wrong_r = np.array(jr); wrong_r[1, 1] = -wrong_r[1, 1]          # one bond's sign ignored in delta
    wrong = ([int(v) for v in wrong_r.ravel()], jdf)

    def worst(delta_bonds):
        w = 0.0
        for k in range(len(states)):
            b = [int(v) for v in states[k]]
            for s in range(L * L):
                k2 = k ^ (1 << s)
                b2 = list(b); b2[s] ^= 1
                lhs = logpi[k] + math.log(R.flip_probability(b, s, jrf, jdf, L, 1.0, beta, delta_bonds))
                rhs = logpi[k2] + math.log(R.flip_probability(b2, s, jrf, jdf, L, 1.0, beta, delta_bonds))
                w = max(w, abs(lhs - rhs))
        return w
    assert worst(None) < 1e-12 * (1 + np.abs(logpi).max())
    assert worst(wrong) > 1.0                        # a flipped sign moves delta by 4: the two sides differ by ~4 beta


@pytest.mark.parametrize("L,seed", [(3, 1), (4, 2), (6, 3)])
def test_gauge_covariance_of_the_restatement(L, seed):
    """bonds g_i g_j J_ij started from g . s give g . (trajectory) with the same stream position"""
    g = np.random.default_rng(seed)
    jr, jd = _ea(L, seed)
    gg = 2 * g.integers(0, 2, size=(L, L)) - 1
    jr2, jd2 = R.gauge(jr, jd, gg)
    gbits = ((gg.ravel() + 1) // 2).astype(np.int64)                 # s -> g s on bits: XOR with NOT g
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


def test_exact_enumeration_of_the_ferromagnet():
    """L = 2, all bonds +1: 8 bonds (doubled), S = 8 for the two aligned states, -8 for the two staggered ones, 0 otherwise"""
    ones = np.ones((2, 2), dtype=np.int8)
    S = R.all_pair_sums(ones, ones)
    assert sorted(S.tolist()) == [-8, -8] + [0] * 12 + [8, 8]
    assert abs(R.exact(1.0, ones, ones) - math.log((2 * math.exp(8) + 2 * math.exp(-8) + 12) / 16)) < 1e-12


def test_enum_and_export_mirrors(P):
    from pigeons_amd import _lib
    import __graft_entry__ as g
    assert _lib.TARGET_SPIN_GLASS == 12
    assert "pte_set_target_spin_glass" in _lib.EXPORTS and hasattr(_lib.load(), "pte_set_target_spin_glass")
    hdr = F.HEADER
    assert "PTE_TARGET_SPIN_GLASS = 12" in hdr and "#define PTE_ABI_VERSION 2\n" in hdr
    assert "int pte_set_target_spin_glass(pte_engine *h, int64_t base_length, const int8_t *bonds_right" in hdr
    jl = F.JULIA
    assert "const TARGET_SPIN_GLASS = Int32(12)\n" in jl and ":pte_set_target_spin_glass" in jl
    assert "SpinGlassLogPotential" in P.__dict__
    # a translation unit of its own, with the flags of the Ising kernels' unit
    flags = dict(g.UNITS)["pte.hip"]
    assert g.LATTICE_UNITS == [("pte_spinglass.hip", [f for f in flags if f != "-DPTE_SPLIT_LANGEVIN"])]
    assert "X(spinglass)" in open(os.path.join(g.CSRC, "pte_automala_params.hpp")).read()


def test_python_validation_messages(P):
    ones = np.ones((4, 4), dtype=np.int8)
    t = P.SpinGlassLogPotential(0.8, ones, -ones)
    assert (t.base_length, t.dim, t.beta) == (4, 16, 0.8) and t.bonds_down.dtype == np.int8
    assert isinstance(P.pt.default_explorer(t), P.IsingMetropolis)
    with pytest.raises(ValueError, match=r"bonds_right must be L x L with L >= 2 \(got shape \(4, 3\)\)"):
        P.SpinGlassLogPotential(1.0, ones[:, :3], ones)
    with pytest.raises(ValueError, match=r"bonds_down must be L x L with L >= 2 \(got shape \(16,\)\)"):
        P.SpinGlassLogPotential(1.0, ones, ones.ravel())
    with pytest.raises(ValueError, match=r"bonds_right must be L x L with L >= 2 \(got shape \(1, 1\)\)"):
        P.SpinGlassLogPotential(1.0, ones[:1, :1], ones[:1, :1])
    with pytest.raises(ValueError, match=r"must have the same shape \(got \(4, 4\) and \(3, 3\)\)"):
        P.SpinGlassLogPotential(1.0, ones, ones[:3, :3])
    with pytest.raises(ValueError, match=r"at most 65536 sites"):
        P.SpinGlassLogPotential(1.0, np.ones((257, 257), dtype=np.int8), np.ones((257, 257), dtype=np.int8))
    bad = np.array(ones, dtype=np.float64); bad[2, 1] = 0.5; bad[3, 3] = 0.0
    with pytest.raises(ValueError, match=r"bonds_right\[2\]\[1\] must be \+1 or -1 \(got 0\.5\): ±J is the supported disorder"):
        P.SpinGlassLogPotential(1.0, bad, ones)
    dil = np.array(ones); dil[0, 3] = 0
    with pytest.raises(ValueError, match=r"bonds_down\[0\]\[3\] must be \+1 or -1 \(got 0\).*diluted"):
        P.SpinGlassLogPotential(1.0, ones, dil)
    a, b = P.SpinGlassLogPotential.edwards_anderson(1.0, 6, seed=5), P.SpinGlassLogPotential.edwards_anderson(1.0, 6, seed=5)
    c = P.SpinGlassLogPotential.edwards_anderson(1.0, 6, seed=6)
    assert np.array_equal(a.bonds_right, b.bonds_right) and np.array_equal(a.bonds_down, b.bonds_down)
    assert not np.array_equal(a.bonds_right, c.bonds_right) and set(np.unique(a.bonds_right)) == {-1, 1}
    g = np.random.default_rng(5)
    assert np.array_equal(a.bonds_right, 2 * g.integers(0, 2, size=(6, 6)) - 1) and np.array_equal(a.bonds_down, 2 * g.integers(0, 2, size=(6, 6)) - 1)
    with pytest.raises(NotImplementedError, match="spin-glass path is explored by IsingMetropolis only"):
        P.PT(P.Inputs(target=a, n_chains=4, n_rounds=2, explorer=P.SliceSampler(), show_report=False))


@pytest.mark.parametrize("dim", [4, 9, 1024, 65536])
def test_accepted_config_reaches_the_device_check(P, dim):
    """fails on the code before the family existed ("target 12 has no device log-potential"): a valid configuration now passes validation"""
    F.no_device()
    for dk in (0, 102):
        F.assert_reaches_the_device_check(P, n_chains=4, target=12, dim=dim, explorer=4, target_params=[1.0], debug_kernel=dk)


@pytest.mark.parametrize("kw,msg", [
    (dict(dim=1), r"spin-glass path needs dim = base_length\^2 with 2 <= base_length and dim <= 65536 \(got 1\)"),
    (dict(dim=10), r"spin-glass path needs dim = base_length\^2"),
    (dict(dim=257 * 257), r"spin-glass path needs dim = base_length\^2 with 2 <= base_length and dim <= 65536 \(got 66049\)"),
    (dict(explorer=2), r"SliceSampler's Bool / Integer coordinate methods are not available on the device .*the spin-glass path is explored by IsingMetropolis only"),
    (dict(explorer=4, explorer2=2), r"SliceSampler's Bool / Integer coordinate methods"),
    (dict(explorer=0), "the spin-glass path is explored by IsingMetropolis only"),
    (dict(explorer=1), "the spin-glass path is explored by IsingMetropolis only"),
    (dict(explorer=3), "the spin-glass path is explored by IsingMetropolis only"),
    (dict(explorer=4, explorer2=3), "the spin-glass path is explored by IsingMetropolis only"),
    (dict(explorer=6), r"AAPS is implemented on the scaled-precision MVN and funnel paths only \(got target 12\)"),
    (dict(debug_kernel=1), "debug_kernel 1 is not available for this explorer"),
    (dict(debug_kernel=101), "debug_kernel 101 is not available for this explorer"),
])
def test_pte_create_refusals(P, kw, msg):
    args = dict(n_chains=4, target=12, dim=16, explorer=4, target_params=[1.0])
    args.update(kw)
    with pytest.raises(P.PteError, match=msg):
        P.Engine(**args)
    if kw.get("debug_kernel") == 101:                # the scalar bit-packed generation has no bond form, in the test build either
        with pytest.raises(P.PteError, match=msg):
            P.Engine(test_build=True, **args)


def test_ising_metropolis_elsewhere_stays_refused(P):
    for target in (0, 2, 11):
        with pytest.raises(P.PteError, match="IsingMetropolis needs the Ising target|is implemented for SliceSampler / AutoMALA / MALA"):
            P.Engine(n_chains=4, target=target, dim=16, explorer=4, target_params=[1.0, 10.0])
    with pytest.raises(P.PteError, match="the Ising path is explored by IsingMetropolis only"):
        P.Engine(n_chains=4, target=3, dim=16, explorer=1, target_params=[1.0])
