"""The 3-D +-J spin-glass family without a GPU: the restatement (tests/lattice3d_ref.py) leaves the enumerated target of a
frustrated 2 x 2 x 2 instance invariant one colour at a time -- and would not if all eight sites were decided at once --, its single-site rule
is in detailed balance, its draws sit where the specification numbers them, it is gauge covariant; the bit-sliced neighbour count of the
DESIGN text counts; the enumerator, the export, the classes and the translation unit are mirrored where they must be, and pte_create refuses
-- before any device work -- what the family does not run, and accepts what it does."""
import itertools
import math
import os

import numpy as np
import pytest

import family_cpu as F
import oracle as O
import lattice3d_ref as R
from family_cpu import P  # noqa: F401  (P: the module's fixture)


def _transition(lat, sites, r):
    """the 256 x 256 matrix of 'every site of `sites` decides from the lattice at entry, independently': row = from, column = to"""
    states = R.all_states()
    T = np.zeros((256, 256))
    for k in range(256):
        p = [R.flip_probability(dl, r) for dl in lat.deltas(states[k], np.asarray(sites))]
        for m in range(1 << len(sites)):
            k2, w = k, 1.0
            for q, s in enumerate(sites):
                if (m >> q) & 1:
                    k2 ^= 1 << int(s); w *= p[q]
                else:
                    w *= 1.0 - p[q]
            T[k, k2] += w
    return T


def test_each_half_sweep_leaves_the_target_invariant_and_an_all_sites_update_does_not():
    """L = 2 (256 states), edwards_anderson(seed=1) -- frustrated: its largest S is below the 24 bonds --, beta = 0.7, beta_target = 0.9:
    pi P = pi to 1e-12 for the colour-0 and the colour-1 half-sweep (sums of 16 products of four probabilities: rounding is ~1e-16); deciding all
    eight sites at once is NOT a kernel for pi, which is what the colours are for"""
    beta, bt = 0.7, 0.9
    jx, jy, jz = R.edwards_anderson(2, 1)
    lat = R.Lattice(jx, jy, jz)
    S = R.all_pair_sums(jx, jy, jz).astype(np.float64)
    assert S.max() < 24                                                            # frustrated
    w = np.exp(np.array([R.ising_lp(beta, bt, s) for s in S]))
    pi = w / w.sum()
    r = R.thresholds(beta, bt)
    assert sorted(lat.active[0].tolist() + lat.active[1].tolist()) == list(range(8)) and lat.active[0].tolist() == [0, 3, 5, 6]
    res = []
    for sites in (lat.active[0], lat.active[1], np.arange(8)):
        T = _transition(lat, sites, r)
        assert np.allclose(T.sum(axis=1), 1.0, rtol=0, atol=1e-14)
        res.append(float(np.max(np.abs(pi @ T - pi))))
    print("residuals: colour 0 %.3g, colour 1 %.3g, all sites at once %.3g" % tuple(res))
    assert res[0] < 1e-12 and res[1] < 1e-12
    assert res[2] > 1e-3


@pytest.mark.parametrize("beta", [0.3, 1.0])
def test_single_site_rule_is_in_detailed_balance(beta):
    """every site of 500 random states of edwards_anderson(1.0, 4, seed=2): pi(x) P(x -> x^s) = pi(x^s) P(x^s -> x) in logs, to rounding (each
    side is one product and one log of an exponential: 1e-12 relative to the largest log weight); the rule's delta is the change of S"""
    L = 4
    jx, jy, jz = R.edwards_anderson(L, 2)
    lat = R.Lattice(jx, jy, jz)
    r = R.thresholds(1.0, beta)
    logp = lambda delta: np.where(delta >= 0, 0.0, np.log([r[max(4, abs(int(v)))] for v in delta]))
    g = np.random.default_rng(7)
    sites = np.arange(lat.d)
    worst, seen = 0.0, set()
    for _ in range(500):
        b = g.integers(0, 2, lat.d)
        S = R.pair_sum(b, jx, jy, jz)
        delta = lat.deltas(b, sites)
        seen |= set(delta.tolist())
        s = int(g.integers(0, lat.d))
        b2 = b.copy(); b2[s] ^= 1
        assert R.pair_sum(b2, jx, jy, jz) - S == delta[s]
        back = np.array([lat.deltas(np.where(sites == q, 1 - b, b), np.array([q]))[0] for q in sites[:8]])
        assert np.array_equal(back, -delta[:8])                                     # the way back has the opposite delta
        lhs = beta * S + logp(delta)
        rhs = beta * (S + delta) + logp(-delta)
        worst = max(worst, float(np.max(np.abs(lhs - rhs))))
    assert seen <= {-12, -8, -4, 0, 4, 8, 12} and {-8, -4, 0, 4, 8} <= seen
    assert worst < 1e-12 * (1 + beta * 3 * lat.d)


@pytest.mark.parametrize("L,n_steps", [(4, 2), (6, 1)])
def test_stream_position_and_draw_numbers(L, n_steps):
    """after sweep() the stream is n_steps d draws on; the uniform of site (z, y, x) in half-sweep h is draw
    h d / 2 + (z L + y) L / 2 + (x >> 1) + 1 of the stream at entry: every decision of every half-sweep restated from mix64"""
    d = L ** 3
    jx, jy, jz = R.edwards_anderson(L, 30 + L)
    lat = R.Lattice(jx, jy, jz)
    bits = np.random.default_rng(L).integers(0, 2, d)
    beta, bt = 0.45, 0.8
    rng = O.OracleRng(seed=123)
    seed, gamma = rng.state
    r = R.thresholds(beta, bt)
    b = bits.copy()
    S = R.pair_sum(b, jx, jy, jz)
    n_rej = 0
    for h in range(2 * n_steps):
        want = b.copy()
        sites = lat.active[h % 2]
        numbers = []
        for s, delta in zip(sites, lat.deltas(b, sites)):
            z, y, x = np.unravel_index(s, (L, L, L))
            assert (x + y + z) % 2 == h % 2
            numbers.append(R.draw_number(L, h, int(z), int(y), int(x)))
            u = R.uniform_of_draw(seed, gamma, numbers[-1])
            if delta >= 0 or not (u > r[-int(delta)]):
                want[s] ^= 1
            else:
                n_rej += 1
        assert numbers == list(range(h * d // 2 + 1, (h + 1) * d // 2 + 1))        # consecutive draws in raster order over the active sites
        S = R.half_sweep(lat, b, h % 2, r, S, rng)
        assert np.array_equal(b, want), "half-sweep %d" % h
        assert S == R.pair_sum(b, jx, jy, jz)
    assert n_rej > 0 and not np.array_equal(b, bits)
    assert rng.state == ((seed + n_steps * d * gamma) & R.M64, gamma)
    rng2 = O.OracleRng(seed=123)
    b2 = bits.copy()
    assert R.sweep(lat, b2, beta, bt, R.pair_sum(bits, jx, jy, jz), rng2, n_steps) == S and np.array_equal(b2, b) and rng2.state == rng.state


@pytest.mark.parametrize("L,seed", [(2, 1), (4, 2), (6, 3)])
def test_gauge_covariance_of_the_restatement(L, seed):
    """bonds g_i g_j J_ij started from g . s give g . (trajectory) with the same stream position"""
    g = np.random.default_rng(seed)
    J1 = R.edwards_anderson(L, seed)
    gg = 2 * g.integers(0, 2, size=(L, L, L)) - 1
    J2 = R.gauge(*J1, gg)
    flip = (1 - gg.ravel()) // 2                                                    # 1 where the gauge turns the spin
    b1 = g.integers(0, 2, size=L ** 3)
    b2 = b1 ^ flip
    l1, l2 = R.Lattice(*J1), R.Lattice(*J2)
    S1, S2 = R.pair_sum(b1, *J1), R.pair_sum(b2, *J2)
    assert S1 == S2
    r1, r2 = O.OracleRng(seed=77), O.OracleRng(seed=77)
    for _ in range(2):
        S1 = R.sweep(l1, b1, 0.6, 0.9, S1, r1, 2)
        S2 = R.sweep(l2, b2, 0.6, 0.9, S2, r2, 2)
        assert S1 == S2 and r1.state == r2.state
        assert np.array_equal(b2, b1 ^ flip)
    assert r1.state != O.OracleRng(seed=77).state


def test_pair_sum_of_the_ferromagnet_and_of_doubled_bonds(P):
    t = P.SpinGlass3DLogPotential.ferromagnet(1.0, 4)
    assert R.pair_sum(np.zeros(64, dtype=np.int64), t.bonds_x, t.bonds_y, t.bonds_z) == 3 * 64
    # L = 2: the two bonds between the same pair of sites are distinct terms -- 24 bonds, and opposite bonds of a pair cancel
    one = np.ones((2, 2, 2), dtype=np.int8)
    assert R.pair_sum(np.zeros(8, dtype=np.int64), one, one, one) == 24
    jx = one.copy(); jx[:, :, 1] = -1
    assert R.pair_sum(np.zeros(8, dtype=np.int64), jx, one, one) == 16
    # the zero state: S = the sum of all bonds
    jx, jy, jz = R.edwards_anderson(6, 9)
    assert R.pair_sum(np.zeros(216, dtype=np.int64), jx, jy, jz) == int(jx.sum()) + int(jy.sum()) + int(jz.sum())


def test_bit_sliced_count_equals_the_integer_count():
    """all 64 patterns of the six neighbour terms, one pattern per bit position of two words"""
    pats = list(itertools.product((0, 1), repeat=6))
    words = [[0, 0] for _ in range(6)]
    for n, p in enumerate(pats):
        for k in range(6):
            words[k][n // 32] |= p[k] << (n % 32)
    none, one, two, more = R.bit_sliced_count([np.array(w, dtype=np.uint32) for w in words])
    for n, p in enumerate(pats):
        got = tuple(int((m[n // 32] >> np.uint32(n % 32)) & 1) for m in (none, one, two, more))
        cnt = sum(p)
        assert got == (int(cnt == 0), int(cnt == 1), int(cnt == 2), int(cnt >= 3)), (p, got)
        assert 4 * cnt - 12 in (-12, -8, -4, 0, 4, 8, 12)


def test_enum_export_and_unit_mirrors(P):
    from pigeons_amd import _lib
    import __graft_entry__ as g
    assert _lib.TARGET_SPIN_GLASS_3D == 13
    assert "pte_set_target_spin_glass_3d" in _lib.EXPORTS and hasattr(_lib.load(), "pte_set_target_spin_glass_3d")
    hdr = F.HEADER
    assert "PTE_TARGET_SPIN_GLASS_3D = 13" in hdr and "#define PTE_ABI_VERSION 2\n" in hdr
    assert "int pte_set_target_spin_glass_3d(pte_engine *h, int64_t base_length, const int8_t *bonds_x" in hdr
    jl = F.JULIA
    assert "const TARGET_SPIN_GLASS_3D = Int32(13)" in jl and ":pte_set_target_spin_glass_3d" in jl
    assert "SpinGlass3DLogPotential" in P.__dict__ and hasattr(P.Engine, "set_target_spin_glass_3d")
    # a translation unit of its own, in a list of its own, with pte_spinglass.hip's flags; the other lists did not grow
    assert g.LATTICE3D_UNITS == [("pte_lattice3d.hip", dict(g.LATTICE_UNITS)["pte_spinglass.hip"])]
    assert len(g.UNITS) == 8 and [u for u, _ in g.LATTICE_UNITS] == ["pte_spinglass.hip"] and [u for u, _ in g.CHECKERBOARD_UNITS] == ["pte_checkerboard.hip"]
    assert "X(lattice3d)" in open(os.path.join(g.CSRC, "pte_automala_params.hpp")).read()
    assert "PTE_DEFINE_RNG_POLICY_SETTER(lattice3d)" in open(os.path.join(g.CSRC, "pte_lattice3d.hpp")).read()
    assert os.path.exists(os.path.join(g.CSRC, "pte_lattice3d.hip")) and os.path.exists(os.path.join(g.CSRC, "pte_lattice3d_params.hpp"))


def test_python_surface_and_its_refusals(P):
    one = np.ones((4, 4, 4), dtype=np.int8)
    t = P.SpinGlass3DLogPotential(0.8, one, -one, one)
    assert (t.base_length, t.dim, t.beta) == (4, 64, 0.8) and t.bonds_y.dtype == np.int8
    assert repr(t) == "SpinGlass3DLogPotential(beta=0.8, base_length=4)"
    assert isinstance(P.pt.default_explorer(t), P.CheckerboardMetropolis)
    assert isinstance(P.pt.default_explorer(P.IsingLogPotential(1.0, 4)), P.IsingMetropolis)                                    # unchanged
    assert isinstance(P.pt.default_explorer(P.SpinGlassLogPotential.edwards_anderson(1.0, 4)), P.IsingMetropolis)             # unchanged
    with pytest.raises(ValueError, match=r"bonds_x must be L x L x L with L >= 2 \(got shape \(4, 4, 3\)\)"):
        P.SpinGlass3DLogPotential(1.0, one[:, :, :3], one, one)
    with pytest.raises(ValueError, match=r"bonds_z must be L x L x L with L >= 2 \(got shape \(4, 4\)\)"):
        P.SpinGlass3DLogPotential(1.0, one, one, one[0])
    with pytest.raises(ValueError, match=r"must have the same shape \(got \(4, 4, 4\), \(2, 2, 2\) and \(4, 4, 4\)\)"):
        P.SpinGlass3DLogPotential(1.0, one, one[:2, :2, :2], one)
    with pytest.raises(ValueError, match=r"base_length must be even \(got bonds_x of shape \(3, 3, 3\)\)"):
        P.SpinGlass3DLogPotential(1.0, one[:3, :3, :3], one[:3, :3, :3], one[:3, :3, :3])
    big = np.ones((34, 34, 34), dtype=np.int8)
    with pytest.raises(ValueError, match=r"base_length must be at most 32 \(got bonds_x of shape \(34, 34, 34\)\): the device holds a row"):
        P.SpinGlass3DLogPotential(1.0, big, big, big)
    bad = np.array(one, dtype=np.float64); bad[2, 1, 3] = 0.5
    with pytest.raises(ValueError, match=r"bonds_y\[2\]\[1\]\[3\] must be \+1 or -1 \(got 0\.5\): ±J is the supported disorder"):
        P.SpinGlass3DLogPotential(1.0, one, bad, one)
    for L in (3, 34, 0):
        with pytest.raises(ValueError, match=r"base_length must be even and in 2\.\.32 \(got %d\)" % L):
            P.SpinGlass3DLogPotential.edwards_anderson(1.0, L)
        with pytest.raises(ValueError, match=r"base_length must be even and in 2\.\.32 \(got %d\)" % L):
            P.SpinGlass3DLogPotential.ferromagnet(1.0, L)
    a, b, c = (P.SpinGlass3DLogPotential.edwards_anderson(1.0, 6, seed=s) for s in (5, 5, 6))
    assert all(np.array_equal(u, v) for u, v in zip((a.bonds_x, a.bonds_y, a.bonds_z), (b.bonds_x, b.bonds_y, b.bonds_z)))
    assert not np.array_equal(a.bonds_x, c.bonds_x) and set(np.unique(a.bonds_z)) == {-1, 1}
    for u, v in zip((a.bonds_x, a.bonds_y, a.bonds_z), R.edwards_anderson(6, 5)):   # one generator, the order x, y, z
        assert np.array_equal(u, v)
    f = P.SpinGlass3DLogPotential.ferromagnet(0.5, 2)
    assert f.dim == 8 and all(np.all(p == 1) for p in (f.bonds_x, f.bonds_y, f.bonds_z))
    # every explorer but CheckerboardMetropolis is refused before any device work
    for ex in (P.IsingMetropolis(), P.SliceSampler(), P.AutoMALA(), P.Compose(P.CheckerboardMetropolis(), P.CheckerboardMetropolis())):
        with pytest.raises(NotImplementedError, match="the device 3-D spin-glass path is explored by CheckerboardMetropolis only"):
            P.PT(P.Inputs(target=a, n_chains=4, n_rounds=2, explorer=ex, show_report=False))


@pytest.mark.parametrize("dim", [8, 64, 216, 1000, 32768])
def test_accepted_config_reaches_the_device_check(P, dim):
    """fails on the code before the family existed ("target 13 has no device log-potential"): a valid configuration now passes validation"""
    F.no_device()
    F.assert_reaches_the_device_check(P, n_chains=4, target=13, dim=dim, explorer=7, target_params=[1.0])


CAP = r"a row of the lattice is held in one 32-bit word, so 32 is the cap although 34\.\.40 would fit the 65536-site limit"
ONLY = r"the 3-D spin-glass path is explored by CheckerboardMetropolis only \(got explorers %d, %d\)"


@pytest.mark.parametrize("kw,msg", [
    (dict(dim=1), r"the 3-D spin-glass path needs dim = base_length\^3 with base_length even and in 2\.\.32 \(got 1\): " + CAP),
    (dict(dim=27), r"needs dim = base_length\^3 with base_length even and in 2\.\.32 \(got 27\)"),
    (dict(dim=16), r"needs dim = base_length\^3 with base_length even and in 2\.\.32 \(got 16\)"),
    (dict(dim=34 ** 3), r"base_length even and in 2\.\.32 \(got 39304\): " + CAP),
    (dict(dim=40 ** 3), r"base_length even and in 2\.\.32 \(got 64000\): " + CAP),
    (dict(explorer=0), ONLY % (0, 0)),
    (dict(explorer=1), ONLY % (1, 0)),
    (dict(explorer=2), ONLY % (2, 0)),
    (dict(explorer=3), ONLY % (3, 0)),
    (dict(explorer=4), ONLY % (4, 0)),
    (dict(explorer=5), ONLY % (5, 0)),
    (dict(explorer=7, explorer2=7), ONLY % (7, 7)),
    (dict(explorer=7, explorer2=4), ONLY % (7, 4)),
    (dict(explorer=4, explorer2=7), ONLY % (4, 7)),
    (dict(explorer=6), r"AAPS is implemented on the scaled-precision MVN and funnel paths only \(got target 13\)"),   # an earlier refusal keeps its place
    (dict(debug_kernel=102), r"the 3-D spin-glass path has one kernel; debug_kernel must be 0 \(got 102\)"),
    (dict(debug_kernel=1), r"the 3-D spin-glass path has one kernel; debug_kernel must be 0 \(got 1\)"),
])
def test_pte_create_refusals(P, kw, msg):
    F.assert_create_refused(P, dict(n_chains=4, target=13, dim=64, explorer=7, target_params=[1.0]), kw, msg)


def test_the_2d_refusals_keep_their_text(P):
    for target in (0, 2, 11):
        with pytest.raises(P.PteError, match="^pte_create: CheckerboardMetropolis needs the Ising or the spin-glass target$"):
            P.Engine(n_chains=4, target=target, dim=16, explorer=7, target_params=[1.0, 10.0])
    for target, name in ((3, "Ising"), (12, "spin-glass")):
        with pytest.raises(P.PteError, match="the %s path is explored by IsingMetropolis only" % name):
            P.Engine(n_chains=4, target=target, dim=16, explorer=3, target_params=[1.0])
        with pytest.raises(P.PteError, match=r"CheckerboardMetropolis needs an even base_length \(got 3\)"):
            P.Engine(n_chains=4, target=target, dim=9, explorer=7, target_params=[1.0])
    with pytest.raises(P.PteError, match="target 14 has no device log-potential"):
        P.Engine(n_chains=4, target=14, dim=16, explorer=2, target_params=[1.0])
