"""Houdayer's cluster move as far as a machine without a device gets: the restatement (tests/cluster_ref.py) enumerated over every
pair of states of the 2 x 2 x 2 cube -- energy conservation, involution, invariance of pi x pi -- the kernel's word-level forms (row closure,
boundary popcount formula, j-th set bit; pigeons.jl_amd/csrc/pte_cluster.hpp) in Python integers against the restatement, the draw's
numbering, the exports and header declarations, the Python refusals, and a valid pair reaching the device check."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import cluster_ref as R
import family_cpu as F
import lattice3d_ref as R3
from family_cpu import P  # noqa: F401  (P: the module's fixture)

M32 = 0xFFFFFFFF


# ---- 1. the 2 x 2 x 2 cube, every pair of states and every seed site -----------------------------------------------------------------------
@pytest.fixture(scope="module")
def cube2():
    shape = (2, 2, 2)
    jx, jy, jz = R3.edwards_anderson(2, 11)
    bonds = [np.asarray(j, dtype=np.int64) for j in (jz, jy, jx)]
    assert any(np.any(b < 0) for b in bonds) and any(np.any(b > 0) for b in bonds)
    states = R3.all_states()                                             # [256][8] of 0 / 1, state i = the bits of i
    E = np.array([R.pair_sum(R.spins(s, shape), bonds) for s in states], dtype=np.int64)
    assert np.array_equal(E, R3.all_pair_sums(jx, jy, jz))              # the family's own pair sum
    return shape, bonds, states, E


def _index(bits):
    return bits @ (1 << np.arange(8))


def test_enumeration_conserves_inverts_and_leaves_pi_x_pi_invariant(cube2):
    """for every t (the set of differing sites) and every seed site of it: the component by the restated flood fill, then all 256 a at once.
    S_a + S_b is conserved, the move is an involution, the specification's delta (4 #(B and x) - 2 #B per direction) is the recomputed
    difference of the energies for a and, negated, for b, and with the seed site drawn with weight 1 / k the product measure pi x pi at
    beta = 0.37 is invariant to 1e-15 (65536 pair states)."""
    shape, bonds, states, E = cube2
    beta = 0.37
    w = np.exp(beta * (E - E.max()).astype(np.float64))
    p = w / w.sum()
    old = np.outer(p, p)
    new = np.zeros_like(old)
    idx = np.arange(256)
    new[idx, idx] += p * p                                               # t empty: nothing moves
    violations, pairs = 0, 256
    spin = (2 * states - 1).reshape((256,) + shape)                       # [256][2][2][2] of +-1
    # the bonds whose term s_i J s_j is -1, per axis, every site owning its + direction bond: the specification's x, as booleans
    minus = [spin * bonds[ax][None] * np.roll(spin, -1, axis=ax + 1) < 0 for ax in range(3)]
    for ti in range(1, 256):
        t = states[ti].astype(bool)
        k = int(t.sum())
        b_states = np.where(t[None, :], 1 - states, states)              # b = a with the sites of t flipped
        ib = _index(b_states)
        for site in np.flatnonzero(t):
            inside = R.component(t, shape, int(site))
            assert inside[site] and not np.any(inside & ~t)
            a2, b2 = np.where(inside[None, :], 1 - states, states), np.where(inside[None, :], 1 - b_states, b_states)
            ia2, ib2 = _index(a2), _index(b2)
            violations += int(np.sum(E[ia2] + E[ib2] != E[idx] + E[ib]))
            # the specification's delta, from the bonds with one end in the cluster: the recomputed difference of the two energies, for a and for b
            Cm = inside.reshape(shape)
            delta = np.zeros(256, dtype=np.int64)
            for ax in range(3):
                B = Cm != np.roll(Cm, -1, axis=ax)
                delta += 4 * np.sum(minus[ax] & B[None], axis=(1, 2, 3)) - 2 * int(B.sum())
            assert np.array_equal(delta, E[ia2] - E[idx]) and np.array_equal(-delta, E[ib2] - E[ib])
            # the involution: from (a', b') the differing sites are still t, the component of the same site is still `inside`
            assert np.array_equal(np.where(t[None, :], 1 - a2, a2), b2)
            assert np.array_equal(_index(np.where(inside[None, :], 1 - a2, a2)), idx) and np.array_equal(_index(np.where(inside[None, :], 1 - b2, b2)), ib)
            np.add.at(new, (ia2, ib2), p[idx] * p[ib] / k)
        pairs += 256
    assert pairs == 65536 and violations == 0
    dev = float(np.max(np.abs(new - old)))
    print("max deviation of pi x pi under the move: %.3g" % dev)
    assert dev <= 1e-15
    assert abs(new.sum() - 1.0) < 1e-12


def test_restated_move_on_the_cube2_pairs(cube2):
    """cluster_ref.move itself -- what the device tests compare with -- on 3000 random (a, b, j): delta equals the recomputed difference of
    the enumerated energies, S_a + S_b is conserved, k and |C| are what they say, and a second move from the same site undoes the first"""
    shape, bonds, states, E = cube2
    g = np.random.default_rng(5)
    for _ in range(3000):
        ia, ib = (int(v) for v in g.integers(0, 256, 2))
        if ia == ib:
            assert R.move(states[ia], states[ib], shape, bonds, j=0) is None
            continue
        k = int(np.sum(states[ia] != states[ib]))
        j = int(g.integers(0, k))
        a2, b2, size, k2, delta = R.move(states[ia], states[ib], shape, bonds, j=j)
        ia2, ib2 = int(_index(a2)), int(_index(b2))
        assert k2 == k and 1 <= size <= k and size == int(np.sum(a2 != states[ia])) == int(np.sum(b2 != states[ib]))
        assert delta == E[ia2] - E[ia] == -(E[ib2] - E[ib])
        site = int(np.flatnonzero(states[ia] != states[ib])[j])
        a3, b3, size3, _, delta3 = R.move(a2, b2, shape, bonds, site=site)
        assert np.array_equal(a3, states[ia]) and np.array_equal(b3, states[ib]) and size3 == size and delta3 == -delta


# ---- 2. the kernel's word-level forms, in Python integers ----------------------------------------------------------------------------------
def popc(v):
    return bin(v).count("1")


def to_words(bits, L, cube):
    """the kernel's working form: the cube one word per row of L bits, the square 32 sites per word"""
    per = L if cube else 32
    return [sum(int(bits[w * per + x]) << x for x in range(per)) for w in range(len(bits) // per)]


def from_words(words, L, cube):
    per = L if cube else 32
    return np.array([(w >> x) & 1 for w in words for x in range(per)], dtype=np.int64)


def fill_ring(n, t, L):
    mask = M32 >> (32 - L)
    up = dn = n
    pu = pd = t
    s = 1
    while s < L:
        up |= pu & (((up << s) | (up >> (L - s))) & mask); pu &= ((pu << s) | (pu >> (L - s))) & mask
        dn |= pd & (((dn >> s) | (dn << (L - s))) & mask); pd &= ((pd >> s) | (pd << (L - s))) & mask
        s <<= 1
    return up | dn


def fill_word(n, t):
    up = dn = n
    pu = pd = t
    for s in (1, 2, 4, 8, 16):
        up |= pu & ((up << s) & M32); pu &= (pu << s) & M32
        dn |= pd & (dn >> s); pd &= pd >> s
    return up | dn


def jth_set_bit(T, j):
    """(word, one-bit mask) of the j-th set bit in the order of the words and of the bits inside them: chunks of 64 words, an inclusive
    prefix sum of the popcounts inside the chunk, then j - before lowest bits cleared"""
    run = 0
    for base in range(0, len(T), 64):
        chunk = T[base:base + 64]
        incl = np.cumsum([popc(v) for v in chunk])
        if j < run + incl[-1]:
            for lane, v in enumerate(chunk):
                before = run + int(incl[lane]) - popc(v)
                if before <= j < before + popc(v):
                    for _ in range(j - before):
                        v &= v - 1
                    return base + lane, v & -v
        run += int(incl[-1])
    raise AssertionError("j >= k")


def component_words(T, seed_w, seed_bit, L, cube):
    """C <- C | (neighbours(C) & t) in place, word after word, until a pass changes nothing -> (C, passes)"""
    n, W = len(T), 1 if cube else L // 32
    Cw = [0] * n
    Cw[seed_w] = seed_bit
    for passes in range(1, n * 32 + 3):
        changed = False
        for w in range(n):
            t = T[w]
            if t == 0:
                continue
            cur = Cw[w]
            i, jj = divmod(w, L if cube else W)
            if cube:
                nb = Cw[i * L + (jj - 1) % L] | Cw[i * L + (jj + 1) % L] | Cw[((i - 1) % L) * L + jj] | Cw[((i + 1) % L) * L + jj]
            else:
                nb = Cw[((i - 1) % L) * W + jj] | Cw[((i + 1) % L) * W + jj] | (Cw[i * W + (jj - 1) % W] >> 31) | ((Cw[i * W + (jj + 1) % W] << 31) & M32)
            start = (cur | nb) & t
            if start == cur and passes != 1:
                continue
            g = fill_ring(start, t, L) if cube else fill_word(start, t)
            if g != cur:
                Cw[w] = g
                changed = True
        if not changed:
            return Cw, passes
    raise AssertionError("no fixed point")


def delta_words(A, Cw, planes, L, cube):
    """sum_dir (4 popcount(B & x) - 2 popcount(B)): B = C xor shift_dir(C), x = a xor shift_dir(a) xor J_dir"""
    n, W = len(A), 1 if cube else L // 32
    mask = M32 >> (32 - L) if cube else M32
    total = 0
    for w in range(n):
        cw, aw = Cw[w], A[w]
        i, jj = divmod(w, L if cube else W)
        if cube:
            rot = lambda v: ((v >> 1) | (v << (L - 1))) & mask
            ry, rz = i * L + (jj + 1) % L, ((i + 1) % L) * L + jj
            terms = [(cw ^ rot(cw), aw ^ rot(aw) ^ planes[0][w]), (cw ^ Cw[ry], aw ^ A[ry] ^ planes[1][w]), (cw ^ Cw[rz], aw ^ A[rz] ^ planes[2][w])]
        else:
            nx, dn = i * W + (jj + 1) % W, ((i + 1) % L) * W + jj
            sh = lambda v, nxt: (v >> 1) | ((nxt << 31) & M32)
            terms = [(cw ^ sh(cw, Cw[nx]), aw ^ sh(aw, A[nx]) ^ planes[0][w]), (cw ^ Cw[dn], aw ^ A[dn] ^ planes[1][w])]
        total += sum(4 * popc(B & x) - 2 * popc(B) for B, x in terms)
    return total


def bond_planes(bonds, L, cube):
    """the device's planes, a set bit where the bond is -1: the cube JX, JY, JZ, the square JR, JD (bonds: per array axis, as cluster_ref)"""
    order = (2, 1, 0) if cube else (1, 0)
    return [to_words((bonds[ax].ravel() < 0).astype(np.int64), L, cube) for ax in order]


def word_move(a, b, L, cube, bonds, j):
    A, B = to_words(a, L, cube), to_words(b, L, cube)
    T = [x ^ y for x, y in zip(A, B)]
    k = sum(popc(v) for v in T)
    seed_w, seed_bit = jth_set_bit(T, j)
    Cw, passes = component_words(T, seed_w, seed_bit, L, cube)
    delta = delta_words(A, Cw, bond_planes(bonds, L, cube), L, cube)
    a2, b2 = from_words([x ^ c for x, c in zip(A, Cw)], L, cube), from_words([x ^ c for x, c in zip(B, Cw)], L, cube)
    return a2, b2, sum(popc(v) for v in Cw), k, delta, passes


@pytest.mark.parametrize("L,cube", [(2, True), (4, True), (6, True), (10, True), (32, False), (64, False)])
def test_word_forms_equal_the_restatement(L, cube):
    d = L ** 3 if cube else L * L
    shape = R.lattice_shape(d, cube)
    g = np.random.default_rng(31 * L + cube)
    bonds = [2 * g.integers(0, 2, size=shape) - 1 for _ in shape]
    for density in (0.5, 0.1, 0.9, 0.02):
        a = g.integers(0, 2, d)
        flip = g.random(d) < density
        flip[int(g.integers(0, d))] = True                                # at least one differing site
        b = np.where(flip, 1 - a, a)
        k = int(flip.sum())
        for j in sorted({0, k - 1, int(g.integers(0, k))}):
            want = R.move(a, b, shape, bonds, j=j)
            got = word_move(a, b, L, cube, bonds, j)
            assert got[2:5] == want[2:5], (L, cube, density, j, got[2:], want[2:])
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
            assert 1 <= got[5] <= got[2] + 1                              # every pass but the last adds a site


def test_row_closure_on_hand_made_rows():
    """the log-step fills: a run of every length at every offset, wrapped on the ring and cut at the word's ends"""
    for L in (2, 4, 6, 10, 16, 32):
        mask = M32 >> (32 - L)
        for start in range(L):
            for length in range(1, L + 1):
                run = sum(1 << ((start + i) % L) for i in range(length))
                other = (1 << ((start + length + 1) % L)) if length + 3 <= L else 0     # a second run, a gap away on either side of the ring
                for seed in range(length):
                    bit = 1 << ((start + seed) % L)
                    assert fill_ring(bit, run | other, L) == run, (L, start, length, seed)
        assert fill_ring(0, mask, L) == 0 and fill_ring(1, mask, L) == mask
    for start in range(32):
        for length in range(1, 33 - start):
            run = ((1 << length) - 1) << start
            other = (1 << (start + length + 1)) if start + length + 1 < 32 else 0
            for seed in (0, length // 2, length - 1):
                assert fill_word(1 << (start + seed), run | other) == run
    assert fill_word(1 << 31, 0x80000001) == 1 << 31 and fill_word(1, 0x80000001) == 1      # nothing wraps inside a word


def test_jth_set_bit():
    g = np.random.default_rng(2)
    for n in (1, 4, 64, 65, 200):
        T = [int(v) for v in g.integers(0, 1 << 32, n)]
        if n > 1:
            T[n // 2] = 0                                                 # a word without a set bit on the way
        sites = [32 * w + x for w, v in enumerate(T) for x in range(32) if (v >> x) & 1]
        for j in (0, 1, len(sites) // 2, len(sites) - 1):
            w, bit = jth_set_bit(T, j)
            assert 32 * w + bit.bit_length() - 1 == sites[j]


# ---- 3. the draw ---------------------------------------------------------------------------------------------------------------------------
def test_draw_numbering_and_seed_index():
    assert R.mix64(R.GAMMA) == 0xE220A8397B1DCDAF                        # SplitMix64's first output from state 0
    assert R.draw(0, 0, 8, 0) == 0xE220A8397B1DCDAF                      # launch 0, chain 0 reads word 1 of the stream
    seed, N = 0xFEDCBA9876543210, 8
    for m in range(3):
        for c in range(N):
            assert R.draw(seed, m, N, c) == R.mix64((seed + (m * N + c + 1) * R.GAMMA) & R.M64)
        assert R.draw(seed, m + 1, N, 0) == R.draw(seed, m, N, N)        # launch m + 1 goes on where launch m stopped
    words = {R.draw(seed, m, N, c) for m in range(4) for c in range(N)}
    assert len(words) == 4 * N
    assert R.draw(seed + (1 << 64), 1, N, 3) == R.draw(seed, 1, N, 3)   # arithmetic mod 2^64
    hi = 0xFFFFFFFF00000000
    for d in (8, 216, 1024, 32768, 65536):
        assert R.seed_index(0, d) == 0 and R.seed_index(hi, d) == d - 1 and R.seed_index(R.M64, d) == d - 1
        assert R.seed_index(0x8000000000000000, d) == d // 2
        for u in (R.draw(seed, 0, N, c) for c in range(N)):
            assert R.seed_index(u, 1) == 0                               # k = 1: the one site
            assert 0 <= R.seed_index(u, d) < d and R.seed_index(u, d) == math.floor((u >> 32) * d / 2.0 ** 32)


# ---- 4. exports, header, units, null handles -----------------------------------------------------------------------------------------------
NAMES = ["pte_overlap_set_cluster_move", "pte_overlap_cluster_move", "pte_overlap_cluster_get"]


def test_exports_header_and_units(P):
    import __graft_entry__ as g
    from pigeons_amd import _lib
    L = _lib.load()
    for name in NAMES:
        assert name in _lib.EXPORTS and hasattr(L, name), name
    hdr = F.HEADER
    assert "#define PTE_ABI_VERSION 2\n" in hdr and _lib.ABI_VERSION == 2
    for decl in ("int pte_overlap_set_cluster_move(pte_overlap *ov, int64_t every, double min_beta, uint64_t seed);",
                 "int pte_overlap_cluster_move(pte_overlap *ov);",
                 "int pte_overlap_cluster_get(const pte_overlap *ov, int64_t *n, int64_t *empty, int64_t *size_sum, int64_t *k_sum, int64_t *abs_ds_sum, int64_t *passes_sum,\n"
                 "                            int64_t *moves_launched);",
                 "int pte_overlap_get(const pte_overlap *ov, int64_t *n, int64_t *hist, int64_t *link_n, int64_t *link_sum, int64_t *link_sum2);"):
        assert decl in hdr, decl
    assert "left it unless the cluster move is on" in hdr
    for name in NAMES:
        assert ":%s" % name in F.JULIA, name
    # a translation unit of its own, in a list of its own, with pte_overlap.hip's flags; the other lists did not grow
    assert g.CLUSTER_UNITS == [("pte_cluster.hip", dict(g.OVERLAP_UNITS)["pte_overlap.hip"])]
    assert len(g.UNITS) == 8 and all(len(u) == 1 for u in (g.LATTICE_UNITS, g.CHECKERBOARD_UNITS, g.LATTICE3D_UNITS, g.OVERLAP_UNITS))
    for f in ("pte_cluster.hip", "pte_cluster.hpp", "pte_cluster_params.hpp"):
        assert os.path.exists(os.path.join(g.CSRC, f)), f
    src = open(os.path.join(g.CSRC, "pte_cluster.hpp")).read()
    assert "asm" not in src and "atomic" not in src.replace("no atomics", "")
    assert "for (int pass = 0, slot = 0; pass <= d; ++pass)" in src and "while (changed" not in src
    # null handles are refused, not dereferenced
    assert L.pte_overlap_set_cluster_move(None, 1, 0.0, 1) == 1 and L.pte_overlap_cluster_move(None) == 1
    assert L.pte_overlap_cluster_get(None, None, None, None, None, None, None, None) == 1
    assert L.pte_overlap_set_cluster_move.argtypes == [C.c_void_p, C.c_int64, C.c_double, C.c_uint64]
    for name in ("HoudayerMove", "ClusterRecord"):
        assert name in P.__dict__, name


# ---- 5. the Python side ---------------------------------------------------------------------------------------------------------------------
def test_houdayer_move_and_cluster_record(P):
    m = P.HoudayerMove()
    assert (m.every, m.min_beta, m.seed) == (1, 0.0, None)
    z = np.zeros(3, dtype=np.int64)
    rec = P.ClusterRecord(np.array([0.0, 0.5, 1.0]), np.array([4, 4, 4]), z, np.array([6, 0, 40]), np.array([8, 0, 40]), z, z)
    f = rec.mean_fraction()
    assert f[0] == 0.75 and np.isnan(f[1]) and f[2] == 1.0
    assert [fld.name for fld in __import__("dataclasses").fields(P.OverlapRecord)] == ["betas", "dim", "n_links", "n", "hist", "link_n", "link_sum", "link_sum2"]
    pair = P.PTPair(None, None)
    assert pair.cluster is None and pair.clusters == [] and pair.cluster_move is None and pair.overlap is None


def test_python_refusals_come_before_any_device_work(P):
    with pytest.raises(ValueError, match=r"HoudayerMove: every must be an integer >= 0 \(got -1\); 0 turns the move off"):
        P.HoudayerMove(every=-1)
    with pytest.raises(ValueError, match=r"HoudayerMove: every must be an integer >= 0 \(got 1\.5\)"):
        P.HoudayerMove(every=1.5)
    with pytest.raises(ValueError, match=r"HoudayerMove: min_beta must be in \[0, 1\] \(got 1\.5\)"):
        P.HoudayerMove(min_beta=1.5)
    with pytest.raises(ValueError, match=r"HoudayerMove: min_beta must be in \[0, 1\] \(got nan\)"):
        P.HoudayerMove(min_beta=float("nan"))
    with pytest.raises(ValueError, match=r"HoudayerMove: min_beta must be in \[0, 1\] \(got -0\.25\)"):
        P.HoudayerMove(min_beta=-0.25)
    with pytest.raises(ValueError, match=r"HoudayerMove: seed must be None or an integer in 0 \.\. 2\^64 - 1 \(got -3\)"):
        P.HoudayerMove(seed=-3)
    with pytest.raises(ValueError, match=r"HoudayerMove: seed must be None or an integer in 0 \.\. 2\^64 - 1 \(got 18446744073709551616\)"):
        P.HoudayerMove(seed=2 ** 64)
    t3 = P.SpinGlass3DLogPotential.edwards_anderson(0.5, 2, seed=1)
    ok = dict(target=t3, n_chains=4, n_rounds=2, explorer=P.CheckerboardMetropolis(3), show_report=False)
    with pytest.raises(TypeError, match=r"pigeons_pair: cluster_move must be None or a HoudayerMove \(got 2\)"):
        P.pigeons_pair(cluster_move=2, **ok)
    for target, explorer, L in ((P.SpinGlassLogPotential.edwards_anderson(1.0, 6), P.IsingMetropolis(1), 6), (P.IsingLogPotential(1.0, 48), P.IsingMetropolis(1), 48)):
        with pytest.raises(NotImplementedError, match=r"pigeons_pair: HoudayerMove runs on the cube and on the 2-D lattices whose base_length is a multiple of 32 "
                                                      r"\(got base_length %d\)" % L):
            P.pigeons_pair(cluster_move=P.HoudayerMove(), **dict(ok, target=target, explorer=explorer))
    # the pair's own refusals still come first and read as before
    with pytest.raises(ValueError, match=r"seed_b must differ from seed \(both 5\)"):
        P.pigeons_pair(seed_b=5, cluster_move=P.HoudayerMove(), **dict(ok, seed=5))
    with pytest.raises(TypeError, match=r"Overlap\.set_cluster_move: expected a HoudayerMove \(got 3\)"):
        P.Overlap.set_cluster_move(object(), 3)


def test_a_valid_pair_with_the_move_reaches_the_device_check(P):
    F.no_device()
    for target, explorer in ((P.SpinGlass3DLogPotential.edwards_anderson(0.5, 2, seed=1), P.CheckerboardMetropolis(3)),
                             (P.SpinGlassLogPotential.edwards_anderson(1.0, 32), P.IsingMetropolis(3)),
                             (P.IsingLogPotential(1.0, 32), P.IsingMetropolis(3))):
        with pytest.raises(P.PteError, match="no HIP device"):
            P.pigeons_pair(target=target, n_chains=4, n_rounds=2, explorer=explorer, show_report=False,
                           cluster_move=P.HoudayerMove(every=2, min_beta=0.25, seed=7))
