"""Houdayer's cluster move on the device (k_cluster_move: pigeons.jl_amd/csrc/pte_cluster.hpp; pte_overlap_*cluster*: include/pte.h)
against its restatement (tests/cluster_ref.py): on natural states, on hand-made sets of differing sites, through min_beta, through the scan
loop, through its refusals, and against the enumerated overlap distribution of a 2 x 2 x 2 instance.

Lattice bits, RNG words, the pair sums and the accumulators are integers and are compared exactly (passes_sum, the kernel's own cost figure,
is bracketed).  suff is read as the next explore step reads it, through the energy_ac1 recorder (tests/test_gpu_spinglass.py does the same),
and against a twin engine whose suff the family's own refresh-stats kernel counted from the moved states.  The one statistical check, the
last, is held to DESIGN 4.20's band, computed from the enumeration."""
import numpy as np
import pytest

import cluster_ref as CR
import lattice3d_ref as R3
from spinglass_ref import ising_lp

pytestmark = pytest.mark.gpu

N = 8
SEED = 0xC0FFEE12345


@pytest.fixture(scope="module")
def P():
    import pigeons_amd
    return pigeons_amd


def _rec(P):
    return [P.round_trip, P.index_process, P.log_sum_ratio, P.swap_acceptance_pr, P.energy_ac1]


def _cube(P, L, beta=0.8, seed=None):
    return P.SpinGlass3DLogPotential.edwards_anderson(beta, L, seed=100 + L if seed is None else seed), P.CheckerboardMetropolis(1), True


def _square(P, L, beta=0.8, seed=None):
    return P.SpinGlassLogPotential.edwards_anderson(beta, L, seed=200 + L if seed is None else seed), P.IsingMetropolis(1), False


def _ising(P, L):
    return P.IsingLogPotential(0.4, L), P.IsingMetropolis(1), False


CASES = {"cube": _cube, "square": _square, "ising": _ising}


def _engine(P, case, seed, n=N):
    target, explorer, _ = case
    return P.PT(P.Inputs(target=target, n_chains=n, n_rounds=4, seed=seed, explorer=explorer, show_report=False, record=_rec(P))).replicas


def _pair_sums(x, shape, bonds):
    return np.array([CR.pair_sum(CR.spins(row, shape), bonds) for row in x], dtype=np.int64)


def _set(eng, x, chain):
    """states and chain map in, the RNG words kept; suff is recounted by the family's refresh-stats kernel (the Ising family: on the host)"""
    eng.set_states(np.asarray(x, dtype=np.float64), np.asarray(chain, dtype=np.int64), None)


def _check_states_and_suff(P, case, eng, seed, x_want, chain, S_want):
    """the engine holds x_want; its suff is S_want as the next explore reads it, and everything that step leaves -- lattice bits, RNG words,
    the recorder -- equals a twin's whose suff was counted afresh from x_want"""
    x, c, rng = eng.states()
    assert np.array_equal(c, chain)
    assert np.array_equal(x, x_want), "lattice bits"
    twin = _engine(P, case, seed, n=len(chain))
    twin.set_states(x, c, rng)
    out = []
    for e in (eng, twin):
        e.reduce()
        e.explore(1); e.swap(1); e.reduce()
        out.append(list(e.states()) + list(e.energy_ac1()))
    for u, v in zip(*out):
        np.testing.assert_array_equal(np.asarray(u), np.asarray(v))
    betas, beta_t, mom = eng.schedule(), case[0].beta, out[0][5]
    for slot, ch in enumerate(chain):
        assert mom[ch, 0] == ising_lp(betas[ch], beta_t, S_want[slot]), "suff of chain %d" % ch


def _passes_bracketed(rec):
    moved = rec.n - rec.empty
    assert np.all(rec.passes_sum >= moved) and np.all(rec.passes_sum <= rec.size_sum + moved), (rec.passes_sum, rec.size_sum, moved)


# ---- 1. natural states -------------------------------------------------------------------------------------------------------------------
# the cube: L = 2 sixteen rows per word, doubled bonds; 4; 6 rows straddle words; 10: 1000 bits, ragged last word; 16; 32: whole-word rows,
# four rows per thread.  The square: 32 a row is a word, the x-wrap inside it; 64 the carry across a row's two words; 96 three words per row
# (not a power of two).  The Ising family (no bond plane) at L = 32.
NATURAL = [("cube", 2), ("cube", 4), ("cube", 6), ("cube", 10), ("cube", 16), ("cube", 32), ("square", 32), ("square", 64), ("square", 96), ("ising", 32)]


@pytest.mark.parametrize("family,L", NATURAL)
def test_two_moves_on_natural_states_equal_the_restatement(P, family, L):
    case = CASES[family](P, L)
    a, b = _engine(P, case, 1), _engine(P, case, 2)
    shape, bonds = CR.lattice_shape(a.d, case[2]), CR.bonds_of(case[0])
    ov = P.Overlap(a, b)
    ov.run_scans(1, 3)                                    # both engines sweep and swap: the states the move meets in a run
    ov.reduce()
    assert ov.reduce_clusters().n.tolist() == [0] * N    # never set: off
    (xa, ca, _), (xb, cb, _) = a.states(), b.states()
    xa, xb = xa.astype(np.int64), xb.astype(np.int64)
    Sa, Sb = _pair_sums(xa, shape, bonds), _pair_sums(xb, shape, bonds)
    betas = a.schedule()
    want = CR.Accumulators(N)
    ov.set_cluster_move(P.HoudayerMove(seed=SEED))
    ov.cluster_move()
    CR.launch(xa, ca, xb, cb, shape, bonds, betas, 0.0, SEED, 0, want, Sa, Sb)
    # every slot of both engines handed another chain, independently; suff stays as the move left it
    g = np.random.default_rng(L)
    ca, cb = (ca + 1) % N, g.permutation(N).astype(np.int64)
    a.set_states(None, ca, None); b.set_states(None, cb, None)
    ov.cluster_move()
    CR.launch(xa, ca, xb, cb, shape, bonds, betas, 0.0, SEED, 1, want, Sa, Sb)
    ov.reduce()
    rec = ov.reduce_clusters()
    want.assert_equal(rec)
    assert rec.n.tolist() == [2] * N and rec.moves_launched == 2 and np.array_equal(rec.betas, betas)
    assert rec.size_sum.sum() > 0 and np.all(rec.size_sum <= rec.k_sum)
    _passes_bracketed(rec)
    assert Sa.tolist() == _pair_sums(xa, shape, bonds).tolist() and Sb.tolist() == _pair_sums(xb, shape, bonds).tolist()
    _check_states_and_suff(P, case, a, 1, xa, ca, Sa)
    _check_states_and_suff(P, case, b, 2, xb, cb, Sb)


# ---- 2. hand-made sets of differing sites ------------------------------------------------------------------------------------------------
def _serpentine(L, without=None):
    """rows 0, 2, .., L - 2 full, neighbouring full rows joined by one site that alternates between column 0 and column L / 2, the last row
    empty (the wrap from row L - 2 to row 0 stays open): one component.  without: the connector left out."""
    t = np.zeros((L, L), dtype=bool)
    t[0:L - 1:2, :] = True
    for i in range(L // 2 - 1):
        if i != without:
            t[2 * i + 1, 0 if i % 2 == 0 else L // 2] = True
    return t


def _hand_made(family, L):
    """[N] boolean sets t, one per chain, and what each must do: (size or None, delta or None)"""
    shape = (L, L, L) if family == "cube" else (L, L)
    d = int(np.prod(shape))
    z = lambda: np.zeros(shape, dtype=bool)
    empty, full, one, last = z(), ~z(), z(), z()
    one.flat[5] = True
    last.flat[d - 1] = True
    wrap, diag = z(), z()
    if family == "cube":
        wrap[2, 3, :] = True; wrap[2, :, 1] = True; wrap[:, 3, 1] = True          # a line round the lattice along every axis, through (2, 3, 1)
        wrap[5, 0, 4] = True                                                     # and a site apart, touching none of it
        diag[0, 0, 0] = True; diag[1, 1, 0] = True; diag[0, 1, 1] = True         # pairwise diagonal
        plane = z(); plane[0, :, :] = True; plane[3, :, :] = True                # two planes, each wrapping in x and y, two layers apart
        sparse = np.random.default_rng(9).random(shape) < 0.3
        sets = [empty, full, one, last, wrap, diag, plane, sparse]
        expect = [(0, 0), (d, 0), (1, None), (1, None), (None, None), (1, None), (L * L, None), (None, None)]
    else:
        wrap[7, :] = True; wrap[:, 20] = True
        wrap[15, 3] = True
        diag[0, 0] = True; diag[1, 1] = True; diag[L - 1, L - 1] = True          # (L - 1, L - 1) and (0, 0): diagonal through the wrap
        sets = [empty, full, one, last, wrap, diag, _serpentine(L), _serpentine(L, without=8)]
        k_serp = int(_serpentine(L).sum())
        expect = [(0, 0), (d, 0), (1, None), (1, None), (None, None), (1, None), (k_serp, None), (None, None)]
    return shape, d, sets, expect


@pytest.mark.parametrize("family,L", [("cube", 6), ("square", 32)])
def test_hand_made_sets(P, family, L):
    case = CASES[family](P, L)
    shape, d, sets, expect = _hand_made(family, L)
    bonds = CR.bonds_of(case[0])
    a, b = _engine(P, case, 1), _engine(P, case, 2)
    g = np.random.default_rng(L)
    ca, cb = g.permutation(N).astype(np.int64), g.permutation(N).astype(np.int64)
    xa = g.integers(0, 2, size=(N, d)).astype(np.int64)
    xb = np.zeros_like(xa)
    for slot_b, c in enumerate(cb):
        row = xa[list(ca).index(c)]
        xb[slot_b] = np.where(sets[c].ravel(), 1 - row, row)
    _set(a, xa, ca); _set(b, xb, cb)
    xa0, xb0 = xa.copy(), xb.copy()
    Sa, Sb = _pair_sums(xa, shape, bonds), _pair_sums(xb, shape, bonds)
    ov = P.Overlap(a, b)
    ov.set_cluster_move(P.HoudayerMove(seed=SEED))
    ov.cluster_move()
    want = CR.Accumulators(N)
    CR.launch(xa, ca, xb, cb, shape, bonds, a.schedule(), 0.0, SEED, 0, want, Sa, Sb)
    ov.reduce()
    rec = ov.reduce_clusters()
    want.assert_equal(rec)
    _passes_bracketed(rec)
    sa = {int(c): s for s, c in enumerate(ca)}
    sb = {int(c): s for s, c in enumerate(cb)}
    for c, (size, delta) in enumerate(expect):
        k = int(sets[c].sum())
        assert rec.k_sum[c] == k and rec.n[c] == 1 and rec.empty[c] == (1 if k == 0 else 0), c
        if size is not None:
            assert rec.size_sum[c] == size, c
        if delta is not None:
            assert rec.abs_ds_sum[c] == delta, c
    assert np.array_equal(xa[sa[0]], xa0[sa[0]]) and np.array_equal(xb[sb[0]], xb0[sb[0]])            # empty: nothing written
    assert np.array_equal(xa[sa[1]], 1 - xa0[sa[1]]) and np.array_equal(xb[sb[1]], 1 - xb0[sb[1]])    # all sites: both copies globally flipped
    flipped = lambda c: (xa[sa[c]] != xa0[sa[c]]).reshape(shape)
    assert flipped(2).ravel().nonzero()[0].tolist() == [5] and flipped(3).ravel().nonzero()[0].tolist() == [d - 1]
    # the wrapping cluster: the seed's component only -- the lines through the crossing, or the site apart
    apart = (5, 0, 4) if family == "cube" else (15, 3)
    lines = sets[4].copy(); lines[apart] = False
    assert rec.size_sum[4] in (1, int(lines.sum())) and np.array_equal(flipped(4), lines if rec.size_sum[4] > 1 else sets[4] & ~lines)
    assert flipped(5).sum() == 1 and (flipped(5) & sets[5]).sum() == 1                                   # diagonal contact does not connect
    if family == "cube":
        assert flipped(6).sum() == L * L and flipped(6)[0].all() != flipped(6)[3].all()                 # one plane of the two
    else:
        assert np.array_equal(flipped(6), sets[6])                                                      # the serpentine: one component, whole
        part = flipped(7)
        assert 0 < part.sum() < sets[7].sum() and not np.any(part & ~sets[7])
        assert part[0:17:2].all() != part[18:31:2].all(), "one side of the missing connector, whole, and none of the other"
        assert rec.passes_sum[6] > 8, "a full row per pass at best, from a seed in the middle: the component is not found in one sweep"
        print("serpentine: %d sites in %d passes; cut: %d sites in %d passes" % (rec.size_sum[6], rec.passes_sum[6], rec.size_sum[7], rec.passes_sum[7]))
    _check_states_and_suff(P, case, a, 1, xa, ca, Sa)
    _check_states_and_suff(P, case, b, 2, xb, cb, Sb)
    # the move is its own inverse: the same draw again (set resets the launch counter) restores both engines, bit for bit
    _set(a, xa, ca); _set(b, xb, cb)
    ov.set_cluster_move(P.HoudayerMove(seed=SEED))
    ov.cluster_move()
    assert np.array_equal(a.states()[0], xa0) and np.array_equal(b.states()[0], xb0)


def test_cube_2_with_differing_double_bonds(P):
    """L = 2: the + and the - neighbour of a site coincide, and the two bonds between them are two terms.  Every chain a different t"""
    case = _cube(P, 2, seed=3)
    t = case[0]
    assert np.any(t.bonds_x[:, :, 0] != t.bonds_x[:, :, 1]) and np.any(t.bonds_y[:, 0, :] != t.bonds_y[:, 1, :]) and np.any(t.bonds_z[0] != t.bonds_z[1])
    shape, bonds = (2, 2, 2), CR.bonds_of(t)
    a, b = _engine(P, case, 1), _engine(P, case, 2)
    g = np.random.default_rng(2)
    ca = cb = np.arange(N, dtype=np.int64)
    xa = g.integers(0, 2, size=(N, 8)).astype(np.int64)
    masks = [0b00000001, 0b00000011, 0b00000101, 0b10000001, 0b01101001, 0b11111111, 0b10010110, 0b00010000]
    xb = np.array([[v ^ ((m >> s) & 1) for s, v in enumerate(row)] for row, m in zip(xa, masks)], dtype=np.int64)
    _set(a, xa, ca); _set(b, xb, cb)
    Sa, Sb = _pair_sums(xa, shape, bonds), _pair_sums(xb, shape, bonds)
    ov = P.Overlap(a, b)
    ov.set_cluster_move(P.HoudayerMove(seed=5))
    want = CR.Accumulators(N)
    for m in range(3):
        ov.cluster_move()
        CR.launch(xa, ca, xb, cb, shape, bonds, a.schedule(), 0.0, 5, m, want, Sa, Sb)
    ov.reduce()
    rec = ov.reduce_clusters()
    want.assert_equal(rec)
    assert rec.abs_ds_sum.sum() > 0
    _check_states_and_suff(P, case, a, 1, xa, ca, Sa)
    _check_states_and_suff(P, case, b, 2, xb, cb, Sb)


# ---- 3. min_beta -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,L", [("cube", 6), ("square", 32)])
def test_chains_below_min_beta_are_untouched(P, family, L):
    case = CASES[family](P, L)
    a, b = _engine(P, case, 1), _engine(P, case, 2)
    shape, bonds = CR.lattice_shape(a.d, case[2]), CR.bonds_of(case[0])
    g = np.random.default_rng(L)
    ca, cb = g.permutation(N).astype(np.int64), g.permutation(N).astype(np.int64)
    xa, xb = g.integers(0, 2, size=(N, a.d)).astype(np.int64), g.integers(0, 2, size=(N, a.d)).astype(np.int64)
    _set(a, xa, ca); _set(b, xb, cb)
    xa0, xb0 = xa.copy(), xb.copy()
    Sa, Sb = _pair_sums(xa, shape, bonds), _pair_sums(xb, shape, bonds)
    betas = a.schedule()
    min_beta = float(betas[4])                           # chain 4 sits on the threshold and takes part
    ov = P.Overlap(a, b)
    ov.set_cluster_move(P.HoudayerMove(min_beta=min_beta, seed=SEED))
    ov.cluster_move()
    want = CR.Accumulators(N)
    CR.launch(xa, ca, xb, cb, shape, bonds, betas, min_beta, SEED, 0, want, Sa, Sb)
    ov.reduce()
    rec = ov.reduce_clusters()
    want.assert_equal(rec)
    assert rec.n.tolist() == [0] * 4 + [1] * 4 and not rec.passes_sum[:4].any() and not rec.k_sum[:4].any() and rec.size_sum[4:].all()
    for c in range(4):
        sa, sb = list(ca).index(c), list(cb).index(c)
        assert np.array_equal(xa[sa], xa0[sa]) and np.array_equal(xb[sb], xb0[sb])
    _check_states_and_suff(P, case, a, 1, xa, ca, Sa)
    _check_states_and_suff(P, case, b, 2, xb, cb, Sb)


# ---- 4. the scan loop --------------------------------------------------------------------------------------------------------------------
def _everything(eng):
    eng.reduce()
    return list(eng.states()) + list(eng.swap_acceptance()) + list(eng.round_trip()) + list(eng.energy_ac1()) + [eng.index_process()]


CLUSTER_FIELDS = ("n", "empty", "size_sum", "k_sum", "abs_ds_sum", "passes_sum")


@pytest.mark.parametrize("family,L", [("cube", 6), ("square", 32)])
def test_run_scans_equals_the_step_by_step_loop(P, family, L):
    """run_scans(1, 6) with every = 2: the move at scans 2, 4 and 6, after both swaps and ahead of the record"""
    case = CASES[family](P, L)
    a, b, a2, b2 = (_engine(P, case, s) for s in (3, 4, 3, 4))
    ov, ov2 = P.Overlap(a, b), P.Overlap(a2, b2)
    for o in (ov, ov2):
        o.set_cluster_move(P.HoudayerMove(every=2, seed=SEED))
    ov.run_scans(1, 6)
    for s in range(1, 7):
        a2.explore(s); a2.swap(s); b2.explore(s); b2.swap(s)
        if s % 2 == 0:
            ov2.cluster_move()
        ov2.record()
    for u, v in zip(_everything(a) + _everything(b), _everything(a2) + _everything(b2)):
        np.testing.assert_array_equal(np.asarray(u), np.asarray(v))
    rec, rec2 = ov.reduce(), ov2.reduce()
    for name in ("n", "hist", "link_n", "link_sum", "link_sum2"):
        assert np.array_equal(getattr(rec, name), getattr(rec2, name)), name
    cl, cl2 = ov.reduce_clusters(), ov2.reduce_clusters()
    for name in CLUSTER_FIELDS:
        assert np.array_equal(getattr(cl, name), getattr(cl2, name)), name
    assert rec.n.tolist() == [6] * N and cl.n.tolist() == [3] * N and cl.moves_launched == 3 == cl2.moves_launched and cl.size_sum.sum() > 0
    ov.reduce()                                          # reduce() zeroes the device's accumulators
    again = ov.reduce_clusters()
    assert all(not getattr(again, name).any() for name in CLUSTER_FIELDS) and again.moves_launched == 0


@pytest.mark.parametrize("family,L", [("cube", 6), ("square", 32)])
def test_the_move_reads_no_engine_rng_words(P, family, L):
    """run_scans with the move on and with it off leave both engines' RNG words equal, while the lattices differ.  Both geometries under
    CheckerboardMetropolis, whose every active site takes one draw whatever it decides: IsingMetropolis draws only where a flip lowers the
    density (pte_ising.hpp), so its stream position follows the states, which the move is there to change."""
    target = CASES[family](P, L)[0]
    case = (target, P.CheckerboardMetropolis(1), family == "cube")
    a, b, a3, b3 = (_engine(P, case, s) for s in (3, 4, 3, 4))
    ov, ov3 = P.Overlap(a, b), P.Overlap(a3, b3)
    ov.set_cluster_move(P.HoudayerMove(every=1, seed=SEED))
    ov.run_scans(1, 6)
    ov3.run_scans(1, 6)
    ov.reduce()
    assert ov.reduce_clusters().size_sum.sum() > 0
    assert not np.array_equal(a3.states()[0], a.states()[0]) and not np.array_equal(b3.states()[0], b.states()[0])
    assert np.array_equal(a3.states()[2], a.states()[2]) and np.array_equal(b3.states()[2], b.states()[2])


@pytest.mark.parametrize("family,L", [("cube", 6), ("square", 32)])
def test_every_0_leaves_each_engine_where_a_run_alone_would(P, family, L):
    """4.20's promise for the new code path: the move set and turned off, run_scans makes today's launches"""
    case = CASES[family](P, L)
    a, b, a2, b2 = (_engine(P, case, s) for s in (1, 2, 1, 2))
    ov = P.Overlap(a, b)
    ov.set_cluster_move(P.HoudayerMove(every=0, seed=SEED))
    ov.run_scans(1, 6)
    a2.run_scans(1, 6); b2.run_scans(1, 6)
    for side, twin in ((a, a2), (b, b2)):
        for u, v in zip(_everything(side), _everything(twin)):
            np.testing.assert_array_equal(np.asarray(u), np.asarray(v))
    assert ov.reduce().n.tolist() == [6] * N
    cl = ov.reduce_clusters()
    assert all(not getattr(cl, name).any() for name in CLUSTER_FIELDS) and cl.moves_launched == 0


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals(P):
    sq6 = _square(P, 6)
    ov6 = P.Overlap(_engine(P, sq6, 1, n=4), _engine(P, sq6, 2, n=4))
    with pytest.raises(P.PteError, match=r"pte_overlap_set_cluster_move: on the 2-D lattices the move runs where base_length % 32 == 0 \(got base_length 6\)"):
        ov6.set_cluster_move(P.HoudayerMove(seed=1))
    with pytest.raises(P.PteError, match=r"pte_overlap_cluster_move: the move was never set; call pte_overlap_set_cluster_move first"):
        ov6.cluster_move()
    case = _cube(P, 4)
    a, b = _engine(P, case, 1, n=4), _engine(P, case, 2, n=4)
    ov = P.Overlap(a, b)
    with pytest.raises(P.PteError, match=r"pte_overlap_cluster_move: the move was never set"):
        ov.cluster_move()
    with pytest.raises(P.PteError, match=r"pte_overlap_set_cluster_move: every must be >= 0 \(got -2\)"):
        ov._chk(ov.L.pte_overlap_set_cluster_move(ov.h, -2, 0.0, 1))
    with pytest.raises(P.PteError, match=r"pte_overlap_set_cluster_move: min_beta must be in \[0, 1\] \(got 1\.5\)"):
        ov._chk(ov.L.pte_overlap_set_cluster_move(ov.h, 1, 1.5, 1))
    with pytest.raises(P.PteError, match=r"pte_overlap_set_cluster_move: min_beta must be in \[0, 1\] \(got -?nan\)"):
        ov._chk(ov.L.pte_overlap_set_cluster_move(ov.h, 1, float("nan"), 1))
    with pytest.raises(P.PteError, match=r"the move was never set"):           # the refused calls left it unset
        ov.cluster_move()
    with pytest.raises(ValueError, match=r"HoudayerMove\(seed=None\) needs the seed of the run"):
        ov.set_cluster_move(P.HoudayerMove())
    ov.set_cluster_move(P.HoudayerMove(seed=2 ** 64 - 1))
    a.set_schedule([0.0, 0.25, 0.5, 1.0])
    with pytest.raises(P.PteError, match=r"pte_overlap_cluster_move: the two engines' schedules differ \(first at chain 1: 0\.25 and 0\.333"):
        ov.cluster_move()
    ov.reduce()
    assert not ov.reduce_clusters().n.any()
    b.set_schedule([0.0, 0.25, 0.5, 1.0])
    ov.cluster_move()
    ov.reduce()
    cl = ov.reduce_clusters()
    assert cl.n.tolist() == [1] * 4 and cl.betas.tolist() == [0.0, 0.25, 0.5, 1.0] and cl.moves_launched == 1


# ---- 6. physics, against enumeration -----------------------------------------------------------------------------------------------------
def _enumerated(beta, S):
    """the exact P(k), k = 0 .. 8, of two independent copies at inverse temperature beta on the 2 x 2 x 2 instance with pair sums S [256]"""
    w = np.exp(beta * (S - S.max()))
    p = w / w.sum()
    idx = np.arange(256)
    ham = np.array([[bin(i ^ j).count("1") for j in idx] for i in idx])
    pk = np.zeros(9)
    np.add.at(pk, ham.ravel(), np.outer(p, p).ravel())
    return pk


def test_overlap_distribution_with_the_move_against_enumeration(P):
    """pigeons_pair with HoudayerMove() on the 2 x 2 x 2 Edwards-Anderson instance of DESIGN 4.20's check: the move leaves pi x pi invariant, so
    <q^2> of every chain of the last round (1024 records) stays within 6 sqrt(2 Var(q^2) / 1024) of the enumerated value at that chain's beta.
    Measured deviations: DESIGN 4.21."""
    beta_t, n_rounds = 0.5, 10
    t = P.SpinGlass3DLogPotential.edwards_anderson(beta_t, 2, seed=1)
    pair = P.pigeons_pair(target=t, n_chains=10, n_rounds=n_rounds, explorer=P.CheckerboardMetropolis(3), show_report=False, cluster_move=P.HoudayerMove())
    assert len(pair.overlaps) == n_rounds == len(pair.clusters) and pair.cluster is pair.clusters[-1]
    assert [int(r.n[0]) for r in pair.clusters] == [2 ** k for k in range(1, n_rounds + 1)] == [r.moves_launched for r in pair.clusters]
    rec, cl = pair.overlap, pair.cluster
    assert rec.n.tolist() == [1024] * 10 and cl.n.tolist() == [1024] * 10 and np.array_equal(cl.betas, rec.betas)
    assert np.array_equal(cl.k_sum, rec.hist @ np.arange(9)), "the move and the record of a scan see the same t"
    assert np.all(cl.size_sum <= cl.k_sum) and np.all(cl.size_sum >= cl.n - cl.empty) and cl.abs_ds_sum.sum() > 0
    frac = cl.mean_fraction()
    assert np.all((frac > 0) & (frac <= 1))
    assert np.array_equal(pair.a.replicas.schedule(), pair.b.replicas.schedule())
    S = R3.all_pair_sums(t.bonds_x, t.bonds_y, t.bonds_z).astype(np.float64)
    q = rec.q_values()
    m = rec.moments()
    for c in range(10):
        pk = _enumerated(rec.betas[c] * beta_t, S)
        q2 = float(pk @ q ** 2)
        var = float(pk @ q ** 4) - q2 * q2
        bound = 6.0 * np.sqrt(2.0 * var / 1024.0)
        print("chain %d beta %.4f: q2 measured %.4f exact %.4f deviation %+.4f bound %.4f fraction %.3f" % (c, rec.betas[c], m["q2"][c], q2, m["q2"][c] - q2, bound, frac[c]))
        assert abs(m["q2"][c] - q2) <= bound, (c, m["q2"][c], q2, bound)
    for each in (pair.a, pair.b):                                          # both stay ordinary PTs
        assert np.isfinite(P.stepping_stone(each)) and P.n_round_trips(each) >= 0
        assert abs(P.stepping_stone(each) - R3.exact(beta_t, t.bonds_x, t.bonds_y, t.bonds_z)) < 0.5
