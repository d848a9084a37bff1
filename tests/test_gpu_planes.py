"""The plane autocorrelation of a lattice pair on the device (k_overlap_planes: pigeons.jl_amd/csrc/pte_overlap_planes.hpp; pte_overlap_*planes*:
include/pte.h) against its restatement (tests/planes_ref.py): on lattices of four densities of differing sites, on special
states with closed forms, through the scan loop, beside the cluster move, through its refusals, and against enumeration.

Every accumulator is an integer and is compared exactly.  The two statistical checks, the last, are held to bands computed from the
enumeration and from the i.i.d. reference (six standard errors of 1024 records with a factor 2 on the variance for the correlation between
consecutive scans, as DESIGN 4.20's), not from the run."""
import numpy as np
import pytest

import lattice3d_ref as R3
import overlap_ref as R
import planes_ref as PR

pytestmark = pytest.mark.gpu

OVERLAP_FIELDS = ("n", "hist", "link_n", "link_sum", "link_sum2")


@pytest.fixture(scope="module")
def P():
    import pigeons_amd
    return pigeons_amd


def _rec(P):
    return [P.round_trip, P.index_process, P.log_sum_ratio, P.swap_acceptance_pr, P.energy_ac1]


def _cube(P, L, beta=0.8):
    return P.SpinGlass3DLogPotential.edwards_anderson(beta, L, seed=100 + L), P.CheckerboardMetropolis(1), True


def _square(P, L, beta=0.8):
    return P.SpinGlassLogPotential.edwards_anderson(beta, L, seed=200 + L), P.IsingMetropolis(1), False


def _ising(P, L):
    return P.IsingLogPotential(0.4, L), P.IsingMetropolis(1), False


CASES = {"cube": _cube, "square": _square, "ising": _ising}


def _engine(P, case, N, seed, n_rounds=4):
    target, explorer, _ = case
    return P.PT(P.Inputs(target=target, n_chains=N, n_rounds=n_rounds, seed=seed, explorer=explorer, show_report=False, record=_rec(P))).replicas


def _pair(P, family, L, N, seeds=(1, 2), planes=True):
    case = CASES[family](P, L)
    a, b = _engine(P, case, N, seeds[0]), _engine(P, case, N, seeds[1])
    ov = P.Overlap(a, b)
    if planes:
        ov.set_planes()
    return a, b, ov, R.lattice_shape(a.d, case[2])


def _set(eng, x, chain):
    eng.set_states(x, chain, None)
    x1, c1, _ = eng.states()
    assert np.array_equal(x1, x) and np.array_equal(c1, chain)


def _everything(eng):
    eng.reduce()
    return list(eng.states()) + list(eng.swap_acceptance()) + list(eng.round_trip()) + list(eng.energy_ac1()) + [eng.index_process()]


# ---- 1. record() against the restatement ------------------------------------------------------------------------------------------------
# the cube: L = 2 r = 1 is its own mirror, sixteen rows per word; 4; 6 and 10 rows straddle words, ragged last word; 16; 32 whole-word rows and
# the zero-shift mask, sixteen rows per lane.  The square: 32 a row is a word; 64; 96 W = 3, 63 lanes take the words; 256 the largest d, 32 rows
# per lane and four columns per output lane.  The Ising family at L = 32.
RECORD_CASES = [("cube", 2, 5), ("cube", 4, 5), ("cube", 6, 5), ("cube", 10, 5), ("cube", 16, 5), ("cube", 32, 3),
                ("square", 32, 5), ("square", 64, 5), ("square", 96, 5), ("square", 256, 2), ("ising", 32, 5)]


@pytest.mark.parametrize("family,L,N", RECORD_CASES)
def test_record_equals_the_restatement(P, family, L, N):
    """four densities of differing sites (0.5, 0.1, 0.9, striped), each recorded twice with a relabelling of the chains in between"""
    a, b, ov, shape = _pair(P, family, L, N)
    d = a.d
    assert (ov.n_axes, ov.base_length, ov.planes_on()) == (len(shape), L, True)
    g = np.random.default_rng(1000 * L + N)
    want, want_overlap = PR.Accumulators(N, shape), R.Accumulators(N, d)
    for trial in range(4):
        xa, xb = PR.states_of_density(g, N, d, shape, trial)
        ca, cb = g.permutation(N).astype(np.int64), g.permutation(N).astype(np.int64)
        _set(a, xa, ca); _set(b, xb, cb)
        ov.record()
        want.record(xa, ca, xb, cb); want_overlap.record(xa, ca, xb, cb, shape, True)
        # every slot of both engines handed another chain, independently
        ca, cb = (ca + 1) % N, g.permutation(N).astype(np.int64)
        a.set_states(None, ca, None); b.set_states(None, cb, None)
        ov.record()
        want.record(xa, ca, xb, cb); want_overlap.record(xa, ca, xb, cb, shape, True)
    rec = ov.reduce()
    want.assert_equal(rec)
    want_overlap.assert_equal(rec)                           # the first kernel's accumulators are what they are without the second
    assert rec.plane_n.tolist() == [8] * N == rec.n.tolist() and rec.plane_corr.shape == (N, len(shape), L)
    PR.hist_identity(rec)
    M = d // L
    assert np.all(rec.plane_corr == rec.plane_corr[:, :, (-np.arange(L)) % L])                      # C(r) = C(L - r)
    assert np.all(rec.plane_corr[:, :, :1] >= np.abs(rec.plane_corr)) and rec.plane_corr.max() <= 8 * L * M * M
    chi0 = rec.chi_sg(0)
    np.testing.assert_allclose(chi0, np.repeat((d * rec.moments()["q2"])[:, None], len(shape), axis=1), rtol=1e-12)   # chi_SG(0) = d <q^2>
    ov.close()
    for eng in (a, b):                                       # destroying the recorder leaves both engines usable
        eng.run_scans(1, 1)


# ---- 2. special states ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,L", [("cube", 6), ("square", 32)])
def test_special_states(P, family, L):
    """chain 0: equal lattices, chain 1: the complement -> C(r) = L M^2 for all r; chains 2 and 3: one differing site, site 0 and site d - 1
    (the last bit before the padding) -> C(0) = (L - 1) M^2 + (M - 2)^2, C(r != 0) = (L - 2) M^2 + 2 M (M - 2)"""
    N = 4
    a, b, ov, shape = _pair(P, family, L, N)
    d = a.d
    M = d // L
    g = np.random.default_rng(L)
    xa, ca = g.integers(0, 2, size=(N, d)).astype(np.float64), g.permutation(N).astype(np.int64)
    cb = g.permutation(N).astype(np.int64)
    xb = np.zeros_like(xa)
    for slot_b, c in enumerate(cb):
        s = xa[list(ca).index(c)].copy()
        if c == 1:
            s = 1.0 - s
        elif c == 2:
            s[0] = 1.0 - s[0]
        elif c == 3:
            s[d - 1] = 1.0 - s[d - 1]
        xb[slot_b] = s
    _set(a, xa, ca); _set(b, xb, cb)
    ov.record()
    rec = ov.reduce()
    assert rec.plane_n.tolist() == [1] * N
    assert np.all(rec.plane_corr[:2] == L * M * M)
    assert np.all(rec.plane_corr[2:, :, 0] == (L - 1) * M * M + (M - 2) ** 2)
    assert np.all(rec.plane_corr[2:, :, 1:] == (L - 2) * M * M + 2 * M * (M - 2))
    PR.hist_identity(rec)
    cl = rec.correlation_length()
    assert cl["chi0"][:2].tolist() == [d, d] and cl["chi_kmin"][:2].tolist() == [0.0, 0.0] and np.all(np.isnan(cl["xi"][:2]))
    assert np.all(cl["xi"][2:] > 0) and np.all(cl["xi_over_L"][2:] == cl["xi"][2:] / L)


@pytest.mark.parametrize("family,L", [("cube", 32), ("square", 64)])
def test_the_complement_where_every_plane_count_is_at_its_maximum(P, family, L):
    N = 2
    a, b, ov, shape = _pair(P, family, L, N)
    d = a.d
    M = d // L
    g = np.random.default_rng(L)
    xa = g.integers(0, 2, size=(N, d)).astype(np.float64)
    chain = np.arange(N, dtype=np.int64)
    _set(a, xa, chain); _set(b, (1.0 - xa)[::-1].copy(), chain[::-1].copy())   # chain c sits in slot N - 1 - c of b
    ov.record()
    rec = ov.reduce()
    assert np.all(rec.plane_corr == L * M * M) and rec.hist[:, d].tolist() == [1] * N
    PR.hist_identity(rec)


# ---- 3. off unless asked for --------------------------------------------------------------------------------------------------------------
def test_off_by_default(P):
    from pigeons_amd.engine import _ip
    a, b, ov, shape = _pair(P, "cube", 6, 4, planes=False)
    assert (ov.n_axes, ov.base_length, ov.planes_on()) == (3, 6, False)
    ov.run_scans(1, 3)
    rec = ov.reduce()
    assert rec.n.tolist() == [3] * 4 and rec.plane_n is None and rec.plane_corr is None and rec.chi_sg() is None and rec.correlation_length() is None
    plane_n, plane_corr = np.full(4, -1, dtype=np.int64), np.full((4, 3, 6), -1, dtype=np.int64)
    assert ov.L.pte_overlap_planes_get(ov.h, _ip(plane_n), _ip(plane_corr)) == 0
    assert not plane_n.any() and not plane_corr.any()
    assert ov.L.pte_overlap_planes_get(ov.h, None, None) == 0                 # NULLs are skipped
    ov.set_planes(False)                                                       # off stays off
    ov.record()
    assert ov.reduce().plane_corr is None


# ---- 4. reading only --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,L", [("cube", 6), ("square", 32)])
def test_the_recorder_only_reads(P, family, L):
    """after run_scans(1, 6) with the feature on, the five accumulators of 4.20 and both engines' states, chain maps, RNG words and reduced
    recorders equal those of a twin pair with it off"""
    N = 6
    a, b, ov, _ = _pair(P, family, L, N)
    a2, b2, ov2, _ = _pair(P, family, L, N, planes=False)
    ov.run_scans(1, 6)
    ov2.run_scans(1, 6)
    for side, twin in ((a, a2), (b, b2)):
        for u, v in zip(_everything(side), _everything(twin)):
            np.testing.assert_array_equal(np.asarray(u), np.asarray(v))
    rec, rec2 = ov.reduce(), ov2.reduce()
    for name in OVERLAP_FIELDS:
        assert np.array_equal(getattr(rec, name), getattr(rec2, name)), name
    assert rec.plane_n.tolist() == [6] * N and rec2.plane_n is None and rec.hist[:, 0].sum() < 6 * N
    PR.hist_identity(rec)


# ---- 5. run_scans equals the step-by-step loop; switching on in the middle; reduce() zeroes --------------------------------------------------
@pytest.mark.parametrize("family,L", [("cube", 6), ("square", 32)])
def test_run_scans_equals_the_step_by_step_loop(P, family, L):
    N = 6
    a, b, ov, shape = _pair(P, family, L, N, seeds=(3, 4))
    a2, b2, ov2, _ = _pair(P, family, L, N, seeds=(3, 4))
    ov.run_scans(1, 5)
    want = PR.Accumulators(N, shape)
    for s in range(1, 6):
        a2.explore(s); a2.swap(s); b2.explore(s); b2.swap(s)
        ov2.record()
        (xa, ca, _), (xb, cb, _) = a2.states(), b2.states()
        want.record(xa, ca, xb, cb)
    rec, rec2 = ov.reduce(), ov2.reduce()
    for name in OVERLAP_FIELDS + ("plane_n", "plane_corr"):
        assert np.array_equal(getattr(rec, name), getattr(rec2, name)), name
    want.assert_equal(rec)
    assert rec.plane_n.tolist() == [5] * N
    for u, v in zip(a.states() + b.states(), a2.states() + b2.states()):
        assert np.array_equal(u, v)
    again = ov.reduce()                                      # reduce() zeroes the device's accumulators; the feature is still on
    assert again.plane_n is not None and not again.plane_n.any() and not again.plane_corr.any() and not again.n.any()


def test_switching_on_after_two_of_five_records(P):
    N = 5
    a, b, ov, shape = _pair(P, "cube", 6, N, planes=False)
    want = PR.Accumulators(N, shape)
    for s in range(1, 6):
        if s == 3:
            ov.set_planes(True)
        ov.run_scans(s, 1)
        if s >= 3:
            (xa, ca, _), (xb, cb, _) = a.states(), b.states()
            want.record(xa, ca, xb, cb)
    rec = ov.reduce()
    assert rec.plane_n.tolist() == [3] * N and rec.n.tolist() == [5] * N
    want.assert_equal(rec)
    ov.set_planes(False)                                     # and off again: the next round's record holds none
    ov.run_scans(6, 2)
    rec = ov.reduce()
    assert rec.n.tolist() == [2] * N and rec.plane_corr is None


# ---- 6. beside the cluster move -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,L", [("cube", 6), ("square", 32)])
def test_with_the_cluster_move_the_records_are_those_of_the_post_move_states(P, family, L):
    N = 5
    a, b, ov, shape = _pair(P, family, L, N)
    ov.set_cluster_move(P.HoudayerMove(every=1, seed=11))
    want, want_overlap = PR.Accumulators(N, shape), R.Accumulators(N, a.d)
    for s in range(1, 5):
        ov.run_scans(s, 1)                                   # explore, swap, the move, then the records: the states left are those recorded
        (xa, ca, _), (xb, cb, _) = a.states(), b.states()
        want.record(xa, ca, xb, cb); want_overlap.record(xa, ca, xb, cb, shape, True)
    rec = ov.reduce()
    want.assert_equal(rec)
    want_overlap.assert_equal(rec)
    cl = ov.reduce_clusters()
    assert cl.moves_launched == 4 and cl.size_sum.sum() > 0
    PR.hist_identity(rec)


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals(P):
    a, b, ov, _ = _pair(P, "square", 6, 4, planes=False)
    assert (ov.n_axes, ov.base_length, ov.n_links) == (0, 6, 0)
    for on in (True, False):
        with pytest.raises(P.PteError, match=r"pte_overlap_set_planes: on the 2-D lattices the plane sums are recorded where base_length % 32 == 0 "
                                             r"\(got base_length 6\)"):
            ov.set_planes(on)
    ov.record()
    rec = ov.reduce()
    assert rec.n.tolist() == [1] * 4 and rec.plane_corr is None
    created = []
    real = P.overlap.PT

    def counting(*args, **kw):
        created.append(1)
        return real(*args, **kw)
    P.overlap.PT = counting
    try:
        with pytest.raises(NotImplementedError, match=r"pigeons_pair: wave_vector=True runs on the cube and on the 2-D lattices whose base_length is a multiple "
                                                      r"of 32 \(got base_length 6\)"):
            P.pigeons_pair(target=P.SpinGlassLogPotential.edwards_anderson(1.0, 6), n_chains=4, n_rounds=2, explorer=P.IsingMetropolis(1), show_report=False,
                           wave_vector=True)
    finally:
        P.overlap.PT = real
    assert created == []                                     # before any device work


# ---- 8. physics ---------------------------------------------------------------------------------------------------------------------------
N_ROUNDS = 10


def _c_of_every_t():
    """C [256][3][2] of the 2 x 2 x 2 lattice for every set t of differing sites, t = the bits of its index"""
    zero = np.zeros(8, dtype=np.int64)
    return np.array([PR.plane_corr(zero, bits, (2, 2, 2)) for bits in R3.all_states()], dtype=np.float64)


def test_plane_correlations_against_enumeration(P):
    """pigeons_pair(wave_vector=True) on the 2 x 2 x 2 Edwards-Anderson instance: for every chain of the last round (1024 records) the means
    of C_axis(0) and C_axis(1) within 6 sqrt(2 Var / 1024) of their values over the 256 x 256 enumerated pair states at that chain's beta.
    Measured deviations: DESIGN 4.22."""
    beta_t = 0.5
    t = P.SpinGlass3DLogPotential.edwards_anderson(beta_t, 2, seed=1)
    pair = P.pigeons_pair(target=t, n_chains=10, n_rounds=N_ROUNDS, explorer=P.CheckerboardMetropolis(3), show_report=False, wave_vector=True)
    assert len(pair.overlaps) == N_ROUNDS and [int(r.plane_n[0]) for r in pair.overlaps] == [2 ** k for k in range(1, N_ROUNDS + 1)]
    rec = pair.overlap
    assert rec.plane_n.tolist() == [1024] * 10 == rec.n.tolist() and rec.plane_corr.shape == (10, 3, 2)
    PR.hist_identity(rec)
    S = R3.all_pair_sums(t.bonds_x, t.bonds_y, t.bonds_z).astype(np.float64)
    C = _c_of_every_t()
    idx = np.arange(256)
    xor = idx[:, None] ^ idx[None, :]                          # the enumeration's own bookkeeping: the pair (i, j) differs at the bits of i ^ j
    worst = 0.0
    for c in range(10):
        w = np.exp(rec.betas[c] * beta_t * (S - S.max()))
        p = w / w.sum()
        pt = np.zeros(256)
        np.add.at(pt, xor.ravel(), np.outer(p, p).ravel())
        for ax in range(3):
            for r in range(2):
                mean = float(pt @ C[:, ax, r])
                var = float(pt @ C[:, ax, r] ** 2) - mean * mean
                bound = 6.0 * np.sqrt(2.0 * var / 1024.0)
                got = int(rec.plane_corr[c, ax, r]) / 1024.0
                print("chain %d beta %.4f axis %d r %d: measured %.4f exact %.4f deviation %+.4f bound %.4f" % (c, rec.betas[c], ax, r, got, mean, got - mean, bound))
                worst = max(worst, abs(got - mean) / bound)
                assert abs(got - mean) <= bound, (c, ax, r, got, mean, bound)
        if c == 0:                                              # the i.i.d. reference: <C(0)> = d, <C(1)> = 0
            assert abs(float(pt @ C[:, 0, 0]) - 8.0) < 1e-12 and abs(float(pt @ C[:, 0, 1])) < 1e-12
    print("largest |deviation| / bound %.3f" % worst)
    cl = rec.correlation_length()
    assert np.all(np.isfinite(cl["chi0"])) and np.all(cl["chi0"] > 0)


def test_the_reference_chain_of_a_cube_is_uncorrelated(P):
    """chain 0 (beta 0) of a cube with L = 4 holds two i.i.d. uniform copies: every q_i is a fair sign, Q[p] a sum of M = 16 of them, so
    <C_axis(r)> = d delta_r0 with Var C(0) = L (2 M^2 - 2 M), Var C(L / 2) = 2 L M^2, Var C(r) = L M^2 otherwise; the means of 1024 records
    within six standard errors, the variance doubled for the correlation between consecutive scans.  Measured deviations: DESIGN 4.22."""
    L = 4
    d, M = L ** 3, L ** 2
    t = P.SpinGlass3DLogPotential.edwards_anderson(0.5, L, seed=1)
    pair = P.pigeons_pair(target=t, n_chains=10, n_rounds=N_ROUNDS, explorer=P.CheckerboardMetropolis(3), show_report=False, wave_vector=True)
    rec = pair.overlap
    assert rec.betas[0] == 0.0 and int(rec.plane_n[0]) == 1024 and rec.plane_corr.shape == (10, 3, L)
    PR.hist_identity(rec)
    for ax in range(3):
        for r in range(L):
            var = L * (2 * M * M - 2 * M) if r == 0 else 2 * L * M * M if 2 * r == L else L * M * M
            mean = d if r == 0 else 0
            bound = 6.0 * np.sqrt(2.0 * var / 1024.0)
            got = int(rec.plane_corr[0, ax, r]) / 1024.0
            print("axis %d r %d: measured %.3f exact %d deviation %+.3f bound %.3f" % (ax, r, got, mean, got - mean, bound))
            assert abs(got - mean) <= bound, (ax, r, got, mean, bound)
