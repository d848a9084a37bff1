"""The replica-overlap recorder on the device (k_overlap: pigeons.jl_amd/csrc/pte_overlap.hpp; pte_overlap_*: include/pte.h)
against its restatement (tests/overlap_ref.py), on special states, through the scan loop, through its refusals, and against the enumerated
overlap distribution of a 2 x 2 x 2 instance.

Every accumulator is an integer and is compared exactly.  The one statistical check, the last, is held to a band computed from the
enumeration (six standard errors of 1024 records with a factor 2 on the variance for the correlation between consecutive scans), not from
the run."""
import numpy as np
import pytest

import lattice3d_ref as R3
import overlap_ref as R

pytestmark = pytest.mark.gpu


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


def _engine(P, case, N, seed, n_rounds=4):
    target, explorer, _ = case
    return P.PT(P.Inputs(target=target, n_chains=N, n_rounds=n_rounds, seed=seed, explorer=explorer, show_report=False, record=_rec(P))).replicas


def _random_states(eng, g):
    x = g.integers(0, 2, size=(eng.N, eng.d)).astype(np.float64)
    chain = g.permutation(eng.N).astype(np.int64)
    eng.set_states(x, chain, None)
    x1, c1, _ = eng.states()
    assert np.array_equal(x1, x) and np.array_equal(c1, chain)
    return x, chain


# ---- 1. record() against the restatement ------------------------------------------------------------------------------------------------
# the cube: L = 2 sixteen rows per word; 4; 6 rows straddle words; 10: 1000 bits, ragged last word; 16; 32: sixteen words per lane, whole-word
# rows.  The square: 6 no link overlap; 32 a row is a word, the x-wrap inside it; 64 the carry across a row's two words; 96 three words per
# row, ragged lane load.  The Ising family at L = 32.
RECORD_CASES = [("cube", 2, 5), ("cube", 4, 5), ("cube", 6, 5), ("cube", 10, 5), ("cube", 16, 5), ("cube", 32, 3),
                ("square", 6, 5), ("square", 32, 5), ("square", 64, 5), ("square", 96, 5), ("ising", 32, 5)]


@pytest.mark.parametrize("family,L,N", RECORD_CASES)
def test_record_equals_the_restatement(P, family, L, N):
    case = {"cube": _cube, "square": _square, "ising": _ising}[family](P, L)
    a, b = _engine(P, case, N, 1), _engine(P, case, N, 2)
    d = a.d
    shape = R.lattice_shape(d, case[2])
    link = case[2] or L % 32 == 0
    ov = P.Overlap(a, b)
    assert (ov.N, ov.d, ov.n_links) == (N, d, (len(shape) * d) if link else 0)
    g = np.random.default_rng(1000 * L + N)
    (xa, ca), (xb, cb) = _random_states(a, g), _random_states(b, g)
    want = R.Accumulators(N, d)
    ov.record()
    want.record(xa, ca, xb, cb, shape, link)
    # every slot of both engines handed another chain, independently
    ca, cb = (ca + 1) % N, g.permutation(N).astype(np.int64)
    a.set_states(None, ca, None); b.set_states(None, cb, None)
    ov.record()
    want.record(xa, ca, xb, cb, shape, link)
    rec = ov.reduce()
    want.assert_equal(rec)
    assert rec.n.tolist() == [2] * N and rec.link_n.tolist() == [2 if link else 0] * N and rec.hist.sum() == 2 * N
    assert (rec.dim, rec.n_links) == (d, ov.n_links) and np.array_equal(rec.betas, a.schedule())
    assert (rec.moments()["ql"] is None) == (not link)
    if d >= 64:
        assert rec.hist[:, 1:d].sum() == 2 * N, "random lattices: no record in the bins k = 0 and k = d"
    ov.close()
    for eng in (a, b):                                   # destroying the recorder leaves both engines usable
        eng.run_scans(1, 1)


# ---- 2. special states ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,L", [("cube", 6), ("square", 32)])
def test_special_states(P, family, L):
    """chain 0: equal lattices -> (0, 0); chain 1: the complement -> (d, 0); chains 2 and 3: one differing site, site 0 and site d - 1 (the
    last bit before the padding) -> (1, 6) on the cube, (1, 4) on the square"""
    case = {"cube": _cube, "square": _square}[family](P, L)
    N = 4
    a, b = _engine(P, case, N, 1), _engine(P, case, N, 2)
    d, one = a.d, 6 if case[2] else 4
    g = np.random.default_rng(L)
    xa, ca = _random_states(a, g)
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
    b.set_states(xb, cb, None)
    ov = P.Overlap(a, b)
    ov.record()
    rec = ov.reduce()
    ks, kls = [0, d, 1, 1], [0, 0, one, one]
    for c in range(N):
        assert rec.hist[c, ks[c]] == 1 and rec.hist[c].sum() == 1 and rec.n[c] == 1, c
        assert (rec.link_n[c], rec.link_sum[c], rec.link_sum2[c]) == (1, kls[c], kls[c] ** 2), c
    m = rec.moments()
    assert m["q2"].tolist() == [1.0, 1.0, (1.0 - 2.0 / d) ** 2, (1.0 - 2.0 / d) ** 2] and m["ql"][0] == 1.0 and m["ql"][1] == 1.0


# ---- 3. same seeds ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,L", [("cube", 6), ("square", 32)])
def test_same_seeds_overlap_completely(P, family, L):
    case = {"cube": _cube, "square": _square}[family](P, L)
    N = 5
    a, b = _engine(P, case, N, 7), _engine(P, case, N, 7)
    ov = P.Overlap(a, b)
    ov.run_scans(1, 8)
    rec = ov.reduce()
    assert rec.hist[:, 0].tolist() == [8] * N and rec.hist.sum() == 8 * N and rec.n.tolist() == [8] * N
    assert rec.link_n.tolist() == [8] * N and rec.link_sum.tolist() == [0] * N and rec.link_sum2.tolist() == [0] * N
    assert a.states()[0].any(), "the lattices did move"


# ---- 4. reading only --------------------------------------------------------------------------------------------------------------------
def _everything(eng):
    eng.reduce()
    return list(eng.states()) + list(eng.swap_acceptance()) + list(eng.round_trip()) + list(eng.energy_ac1()) + [eng.index_process()]


@pytest.mark.parametrize("family,L", [("cube", 6), ("square", 32)])
def test_the_recorder_only_reads(P, family, L):
    """after Overlap.run_scans(1, 6) each engine's states, chain maps, RNG words and reduced recorders are those of a twin run alone"""
    case = {"cube": _cube, "square": _square}[family](P, L)
    N = 6
    a, b, a2, b2 = (_engine(P, case, N, s) for s in (1, 2, 1, 2))
    ov = P.Overlap(a, b)
    ov.run_scans(1, 6)
    a2.run_scans(1, 6); b2.run_scans(1, 6)
    for pair_side, twin in ((a, a2), (b, b2)):
        for u, v in zip(_everything(pair_side), _everything(twin)):
            np.testing.assert_array_equal(np.asarray(u), np.asarray(v))
    rec = ov.reduce()
    assert rec.n.tolist() == [6] * N and rec.hist[:, 0].sum() < 6 * N, "different seeds: the runs are not copies of each other"
    assert a.swap_acceptance()[1].sum() > 0 and a.energy_ac1()[1].tolist() == [6] * N


# ---- 5. run_scans equals the step-by-step loop --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,L", [("cube", 6), ("square", 32)])
def test_run_scans_equals_the_step_by_step_loop(P, family, L):
    case = {"cube": _cube, "square": _square}[family](P, L)
    N = 6
    a, b, a2, b2 = (_engine(P, case, N, s) for s in (3, 4, 3, 4))
    ov, ov2 = P.Overlap(a, b), P.Overlap(a2, b2)
    ov.run_scans(1, 5)
    for s in range(1, 6):
        a2.explore(s); a2.swap(s); b2.explore(s); b2.swap(s)
        ov2.record()
    rec, rec2 = ov.reduce(), ov2.reduce()
    for name in ("n", "hist", "link_n", "link_sum", "link_sum2"):
        assert np.array_equal(getattr(rec, name), getattr(rec2, name)), name
    assert rec.n.tolist() == [5] * N and rec.link_n.tolist() == [5] * N and rec.link_sum.sum() > 0
    for u, v in zip(a.states() + b.states(), a2.states() + b2.states()):
        assert np.array_equal(u, v)
    again = ov.reduce()                                  # reduce() zeroes the device's accumulators
    assert all(not getattr(again, name).any() for name in ("n", "hist", "link_n", "link_sum", "link_sum2"))


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------------
def test_create_refusals(P):
    Lb = P._lib
    cube4, cube6, sq32, isg32 = _cube(P, 4), _cube(P, 6), _square(P, 32), _ising(P, 32)
    a = _engine(P, cube4, 4, 1)
    with pytest.raises(P.PteError, match=r"pte_overlap_create: a and b are the same engine"):
        P.Overlap(a, a)
    mvn = [P.PT(P.Inputs(target=P.toy_mvn_target(4), n_chains=4, n_rounds=2, seed=s, show_report=False)).replicas for s in (1, 2)]
    with pytest.raises(P.PteError, match=r"pte_overlap_create: engine a has target 0; the overlap is recorded on the lattice targets"):
        P.Overlap(*mvn)
    with pytest.raises(P.PteError, match=r"engine b has target 0"):
        P.Overlap(a, mvn[1])
    with pytest.raises(P.PteError, match=r"the engines differ: target 12 and 3, dim 1024 and 1024, 4 and 4 chains"):
        P.Overlap(_engine(P, sq32, 4, 1), _engine(P, isg32, 4, 2))
    with pytest.raises(P.PteError, match=r"the engines differ: target 13 and 13, dim 64 and 216, 4 and 4 chains"):
        P.Overlap(a, _engine(P, cube6, 4, 2))
    with pytest.raises(P.PteError, match=r"the engines differ: target 13 and 13, dim 64 and 64, 4 and 5 chains"):
        P.Overlap(a, _engine(P, cube4, 5, 2))
    ising = dict(target=Lb.TARGET_ISING, dim=1024, explorer=Lb.EXPLORER_ISING_METROPOLIS, target_params=[0.4])
    shards = [P.Engine(n_chains=4, rank=0, world_size=2, seed=s, **ising) for s in (1, 2)]
    with pytest.raises(P.PteError, match=r"world_size must be 1 \(got 2 and 2\)"):
        P.Overlap(*shards)
    legs = [P.Engine(n_chains=3, n_chains_variational=3, seed=s, **ising) for s in (1, 2)]
    with pytest.raises(P.PteError, match=r"n_chains_variational must be 0 \(got 3 and 3\)"):
        P.Overlap(*legs)
    bare = P.Engine(n_chains=4, target=Lb.TARGET_SPIN_GLASS_3D, dim=64, explorer=Lb.EXPLORER_CHECKERBOARD_METROPOLIS, target_params=[0.8], seed=2)
    with pytest.raises(P.PteError, match=r"pte_overlap_create: engine b has no bonds yet; call pte_set_target_spin_glass_3d first"):
        P.Overlap(a, bare)
    with pytest.raises(P.PteError, match=r"the engines' bonds differ \(first at word \d+ of the device planes\)"):
        P.Overlap(a, _engine(P, _cube(P, 4, seed=5), 4, 2))
    with pytest.raises(P.PteError, match=r"the engines' bonds differ \(first at site \d+ of the device planes\)"):
        P.Overlap(_engine(P, sq32, 4, 1), _engine(P, _square(P, 32, seed=5), 4, 2))
    import torch
    if torch.cuda.device_count() >= 2:                   # (two devices: the one refusal a single-GPU machine cannot reach)
        other = P.PT(P.Inputs(target=cube4[0], n_chains=4, n_rounds=2, seed=2, explorer=cube4[1], show_report=False, device=1)).replicas
        with pytest.raises(P.PteError, match=r"the engines are on different devices \(0 and 1\)"):
            P.Overlap(a, other)
    # N (d + 1) 8 bytes = 4096 x 65537 x 8 > 2 GiB
    big = [P.Engine(n_chains=4096, seed=s, target=Lb.TARGET_ISING, dim=65536, explorer=Lb.EXPLORER_ISING_METROPOLIS, target_params=[0.4],
                    max_scans_per_round=2) for s in (1, 2)]
    with pytest.raises(P.PteError, match=r"the histograms of 4096 chains x 65537 bins take 2147516416 bytes, more than the 2 GiB"):
        P.Overlap(*big)
    ok = P.Overlap(a, _engine(P, cube4, 4, 2))           # and the pair that is none of the above
    ok.record()
    assert ok.reduce().n.tolist() == [1] * 4


def test_record_and_run_scans_refuse_unequal_schedules(P):
    case = _cube(P, 4)
    a, b = _engine(P, case, 4, 1), _engine(P, case, 4, 2)
    ov = P.Overlap(a, b)
    a.set_schedule([0.0, 0.25, 0.5, 1.0])
    with pytest.raises(P.PteError, match=r"pte_overlap_record: the two engines' schedules differ \(first at chain 1: 0\.25 and 0\.333"):
        ov.record()
    with pytest.raises(P.PteError, match=r"pte_overlap_run_scans: the two engines' schedules differ"):
        ov.run_scans(1, 2)
    assert not ov.reduce().n.any()
    b.set_schedule([0.0, 0.25, 0.5, 1.0])
    ov.run_scans(1, 2)
    rec = ov.reduce()
    assert rec.n.tolist() == [2] * 4 and rec.betas.tolist() == [0.0, 0.25, 0.5, 1.0]


# ---- 7. physics, against enumeration -------------------------------------------------------------------------------------------------------
def _enumerated(beta, S):
    """the exact P(k), k = 0 .. 8, of two independent copies at inverse temperature beta on the 2 x 2 x 2 instance with pair sums S [256]"""
    w = np.exp(beta * (S - S.max()))
    p = w / w.sum()
    idx = np.arange(256)
    ham = np.array([[bin(i ^ j).count("1") for j in idx] for i in idx])
    pk = np.zeros(9)
    np.add.at(pk, ham.ravel(), np.outer(p, p).ravel())
    return pk


def test_overlap_distribution_against_enumeration(P):
    """pigeons_pair on the 2 x 2 x 2 Edwards-Anderson instance: <q^2> of every chain of the last round (1024 records) within
    6 sqrt(2 Var(q^2) / 1024) of the enumerated value at that chain's beta.  Measured deviations: DESIGN 4.20."""
    beta_t, n_rounds = 0.5, 10
    t = P.SpinGlass3DLogPotential.edwards_anderson(beta_t, 2, seed=1)
    pair = P.pigeons_pair(target=t, n_chains=10, n_rounds=n_rounds, explorer=P.CheckerboardMetropolis(3), show_report=False)
    assert len(pair.overlaps) == n_rounds and pair.overlap is pair.overlaps[-1]
    assert [int(r.n[0]) for r in pair.overlaps] == [2 ** k for k in range(1, n_rounds + 1)]
    rec = pair.overlap
    assert rec.hist.sum(axis=1).tolist() == [1024] * 10 and rec.n.tolist() == [1024] * 10 and rec.link_n.tolist() == [1024] * 10
    assert (rec.dim, rec.n_links) == (8, 24)
    assert np.array_equal(pair.a.replicas.schedule(), pair.b.replicas.schedule())
    assert np.array_equal(pair.a.shared.tempering.schedule.grids, pair.b.shared.tempering.schedule.grids)
    assert rec.betas[0] == 0.0 and rec.betas[-1] == 1.0 and np.all(np.diff(rec.betas) > 0)
    S = R3.all_pair_sums(t.bonds_x, t.bonds_y, t.bonds_z).astype(np.float64)
    q = rec.q_values()
    m = rec.moments()
    for c in range(10):
        pk = _enumerated(rec.betas[c] * beta_t, S)
        q2 = float(pk @ q ** 2)
        var = float(pk @ q ** 4) - q2 * q2
        if c == 0:
            assert abs(q2 - 0.125) < 1e-15                                 # the i.i.d. reference: q is the mean of 8 fair signs
        if c == 9:
            assert abs(q2 - 0.3836) < 5e-5 and abs(var - 0.1272) < 5e-5   # the figures of the specification
        bound = 6.0 * np.sqrt(2.0 * var / 1024.0)
        print("chain %d beta %.4f: q2 measured %.4f exact %.4f deviation %+.4f bound %.4f" % (c, rec.betas[c], m["q2"][c], q2, m["q2"][c] - q2, bound))
        assert abs(m["q2"][c] - q2) <= bound, (c, m["q2"][c], q2, bound)
    for each in (pair.a, pair.b):                                          # both stay ordinary PTs
        assert np.isfinite(P.stepping_stone(each)) and P.n_round_trips(each) >= 0
        assert abs(P.stepping_stone(each) - R3.exact(beta_t, t.bonds_x, t.bonds_y, t.bonds_z)) < 0.5
