"""The 3-D +-J spin-glass family on the device (k_explore_checkerboard3d, k_refresh_lattice3d_stats: pigeons.jl_amd/csrc/pte_lattice3d.hpp)
against its restatement (tests/lattice3d_ref.py), against a Mattis gauge of itself, through the engine's plumbing, and against the enumerated
evidence of two 2 x 2 x 2 instances.

Everything here is integer or bit valued -- lattice bits, RNG words, the pair sum -- and is compared exactly; log potentials are the
two-operation interpolation of ising_lp and are compared exactly too.  (The device's exp and math.exp may differ in the last place of a
threshold: that moves a decision with probability ~2^-52 per draw, the exposure the exact lattice tests of the 2-D kernels have.)  The
evidence is held to the 0.5 band of tests/test_gpu_checkerboard.py's 4 x 4 enumerations."""
import numpy as np
import pytest

import lattice3d_ref as R
from test_gpu_spinglass import TINY, REC, _randomise, _check_suff          # the tiny-beta ladder and the protocol helpers of the spin-glass tests

pytestmark = pytest.mark.gpu

KERNEL = "k_explore_checkerboard3d"


@pytest.fixture(scope="module")
def P():
    import pigeons_amd
    return pigeons_amd


def _pt(P, target, N, n_steps=3, n_rounds=3, seed=1, record=None, **kw):
    return P.PT(P.Inputs(target=target, n_chains=N, n_rounds=n_rounds, seed=seed, explorer=P.CheckerboardMetropolis(n_steps), show_report=False,
                         record=REC(P) if record is None else record, **kw))


def _bonds(t):
    return t.bonds_x, t.bonds_y, t.bonds_z


def _two_explores_equal_the_restatement(P, t, L, N, n_steps, beta_t):
    """explore(1) from random lattices, then -- every slot handed another chain, the statistics left as the kernel wrote them -- explore(2):
    lattice bits, RNG words and suff per chain at both ends of each step (_check_suff), all exact.  suff before the first step is what
    k_refresh_lattice3d_stats counted for the lattices just set."""
    d = L ** 3
    J = _bonds(t)
    pt = _pt(P, t, N, n_steps=n_steps, record=[P.energy_ac1])
    eng = pt.replicas
    assert eng.kernel_name() == KERNEL and eng.scan_loop_name() == ""
    g = np.random.default_rng(L)
    betas, x, chain, rng = _randomise(eng, N, d, g)
    S = np.array([R.pair_sum(x[s], *J) for s in range(N)])
    for scan in (1, 2):
        eng.explore(scan)
        x1, c1, r1 = eng.states()
        xr, rr, S1 = R.explore(x, chain, rng, betas, *J, beta_t, n_steps, S)
        assert np.array_equal(c1, chain)
        assert np.array_equal(r1, rr), "RNG words"
        assert np.array_equal(x1, xr), "lattice bits"
        # the stream advance of every tempered slot is exactly n_steps d gamma (the refreshed one: d gamma)
        for slot in range(N):
            adv = (int(r1[slot, 0]) - int(rng[slot, 0])) % (1 << 64)
            assert adv == ((d if chain[slot] == 0 else n_steps * d) * int(rng[slot, 1])) % (1 << 64) and r1[slot, 1] == rng[slot, 1]
        eng.swap(scan); eng.reduce()
        _check_suff(eng, chain, betas, beta_t, S, S1)
        x, _, rng = eng.states()
        assert np.array_equal(x, xr)
        S = S1
        chain = (chain + 1) % N
        eng.set_states(None, chain, rng)
    assert S.tolist() == [R.pair_sum(x[s], *J) for s in range(N)]
    assert not np.array_equal(x, np.zeros_like(x))


# L: 2 doubled bonds, 16 rows per HBM word; 4; 6: rows straddle HBM words, 36 of 64 lanes busy; 8: one row per lane; 10: 1000 bits, ragged last
# HBM word; 16: four rows per lane; 30: the largest mask below a whole word; 32: whole-word rows, the shift-by-L edge
SHAPES = [(2, 5, 3), (4, 5, 1), (6, 5, 3), (8, 5, 3), (10, 5, 1), (16, 5, 3), (30, 3, 1), (32, 3, 1)]


@pytest.mark.parametrize("L,N,n_steps", SHAPES)
def test_explores_equal_the_restatement(P, L, N, n_steps):
    t = P.SpinGlass3DLogPotential.edwards_anderson(0.8, L, seed=100 + L)
    assert all(np.any(j < 0) for j in _bonds(t))
    _two_explores_equal_the_restatement(P, t, L, N, n_steps, 0.8)


@pytest.mark.parametrize("L,N,n_steps", [(6, 5, 3), (32, 3, 1)])
def test_explores_equal_the_restatement_on_the_ferromagnet(P, L, N, n_steps):
    _two_explores_equal_the_restatement(P, P.SpinGlass3DLogPotential.ferromagnet(0.8, L), L, N, n_steps, 0.8)


@pytest.mark.parametrize("L,n_steps", [(6, 3), (32, 1)])
def test_ladders_with_tiny_betas(P, L, n_steps):
    """r4, r8 and r12 round to 1 (or to its neighbour) at the lower betas of this ladder: almost every site flips, the thresholds sit at the top
    of the 52-bit range; one explore of a frustrated instance against the restatement"""
    N = len(TINY)
    t = P.SpinGlass3DLogPotential.edwards_anderson(1.0, L, seed=3 * L)
    fr = _pt(P, t, N, n_steps=n_steps, n_rounds=2, seed=6)
    betas, x, chain, rng = _randomise(fr.replicas, N, L ** 3, np.random.default_rng(L), betas=TINY)
    fr.replicas.explore(1)
    x1, c1, r1 = fr.replicas.states()
    xr, rr, _ = R.explore(x, chain, rng, betas, *_bonds(t), 1.0, n_steps)
    assert np.array_equal(r1, rr) and np.array_equal(x1, xr) and np.array_equal(c1, chain)


@pytest.mark.parametrize("L", [6, 32])
def test_mattis_gauge_maps_the_tempered_slots_onto_each_other(P, L):
    """bonds g_i g_j J_ij started (pte_set_state) from g . s with the same streams: after one explore the tempered slots hold g . (the states
    of the ungauged instance), the streams agree and suff is equal (the refreshed slot draws its bits anew: the gauge does not apply to it)"""
    N, d, beta_t = 4, L ** 3, 0.9
    t1 = P.SpinGlass3DLogPotential.edwards_anderson(beta_t, L, seed=L)
    g = np.random.default_rng(10 + L)
    gg = 2 * g.integers(0, 2, size=(L, L, L)) - 1
    t2 = P.SpinGlass3DLogPotential(beta_t, *R.gauge(*_bonds(t1), gg))
    flip = ((1 - gg.ravel()) // 2).astype(np.float64)
    a, b = _pt(P, t1, N, n_steps=2, record=[P.energy_ac1]).replicas, _pt(P, t2, N, n_steps=2, record=[P.energy_ac1]).replicas
    betas, x, chain, rng = _randomise(a, N, d, g)
    b.set_schedule(betas)
    b.set_states(np.abs(x - flip[None, :]), chain, rng)
    a.explore(1); b.explore(1)
    xa, _, ra = a.states()
    xb, _, rb = b.states()
    assert np.array_equal(ra, rb)
    tempered = chain != 0
    assert tempered.sum() == N - 1
    assert np.array_equal(xb[tempered], np.abs(xa[tempered] - flip[None, :])) and not np.array_equal(xa[tempered], x[tempered])
    for e in (a, b):
        e.swap(1); e.reduce()
    (_, na, ma), (_, nb, mb) = a.energy_ac1(), b.energy_ac1()
    for c in chain[tempered]:
        assert na[c] == nb[c] == 1 and np.array_equal(ma[c], mb[c])
        slot = int(np.flatnonzero(chain == c)[0])
        assert ma[c, 1] == R.ising_lp(betas[c], beta_t, R.pair_sum(xa[slot], *_bonds(t1)))


def test_evidence_of_a_frustrated_instance_and_of_the_ferromagnet(P):
    """L = 2, beta = 1, 10 chains, 10 rounds: |stepping_stone - exact| < 0.5 with exact = log sum_s exp(beta S(s)) - 8 log 2 over the 256 states.
    The test prints its values; DESIGN 4.19 holds the ones measured on one MI355X."""
    t = P.SpinGlass3DLogPotential.edwards_anderson(1.0, 2, seed=1)
    assert R.all_pair_sums(*_bonds(t)).max() < 24                                   # frustrated
    pt = P.pigeons(target=t, n_chains=10, n_rounds=10, show_report=False)          # (the family's default explorer)
    exact = R.exact(1.0, *_bonds(t))
    print("spin glass: stepping_stone %.6f exact %.6f" % (P.stepping_stone(pt), exact))
    f = P.SpinGlass3DLogPotential.ferromagnet(1.0, 2)
    ferro = P.pigeons(target=f, n_chains=10, n_rounds=10, explorer=P.CheckerboardMetropolis(), show_report=False)
    exact_f = R.exact(1.0, *_bonds(f))
    print("ferromagnet: stepping_stone %.6f exact %.6f" % (P.stepping_stone(ferro), exact_f))
    assert pt.replicas.kernel_name() == ferro.replicas.kernel_name() == KERNEL
    assert abs(P.stepping_stone(ferro) - exact_f) < 0.5
    assert abs(P.stepping_stone(pt) - exact) < 0.5


def _inputs(P, seed, n_rounds, checkpoint=False):
    t = P.SpinGlass3DLogPotential.edwards_anderson(1.0, 6, seed=4)
    return P.Inputs(target=t, n_chains=8, n_rounds=n_rounds, seed=seed, checkpoint=checkpoint, show_report=False, explorer=P.CheckerboardMetropolis(),
                    record=[P.round_trip, P.index_process, P.log_sum_ratio])


def test_two_runs_are_equal_bit_for_bit(P):
    a, b = P.pigeons(P.PT(_inputs(P, 3, 5))), P.pigeons(P.PT(_inputs(P, 3, 5)))
    assert a.replicas.kernel_name() == KERNEL
    for u, v in zip(a.replicas.states(), b.replicas.states()):
        assert np.array_equal(u, v)
    assert np.array_equal(a.reduced_recorders.index_process, b.reduced_recorders.index_process)
    assert P.stepping_stone(a) == P.stepping_stone(b)
    c = P.pigeons(P.PT(_inputs(P, 4, 5)))
    assert not np.array_equal(a.replicas.states()[0], c.replicas.states()[0])


def test_sharded_equals_single_engine(P):
    one, many = P.PT(_inputs(P, 1, 5)), P.PT(_inputs(P, 1, 5), n_shards=4)
    for _ in range(5):
        assert P.next_round(one) and P.next_round(many)
        ra = P.run_one_round(one); P.adapt(one, ra)
        rb = P.run_one_round(many); P.adapt(many, rb)
        assert np.array_equal(ra.index_process, rb.index_process) and ra.round_trip == rb.round_trip
    for u, v in zip(one.replicas.states(), many.shards.states()):
        assert np.array_equal(u, v)
    assert many.shards.n_boundary_swaps > 0


def test_checkpoint_resume_equals_uninterrupted(P, tmp_path):
    straight = P.pigeons(P.PT(_inputs(P, 5, 6)))
    folder = str(tmp_path / "exec")
    P.pigeons(P.PT(_inputs(P, 5, 3, checkpoint=True)), exec_folder=folder)
    resumed = P.pigeons(P.load_checkpoint(folder, n_rounds_increment=3))
    assert resumed.replicas.kernel_name() == KERNEL
    assert np.array_equal(straight.reduced_recorders.index_process, resumed.reduced_recorders.index_process)
    assert np.array_equal(straight.shared.tempering.schedule.grids, resumed.shared.tempering.schedule.grids)
    for u, v in zip(straight.replicas.states(), resumed.replicas.states()):
        assert np.array_equal(u, v)


def test_replacing_the_bonds_refreshes_suff(P):
    """the kernel carries suff through its sweeps: after new bonds arrive, one explore must continue from THEIR pair sum"""
    L, N, beta_t = 6, 4, 0.9
    t1 = P.SpinGlass3DLogPotential.edwards_anderson(beta_t, L, seed=1)
    t2 = P.SpinGlass3DLogPotential.edwards_anderson(beta_t, L, seed=2)
    pt = _pt(P, t1, N, n_steps=2, record=[P.energy_ac1])
    eng = pt.replicas
    betas, x, chain, rng = _randomise(eng, N, L ** 3, np.random.default_rng(3))
    S1 = [R.pair_sum(x[k], *_bonds(t1)) for k in range(N)]
    S2 = [R.pair_sum(x[k], *_bonds(t2)) for k in range(N)]
    assert all(a != b for a, b in zip(S1, S2))
    eng.set_target_spin_glass_3d(*_bonds(t2))
    eng.explore(1)
    x1, c1, r1 = eng.states()
    xr, rr, S = R.explore(x, chain, rng, betas, *_bonds(t2), beta_t, 2, S2)
    assert np.array_equal(x1, xr) and np.array_equal(r1, rr)
    eng.swap(1); eng.reduce()
    _check_suff(eng, chain, betas, beta_t, S2, S)


def test_state_calls_need_the_bonds_and_the_setter_validates(P):
    Lb = P._lib
    eng = P.Engine(n_chains=4, target=Lb.TARGET_SPIN_GLASS_3D, dim=64, explorer=Lb.EXPLORER_CHECKERBOARD_METROPOLIS, target_params=[1.0])
    for call in (lambda: eng.explore(1), lambda: eng.swap(1), lambda: eng.run_scans(1, 2), lambda: eng.states()):
        with pytest.raises(P.PteError, match="the 3-D spin-glass target has no bonds yet; call pte_set_target_spin_glass_3d first"):
            call()
    one = np.ones((4, 4, 4), dtype=np.int8)
    two = np.ones((2, 2, 2), dtype=np.int8)
    with pytest.raises(P.PteError, match=r"base_length must be the engine's 4 \(dim = 64\) \(got 2\)"):
        eng.set_target_spin_glass_3d(two, two, two)
    bad = np.array(one); bad[2, 1, 3] = 0; bad[3, 3, 3] = 2
    with pytest.raises(P.PteError, match=r"bonds_x\[39\] must be \+1 or -1 \(got 0\): ±J is the supported disorder -- real-valued or diluted"):
        eng.set_target_spin_glass_3d(bad, one, one)
    with pytest.raises(P.PteError, match=r"bonds_z\[63\] must be \+1 or -1 \(got 2\): ±J is the supported disorder"):
        eng.set_target_spin_glass_3d(one, one, np.where(bad == 0, 1, bad))
    with pytest.raises(P.PteError, match=r"bonds_y\[39\]"):                          # the planes are read in the order x, y, z
        eng.set_target_spin_glass_3d(one, bad, bad)
    import ctypes as C
    i8 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int8))
    with pytest.raises(P.PteError, match="pte_set_target_spin_glass_3d: null argument"):
        eng._chk(eng.L.pte_set_target_spin_glass_3d(eng.h, 4, i8(one), None, i8(one)))
    with pytest.raises(P.PteError, match="has no bonds yet"):                        # a refused call left the engine as it was
        eng.explore(1)
    flat = P.Engine(n_chains=4, target=Lb.TARGET_SPIN_GLASS, dim=64, explorer=Lb.EXPLORER_CHECKERBOARD_METROPOLIS, target_params=[1.0])
    with pytest.raises(P.PteError, match="pte_set_target_spin_glass_3d: this engine's target is 12, not PTE_TARGET_SPIN_GLASS_3D"):
        flat.set_target_spin_glass_3d(one, one, one)
    eng.set_target_spin_glass_3d(one, -one, one)
    eng.explore(1)
    assert eng.states()[0].shape == (4, 64) and eng.kernel_name() == KERNEL and eng.scan_loop_name() == ""
