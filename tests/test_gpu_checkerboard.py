"""CheckerboardMetropolis on the device (k_explore_checkerboard, k_explore_checkerboard_sites: pigeons.jl_amd/csrc/pte_checkerboard.hpp) against
its restatement (tests/checkerboard_ref.py), the packed kernel against the sites kernel, the all-ferromagnetic spin glass against the Ising
target, and against the enumerated evidence of a 4 x 4 instance.

Everything here is integer or bit valued -- lattice bits, RNG words, the pair sum -- and is compared exactly; log potentials are the
two-operation interpolation of ising_lp and are compared exactly too.  (The device's exp and math.exp may differ in the last place of r4 / r8:
that moves a decision with probability ~2^-52 per draw, the exposure the exact lattice tests of IsingMetropolis have.)  The evidence is held to
the 0.5 band of tests/test_gpu_spinglass.py's evidence test, on its instance and run length."""
import numpy as np
import pytest

import checkerboard_ref as R
from test_gpu_spinglass import TINY, REC, _ones, _randomise, _check_suff          # the tiny-beta ladder and the protocol helpers of the spin-glass tests

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def P():
    import pigeons_amd
    return pigeons_amd


def _pt(P, target, N, n_steps=3, n_rounds=3, seed=1, debug_kernel=0, record=None, **kw):
    return P.PT(P.Inputs(target=target, n_chains=N, n_rounds=n_rounds, seed=seed, explorer=P.CheckerboardMetropolis(n_steps), show_report=False,
                         record=REC(P) if record is None else record, **kw), debug_kernel=debug_kernel)


def _kernel(L, debug_kernel=0):
    return "k_explore_checkerboard" if L % 32 == 0 and debug_kernel == 0 else "k_explore_checkerboard_sites"


def _two_explores_equal_the_restatement(P, t, jr, jd, L, N, n_steps, beta_t):
    """explore(1) from random lattices, then -- every slot handed another chain, the statistics left as the kernel wrote them -- explore(2):
    lattice bits, RNG words and suff per chain at both ends of each step (_check_suff), all exact"""
    d = L * L
    pt = _pt(P, t, N, n_steps=n_steps, record=[P.energy_ac1])
    eng = pt.replicas
    assert eng.kernel_name() == _kernel(L) and eng.scan_loop_name() == ""
    g = np.random.default_rng(L)
    betas, x, chain, rng = _randomise(eng, N, d, g)
    S = np.array([R.pair_sum(x[s], jr, jd) for s in range(N)])
    for scan in (1, 2):
        eng.explore(scan)
        x1, c1, r1 = eng.states()
        xr, rr, S1 = R.explore(x, chain, rng, betas, jr, jd, beta_t, n_steps, S)
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
    assert S.tolist() == [R.pair_sum(x[s], jr, jd) for s in range(N)]
    assert not np.array_equal(x, np.zeros_like(x))


# L: 2 the sites kernel with doubled bonds; 4; 6: L / 2 odd, wraps; 32: one word per row, the wrap inside the word, half the lanes idle; 64: carries
# across words at both row ends; 96: a middle word; 256: 32 words per lane, the full LDS budget
@pytest.mark.parametrize("L,N,n_steps", [(2, 5, 3), (4, 5, 1), (6, 5, 3), (32, 5, 3), (64, 5, 1), (96, 5, 3), (256, 3, 1)])
def test_explores_equal_the_restatement_on_the_spin_glass(P, L, N, n_steps):
    t = P.SpinGlassLogPotential.edwards_anderson(0.8, L, seed=100 + L)
    assert np.any(t.bonds_right < 0) and np.any(t.bonds_down < 0)
    _two_explores_equal_the_restatement(P, t, t.bonds_right, t.bonds_down, L, N, n_steps, 0.8)


@pytest.mark.parametrize("L,N,n_steps", [(6, 5, 3), (32, 5, 3), (64, 5, 1)])
def test_explores_equal_the_restatement_on_the_ising_target(P, L, N, n_steps):
    _two_explores_equal_the_restatement(P, P.IsingLogPotential(0.8, L), _ones(L), _ones(L), L, N, n_steps, 0.8)


@pytest.mark.parametrize("spin_glass", [False, True])
@pytest.mark.parametrize("L", [32, 64, 96])
def test_packed_kernel_equals_the_sites_kernel(P, L, spin_glass):
    t = P.SpinGlassLogPotential.edwards_anderson(0.7, L, seed=L) if spin_glass else P.IsingLogPotential(0.7, L)
    a, b = _pt(P, t, 4, seed=7), _pt(P, t, 4, seed=7, debug_kernel=P._lib.KERNEL_ISING_BYTES)
    assert a.replicas.kernel_name() == "k_explore_checkerboard" and b.replicas.kernel_name() == "k_explore_checkerboard_sites"
    for _ in range(3):
        assert P.next_round(a) and P.next_round(b)
        ra = P.run_one_round(a); P.adapt(a, ra)
        rb = P.run_one_round(b); P.adapt(b, rb)
        assert np.array_equal(ra.index_process, rb.index_process) and ra.round_trip == rb.round_trip
        for u, v in zip(ra.swap_acceptance_pr + ra.log_sum_ratio, rb.swap_acceptance_pr + rb.log_sum_ratio):
            assert np.array_equal(u, v)
        assert np.array_equal(a.shared.tempering.schedule.grids, b.shared.tempering.schedule.grids)
    for u, v in zip(a.replicas.states(), b.replicas.states()):
        assert np.array_equal(u, v)


@pytest.mark.parametrize("L,N,rounds", [(6, 10, 6), (32, 4, 3)])
def test_ferromagnetic_twin_equals_the_ising_target(P, L, N, rounds):
    """bonds all +1 against IsingLogPotential with the same seed, whole runs with swaps and adaptation: every recorder and state bit"""
    a = _pt(P, P.SpinGlassLogPotential(0.6, _ones(L), _ones(L)), N, n_rounds=rounds, seed=2)
    b = _pt(P, P.IsingLogPotential(0.6, L), N, n_rounds=rounds, seed=2)
    for _ in range(rounds):
        assert P.next_round(a) and P.next_round(b)
        ra = P.run_one_round(a); P.adapt(a, ra)
        rb = P.run_one_round(b); P.adapt(b, rb)
        assert np.array_equal(ra.index_process, rb.index_process) and ra.round_trip == rb.round_trip
        for u, v in zip(ra.swap_acceptance_pr, rb.swap_acceptance_pr):
            assert np.array_equal(u, v)
        assert np.array_equal(a.shared.tempering.schedule.grids, b.shared.tempering.schedule.grids)
        assert P.stepping_stone_pair(a) == P.stepping_stone_pair(b)
        for u, v in zip(a.replicas.states(), b.replicas.states()):
            assert np.array_equal(u, v)


@pytest.mark.parametrize("L", [6, 32, 64])
def test_ladders_with_tiny_betas(P, L):
    """r4 and r8 round to 1 (or to its neighbour) at the lower betas of this ladder: almost every site flips, the thresholds sit at the top of
    the 52-bit range; one explore of a frustrated instance against the restatement"""
    N = len(TINY)
    t = P.SpinGlassLogPotential.edwards_anderson(1.0, L, seed=3 * L)
    fr = _pt(P, t, N, n_rounds=2, seed=6)
    betas, x, chain, rng = _randomise(fr.replicas, N, L * L, np.random.default_rng(L), betas=TINY)
    fr.replicas.explore(1)
    x1, c1, r1 = fr.replicas.states()
    xr, rr, _ = R.explore(x, chain, rng, betas, t.bonds_right, t.bonds_down, 1.0, 3)
    assert np.array_equal(r1, rr) and np.array_equal(x1, xr) and np.array_equal(c1, chain)


def test_evidence_of_a_frustrated_instance_and_of_its_ferromagnetic_twin(P):
    """L = 4, beta = 1, 10 chains, 10 rounds: |stepping_stone - exact| < 0.5 with exact = log sum_s exp(beta S(s)) - 16 log 2 by enumeration.
    Measured on one MI355X: 11.428 against 11.472 (frustrated), 21.691 against 21.608 (ferromagnet); the test prints its values."""
    t = P.SpinGlassLogPotential.edwards_anderson(1.0, 4, seed=2)
    assert R.all_pair_sums(t.bonds_right, t.bonds_down).max() < 32                  # frustrated
    pt = P.pigeons(target=t, n_chains=10, n_rounds=10, explorer=P.CheckerboardMetropolis(), show_report=False)
    exact = R.exact(1.0, t.bonds_right, t.bonds_down)
    print("spin glass: stepping_stone %.6f exact %.6f" % (P.stepping_stone(pt), exact))
    ferro = P.pigeons(target=P.IsingLogPotential(1.0, 4), n_chains=10, n_rounds=10, explorer=P.CheckerboardMetropolis(), show_report=False)
    exact_f = R.exact(1.0, _ones(4), _ones(4))
    print("ferromagnet: stepping_stone %.6f exact %.6f" % (P.stepping_stone(ferro), exact_f))
    assert pt.replicas.kernel_name() == ferro.replicas.kernel_name() == "k_explore_checkerboard_sites"
    assert abs(P.stepping_stone(ferro) - exact_f) < 0.5
    assert abs(P.stepping_stone(pt) - exact) < 0.5


def _inputs(P, seed, n_rounds, checkpoint=False):
    t = P.SpinGlassLogPotential.edwards_anderson(1.0, 8, seed=4)
    return P.Inputs(target=t, n_chains=8, n_rounds=n_rounds, seed=seed, checkpoint=checkpoint, show_report=False, explorer=P.CheckerboardMetropolis(),
                    record=[P.round_trip, P.index_process, P.log_sum_ratio])


def test_two_runs_are_equal_bit_for_bit(P):
    a, b = P.pigeons(P.PT(_inputs(P, 3, 5))), P.pigeons(P.PT(_inputs(P, 3, 5)))
    assert a.replicas.kernel_name() == "k_explore_checkerboard_sites"
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
    assert resumed.replicas.kernel_name() == "k_explore_checkerboard_sites"
    assert np.array_equal(straight.reduced_recorders.index_process, resumed.reduced_recorders.index_process)
    assert np.array_equal(straight.shared.tempering.schedule.grids, resumed.shared.tempering.schedule.grids)
    for u, v in zip(straight.replicas.states(), resumed.replicas.states()):
        assert np.array_equal(u, v)


def test_replacing_the_bonds_refreshes_suff(P):
    """the kernels carry suff through their sweeps: after new bonds arrive, one explore must continue from THEIR pair sum"""
    L, N, beta_t = 6, 4, 0.9
    d = L * L
    t1 = P.SpinGlassLogPotential.edwards_anderson(beta_t, L, seed=1)
    t2 = P.SpinGlassLogPotential.edwards_anderson(beta_t, L, seed=2)
    pt = _pt(P, t1, N, n_steps=2, record=[P.energy_ac1])
    eng = pt.replicas
    betas, x, chain, rng = _randomise(eng, N, d, np.random.default_rng(3))
    S1 = [R.pair_sum(x[k], t1.bonds_right, t1.bonds_down) for k in range(N)]
    S2 = [R.pair_sum(x[k], t2.bonds_right, t2.bonds_down) for k in range(N)]
    assert all(a != b for a, b in zip(S1, S2))
    eng.set_target_spin_glass(t2.bonds_right, t2.bonds_down)
    eng.explore(1)
    x1, c1, r1 = eng.states()
    xr, rr, S = R.explore(x, chain, rng, betas, t2.bonds_right, t2.bonds_down, beta_t, 2, S2)
    assert np.array_equal(x1, xr) and np.array_equal(r1, rr)
    eng.swap(1); eng.reduce()
    _check_suff(eng, chain, betas, beta_t, S2, S)
