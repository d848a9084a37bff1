"""The +-J spin-glass family on the device (k_explore_spinglass, k_explore_spinglass_spec, k_refresh_spinglass_stats:
pigeons.jl_amd/csrc/pte_spinglass.hpp) against its restatement (tests/spinglass_ref.py), against the Ising family where the bonds are
all +1 or a gauge transform of that (a Mattis instance), and against the enumerated evidence of a 4 x 4 instance.

Everything here is integer or bit valued -- lattice bits, RNG words, the bond-weighted pair sum -- and is compared exactly; log potentials are
the two-operation interpolation of ising_lp and are compared exactly too.  The evidence is held to the 0.5 band of
tests/test_gpu_parity.py::test_ising_ground_state_and_logz."""
import numpy as np
import pytest

import oracle as O
import spinglass_ref as R

pytestmark = pytest.mark.gpu

REC = lambda P: [P.round_trip, P.index_process, P.log_sum_ratio, P.swap_acceptance_pr]


@pytest.fixture(scope="module")
def P():
    import pigeons_amd
    return pigeons_amd


def _ones(L):
    return np.ones((L, L), dtype=np.int8)


def _pt(P, target, N, n_steps=3, n_rounds=3, seed=1, debug_kernel=0, record=None, **kw):
    ex = P.IsingMetropolis(n_steps)
    return P.PT(P.Inputs(target=target, n_chains=N, n_rounds=n_rounds, seed=seed, explorer=ex, show_report=False,
                         record=REC(P) if record is None else record, **kw), debug_kernel=debug_kernel)


def _randomise(eng, N, d, g, betas=None):
    """a random ladder, random lattices, a random chain permutation; the engine's own streams"""
    if betas is None:
        betas = np.concatenate([[0.0], np.sort(g.uniform(0.0, 1.0, N - 2)), [1.0]])
    eng.set_schedule(betas)
    x = g.integers(0, 2, size=(N, d)).astype(np.float64)
    chain = g.permutation(N).astype(np.int64)
    _, _, rng = eng.states()
    eng.set_states(x, chain, rng)
    return betas, x, chain, rng


def _check_suff(eng, chain, betas, beta_t, S_before, S_after):
    """suff of every slot before and after the explore step just reduced, through the energy_ac1 recorder: after ONE step its two means are
    the chain's log potential at kernel entry (from the suff the slot held) and at kernel exit -- ising_lp's two operations, compared exactly"""
    _, n, mom = eng.energy_ac1()
    for slot in range(len(chain)):
        c = int(chain[slot])
        assert n[c] == 1
        assert mom[c, 0] == R.ising_lp(betas[c], beta_t, S_before[slot]), "suff of chain %d before the step" % c
        assert mom[c, 1] == R.ising_lp(betas[c], beta_t, S_after[slot]), "suff of chain %d after the step" % c


def test_state_calls_need_the_bonds_and_the_setter_validates(P):
    Lb = P._lib
    eng = P.Engine(n_chains=4, target=Lb.TARGET_SPIN_GLASS, dim=16, explorer=Lb.EXPLORER_ISING_METROPOLIS, target_params=[1.0])
    for call in (lambda: eng.explore(1), lambda: eng.swap(1), lambda: eng.run_scans(1, 2), lambda: eng.states()):
        with pytest.raises(P.PteError, match="the spin-glass target has no bonds yet; call pte_set_target_spin_glass first"):
            call()
    ones = _ones(4)
    with pytest.raises(P.PteError, match=r"base_length must be the engine's 4 \(dim = 16\) \(got 3\)"):
        eng.set_target_spin_glass(_ones(3), _ones(3))
    bad = np.array(ones); bad[2, 1] = 0; bad[3, 3] = 2
    with pytest.raises(P.PteError, match=r"bonds_right\[9\] must be \+1 or -1 \(got 0\): ±J is the supported disorder -- real-valued or diluted"):
        eng.set_target_spin_glass(bad, ones)
    with pytest.raises(P.PteError, match=r"bonds_down\[15\] must be \+1 or -1 \(got 2\): ±J is the supported disorder"):
        eng.set_target_spin_glass(ones, np.where(bad == 0, 1, bad))
    with pytest.raises(P.PteError, match=r"bonds_right\[9\]"):                       # the right plane is read first
        eng.set_target_spin_glass(bad, bad)
    i8 = lambda a: a.ctypes.data_as(__import__("ctypes").POINTER(__import__("ctypes").c_int8))
    with pytest.raises(P.PteError, match="pte_set_target_spin_glass: null argument"):
        eng._chk(eng.L.pte_set_target_spin_glass(eng.h, 4, None, i8(ones)))
    with pytest.raises(P.PteError, match="has no bonds yet"):                        # a refused call left the engine as it was
        eng.explore(1)
    ising = P.Engine(n_chains=4, target=Lb.TARGET_ISING, dim=16, explorer=Lb.EXPLORER_ISING_METROPOLIS, target_params=[1.0])
    with pytest.raises(P.PteError, match="pte_set_target_spin_glass: this engine's target is 3, not PTE_TARGET_SPIN_GLASS"):
        ising.set_target_spin_glass(ones, ones)
    eng.set_target_spin_glass(ones, -ones)
    eng.explore(1)
    assert eng.states()[0].shape == (4, 16) and eng.kernel_name() == "k_explore_spinglass" and eng.scan_loop_name() == ""


# L: the smallest sizes at which each code path can go wrong (2: the byte kernel with doubled bonds; 3, 5: odd, wraps; 32: ONE_WORD -- bit 31's
# right neighbour is bit 0 of the word just swept, column 0's left bond is bit 31 of the same bond word; 64: the carry of the left bond across
# words and the row-end wrap; 96: a middle word with no wrap; 256: the full LDS budget)
@pytest.mark.parametrize("L,N,n_steps", [(2, 5, 3), (3, 5, 1), (5, 5, 3), (32, 5, 3), (64, 5, 1), (96, 5, 3), (256, 3, 1)])
def test_one_explore_equals_the_restatement(P, L, N, n_steps):
    """explore(1) from random lattices, then -- every slot handed another chain, the statistics left as the kernel wrote them -- explore(2):
    lattice bits, RNG words and suff per chain, all exact.  suff is read at both ends of each step (_check_suff): before the first it is what
    k_refresh_spinglass_stats counted for the lattices just set, before the second what the first step left, the refreshed slot's included."""
    d, beta_t = L * L, 0.8
    t = P.SpinGlassLogPotential.edwards_anderson(beta_t, L, seed=100 + L)
    jr, jd = t.bonds_right, t.bonds_down
    assert np.any(jr < 0) and np.any(jd < 0)
    pt = _pt(P, t, N, n_steps=n_steps, record=[P.energy_ac1])
    eng = pt.replicas
    assert eng.kernel_name() == ("k_explore_spinglass_spec" if L % 32 == 0 else "k_explore_spinglass")
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
        eng.swap(scan); eng.reduce()
        _check_suff(eng, chain, betas, beta_t, S, S1)
        # the next step: the lattices and streams as they are now (the swap moved chains and drew), every slot under another chain
        x, _, rng = eng.states()
        assert np.array_equal(x, xr)
        S = S1
        chain = (chain + 1) % N
        eng.set_states(None, chain, rng)
    assert S.tolist() == [R.pair_sum(x[s], jr, jd) for s in range(N)]


@pytest.mark.parametrize("L", [32, 64, 96])
def test_byte_kernel_equals_the_speculative_kernel(P, L):
    t = P.SpinGlassLogPotential.edwards_anderson(0.7, L, seed=L)
    a, b = _pt(P, t, 4, seed=7), _pt(P, t, 4, seed=7, debug_kernel=P._lib.KERNEL_ISING_BYTES)
    assert a.replicas.kernel_name() == "k_explore_spinglass_spec" and b.replicas.kernel_name() == "k_explore_spinglass"
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


TINY = np.array([0.0, 1e-18, 3e-16, 5e-14, 2e-13, 1e-11, 2.6e-7, 5e-6, 3e-3, 0.2, 0.6, 1.0])     # test_ising_ladders_with_tiny_betas


@pytest.mark.parametrize("L", [8, 32, 64])
def test_ladders_with_tiny_betas(P, L):
    """beta beta_target below PTE_ISING_FILTER_MIN = 1e-13 takes the exact arithmetic ("ratio >= 1 draws nothing" at 1e-18), above it the
    guard-banded thresholds decide: the all-ferro instance against the Ising engine after each of three calls of 8 scans, a frustrated one
    against the restatement for one explore"""
    N = len(TINY)
    sg = _pt(P, P.SpinGlassLogPotential(1.0, _ones(L), _ones(L)), N, n_rounds=6, seed=5)
    isg = _pt(P, P.IsingLogPotential(1.0, L), N, n_rounds=6, seed=5)
    sg.replicas.set_schedule(TINY); isg.replicas.set_schedule(TINY)
    for k in range(3):
        sg.replicas.run_scans(1 + 8 * k, 8); isg.replicas.run_scans(1 + 8 * k, 8)
        for u, v in zip(sg.replicas.states(), isg.replicas.states()):
            assert np.array_equal(u, v)
    t = P.SpinGlassLogPotential.edwards_anderson(1.0, L, seed=3 * L)
    fr = _pt(P, t, N, n_rounds=2, seed=6)
    betas, x, chain, rng = _randomise(fr.replicas, N, L * L, np.random.default_rng(L), betas=TINY)
    fr.replicas.explore(1)
    x1, c1, r1 = fr.replicas.states()
    xr, rr, _ = R.explore(x, chain, rng, betas, t.bonds_right, t.bonds_down, 1.0, 3)
    assert np.array_equal(r1, rr) and np.array_equal(x1, xr) and np.array_equal(c1, chain)


@pytest.mark.parametrize("L,N,rounds", [(5, 10, 6), (32, 4, 3), (64, 4, 3)])
def test_ferromagnetic_twin_equals_the_ising_family(P, L, N, rounds):
    """bonds all +1 against IsingLogPotential with the same seed, whole runs with swaps and adaptation: every recorder and state bit"""
    rec = REC(P)
    a = _pt(P, P.SpinGlassLogPotential(0.6, _ones(L), _ones(L)), N, n_rounds=rounds, seed=2, record=rec)
    b = _pt(P, P.IsingLogPotential(0.6, L), N, n_rounds=rounds, seed=2, record=rec)
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


def test_mattis_instance_is_the_gauged_ising_engine(P):
    """J_ij = g_i g_j, the state set to g . s0: one explore gives g . (the Ising engine's lattice) on every tempered chain with the same RNG
    words, the Ising engine's draw on the reference chain; suff is the bond-weighted sum on every slot, which the gauge leaves equal to the
    ferromagnet's on the tempered chains"""
    L, N = 64, 5
    d = L * L
    g = np.random.default_rng(11)
    gg = 2 * g.integers(0, 2, size=(L, L)) - 1
    notg = (1 - (gg.ravel() + 1) // 2).astype(np.float64)
    jr, jd = R.mattis(gg)
    sg = _pt(P, P.SpinGlassLogPotential(0.5, jr, jd), N, seed=9, record=[P.energy_ac1])
    isg = _pt(P, P.IsingLogPotential(0.5, L), N, seed=9, record=[P.energy_ac1])
    betas, x, chain, rng = _randomise(isg.replicas, N, d, g)
    sg.replicas.set_schedule(betas)
    sg.replicas.set_states(np.abs(x - notg[None, :]), chain, rng)          # bits XOR NOT g
    sg.replicas.explore(1); isg.replicas.explore(1)
    xs, cs, rs = sg.replicas.states()
    xi, ci, ri = isg.replicas.states()
    assert np.array_equal(rs, ri) and np.array_equal(cs, ci)
    for slot in range(N):
        if chain[slot] == 0:
            assert np.array_equal(xs[slot], xi[slot])
        else:
            assert np.array_equal(xs[slot], np.abs(xi[slot] - notg))
            assert R.pair_sum(xs[slot], jr, jd) == R.pair_sum(xi[slot], _ones(L), _ones(L))
    assert not np.array_equal(xi, x)
    S_sg = np.array([R.pair_sum(xs[k], jr, jd) for k in range(N)])
    for e_, xx, bonds in ((sg.replicas, np.abs(x - notg[None, :]), (jr, jd)), (isg.replicas, x, (_ones(L), _ones(L)))):
        e_.swap(1); e_.reduce()
        before = [R.pair_sum(xx[k], *bonds) for k in range(N)]
        after = S_sg if e_ is sg.replicas else [R.pair_sum(xi[k], _ones(L), _ones(L)) for k in range(N)]
        _check_suff(e_, chain, betas, 0.5, before, after)
    # the refreshed slot holds the Ising engine's draw under the Mattis bonds: its suff is the bond-weighted sum, not the ferromagnet's --
    # the chain that sits on it next reads it at kernel entry
    ref_slot = int(np.flatnonzero(chain == 0)[0])
    assert S_sg[ref_slot] != R.pair_sum(xs[ref_slot], _ones(L), _ones(L))
    x2, _, rng2 = sg.replicas.states()
    chain2 = (chain + 2) % N
    sg.replicas.set_states(None, chain2, rng2)
    sg.replicas.explore(2)
    after2 = [R.pair_sum(row, jr, jd) for row in sg.replicas.states()[0]]
    sg.replicas.swap(2); sg.replicas.reduce()
    _check_suff(sg.replicas, chain2, betas, 0.5, S_sg, after2)


def test_evidence_of_a_frustrated_instance_and_of_its_ferromagnetic_twin(P):
    """L = 4, beta = 1, 10 chains, 10 rounds: |stepping_stone - exact| < 0.5 with exact = log sum_s exp(beta S(s)) - 16 log 2 by enumeration,
    on the new family and -- the same estimator on the path every Ising test trusts -- on IsingLogPotential against its own enumeration"""
    t = P.SpinGlassLogPotential.edwards_anderson(1.0, 4, seed=2)
    assert R.all_pair_sums(t.bonds_right, t.bonds_down).max() < 32                  # frustrated
    pt = P.pigeons(target=t, n_chains=10, n_rounds=10, show_report=False)
    exact = R.exact(1.0, t.bonds_right, t.bonds_down)
    print("spin glass: stepping_stone %.6f exact %.6f" % (P.stepping_stone(pt), exact))
    ferro = P.pigeons(target=P.IsingLogPotential(1.0, 4), n_chains=10, n_rounds=10, show_report=False)
    exact_f = R.exact(1.0, _ones(4), _ones(4))
    print("ferromagnet: stepping_stone %.6f exact %.6f" % (P.stepping_stone(ferro), exact_f))
    assert abs(P.stepping_stone(ferro) - exact_f) < 0.5
    assert abs(P.stepping_stone(pt) - exact) < 0.5


def _inputs(P, seed, n_rounds, checkpoint=False):
    t = P.SpinGlassLogPotential.edwards_anderson(1.0, 8, seed=4)
    return P.Inputs(target=t, n_chains=8, n_rounds=n_rounds, seed=seed, checkpoint=checkpoint, show_report=False,
                    record=[P.round_trip, P.index_process, P.log_sum_ratio])


def test_two_runs_are_equal_bit_for_bit(P):
    a, b = P.pigeons(P.PT(_inputs(P, 3, 5))), P.pigeons(P.PT(_inputs(P, 3, 5)))
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
    assert np.array_equal(straight.reduced_recorders.index_process, resumed.reduced_recorders.index_process)
    assert np.array_equal(straight.shared.tempering.schedule.grids, resumed.shared.tempering.schedule.grids)
    for u, v in zip(straight.replicas.states(), resumed.replicas.states()):
        assert np.array_equal(u, v)


def test_replacing_the_bonds_refreshes_suff(P):
    """the byte kernel carries suff through its sweep: after new bonds arrive, one explore must continue from THEIR pair sum"""
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
