"""The guard band of the five IsingMetropolis kernels (lattice_thresholds, csrc/pte_ising.hpp) held to the exact rule draw by draw: schedules
built by tests/lattice_band.py put one chosen draw of every replica inside the band (both signs, and strictly between the exact ratio and
the plain threshold), in the speculative kernels' window outside the band, and far outside -- at the rows, bits, quads, buffer places and
bond signs where the kernels take different code.  Everything compared is integer or bit valued (lattice bits, RNG words, the pair sum
through ising_lp's two operations) and is compared exactly, against tests/spinglass_ref.py and, for the Ising family, against the oracle."""
import functools

import numpy as np
import pytest

import lattice_band as B
import oracle as O
import spinglass_ref as R

pytestmark = pytest.mark.gpu

SEED = 12                        # tests/test_lattice_band_cpu.py holds the coverage of these builds: same seed, n_steps 1 and 2, every shape


@pytest.fixture(scope="module")
def P():
    import pigeons_amd
    return pigeons_amd


@functools.lru_cache(maxsize=None)
def _shape(family, L, n_steps):
    """the built cases of one shape as ladders, each with the restatement's explore step: built once per module"""
    sh = B.build(L, family, n_steps, seed=SEED)
    lads = B.ladders(sh, seed=SEED)
    for lad in lads:
        lad["S0"] = np.array([R.pair_sum(row, sh["jr"], sh["jd"]) for row in lad["x"]])
        lad["ref"] = R.explore(lad["x"], lad["chain"], lad["rng"], lad["betas"], sh["jr"], sh["jd"], 1.0, n_steps, lad["S0"])
    return sh, lads


@functools.lru_cache(maxsize=None)
def _second_scan(family, L, n_steps, i, chain2, rng2):
    """the restatement's second explore step of ladder i from the lattices its first step left, under the chains and streams the engine's
    swap left (the arguments: the same for every kernel that got the first scan right, so computed once)"""
    sh, lads = _shape(family, L, n_steps)
    xr, _, S1 = lads[i]["ref"]
    return R.explore(xr, np.frombuffer(chain2, dtype=np.int64), np.frombuffer(rng2, dtype=np.uint64).reshape(-1, 2), lads[i]["betas"],
                     sh["jr"], sh["jd"], 1.0, n_steps, S1)


def _engine(P, sh, N, debug_kernel=0):
    L = sh["L"]
    target = P.IsingLogPotential(1.0, L) if sh["family"] == "ising" else P.SpinGlassLogPotential(1.0, sh["jr"], sh["jd"])
    pt = P.PT(P.Inputs(target=target, n_chains=N, n_rounds=2, seed=1, explorer=P.IsingMetropolis(sh["n_steps"]), show_report=False,
                       record=[P.energy_ac1]), debug_kernel=debug_kernel)
    return pt.replicas


def _check_suff(eng, chain, betas, S_before, S_after):
    """tests/test_gpu_spinglass.py::_check_suff: after ONE explore step the energy_ac1 recorder's two means are the chain's log potential at
    kernel entry and exit -- ising_lp's two operations on suff, compared exactly"""
    _, n, mom = eng.energy_ac1()
    for slot in range(len(chain)):
        c = int(chain[slot])
        assert n[c] == 1
        assert mom[c, 0] == R.ising_lp(betas[c], 1.0, S_before[slot]), "suff of chain %d before the step" % c
        assert mom[c, 1] == R.ising_lp(betas[c], 1.0, S_after[slot]), "suff of chain %d after the step" % c


def _where(lad, x1, xr, r1, rr):
    """the cases whose replica differs, for the assertion's message"""
    bad = [s for s in range(len(lad["cases"])) if not (np.array_equal(x1[s], xr[s]) and np.array_equal(r1[s], rr[s]))]
    return "; ".join("%s eps %+.1e %s k %d site %d delta %d" % (lad["cases"][s]["kind"], lad["cases"][s]["eps"], lad["cases"][s]["cls"],
                                                                 lad["cases"][s]["k"], lad["cases"][s]["draw"][2], lad["cases"][s]["draw"][3])
                     for s in bad[:6])


def _run(P, family, L, n_steps, kernel, debug_kernel=0):
    sh, lads = _shape(family, L, n_steps)
    assert len(sh["cases"]) >= 8
    for lad in lads:
        betas, x, chain, rng = lad["betas"], lad["x"], lad["chain"], lad["rng"]
        N = len(chain)
        assert N <= 48
        eng = _engine(P, sh, N, debug_kernel)
        assert eng.kernel_name() == kernel
        eng.set_schedule(betas)
        eng.set_states(x, chain, rng)
        eng.explore(1)
        x1, c1, r1 = eng.states()
        xr, rr, S1 = lad["ref"]
        assert np.array_equal(c1, chain)
        assert np.array_equal(r1, rr), "RNG words: " + _where(lad, x1, xr, r1, rr)
        assert np.array_equal(x1, xr), "lattice bits: " + _where(lad, x1, xr, r1, rr)
        eng.swap(1); eng.reduce()
        _check_suff(eng, chain, betas, lad["S0"], S1)
        # a later scan: the swap moved chains and drew, no chain has a tuned draw any more -- a band decision left suff and the stream
        # where the next step needs them
        x2, chain2, rng2 = eng.states()
        assert np.array_equal(x2, xr) and not np.array_equal(chain2, chain)
        eng.explore(2)
        x3, c3, r3 = eng.states()
        xq, rq, _ = _second_scan(family, L, n_steps, lads.index(lad), chain2.tobytes(), rng2.tobytes())
        assert np.array_equal(c3, chain2) and np.array_equal(r3, rq) and np.array_equal(x3, xq)


# L: 6 / 5 the byte kernels; 32 the speculative kernels with one word per row; 64 their general instantiation; 96 a middle word (W = 3)
@pytest.mark.parametrize("L,n_steps", [(6, 1), (6, 2), (32, 1), (32, 2), (64, 1), (64, 2), (96, 1), (96, 2)])
def test_ising_band_cases_equal_the_restatement(P, L, n_steps):
    _run(P, "ising", L, n_steps, "k_explore_ising_spec" if L % 32 == 0 else "k_explore_ising")


@pytest.mark.parametrize("L,n_steps", [(5, 1), (5, 2), (32, 1), (32, 2), (64, 1), (64, 2)])
def test_spinglass_band_cases_equal_the_restatement(P, L, n_steps):
    _run(P, "ea", L, n_steps, "k_explore_spinglass_spec" if L % 32 == 0 else "k_explore_spinglass")


@pytest.mark.parametrize("L", [32, 64])
@pytest.mark.parametrize("impl", ["bits", "bytes"])
def test_scalar_ising_kernels_on_the_band_cases(P, L, impl):
    """the same cases through the scalar bit-packed sweep (test build) and the byte-lattice sweep of the bit-packed shapes"""
    dk, name = {"bits": (P._lib.KERNEL_ISING_BITS, "k_explore_ising_bits"), "bytes": (P._lib.KERNEL_ISING_BYTES, "k_explore_ising")}[impl]
    _run(P, "ising", L, 2, name, debug_kernel=dk)


@pytest.mark.parametrize("L", [32, 64])
def test_ising_band_cases_equal_the_oracle_after_a_whole_scan(P, L):
    """the oracle as second reference: the same ladders and states, one scan (explore and swap), states, chains and RNG words"""
    n_steps = 2
    sh, lads = _shape("ising", L, n_steps)
    for lad in lads:
        N = len(lad["chain"])
        eng = _engine(P, sh, N)
        ref = O.OraclePT(target=O.TARGET_ISING, explorer=O.EXPLORER_ISING, dim=L * L, p0=1.0, n_chains=N, seed=1, slice_n_passes=n_steps)
        eng.set_schedule(lad["betas"]); ref.set_schedule(lad["betas"])
        ref.begin_round()
        eng.set_states(lad["x"], lad["chain"], lad["rng"]); ref.set_states(lad["x"], lad["chain"], lad["rng"])
        eng.run_scans(1, 1); ref.run_scans(1)
        x, chain, rng = eng.states()
        xr, cr, rr = ref.states()
        assert np.array_equal(chain, cr) and np.array_equal(rng, rr) and np.array_equal(x, xr)
        assert np.array_equal(x, lad["ref"][0]) and not np.array_equal(chain, lad["chain"])
