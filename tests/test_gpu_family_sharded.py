"""Every target family across the shard boundary of the production path: k_swap_stats -> k_boundary_pack -> (the group's stream-ordered
copies, or the step-by-step driver's) -> k_boundary_stats_in -> k_swap_decide -> k_boundary_apply, against one engine over the same chains.

(a) the eight data families on the interpolated path, each with the small model its own GPU test file builds (that file's _inputs), under
    family_gpu.assert_sharded_equals_single -- every recorder round by round and the per-boundary, per-side swap counts, bit for bit.
    Geometries (driver, chains N, shards G): ("group", 8, 4) interior shards have both sides active in one scan; ("group", 9, 3) three
    chains per shard, the boundaries fall on both DEO parities; ("group", 6, 6) one chain per shard, slot 0 serves both sides and every
    pair is a boundary pair; ("device", 8, 4) the same kernels driven step by step.  The family's own explorer everywhere, AutoMALA once
    at ("group", 8, 4) where the family has a gradient.  Four rounds, 30 scans.
(b) the lattice families in the same geometries, at the widths where the bit-packed row is not one 8-byte word: the 2-D spin glass under
    IsingMetropolis at L = 9 (81 bits: 3 32-bit words in 2 8-byte words) and L = 32 (the lane-speculative kernel, 16 words), under
    CheckerboardMetropolis at L = 12 and L = 32, the 3-D spin glass at L = 6 (7 32-bit words in 4), the Ising target at L = 9.
    CheckerboardMetropolis is defined on even L only (the target refuses an odd one by name), so its odd-word case is L = 12: 144 bits,
    5 32-bit words in 3.  The inverse temperatures are chosen for the ladder, not for the physics: N <= 9 chains and 30 scans must leave
    every boundary pair an accepted swap, and the spread of the log ratio grows with beta times the root of the number of bonds.
(c) one swap across an engine boundary against the 60-digit definition: the battery of tests/test_gpu_family_edges.py (e), the same
    replicas laid out on shard engines (one chain per shard; two shards where N is even) and driven through the two-phase calls without an
    explore.  Log ratios, acceptance and decision as there; then every slot holds the state, the RNG words (advanced by the swap's one draw)
    and the replica id that the decision sends there, and the next explore step's energy_ac1 `before` is the definition's log density of
    that state at the slot's chain -- suff and suff2 travelled.  (Of the battery's 330 pairs over the two scans the definition accepts 185,
    in every group but dense-d65@0; with one chain per shard each of them is an export and an import on both sides.)
(d) the same boundary pairs through the message kernels (device_messages=True, one chain per shard), against a single-engine twin bit for
    bit and against the definition at the states the twin's explore step left.
(e) pte_set_state refuses a chain argument that is no permutation of the local chains and then has changed nothing.

Nothing here has a tolerance of its own: comparisons are exact, or use LP_RTOL / LP_ATOL of tests/test_gpu_family_edges.py."""
import dataclasses
import math

import numpy as np
import pytest
from mpmath import mp, mpf

import family_edges as E
import family_gpu as G
import oracle as O
import test_gpu_ar1
import test_gpu_changepoint
import test_gpu_dense
import test_gpu_family_edges as T
import test_gpu_glm
import test_gpu_hier
import test_gpu_mixture
import test_gpu_mixture_model
import test_gpu_varsel
from family_gpu import P  # noqa: F401  (the fixture)
from test_gpu_family_edges import GROUP_IDS, GROUPS, LP_ATOL, LP_RTOL

pytestmark = pytest.mark.gpu

GEOMETRIES = [("group", 8, 4), ("group", 9, 3), ("group", 6, 6), ("device", 8, 4)]
GEOMETRY_IDS = ["%s-N%d-G%d" % g for g in GEOMETRIES]
DRIVER_KW = {"group": dict(transport="group"), "device": dict(device_messages=True)}
SEED = 4                  # with it every boundary pair of every case below has an accepted swap (the helper asserts it)

# family -> (the maker of its test file, whether it takes an explorer)
DATA_FAMILIES = {"glm": (test_gpu_glm._inputs, True), "hier": (test_gpu_hier._inputs, True), "ar1": (test_gpu_ar1._inputs, True),
                 "dense": (test_gpu_dense._inputs, True), "mixture": (test_gpu_mixture._bimodal, True),
                 "mixture_model": (test_gpu_mixture_model._inputs, True), "varsel": (test_gpu_varsel._inputs, False),
                 "changepoint": (test_gpu_changepoint._inputs, False)}
RECORD = ["round_trip", "index_process", "log_sum_ratio", "swap_acceptance_pr", "energy_ac1", "online"]


def _data_cases():
    out = [pytest.param(f, "own", g, id="%s-%s" % (f, gid)) for f in DATA_FAMILIES for g, gid in zip(GEOMETRIES, GEOMETRY_IDS)]
    return out + [pytest.param(f, "automala", GEOMETRIES[0], id="%s-automala-%s" % (f, GEOMETRY_IDS[0]))
                  for f, (_, takes) in DATA_FAMILIES.items() if takes]


@pytest.mark.parametrize("family,explorer,geometry", _data_cases())
def test_data_family_across_the_message_kernels(P, family, explorer, geometry):
    driver, N, n_shards = geometry
    make, _ = DATA_FAMILIES[family]
    kw = dict(explorer=P.AutoMALA()) if explorer == "automala" else {}
    mk = lambda: G.with_recorders(P, dataclasses.replace(make(P, seed=SEED, n_rounds=4, **kw), n_chains=N), *RECORD)
    counts = G.assert_sharded_equals_single(P, mk, n_shards, **DRIVER_KW[driver])
    print("%s %s %s: accepted swaps per boundary %s" % (family, explorer, geometry, counts))


# ---- (b) -------------------------------------------------------------------------------------------------------------------------------
def _lattice_target(P, name):
    if name == "spinglass-L9":
        return P.SpinGlassLogPotential.edwards_anderson(0.4, 9, seed=4), P.IsingMetropolis()
    if name == "spinglass-L32":
        return P.SpinGlassLogPotential.edwards_anderson(0.1, 32, seed=4), P.IsingMetropolis()
    if name == "checkerboard-L12":
        return P.SpinGlassLogPotential.edwards_anderson(0.3, 12, seed=4), P.CheckerboardMetropolis()
    if name == "checkerboard-L32":
        return P.SpinGlassLogPotential.edwards_anderson(0.1, 32, seed=4), P.CheckerboardMetropolis()
    if name == "spinglass3d-L6":
        return P.SpinGlass3DLogPotential.edwards_anderson(0.2, 6, seed=4), P.CheckerboardMetropolis()
    if name == "ising-L9":
        return P.IsingLogPotential(0.25, 9), P.IsingMetropolis()
    raise KeyError(name)


LATTICES = ["spinglass-L9", "spinglass-L32", "checkerboard-L12", "checkerboard-L32", "spinglass3d-L6", "ising-L9"]
LATTICE_WORDS = {"spinglass-L9": 2, "spinglass-L32": 16, "checkerboard-L12": 3, "checkerboard-L32": 16, "spinglass3d-L6": 4, "ising-L9": 2}


@pytest.mark.parametrize("geometry", GEOMETRIES, ids=GEOMETRY_IDS)
@pytest.mark.parametrize("lattice", LATTICES)
def test_lattice_family_across_the_message_kernels(P, lattice, geometry):
    driver, N, n_shards = geometry

    def mk():
        target, explorer = _lattice_target(P, lattice)
        return P.Inputs(target=target, n_chains=N, n_rounds=4, seed=SEED, explorer=explorer, show_report=False,
                        record=[P.round_trip, P.index_process, P.log_sum_ratio, P.swap_acceptance_pr, P.energy_ac1])
    probe = P.PT(mk(), n_shards=n_shards).shards.engines[0]
    assert probe.payload_words() == LATTICE_WORDS[lattice] + 6 and probe.message_words() == LATTICE_WORDS[lattice] + 8
    counts = G.assert_sharded_equals_single(P, mk, n_shards, **DRIVER_KW[driver])
    print("%s %s: accepted swaps per boundary %s" % (lattice, geometry, counts))


# ---- (c), (d): the battery's replicas on shard engines ------------------------------------------------------------------------------------
_MP = {}


def _mp_lp(gi, c, i):
    """the 60-digit log density of battery state i of group gi at chain c's beta (kept: the geometries and scans ask for the same values)"""
    if (gi, c, i) not in _MP:
        shape, _, states = GROUPS[gi]
        betas, x, _, _ = T.layout(gi, shape, states)
        _MP[(gi, c, i)] = E.mp_lp(shape, betas[c], x[i])
    return _MP[(gi, c, i)]


def _explorer(P, shape):
    return P.SliceSampler(w=1.0, p=1, n_passes=1) if shape.family == "changepoint" else P.SliceSampler(w=0.25, p=3, n_passes=1)


def _shards(P, shape, n_shards, betas, x, chain, rng, **pt_kw):
    """(pt, owner): n_shards engines over the chains of `chain`; shard g holds the replicas whose chain is in its range, in replica order --
    owner[g][slot] is the replica, and the engine numbers that slot's replica g K + slot"""
    N = len(chain)
    target, ref_dim = E.device_target(P, shape)
    pt = P.PT(P.Inputs(target=target, reference=P.ScaledPrecisionNormalLogPotential(shape.ref_prec, ref_dim), n_chains=N, n_rounds=2,
                       explorer=_explorer(P, shape), show_report=False, record=[P.log_sum_ratio, P.swap_acceptance_pr, P.energy_ac1]),
              n_shards=n_shards, **pt_kw)
    K = N // n_shards
    owner = []
    for g, e in enumerate(pt.shards.engines):
        assert (e.c0, e.K) == (g * K, K)
        idx = np.flatnonzero((chain >= g * K) & (chain < (g + 1) * K))
        e.set_schedule(betas)
        e.set_states(x[idx], chain[idx], rng[idx])
        assert np.array_equal(e.replica_ids(), g * K + np.arange(K))
        owner.append(idx)
    return pt, owner


def two_phase_swap(engines, scan):
    """LoopbackShards.run_scans' loop for one scan without its explore -> the boundaries (lower shard) whose swap was accepted"""
    n = len(engines)
    begun = [e.swap_begin(scan) for e in engines]
    accepted = []
    for g, e in enumerate(engines):
        stats, active = begun[g]
        nbr = np.zeros(4)
        if active[0]:
            assert g > 0 and begun[g - 1][1][1]
            nbr[0:2] = begun[g - 1][0][2:4]
        if active[1]:
            assert g + 1 < n and begun[g + 1][1][0]
            nbr[2:4] = begun[g + 1][0][0:2]
        accepted.append(e.swap_finish(scan, nbr))
    crossed = []
    for g in range(n - 1):
        a, b = accepted[g][1], accepted[g + 1][0]
        assert a == b, "both sides of a boundary must take the same decision"
        if a:
            w = engines[g].payload_words()
            lo = np.zeros(w); hi = np.zeros(w)
            engines[g].boundary_export(1, lo.ctypes.data, False)
            engines[g + 1].boundary_export(0, hi.ctypes.data, False)
            engines[g].boundary_import(1, hi.ctypes.data, False)
            engines[g + 1].boundary_import(0, lo.ctypes.data, False)
            crossed.append(g)
    return crossed


def _global_swap_recorders(engines):
    """(up, up_n, dn, dn_n, acc, acc_n) keyed by the pair's lower chain, the shards' slices side by side (after their reduce())"""
    lsr = [e.log_sum_ratio() for e in engines]
    acc = [e.swap_acceptance() for e in engines]
    return tuple(np.concatenate([p[k] for p in lsr]) for k in range(4)) + tuple(np.concatenate([p[k] for p in acc]) for k in range(2))


def _advanced(rng):
    """the RNG words after the swap's one draw: the seed word moves on by gamma"""
    out = rng.copy()
    out[:, 0] = rng[:, 0] + rng[:, 1]
    return out


def _assert_slots_hold(engines, owner, expect, x, rng, what):
    """every slot of every shard: chain label c, and the state, RNG words and replica id of the replica that `expect` puts on c"""
    K = engines[0].K
    holder = {int(c): i for i, c in enumerate(expect)}
    rid_of = {int(i): g * K + s for g, idx in enumerate(owner) for s, i in enumerate(idx)}
    for g, e in enumerate(engines):
        xs, cs, rs = e.states()
        ids = e.replica_ids()
        assert sorted(cs) == list(range(g * K, (g + 1) * K)), what + (g, cs)
        for s in range(K):
            i = holder[int(cs[s])]
            assert ids[s] == rid_of[i], what + (g, s, "replica id", ids[s], rid_of[i])
            assert np.array_equal(xs[s], x[i]), what + (g, s, "state")
            assert np.array_equal(rs[s], rng[i]), what + (g, s, "rng", rs[s], rng[i])


def _geometries(N):
    return sorted({N, 2} if N % 2 == 0 else {N})


@pytest.mark.parametrize("gi", range(len(GROUPS)), ids=GROUP_IDS)
def test_one_swap_across_an_engine_boundary(P, gi):
    shape, _, states = GROUPS[gi]
    (betas, x, chain, rng), want = T.swap_expected(gi)
    N = len(states)
    for scan in (1, 2):
        for c, (_, _, _, _, alpha, u) in want[scan].items():
            assert abs(mpf(u) - alpha) >= 1e-6, (shape.id, scan, c, u, float(alpha))
    rng1 = _advanced(rng)
    for n_shards in _geometries(N):
        K = N // n_shards
        for scan in (1, 2):
            pt, owner = _shards(P, shape, n_shards, betas, x, chain, rng)
            engines = pt.shards.engines
            crossed = two_phase_swap(engines, scan)
            for e in engines:
                e.reduce()
            up, un, dn, dnn, acc, acc_n = _global_swap_recorders(engines)
            assert len(up) == N - 1
            expect = chain.copy()
            crossing = []
            for c in range(N - 1):
                what = (shape.id, n_shards, scan, c)
                if c not in want[scan]:
                    assert un[c] == 0 and dnn[c] == 0 and acc_n[c] == 0, what
                    continue
                nu, du, nd, dd, alpha, u = want[scan][c]
                assert un[c] == 1 and dnn[c] == 1 and acc_n[c] == 1, what
                assert math.isfinite(up[c]) and math.isfinite(dn[c]), what
                assert abs(mpf(float(up[c])) - (nu - du)) <= LP_RTOL * (abs(nu) + abs(du)) + LP_ATOL, what + (up[c], float(nu - du))
                assert abs(mpf(float(dn[c])) - (nd - dd)) <= LP_RTOL * (abs(nd) + abs(dd)) + LP_ATOL, what + (dn[c], float(nd - dd))
                with np.errstate(over="ignore"):
                    assert math.isclose(acc[c], min(1.0, float(np.exp(up[c] + dn[c]))), rel_tol=1e-9, abs_tol=1e-300), what
                if u < alpha:
                    i, j = (int(np.flatnonzero(chain == k)[0]) for k in (c, c + 1))
                    expect[i], expect[j] = c + 1, c
                    if (c + 1) % K == 0:
                        crossing.append(c // K)
            what = (shape.id, n_shards, scan)
            assert crossed == crossing, what + (crossed, crossing)
            _assert_slots_hold(engines, owner, expect, x, rng1, what)
            # suff and suff2 travelled with the row: the next explore step starts from the definition's log density of the state each chain holds now
            for e in engines:
                e.explore(1)
            two_phase_swap(engines, 2)
            holder = {int(c): i for i, c in enumerate(expect)}
            for g, e in enumerate(engines):
                e.reduce()
                _, n, mom = e.energy_ac1()
                for cl in range(K):
                    c = g * K + cl
                    assert n[cl] == 1, what + (c,)
                    T._lp_close(mom[cl, 0], _mp_lp(gi, c, holder[c]), ("before", shape.id, n_shards, scan, c, states[holder[c]][0]))


# ---- (d) -------------------------------------------------------------------------------------------------------------------------------
_NEAR = {}                 # gi -> (pairs, pairs within 1e-6 of the decision's edge)


def _message_kernels_case(P, gi):
    shape, _, states = GROUPS[gi]
    betas, x, chain, rng = T.layout(gi, shape, states)
    N = len(states)
    # the twin: one engine, the same replicas; its explore step's states are where the definition is evaluated
    twin = T._engine(P, shape, _explorer(P, shape), betas, x, chain, rng, record=[P.log_sum_ratio, P.swap_acceptance_pr, P.energy_ac1])
    twin.explore(1)
    x1, c1, r1 = twin.states()
    assert np.array_equal(c1, chain)
    twin.swap(1)
    x2, c2, r2 = twin.states()
    twin.reduce()
    t_up, t_un, t_dn, t_dnn = twin.log_sum_ratio()
    t_acc, t_accn = twin.swap_acceptance()
    # the shards: one chain each, one scan of the message kernels
    pt, owner = _shards(P, shape, N, betas, x, chain, rng, device_messages=True)
    engines = pt.shards.engines
    pt.shards.run_scans(1, 1)
    applied = [list(e.shard_sync()) for e in engines]
    for e in engines:
        e.reduce()
    up, un, dn, dnn, acc, acc_n = _global_swap_recorders(engines)
    for a, b in ((up, t_up), (un, t_un), (dn, t_dn), (dnn, t_dnn), (acc, t_acc), (acc_n, t_accn)):
        assert np.array_equal(a, b), (shape.id, a, b)
    _assert_slots_hold(engines, owner, c2, x2, r2, (shape.id, "twin"))
    slot = {int(chain[i]): i for i in range(N)}
    near = pairs = 0
    for c in range(0, N - 1, 2):
        i, j = slot[c], slot[c + 1]
        what = (shape.id, c)
        swapped = bool(c2[i] == c + 1)
        assert swapped == bool(c2[j] == c) and (swapped or (c2[i] == c and c2[j] == c + 1)), what
        assert applied[c][1] == int(swapped) and applied[c + 1][0] == int(swapped), what + (applied[c], applied[c + 1])
        nu, du = E.mp_lp(shape, betas[c + 1], x1[i]), E.mp_lp(shape, betas[c], x1[i])
        nd, dd = E.mp_lp(shape, betas[c], x1[j]), E.mp_lp(shape, betas[c + 1], x1[j])
        assert un[c] == 1 and dnn[c] == 1 and acc_n[c] == 1, what
        assert abs(mpf(float(up[c])) - (nu - du)) <= LP_RTOL * (abs(nu) + abs(du)) + LP_ATOL, what + (up[c], float(nu - du))
        assert abs(mpf(float(dn[c])) - (nd - dd)) <= LP_RTOL * (abs(nd) + abs(dd)) + LP_ATOL, what + (dn[c], float(nd - dd))
        with np.errstate(over="ignore"):
            assert math.isclose(acc[c], min(1.0, float(np.exp(up[c] + dn[c]))), rel_tol=1e-9, abs_tol=1e-300), what
        alpha = min(mpf(1), mp.exp((nu - du) + (nd - dd)))
        u = O.OracleRng(state=(int(r1[i, 0]), int(r1[i, 1]))).rand()
        pairs += 1
        if abs(mpf(u) - alpha) < 1e-6:             # too close to call from the definition: the twin's decision (held above) stands alone
            near += 1
            continue
        assert swapped == bool(u < alpha), what + (u, float(alpha))
    for c in range(1, N - 1, 2):
        assert un[c] == 0 and dnn[c] == 0 and acc_n[c] == 0, (shape.id, c)
    _NEAR[gi] = (pairs, near)


@pytest.mark.parametrize("gi", range(len(GROUPS)), ids=GROUP_IDS)
def test_one_scan_of_the_message_kernels_against_a_twin_and_the_definition(P, gi):
    _message_kernels_case(P, gi)


def test_few_message_kernel_pairs_were_too_close_to_call(P):
    """over all groups at most 2 % of the pairs of (d) were left to the twin alone (a group the cases above have not run is run here)"""
    for gi in range(len(GROUPS)):
        if gi not in _NEAR:
            _message_kernels_case(P, gi)
    pairs, near = (sum(v[k] for v in _NEAR.values()) for k in (0, 1))
    print("message kernels against the definition: %d pairs, %d within 1e-6 of the decision's edge" % (pairs, near))
    assert near <= 0.02 * pairs, (near, pairs)


# ---- (e) -------------------------------------------------------------------------------------------------------------------------------
def _set_state_inputs(P, family):
    if family == "glm":
        return test_gpu_glm._inputs(P, seed=SEED, n_rounds=2)
    target, explorer = _lattice_target(P, "spinglass-L9")
    return P.Inputs(target=target, n_chains=8, n_rounds=2, seed=SEED, explorer=explorer, show_report=False)


@pytest.mark.parametrize("sharded", [True, False], ids=["shard-1-of-2", "single"])
@pytest.mark.parametrize("family", ["glm", "spinglass"])
def test_a_refused_set_state_changes_nothing(P, family, sharded):
    def engine():
        pt = P.PT(_set_state_inputs(P, family), n_shards=2) if sharded else P.PT(_set_state_inputs(P, family))
        return pt, (pt.shards.engines[1] if sharded else pt.replicas)
    (pt_a, eng), (pt_b, twin) = engine(), engine()
    if family == "spinglass":                                    # (the lattice starts from one row everywhere: give the slots rows of their own)
        for e in (eng, twin):
            e.explore(1)
    x, chain, rng = eng.states()
    for u, v in zip((x, chain, rng), twin.states()):
        assert np.array_equal(u, v)
    other = (1.0 - x) if family == "spinglass" else x + 1.0
    outside, repeated = chain.copy(), chain.copy()
    outside[0] = eng.c0 - 1 if sharded else eng.N                # (on the shard: a chain of the run, of the other shard)
    repeated[0] = repeated[1]
    for bad in (outside, repeated):
        with pytest.raises(P.PteError, match="pte_set_state: chain is not a permutation of the local chains"):
            eng.set_states(other, bad, rng[::-1].copy())
        for u, v in zip(eng.states(), twin.states()):
            assert np.array_equal(u, v)
    for e in (eng, twin):
        e.explore(2 if family == "spinglass" else 1)
    for u, v in zip(eng.states(), twin.states()):
        assert np.array_equal(u, v)
    eng.set_states(other, chain[::-1].copy(), rng)               # and a permutation is taken
    x2, c2, _ = eng.states()
    assert np.array_equal(c2, chain[::-1]) and not np.array_equal(x2, twin.states()[0])
