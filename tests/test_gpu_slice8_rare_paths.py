"""The three rarely taken paths of lane 0 in the speculative round of the default SliceSampler kernel (pte_slice8.hpp), after round 8 moved
the DECISIONS to enter them to the scalar side of the round:

  * the head exponential of the certain hypothesis needs the ziggurat's slow path      <- bit p of a window-wide mask built when the window is filled
  * it needs more than S8_BD = 3 doublings                                             <- bit 0 of the one compare the doubling block ends with
  * it needs more than S8_BS = 9 shrinkage proposals                                   <- bit 0 of the EXEC mask the shrinkage block ends with

Nothing about WHICH path a round takes changed, so every comparison is array_equal against the oracle (tests/oracle.py): replica states, chains,
RNG words (the same draws consumed), index process and the swap / explorer recorders, per round, over rounds 1-2 (2 + 4 = 6 scans, with the
schedule adaptation in between).  The one exception is the one tests/test_gpu_slice8_doubling.py documents (ORACLE_RTOL: the mean of the swap
acceptance probabilities goes through the device's exp); its helpers and tolerances are used as they are.

Cases: 8-16 chains; d = 64 (a quarter of the 256-coordinate block a round works in), 192 (three of its four 64-chunks), 256 (one full block).
  w = 0.5   more than a third of the updates double more than three times: lane 0's doubling continuation
  w = 40    a seventh of the updates needs more than nine proposals: lane 0's shrinkage continuation
  w = 10    the default; at d = 256 this is also the case the slow-path mask is checked on (below)
  p = 4     the smallest p the default-range instantiation accepts (kcap = 4: one step of headroom beyond the budget)
  max_iter = 9   cap_iters == S8_BS: an unfinished lane 0 may NOT continue and goes to the exact sequential procedure, which raises what the
            reference raises.  The oracle raises in the first scan at these sizes (a few per cent of the updates need a tenth proposal), so
            the expectation is that error.
  p = 3, p = 21  the generic instantiation (keeps the complete conditions)
The many-replica twin (> 2048 chains) is too large for this file; tests/test_gpu_slice8_doubling.py and tests/test_gpu_parity.py run it.

What the CPU tests below establish with the oracle alone (its generator and the reference's procedure restated in Python, held to the
oracle's own states after the first scan), for the updates that start in the FIRST window of every replica and scan -- the only ones whose
window position is known without the kernel (a scan starts with a fresh window at p = 0; later windows start wherever a round happened to
end).  Counts at seed 3, printed by the tests:
  (8, 256, w = 10):  2825 updates, slow-path head exponentials at p < 64: 14, at 384 <= p <= 432: 4
  (8, 64, w = 0.5):  2215 updates, 843 with more than three doublings
  (8, 192, w = 40):  2195 updates, 318 with more than nine proposals
On "both ends of the mask": lane 0's position is p <= REFILL_AT = 432 when the round tests it (beyond, the window is refilled first), so of
the eight 64-draw ballots of a 512-draw window the round can index the first seven; the LAST 64 positions (448-511) are never lane 0's.  The
ends asked for here are therefore the first ballot word (p < 64) and the last one the round can reach (384 <= p <= 432).

Split calls: pte_run_scans(1, 3) followed by pte_run_scans(4, 5) -- the second argument is a count, the first the number of the call's first
scan, which fixes the DEO parity -- equals one call of eight scans, in both forms of the scan loop."""
import numpy as np
import pytest

import oracle as O
from test_gpu_slice8_doubling import NAMES, ORACLE_RTOL, _rows

ROUNDS = 2                       # 2 + 4 = 6 scans
SEED = 3
DEFAULT = ("k_explore_slice8", "k_scans_slice8")
GENERIC = ("k_explore_slice8_generic", "k_scans_slice8_generic")
REFILL_AT = 432                  # pte_slice7.hpp: PTE_S7_WIN - PTE_S7_MARGIN

#        name        N   d    w     p  max_iter  kernels
CASES = {"w0.5":    (8,  64,  0.5,  20, 1024, DEFAULT),
         "w40":     (8,  192, 40.0, 20, 1024, DEFAULT),
         "w10":     (8,  256, 10.0, 20, 1024, DEFAULT),
         "p4":      (12, 192, 0.5,  4,  1024, DEFAULT),
         "p3":      (8,  64,  0.5,  3,  1024, GENERIC),
         "p21":     (16, 256, 0.5,  21, 1024, GENERIC)}
MAX_ITER_CASE = (8, 64, 40.0, 20, 9, DEFAULT)

_REF = {}


def _oracle(N, d, w, p, max_iter):
    return O.OraclePT(n_chains=N, dim=d, seed=SEED, explorer=O.EXPLORER_SLICE, slice_w=w, slice_p=p, slice_max_iter=max_iter)


def _reference(N, d, w, p, max_iter):
    """the oracle's rounds, computed once per configuration and left unchanged: per round the recorders and the states after it"""
    key = (N, d, w, p, max_iter)
    if key not in _REF:
        ref, out = _oracle(N, d, w, p, max_iter), []
        for _ in range(ROUNDS):
            ref.run_round()
            m, n = ref.swap_pr()
            am, an, ss, sn = ref.explorer_stats()
            x, chain, rng = ref.states()
            row = [ref.index_process(), np.array(ref.round_trip()), n, m, an, am, sn, ss, chain, rng, x]
            for a in row:
                a.setflags(write=False)
            out.append(row)
        _REF[key] = out
    return _REF[key]


# ---- the reference's coordinate update restated, to learn WHERE in a replica's stream things happen (the oracle reports states, not draws)
def _replay(x, seed, gamma, prec, w, p, max_iter, whole_scan):
    """one replica's explore step on toy_mvn_target (log density -prec / 2 sum x^2) with the oracle's generator:
    -> [(draws consumed before this update = window position of its head exponential, slow-path exponential?, doublings, proposals)], x after.
    Stops after the first window (position > REFILL_AT) unless whole_scan."""
    x = x.copy()
    rng = O.OracleRng(state=(int(seed), int(gamma)))
    pos, out = 0, []
    for _ in range(3):                                                       # n_passes
        for c in range(len(x)):
            if pos > REFILL_AT and not whole_scan:
                return out, x
            S = float(np.dot(x, x)) - x[c] * x[c]

            def lp(v):
                return -0.5 * prec * (S + v * v)
            s0 = rng.state[0]
            E = rng.randexp()
            used = next(k for k in range(1, 64) if (s0 + k * int(gamma)) % 2 ** 64 == rng.state[0])     # the fast path takes ONE draw
            z = lp(x[c]) - E
            L = x[c] - w * rng.rand()
            R = L + w
            K = p
            while K > 0 and (z < lp(L) or z < lp(R)):
                if rng.rand() <= 0.5:
                    L = L - (R - L)
                else:
                    R = R + (R - L)
                K -= 1
            n = 0
            while True:
                n += 1
                assert n <= max_iter
                v = L + rng.rand() * (R - L)
                if z < lp(v):
                    break
                if v < x[c]:
                    L = v
                else:
                    R = v
            x[c] = v
            out.append((pos, used > 1, p - K, n))
            pos += used + 1 + (p - K) + n
    return out, x


_EVENTS = {}


def _first_window_events(name):
    """every update that starts in the first window of a replica and scan of the case, over its ROUNDS rounds; the restated procedure is held
    to the oracle's states after the whole first scan"""
    if name not in _EVENTS:
        N, d, w, p, max_iter, _ = CASES[name]
        ref, ev = _oracle(N, d, w, p, max_iter), []
        for rnd in range(1, ROUNDS + 1):
            ref.begin_round()
            for s in range(2 ** rnd):
                x, chain, rng = ref.states()
                beta = ref.schedule()
                ref.run_scans(1)
                x_after = ref.states()[0]
                for r in range(N):
                    if chain[r] == 0:                                        # the reference chain is refreshed iid, not by the explorer
                        continue
                    prec = (1.0 - beta[chain[r]]) * 1.0 + beta[chain[r]] * 10.0
                    first = rnd == 1 and s == 0
                    e, xe = _replay(x[r], rng[r, 0], rng[r, 1], prec, w, p, max_iter, whole_scan=first)
                    if first:
                        assert np.array_equal(xe, x_after[r]), "the restated update does not reproduce the oracle's scan"
                    ev += [t for t in e if t[0] <= REFILL_AT]
            ref.end_round()
        _EVENTS[name] = ev
    return _EVENTS[name]


def test_slow_path_exponentials_at_both_ends_of_the_mask():
    """CPU, the oracle alone: the w = 10, d = 256 case holds slow-path head exponentials in the first ballot word of a window (p < 64) and in
    the last one lane 0 can reach (384 <= p <= REFILL_AT; see the module docstring for why not 448-511)."""
    ev = _first_window_events("w10")
    lo = sum(1 for pos, slow, _, _ in ev if slow and pos < 64)
    hi = sum(1 for pos, slow, _, _ in ev if slow and pos >= 384)
    print("%d updates in first windows, %d slow-path heads; at p < 64: %d, at 384 <= p <= %d: %d" % (len(ev), sum(e[1] for e in ev), lo, REFILL_AT, hi))
    assert lo >= 1 and hi >= 1


def test_continuations_are_exercised():
    """CPU, the oracle alone: w = 0.5 sends many updates beyond three doublings, w = 40 beyond nine proposals (every update is lane 0 of some
    round or a speculative hypothesis that then fails its budget and BECOMES lane 0 of the next round)."""
    dbl = sum(1 for _, _, k, _ in _first_window_events("w0.5") if k > 3)
    shr = sum(1 for _, _, _, n in _first_window_events("w40") if n > 9)
    print("beyond three doublings at w = 0.5: %d; beyond nine proposals at w = 40: %d" % (dbl, shr))
    assert dbl >= 100 and shr >= 100


def test_max_iter_at_the_budget_is_an_error_in_the_oracle():
    """CPU, the oracle alone: with max_iter = 9 some update needs a tenth proposal, so the case exists -- the oracle raises"""
    N, d, w, p, max_iter, _ = MAX_ITER_CASE
    ref = _oracle(N, d, w, p, max_iter)
    with pytest.raises(RuntimeError, match="maximum number of iterations"):
        for _ in range(ROUNDS):
            ref.run_round()


def _hold_to_oracle(P, name, two_launches):
    from pigeons_amd import _lib
    N, d, w, p, max_iter, (kernel, scan_loop) = CASES[name]
    got = _rows(P, N, d, P.SliceSampler(w=w, p=p, max_iter=max_iter), ROUNDS, SEED, _lib.KERNEL_TWO_LAUNCHES if two_launches else 0,
                (kernel, "" if two_launches else scan_loop))
    ref = _reference(N, d, w, p, max_iter)
    bad = []
    for r in range(ROUNDS):
        for nm, a, b in zip(NAMES, got[r], ref[r]):
            if not np.array_equal(a, b, equal_nan=True):
                dif = float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300))) if a.shape == b.shape else float("inf")
                print("round %d %s against the oracle: largest relative difference %.3e" % (r + 1, nm, dif))
                if not dif <= ORACLE_RTOL.get(nm, 0.0):
                    bad.append((r + 1, nm, dif))
    assert not bad, bad


@pytest.mark.gpu
@pytest.mark.parametrize("two_launches", [False, True])
@pytest.mark.parametrize("name", sorted(CASES))
def test_rare_paths_against_the_oracle(P, name, two_launches):
    _hold_to_oracle(P, name, two_launches)


@pytest.mark.gpu
@pytest.mark.parametrize("two_launches", [False, True])
def test_max_iter_at_the_budget_raises_as_the_oracle_does(P, two_launches):
    """cap_iters == S8_BS: lane 0, unfinished after nine proposals, must go to the exact sequential procedure (not into its loop), which raises"""
    from pigeons_amd import _lib
    N, d, w, p, max_iter, (kernel, scan_loop) = MAX_ITER_CASE
    pt = P.PT(P.Inputs(target=P.toy_mvn_target(d), n_chains=N, n_rounds=ROUNDS, seed=SEED, explorer=P.SliceSampler(w=w, p=p, max_iter=max_iter),
                       record=[P.round_trip, P.index_process, P.log_sum_ratio], show_report=False),
              debug_kernel=_lib.KERNEL_TWO_LAUNCHES if two_launches else 0)
    assert (pt.replicas.kernel_name(), pt.replicas.scan_loop_name()) == (kernel, "" if two_launches else scan_loop)
    with pytest.raises(P.PteError, match="Maximum number of iterations"):
        for _ in range(ROUNDS):
            P.next_round(pt); P.run_one_round(pt)


@pytest.mark.gpu
@pytest.mark.parametrize("two_launches", [False, True])
@pytest.mark.parametrize("name", ["w10", "w0.5"])
def test_split_calls_equal_one_call(P, name, two_launches):
    """scans 1-3 and 4-8 in two calls (a fresh window, mask and p = 0 at the head of every scan; epochs carry over) against one call of eight"""
    from pigeons_amd import _lib
    N, d, w, p, max_iter, _ = CASES[name]
    out = []
    for calls in ([(1, 8)], [(1, 3), (4, 5)]):
        pt = P.PT(P.Inputs(target=P.toy_mvn_target(d), n_chains=N, n_rounds=4, seed=SEED, explorer=P.SliceSampler(w=w, p=p, max_iter=max_iter),
                           record=[P.round_trip, P.index_process, P.log_sum_ratio], show_report=False),
                  debug_kernel=_lib.KERNEL_TWO_LAUNCHES if two_launches else 0)
        e = pt.replicas
        for first, n in calls:
            e.run_scans(first, n)
        e.reduce()
        out.append([np.array(a).copy() for a in (e.index_process(), *e.swap_acceptance(), *e.states())])
    for a, b in zip(*out):
        assert np.array_equal(a, b, equal_nan=True)
    ref = _oracle(N, d, w, p, max_iter)
    ref.begin_round(); ref.run_scans(8)
    x, chain, rng = ref.states()
    assert np.array_equal(out[0][-3], x) and np.array_equal(out[0][-2], chain) and np.array_equal(out[0][-1], rng)


@pytest.fixture(scope="module")
def P():
    import pigeons_amd
    return pigeons_amd
