"""Lane 0's slow-path head exponential in the default SliceSampler kernel after round 11 (pte_slice8.hpp): the fill of a draw window decides
the slow-path exponentials it can (the rule and its host restatement: tests/test_slice8_slow_resolve_rule.py) and leaves a record per lane;
behind the slow-mask branch lane 0 looks its position up and runs the sequential procedure of round 10 only where there is no record.

Where the value comes from changes, not the value: every comparison is array_equal -- replica states, chains, RNG words (the same draws
consumed), index process, swap and explorer recorders, per round -- against the oracle AND against the exact sequential kernel on the same
device (k_explore_slice, debug_kernel = 1), with the helpers and the one tolerance of tests/test_gpu_slice8_doubling.py (ORACLE_RTOL: the
mean of the swap acceptance probabilities goes through the device's exp).

Case: the small shape of tests/test_gpu_slice8_slow_exp.py with a row that crosses the 256-coordinate block and ends in a partial one --
N = 6, d = 300, rounds 1-3 = 14 scans = 5 x 300 x 3 x 14 = 63 k explorer exponentials -- at w = 0.5 (lane 0 re-reads its draws a second time
after the head moved them: more than three doublings), 10 (the default) and 40 (long shrinkage), under both ziggurat-tail policies, in both
forms of the scan loop (k_scans_slice8, and k_explore_slice8 + a swap launch per scan).

The CPU test classifies every slow-path HEAD exponential of the case from the oracle's own stream (the reference's coordinate update restated
in Python and held to the oracle's states after every scan), by what the sequential procedure does there:
    wedge accept               two draws, layer > 0                    -> the fill's record (x, 2)
    next candidate fast        three draws                             -> the fill's record (s_e[i + 2], 3)
    tail                       layer 0                                 -> no record: sequential path, reads the policy word
    deeper                     four draws or more                      -> no record: sequential path
(which of the first two kinds find their record also depends on where the head stands in its window -- the last two positions and a lane's
earlier slow draw have none -- so both paths behind the branch run for them too).  Each class must occur at least five times per case.
Counts at seed 3, printed by the test (wedge accept / next candidate fast / tail / deeper):
    default policy  w = 0.5: 681 / 665 / 31 / 13    w = 10: 686 / 643 / 29 / 12    w = 40: 667 / 718 / 26 / 16
    log1p policy    w = 0.5: 699 / 643 / 30 / 15    w = 10: 716 / 649 / 33 / 15    w = 40: 673 / 690 / 27 / 14"""
import numpy as np
import pytest

import oracle as O
from test_gpu_slice8_doubling import NAMES, ORACLE_RTOL, _rows
from test_gpu_slice8_slow_exp import MASK52, MASK64, POLICIES, _mix64, _policy

N, D, P_DBL, MAX_ITER = 6, 300, 20, 1024
WIDTHS = [0.5, 10.0, 40.0]
ROUNDS = 3                       # 2 + 4 + 8 = 14 scans
SEED = 3
CLASSES = ("wedge accept", "next candidate fast", "tail", "deeper")


def _oracle(w):
    return O.OraclePT(n_chains=N, dim=D, seed=SEED, explorer=O.EXPLORER_SLICE, slice_w=w, slice_p=P_DBL, slice_max_iter=MAX_ITER)


_REF, _SEQ = {}, {}


def _reference(pname, w):
    """the oracle's rounds under the policy, computed once and left unchanged: per round the recorders and the states after it"""
    if (pname, w) not in _REF:
        with _policy(POLICIES[pname]):
            ref, out = _oracle(w), []
            for _ in range(ROUNDS):
                ref.run_round()
                m, n = ref.swap_pr()
                am, an, ss, sn = ref.explorer_stats()
                x, chain, rng = ref.states()
                row = [ref.index_process(), np.array(ref.round_trip()), n, m, an, am, sn, ss, chain, rng, x]
                for a in row:
                    a.setflags(write=False)
                out.append(row)
        _REF[pname, w] = out
    return _REF[pname, w]


def _sequential(P, pname, w):
    """the exact sequential kernel's run on the same device under the policy (the caller has set it), computed once"""
    from pigeons_amd import _lib
    if (pname, w) not in _SEQ:
        _SEQ[pname, w] = _rows(P, N, D, P.SliceSampler(w=w, p=P_DBL, max_iter=MAX_ITER), ROUNDS, SEED, _lib.KERNEL_SLICE_SEQUENTIAL, ("k_explore_slice", ""))
        for row in _SEQ[pname, w]:
            for a in row:
                a.setflags(write=False)
    return _SEQ[pname, w]


def _head_class(s0, gamma, used, ke):
    """what the sequential procedure did for the exponential drawn from stream state s0 with `used` > 1 draws"""
    ri = _mix64((s0 + gamma) & MASK64) & MASK52
    assert not ri < int(ke[ri & 0xFF])
    if ri & 0xFF == 0:
        assert used == 2
        return "tail"
    if used == 2:
        return "wedge accept"
    r2 = _mix64((s0 + 3 * gamma) & MASK64) & MASK52
    if used == 3:
        assert r2 < int(ke[r2 & 0xFF])
        return "next candidate fast"
    assert used >= 4 and not r2 < int(ke[r2 & 0xFF])
    return "deeper"


def _replay_scan(x, seed, gamma, prec, w, ke, counts):
    """one replica's explore step on toy_mvn_target (log density -prec / 2 sum x^2), its slow-path head exponentials counted by class: -> x after"""
    x = x.copy()
    seed, gamma = int(seed), int(gamma)
    rng = O.OracleRng(state=(seed, gamma))
    ginv = pow(gamma, -1, 1 << 64)
    for _ in range(3):                                                       # n_passes
        for c in range(len(x)):
            S = float(np.dot(x, x)) - x[c] * x[c]

            def lp(v):
                return -0.5 * prec * (S + v * v)
            s0 = rng.state[0]
            E = rng.randexp()
            used = ((rng.state[0] - s0) * ginv) & MASK64
            if used > 1:
                counts[_head_class(s0, gamma, used, ke)] += 1
            z = lp(x[c]) - E
            L = x[c] - w * rng.rand()
            R = L + w
            K = P_DBL
            while K > 0 and (z < lp(L) or z < lp(R)):
                if rng.rand() <= 0.5:
                    L = L - (R - L)
                else:
                    R = R + (R - L)
                K -= 1
            n = 0
            while True:
                n += 1
                assert n <= MAX_ITER
                v = L + rng.rand() * (R - L)
                if z < lp(v):
                    break
                if v < x[c]:
                    L = v
                else:
                    R = v
            x[c] = v
    return x


@pytest.mark.parametrize("w", WIDTHS)
@pytest.mark.parametrize("pname", sorted(POLICIES))
def test_the_streams_hold_every_class_of_slow_head(pname, w):
    """CPU, the oracle alone: a condition on the input, not a measurement -- each class of slow-path head occurs at least five times"""
    ke = O.zig_table("ke")
    counts = {k: 0 for k in CLASSES}
    with _policy(POLICIES[pname]):
        ref = _oracle(w)
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
                    xe = _replay_scan(x[r], rng[r, 0], rng[r, 1], prec, w, ke, counts)
                    assert np.array_equal(xe, x_after[r]), "the restated update does not reproduce the oracle's scan"
            ref.end_round()
    print("%s policy, w = %g: slow-path heads: %s" % (pname, w, ", ".join("%s %d" % (k, counts[k]) for k in CLASSES)))
    assert all(counts[k] >= 5 for k in CLASSES), counts


@pytest.mark.gpu
@pytest.mark.parametrize("two_launches", [False, True])
@pytest.mark.parametrize("w", WIDTHS)
@pytest.mark.parametrize("pname", sorted(POLICIES))
def test_against_the_oracle_and_the_sequential_kernel(P, pname, w, two_launches):
    from pigeons_amd import _lib
    ref = _reference(pname, w)
    with _policy(POLICIES[pname], P):
        seq = _sequential(P, pname, w)
        got = _rows(P, N, D, P.SliceSampler(w=w, p=P_DBL, max_iter=MAX_ITER), ROUNDS, SEED, _lib.KERNEL_TWO_LAUNCHES if two_launches else 0,
                    ("k_explore_slice8", "" if two_launches else "k_scans_slice8"))
    bad = []
    for r in range(ROUNDS):
        for name, a, b, c in zip(NAMES, got[r], ref[r], seq[r]):
            if not np.array_equal(a, c, equal_nan=True):
                bad.append((r + 1, name, "sequential kernel"))
            if not np.array_equal(a, b, equal_nan=True):
                dif = float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300))) if a.shape == b.shape else float("inf")
                print("round %d %s against the oracle: largest relative difference %.3e" % (r + 1, name, dif))
                if not dif <= ORACLE_RTOL.get(name, 0.0):
                    bad.append((r + 1, name, "oracle", dif))
    assert not bad, bad


@pytest.fixture(scope="module")
def P():
    import pigeons_amd
    return pigeons_amd
