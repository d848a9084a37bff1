"""Lane 0's slow-path head exponential in the default SliceSampler kernel after round 10 (pte_slice8.hpp).

Round 10 changed how the block behind the slow-mask bit test gets its inputs, not what it computes: the slow-path exponential of the certain
hypothesis (and of the exact sequential procedure) runs randexp_from_raw_hot (pte_device.hpp) -- the policy word (include/pte_rng_policy.h:
which formula the ziggurat TAIL uses) comes from the kernel's own LDS copy, read on the tail branch only, and the table words of a candidate
are requested together.
So every comparison is array_equal -- replica states, chains, RNG words (the same draws consumed), index process, swap and explorer recorders,
per round -- against the oracle AND against the exact sequential kernel on the same device (k_explore_slice, debug_kernel = 1, which reads the
policy word the old way), with the helpers and the one tolerance of tests/test_gpu_slice8_doubling.py (ORACLE_RTOL: the mean of the swap
acceptance probabilities goes through the device's exp).

Case: N = 16, d = 256, w = 10 (the defaults), rounds 1-2 = 6 scans = 15 x 256 x 3 x 6 = 69 k explorer exponentials (the reference chain is
refreshed iid), in both forms of the scan loop (k_scans_slice8, and k_explore_slice8 + a swap launch per scan), under BOTH tail policies: the
default and RNG_TAIL_LOG1P, set on the engine and on the oracle and restored in a `finally`.  The copy of the policy word is the one thing here
that can be wrong without any other test noticing: under the default policy a kernel that ignored it would still pass.

What the CPU test below establishes for this seed with the oracle's generator alone (the reference's coordinate update restated in Python and
held to the oracle's states after EVERY scan): how many head exponentials take the ziggurat's slow path, how many of those reach the TAIL
(layer 0, beyond ke[0]: the only draws that read the policy word), and how many 512-draw windows a replica's scan consumes (a refill each).
Counts at seed 3, printed by the test: default policy 1534 slow-path heads, 23 tail draws; log1p policy 1526 and 23; every replica and scan
consumes 8 to 10 windows."""
import numpy as np
import pytest

import oracle as O
from test_gpu_slice8_doubling import NAMES, ORACLE_RTOL, _rows

N, D, W, P_DBL, MAX_ITER = 16, 256, 10.0, 20, 1024
ROUNDS = 2                       # 2 + 4 = 6 scans
SEED = 3
WIN = 512                        # pte_slice7.hpp: PTE_S7_WIN draws per window
POLICIES = {"default": 0, "log1p": O.RNG_TAIL_LOG1P}
MASK64, MASK52 = (1 << 64) - 1, (1 << 52) - 1


class _policy:
    """the tail policy on the oracle (and, with the package, on the engine) for a `with` block; the default again afterwards, whatever happens"""

    def __init__(self, policy, P=None):
        self.policy, self.P = policy, P

    def __enter__(self):
        try:
            O.set_rng_policy(self.policy)
            if self.P is not None:
                from pigeons_amd.engine import set_rng_policy
                set_rng_policy(self.policy)
        except BaseException:
            self.__exit__()
            raise

    def __exit__(self, *exc):
        try:
            if self.P is not None:
                from pigeons_amd.engine import set_rng_policy
                set_rng_policy(0)
        finally:
            O.set_rng_policy(0)


def _oracle():
    return O.OraclePT(n_chains=N, dim=D, seed=SEED, explorer=O.EXPLORER_SLICE, slice_w=W, slice_p=P_DBL, slice_max_iter=MAX_ITER)


_REF, _SEQ = {}, {}


def _reference(pname):
    """the oracle's rounds under the policy, computed once and left unchanged: per round the recorders and the states after it"""
    if pname not in _REF:
        with _policy(POLICIES[pname]):
            ref, out = _oracle(), []
            for _ in range(ROUNDS):
                ref.run_round()
                m, n = ref.swap_pr()
                am, an, ss, sn = ref.explorer_stats()
                x, chain, rng = ref.states()
                row = [ref.index_process(), np.array(ref.round_trip()), n, m, an, am, sn, ss, chain, rng, x]
                for a in row:
                    a.setflags(write=False)
                out.append(row)
        _REF[pname] = out
    return _REF[pname]


def _sequential(P, pname):
    """the exact sequential kernel's run on the same device under the policy (the caller has set it), computed once"""
    from pigeons_amd import _lib
    if pname not in _SEQ:
        _SEQ[pname] = _rows(P, N, D, P.SliceSampler(w=W, p=P_DBL, max_iter=MAX_ITER), ROUNDS, SEED, _lib.KERNEL_SLICE_SEQUENTIAL, ("k_explore_slice", ""))
        for row in _SEQ[pname]:
            for a in row:
                a.setflags(write=False)
    return _SEQ[pname]


# ---- the reference's coordinate update restated with the oracle's generator, to learn what the streams hold (the oracle reports states, not draws)
def _mix64(z):
    z = ((z ^ (z >> 30)) * 0xbf58476d1ce4e5b9) & MASK64
    z = ((z ^ (z >> 27)) * 0x94d049bb133111eb) & MASK64
    return z ^ (z >> 31)


def _reaches_tail(s0, gamma, used, ke):
    """does the exponential drawn from stream state s0 with `used` draws evaluate the ziggurat's tail?  Candidates sit at draws 1, 3, 5, ...
    (a rejected wedge candidate consumed a uniform); the tail is a candidate in layer 0 beyond ke[0], and ends the procedure"""
    k = 1
    while k <= used:
        ri = _mix64((s0 + k * gamma) & MASK64) & MASK52
        idx = ri & 0xFF
        if ri < int(ke[idx]):
            assert k == used
            return False
        if idx == 0:
            assert k + 1 == used
            return True
        k += 2
    assert k == used + 1                                                   # (the wedge accepted the last candidate)
    return False


def _replay_scan(x, seed, gamma, prec, ke):
    """one replica's explore step on toy_mvn_target (log density -prec / 2 sum x^2): -> x after, draws consumed, slow-path head exponentials, tail draws"""
    x = x.copy()
    seed, gamma = int(seed), int(gamma)
    rng = O.OracleRng(state=(seed, gamma))
    ginv = pow(gamma, -1, 1 << 64)
    slow = tails = 0
    for _ in range(3):                                                       # n_passes
        for c in range(len(x)):
            S = float(np.dot(x, x)) - x[c] * x[c]

            def lp(v):
                return -0.5 * prec * (S + v * v)
            s0 = rng.state[0]
            E = rng.randexp()
            used = ((rng.state[0] - s0) * ginv) & MASK64
            if used > 1:
                slow += 1
                tails += _reaches_tail(s0, gamma, used, ke)
            z = lp(x[c]) - E
            L = x[c] - W * rng.rand()
            R = L + W
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
    return x, ((rng.state[0] - seed) * ginv) & MASK64, slow, tails


@pytest.mark.parametrize("pname", sorted(POLICIES))
def test_the_streams_hold_slow_paths_tails_and_refills(pname):
    """CPU, the oracle alone, under each policy: at least 100 slow-path head exponentials and at least 3 ziggurat-tail draws over the six
    scans, and every replica's scan runs through at least five windows.  (Every slow-path exponential is lane 0's in some round: a speculative
    hypothesis that meets one ends the chase and its coordinate is lane 0 of the next round.  A window serves at most 512 draws, so a scan
    that consumes n draws refills at least n // 512 times.)"""
    ke = O.zig_table("ke")
    with _policy(POLICIES[pname]):
        ref = _oracle()
        slow = tails = updates = 0
        windows = []
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
                    xe, draws, sl, tl = _replay_scan(x[r], rng[r, 0], rng[r, 1], prec, ke)
                    assert np.array_equal(xe, x_after[r]), "the restated update does not reproduce the oracle's scan"
                    slow += sl; tails += tl; updates += 3 * D
                    windows.append(draws // WIN)
            ref.end_round()
    print("%s policy: %d updates, %d slow-path head exponentials, %d ziggurat-tail draws; windows per replica and scan: %d .. %d"
          % (pname, updates, slow, tails, min(windows), max(windows)))
    assert slow >= 100 and tails >= 3
    assert min(windows) >= 5


def test_the_two_policies_differ_in_the_oracle():
    """CPU: the tail draws above change the run -- the states after round 2 differ between the policies, so a kernel that read the wrong word
    (or none) cannot pass both GPU cases"""
    a, b = _reference("default"), _reference("log1p")
    assert not np.array_equal(a[-1][-1], b[-1][-1])


@pytest.mark.gpu
@pytest.mark.parametrize("two_launches", [False, True])
@pytest.mark.parametrize("pname", sorted(POLICIES))
def test_against_the_oracle_and_the_sequential_kernel(P, pname, two_launches):
    from pigeons_amd import _lib
    ref = _reference(pname)
    with _policy(POLICIES[pname], P):
        seq = _sequential(P, pname)
        got = _rows(P, N, D, P.SliceSampler(w=W, p=P_DBL, max_iter=MAX_ITER), ROUNDS, SEED, _lib.KERNEL_TWO_LAUNCHES if two_launches else 0,
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
