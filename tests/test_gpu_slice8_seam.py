"""The seam between the doubling block and the shrinkage block of the default SliceSampler kernel after round 9 (pte_slice8.hpp): the nine
shrinkage draws of a hypothesis are requested at the end of the doubling block, at an address the doubling steps advance themselves, and
the shrinkage block waits for them read by read.  Scheduling only: no draw, decision, state or recorder changes, so every comparison is
array_equal -- states, chains, RNG words, index process, swap and explorer recorders over rounds 1-4 (30 scans) -- against the exact
sequential kernel on the same device and against the oracle (the swap recorder's mean against the oracle within ORACLE_RTOL of
tests/test_gpu_slice8_doubling.py, whose helpers and cached references this module shares).

What the cases put on the new code:
  w = 0.5   lane 0 runs past the doubling budget in 42-51 % of the updates (tests/test_gpu_slice8_doubling.py counts them): its draws
            move AFTER they were requested, and the out-of-line path re-reads them, recomputes the threshold, the width and the draw
            count, while the first request may still be in flight;
  w = 10    the default: both paths, the likely one most of the time;
  w = 40    (6, 33): long shrinkage -- lane 0 goes past nine proposals, reading on from a pointer derived from its doubling count;
  d = 300   crosses the end of a 256-coordinate block; d = 33 / 70: a partial chunk, a ragged second chunk.
In (5, 300) at w = 0.5 some updates take BOTH of lane 0's re-reads -- a slow-path exponential at the head (the draws of the coordinate
move by the extra draws it consumed) and then more than three doublings: test_slow_head_then_beyond_the_budget counts them on the CPU."""
import pytest

import oracle as O
import test_gpu_slice8_doubling as D

CASES = [(N, d, w) for (N, d) in D.SHAPES for w in (0.5, 10.0)] + [(6, 33, 40.0)]
SEED = 3


def _count_slow_head_then_beyond(N, d, w, seed, sweeps=9, budget=3, p=20):
    """(updates simulated, those with a slow-path exponential, those which also double more than `budget` times) for the oracle's states and
    schedule after round 3, fresh draws from the oracle's generator on every coordinate of every replica, `sweeps` times over.  The
    ziggurat's fast path consumes exactly one word of the stream: an exponential that advanced the generator further took the slow path."""
    ref = D._reference(N, d, w, p, D.ROUNDS, seed)
    chain, x, betas = ref[2][8], ref[2][10], ref[2][11]
    rng = O.OracleRng(seed=12345)
    gamma = rng.state[1]
    total = slow = both = 0
    for _ in range(sweeps):
        for r in range(N):
            prec = (1.0 - betas[chain[r]]) * 1.0 + betas[chain[r]] * 10.0
            for c in range(d):
                s0 = rng.state[0]
                E = rng.randexp()
                is_slow = rng.state[0] != (s0 + gamma) % 2 ** 64
                Q = x[r, c] * x[r, c] + E / (0.5 * prec)
                L = x[r, c] - w * rng.rand(); R = L + w
                k = 0
                while k < p and (L * L < Q or R * R < Q):
                    if rng.rand() <= 0.5:
                        L -= R - L
                    else:
                        R += R - L
                    k += 1
                total += 1; slow += is_slow; both += is_slow and k > budget
    return total, slow, both


def test_slow_head_then_beyond_the_budget():
    """CPU, the oracle alone.  The (5, 300), w = 0.5 run makes 5 x 300 x 3 x 30 = 135 000 coordinate updates; 2.3 % of the exponentials take
    the ziggurat's slow path and 42 % of the updates double more than three times, independently: over a thousand updates in which lane 0
    re-reads its draws twice.  Counted here on a tenth of that (13 500 updates, expected ~130) -- found: 295 slow-path exponentials, 130 of
    them followed by more than three doublings."""
    total, slow, both = _count_slow_head_then_beyond(5, 300, 0.5, SEED)
    print("%d updates: %d with a slow-path exponential, %d of them beyond three doublings" % (total, slow, both))
    assert total == 13500 and both >= 1
    assert 0.01 < slow / total < 0.05               # (the counter does see the slow path: 2.3 % expected)


@pytest.mark.gpu
@pytest.mark.parametrize("two_launches", [False, True])
@pytest.mark.parametrize("N,d,w", CASES)
def test_default_kernel(P, N, d, w, two_launches):
    D._hold_to_oracle(P, N, d, w, 20, D.ROUNDS, SEED, two_launches, "k_explore_slice8", "k_scans_slice8")


@pytest.fixture(scope="module")
def P():
    import pigeons_amd
    return pigeons_amd
