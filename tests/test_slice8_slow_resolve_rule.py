"""The rule by which the default SliceSampler kernel decides the slow-path exponentials of a draw window when the window is FILLED (round 11,
pte_slice8.hpp), restated on the host and held to the oracle's sequential randexp.  CPU only.

A window holds WIN = 512 consecutive draws of a replica's stream: s_u[i] the draw as a uniform, s_e[i] the draw as a fast-path exponential or
NaN where the ziggurat's fast path does not apply.  For a slow position i in layer idx = ri & 0xFF with x = (double)ri * we[idx]:

    idx == 0 (the ziggurat's tail)                                          unresolved: "tail"
    i + 2 >= WIN                                                            unresolved: "edge"
    (fe[idx - 1] - fe[idx]) * s_u[i + 1] + fe[idx] < exp(-x)                (Ex, used) = (x, 2)
    otherwise, s_e[i + 2] is not NaN                                        (Ex, used) = (s_e[i + 2], 3)
    otherwise                                                               unresolved: "deeper"

and the kernel's table has one slot per lane of the fill (lane = i & 63, eight draws each): of two slow draws of one lane the LAST is decided,
the earlier one is unresolved: "displaced".  Whatever is unresolved takes the sequential path in the kernel, so the rule only has to be RIGHT
where it answers: every (Ex, used) it gives must be what randexp returns and consumes when it is called at that stream position, bit for bit.

The tables are the device header's (pigeons.jl_amd/csrc/zig_tables.h, parsed as tests/test_zig_tables.py does); exp is libm's, as in the
oracle; the streams are SplittableRandom streams seeded by the oracle's generator."""
import math

import numpy as np

import oracle as O
from test_zig_tables import _header_tables

WIN = 512
M64, MASK52 = (1 << 64) - 1, (1 << 52) - 1
UNRESOLVED = ("tail", "edge", "deeper", "displaced")


def _mix64_np(z):
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xbf58476d1ce4e5b9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94d049bb133111eb)
    return z ^ (z >> np.uint64(31))


def tables():
    t = _header_tables()
    return t["ke"], t["we"].view(np.float64), t["fe"].view(np.float64)


def window(seed, gamma, tab):
    """the window behind stream state `seed`: draw i is mix64(seed + (i + 1) gamma) -> (s_u, s_e, layer, x) as the fill computes them"""
    ke, we, fe = tab
    with np.errstate(over="ignore"):
        r = _mix64_np(np.uint64(seed) + np.arange(1, WIN + 1, dtype=np.uint64) * np.uint64(gamma))
    ri = r & np.uint64(MASK52)
    idx = (ri & np.uint64(0xFF)).astype(np.int64)
    x = ri.astype(np.float64) * we[idx]                                     # (ri < 2^52: the conversion is exact)
    s_u = (ri | np.uint64(0x3ff0000000000000)).view(np.float64) - 1.0
    s_e = np.where(ri < ke[idx], x, np.nan)
    return s_u, s_e, idx, x


def resolve(s_u, s_e, idx, x, tab):
    """{slow position i: (Ex, used) or one of UNRESOLVED} for one window"""
    ke, we, fe = tab
    slow = np.nonzero(np.isnan(s_e))[0]
    last_of_lane = {}
    for i in slow:
        last_of_lane[int(i) & 63] = int(i)
    out = {}
    for i in map(int, slow):
        k = int(idx[i])
        if last_of_lane[i & 63] != i:
            out[i] = "displaced"
        elif k == 0:
            out[i] = "tail"
        elif i + 2 >= WIN:
            out[i] = "edge"
        elif (fe[k - 1] - fe[k]) * s_u[i + 1] + fe[k] < math.exp(-x[i]):
            out[i] = (float(x[i]), 2)
        elif not math.isnan(s_e[i + 2]):
            out[i] = (float(s_e[i + 2]), 3)
        else:
            out[i] = "deeper"
    return out


def sequential(seed, gamma, i):
    """randexp called at window position i: (value, draws consumed)"""
    s0 = (seed + i * gamma) & M64
    rng = O.OracleRng(state=(s0, gamma))
    E = rng.randexp()
    return E, (((rng.state[0] - s0) & M64) * pow(gamma, -1, 1 << 64)) & M64


def test_the_rule_answers_what_randexp_answers():
    """at least 10^5 slow positions of random streams: a resolved record equals the sequential result bit for bit, an unresolved position is
    in one of the stated cases and the sequential procedure confirms the case (tail: two draws in layer 0; deeper: four draws or more)"""
    tab = tables()
    src = O.OracleRng(seed=20261020)
    n_slow, counts = 0, {k: 0 for k in UNRESOLVED + ("wedge", "next")}
    windows = 0
    while n_slow < 100000:
        seed, gamma = src.next_u64() & M64, (src.next_u64() | 1) & M64
        for w in range(16):                                                 # sixteen consecutive windows of the stream
            ws = (seed + w * WIN * gamma) & M64
            s_u, s_e, idx, x = window(ws, gamma, tab)
            for i, got in resolve(s_u, s_e, idx, x, tab).items():
                E, used = sequential(ws, gamma, i)
                n_slow += 1
                assert used >= 2
                if isinstance(got, tuple):
                    assert got[1] == used and np.float64(got[0]).view(np.uint64) == np.float64(E).view(np.uint64), (ws, gamma, i, got, E, used)
                    counts["wedge" if used == 2 else "next"] += 1
                else:
                    assert got in UNRESOLVED
                    counts[got] += 1
                    if got == "tail":
                        assert idx[i] == 0 and used == 2
                    elif got == "edge":
                        assert i + 2 >= WIN
                    elif got == "deeper":
                        assert used >= 4
                    else:
                        assert any(j > i and (j & 63) == (i & 63) and math.isnan(s_e[j]) for j in range(i + 64, WIN, 64))
            windows += 1
    res = counts["wedge"] + counts["next"]
    print("%d windows, %d slow positions (%.2f %% of the draws): resolved %d (%.1f %%: wedge %d, next candidate fast %d); unresolved: %s"
          % (windows, n_slow, 100.0 * n_slow / (windows * WIN), res, 100.0 * res / n_slow, counts["wedge"], counts["next"],
             ", ".join("%s %d" % (k, counts[k]) for k in UNRESOLVED)))
    assert all(counts[k] > 0 for k in counts)
