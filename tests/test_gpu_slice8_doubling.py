"""The speculative round of the default SliceSampler kernel after round 7 -- slice tests as one fused operation, the doubling step of
k_explore_slice8 as arithmetic on the interval ends instead of selects (pte_slice8.hpp) -- held to the oracle where those blocks decide things.

The rewritten blocks change no result: a hypothesis is used only if every |d| it tested clears the filter's margin, and everything else goes to
the exact sequential procedure, which is untouched.  So every comparison here is array_equal, over rounds 1-4 (30 scans): replica states, chains,
RNG words (every replica consumed exactly the same draws), index process, swap and explorer recorders -- against the oracle, and against the
exact sequential kernel on the same device.  One quantity cannot be bit-equal to the CPU's whatever the kernel does, the mean of the swap
acceptance probabilities (device exp against libm: up to 4.1e-16 relative in these cases): see ORACLE_RTOL.

Shapes: a partial 64-chunk (d = 33), a row with a ragged second chunk (d = 70), a row crossing the 256-coordinate block (d = 300), each with
w = 0.5 (most coordinates double three times or more: the speculative budget S8_BD = 3, lane 0's continuation loop and -- in the generic kernel
with p = 2 -- the reference's own limit), w = 10 (the default: a few doublings on the hot chains) and w = 40 (almost none double; long shrinkage).
Share of coordinate updates that need MORE than three doublings (the budget of a speculative hypothesis) at w = 0.5, estimated on the CPU from
the oracle's states and schedule after round 3 with the oracle's own generator (test_small_w_exceeds_the_doubling_budget):
(6, 33): 0.47, (8, 70): 0.51, (5, 300): 0.42; at w = 10: 0.02-0.03, at w = 40: 0.01.
Kernels: k_explore_slice8 / k_scans_slice8 (default range), k_scans_slice8_generic (p = 2 and p = 25), k_explore_slice8_lds10k (2304 chains);
every case in both forms of the scan loop (one launch per call, and an explore + a swap launch per scan)."""
import numpy as np
import pytest

import oracle as O

SHAPES = [(6, 33), (8, 70), (5, 300)]
WIDTHS = [0.5, 10.0, 40.0]
ROUNDS = 4                       # 2 + 4 + 8 + 16 = 30 scans

_REF = {}


def _reference(N, d, w, p, rounds, seed):
    """the oracle's run, computed once per configuration and shared by the cases that need it: per round the recorders, the states after it"""
    key = (N, d, w, p, rounds, seed)
    if key not in _REF:
        ref = O.OraclePT(n_chains=N, dim=d, seed=seed, explorer=O.EXPLORER_SLICE, slice_w=w, slice_p=p)
        out = []
        for _ in range(rounds):
            ref.run_round()
            m, n = ref.swap_pr()
            am, an, ss, sn = ref.explorer_stats()
            x, chain, rng = ref.states()
            row = [ref.index_process(), np.array(ref.round_trip()), n, m, an, am, sn, ss, chain, rng, x, ref.schedule()]
            for a in row:
                a.setflags(write=False)
            out.append(row)
        _REF[key] = out
    return _REF[key]


NAMES = ["index_process", "round_trip", "swap_n", "swap_mean", "explorer_acc_n", "explorer_acc_mean", "explorer_steps_n", "explorer_steps_sum",
         "chain", "rng", "x"]
# The swap recorder's mean is a mean of exp(.) values: the device's exp and the CPU's libm are each within an ulp of the true value, so two
# correct implementations differ by up to 2 ulp per term and the mean of at most 16 positive terms by 2 ulp plus its own accumulation
# (<= 16 roundings): 18 x 2^-53 -- asked for here as 32 x 2^-53 = 3.6e-15.  It is held BIT FOR BIT to the exact sequential kernel on the same
# device instead (k_explore_slice, which round 7 does not touch and which the oracle pins), like everything else.
ORACLE_RTOL = {"swap_mean": 32 * 2.0 ** -53}

_SEQ = {}


def _rows(P, N, d, explorer, rounds, seed, debug_kernel, names=None):
    pt = P.PT(P.Inputs(target=P.toy_mvn_target(d), n_chains=N, n_rounds=rounds, seed=seed, explorer=explorer,
                       record=[P.round_trip, P.index_process, P.log_sum_ratio], show_report=False), debug_kernel=debug_kernel)
    if names is not None:
        assert (pt.replicas.kernel_name(), pt.replicas.scan_loop_name()) == names
    out = []
    for r in range(rounds):
        assert P.next_round(pt)
        red = P.run_one_round(pt); P.adapt(pt, red)
        m, n = red.swap_acceptance_pr
        am, an = red.explorer_acceptance_pr
        ss, sn = red.explorer_n_steps
        x, chain, rng = pt.replicas.states()
        out.append([np.array(a).copy() for a in (red.index_process, red.round_trip, n, m, an, am, sn, ss, chain, rng, x)])
    return out


def _sequential(P, N, d, w, p, rounds, seed):
    """the exact sequential kernel's run on the same device, computed once per configuration"""
    from pigeons_amd import _lib
    key = (N, d, w, p, rounds, seed)
    if key not in _SEQ:
        _SEQ[key] = _rows(P, N, d, P.SliceSampler(w=w, p=p), rounds, seed, _lib.KERNEL_SLICE_SEQUENTIAL, ("k_explore_slice", ""))
        for row in _SEQ[key]:
            for a in row:
                a.setflags(write=False)
    return _SEQ[key]


def _hold_to_oracle(P, N, d, w, p, rounds, seed, two_launches, kernel, scan_loop):
    from pigeons_amd import _lib
    got = _rows(P, N, d, P.SliceSampler(w=w, p=p), rounds, seed, _lib.KERNEL_TWO_LAUNCHES if two_launches else 0,
                (kernel, "" if two_launches else scan_loop))
    ref, seq = _reference(N, d, w, p, rounds, seed), _sequential(P, N, d, w, p, rounds, seed)
    bad = []
    for r in range(rounds):
        for name, a, b, c in zip(NAMES, got[r], ref[r], seq[r]):
            b = np.asarray(b)
            if not np.array_equal(a, c, equal_nan=True):
                bad.append((r + 1, name, "sequential kernel"))
            if not np.array_equal(a, b, equal_nan=True):
                dif = float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300))) if a.shape == b.shape else float("inf")
                print("round %d %s against the oracle: largest relative difference %.3e" % (r + 1, name, dif))
                if not dif <= ORACLE_RTOL.get(name, 0.0):
                    bad.append((r + 1, name, "oracle", dif))
    assert not bad, bad


def _share_beyond_budget(N, d, w, seed, budget=3, p=20, draws=40):
    """share of coordinate updates whose doubling procedure (SliceSampler.jl:115-139) takes more than `budget` steps, for the oracle's
    states and schedule after round 3: fresh E, u0 and V draws from the oracle's generator on every coordinate of every replica"""
    ref = _reference(N, d, w, p, ROUNDS, seed)
    chain, x, betas = ref[2][8], ref[2][10], ref[2][11]
    rng = O.OracleRng(seed=12345)
    beyond = total = 0
    for r in range(N):
        prec = (1.0 - betas[chain[r]]) * 1.0 + betas[chain[r]] * 10.0          # toy_mvn_target: log density -prec / 2 * sum x^2
        for c in range(0, d, max(1, d // draws)):
            Q = x[r, c] * x[r, c] + rng.randexp() / (0.5 * prec)               # the slice { v : v^2 < Q }
            L = x[r, c] - w * rng.rand(); R = L + w
            k = 0
            while k < p and (L * L < Q or R * R < Q):
                if rng.rand() <= 0.5:
                    L -= R - L
                else:
                    R += R - L
                k += 1
            beyond += k > budget; total += 1
    return beyond / total


@pytest.mark.parametrize("N,d", SHAPES)
def test_small_w_exceeds_the_doubling_budget(N, d):
    """CPU, the oracle alone: at w = 0.5 a sizeable share of the coordinate updates -- at least a quarter is asked for; see the module
    docstring for the shares found -- needs more than the three doubling steps a speculative hypothesis may take, so these cases do exercise the
    budget, lane 0's continuation loop and the steps beyond.  (The slice of a coordinate is about 2 sqrt(x^2 + 2 E / prec) wide with prec in
    [1, 10]: 1 to 4 against an interval of 0.5, which three doublings bring to 4 at best.)  At w = 10 and 40 an end of the first interval
    falls inside the slice for about (slice width) / w of the updates and each step then moves the wrong end half of the time: a few per cent."""
    share = {w: _share_beyond_budget(N, d, w, seed=3) for w in WIDTHS}
    print("share of updates beyond three doublings: " + ", ".join("w = %g: %.3f" % (w, s) for w, s in share.items()))
    assert share[0.5] >= 0.25
    assert share[10.0] < share[0.5] and share[40.0] < share[0.5]


@pytest.mark.gpu
@pytest.mark.parametrize("two_launches", [False, True])
@pytest.mark.parametrize("w", WIDTHS)
@pytest.mark.parametrize("N,d", SHAPES)
def test_default_kernel(P, N, d, w, two_launches):
    _hold_to_oracle(P, N, d, w, 20, ROUNDS, 3, two_launches, "k_explore_slice8", "k_scans_slice8")


@pytest.mark.gpu
@pytest.mark.parametrize("two_launches", [False, True])
@pytest.mark.parametrize("p", [2, 25])
@pytest.mark.parametrize("N,d", [(8, 70), (5, 300)])
def test_generic_kernel(P, N, d, p, two_launches):
    """p = 2: the reference's own limit ends the doubling before the speculative budget does; p = 25: beyond the window headroom of the default
    instantiation.  The select loop of this kernel takes the same arithmetic form of the doubling step."""
    _hold_to_oracle(P, N, d, 0.5, p, ROUNDS, 3, two_launches, "k_explore_slice8_generic", "k_scans_slice8_generic")


@pytest.mark.gpu
@pytest.mark.parametrize("two_launches", [False, True])
def test_many_replica_twin(P, two_launches):
    """2304 chains: the 10 KB-LDS twin with the EXEC-mask doubling steps (more workgroups than the fused loop takes: launches per scan either way)"""
    _hold_to_oracle(P, 2304, 40, 0.5, 20, 2, 3, two_launches, "k_explore_slice8_lds10k", "")


@pytest.fixture(scope="module")
def P():
    import pigeons_amd
    return pigeons_amd
