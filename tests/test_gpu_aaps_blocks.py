"""k_explore_aaps in every one of its sixteen instantiations (E = 1, 2, 4, 8 blocks per lane x {MVN, funnel} x {ragged, whole blocks}) and
on its failure paths against the restatement (tests/aaps_ref.py) at one transition, over the case table of tests/aaps_blocks.py: the sizes
where the funnel spills into AGPRs and runs one wave per SIMD (E = 8), AmTarget's funnel tree changes its packing, the lockstep sums of
|p|^2, h and |x|^2 take their E >= 4 branch and the momentum draw meets trailing blocks that are whole, partly filled or empty; the
non-finite stay and the step cap as declared properties of their cases; the reference chain's i.i.d. draw, from the fixed reference and
from a GaussianReference; the statistics the epilogue leaves for the swap, in registers (the traces) and in memory (the log ratios); and
the chain-sharded engine on the funnel.  tests/test_aaps_blocks_cpu.py holds the table to its coverage, shows that no decision of the
restatement on these inputs is within 1e-7 of a tie, and that rounding alone moves these trajectories by 4e-12 at the most.

The assertions and tolerances are those of tests/test_gpu_aaps.py: RNG words and step counts equal, states and the mean acceptance within
1e-9 relative (states: + 1e-12); log densities within 1e-11 relative + 1e-11 (test_log_density_at_every_beta's).  The restatement of a
case runs once (aaps_blocks.reference) and is nearly all of the time."""
import math

import numpy as np
import pytest

import aaps_blocks as B

pytestmark = pytest.mark.gpu

RTOL = 1e-9
LP_RTOL = 1e-11


@pytest.fixture(scope="module")
def P():
    import pigeons_amd
    return pigeons_amd


def _engine(P, case, **kw):
    """an engine at the case's schedule, states, chain permutation, adaptation and variational reference; its own RNG words are the ones
    tests/test_aaps_blocks_cpu.py ran the restatement from"""
    inp, funnel = B.inputs(case), case.target == "funnel"
    pc = {"identity": P.IdentityPreconditioner, "diagonal": P.DiagonalPreconditioner, "mix": P.MixDiagonalPreconditioner}[case.precond]()
    pt = P.PT(P.Inputs(target=P.Funnel(case.d) if funnel else P.toy_mvn_target(case.d),
                       reference=P.ScaledPrecisionNormalLogPotential(B.FUNNEL_REF_PREC, case.d) if funnel else None, n_chains=case.N, n_rounds=2,
                       explorer=P.AAPS(step_size=case.step, K=case.K, preconditioner=pc), seed=case.seed, show_report=False, **kw))
    eng = pt.replicas
    assert eng.kernel_name() == "k_explore_aaps" and eng.scan_loop_name() == ""
    eng.set_schedule(inp.betas)
    _, _, rng = eng.states()
    assert np.array_equal(rng, inp.words)
    eng.set_states(inp.x, inp.chain, rng)
    eng.set_explorer_adaptation(case.step, inp.std)
    if case.vref:
        eng.set_variational_reference(inp.vm, inp.vs, inp.uses)
    return pt, eng


def _explore_once(P, case):
    """-> (inputs, states, RNG words, explorer_stats) after one explore; the chains stay"""
    inp = B.inputs(case)
    _, eng = _engine(P, case)
    eng.explore(1)                                   # (no error is raised: not at a failed transition, not at the cap)
    x1, c1, r1 = eng.states()
    eng.reduce()
    assert np.array_equal(c1, inp.chain)
    return inp, x1, r1, eng.explorer_stats()


def _rel(a, b):
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300)))


def _check_reference_chain(case, inp, x1, r1, stats):
    """sample_iid!: d normals in draw order times the reference's sd, or times the GaussianReference's std plus its mean; no explorer
    recorder touched"""
    am, an, ss, sn = stats
    i = int(np.flatnonzero(inp.chain == 0)[0])
    want, words = B.reference_chain_draw(case, inp, inp.words[i])
    assert (int(r1[i, 0]), int(r1[i, 1])) == tuple(words), case
    np.testing.assert_allclose(x1[i], want, rtol=RTOL, atol=1e-12, err_msg="%s reference chain" % case.id)
    assert an[0] == 0 and sn[0] == 0, case
    return _rel(x1[i], want)


@pytest.mark.parametrize("case", B.TRANSITION_CASES + B.UNSTABLE_CASES, ids=[c.id for c in B.TRANSITION_CASES + B.UNSTABLE_CASES])
def test_one_transition_parity(P, case):
    inp, x1, r1, stats = _explore_once(P, case)
    am, an, ss, sn = stats
    ref = B.reference(case)
    worst_x = worst_acc = 0.0
    stayed_at_zero = moved = 0
    for i, res in ref.items():
        c = int(inp.chain[i])
        what = "%s replica %d chain %d" % (case.id, i, c)
        assert (int(r1[i, 0]), int(r1[i, 1])) == tuple(res["words"]), what
        np.testing.assert_allclose(x1[i], res["x"], rtol=RTOL, atol=1e-12, err_msg=what)
        assert an[c] == 1 and sn[c] == 1 and ss[c] == res["steps"], (what, ss[c], res["steps"])
        np.testing.assert_allclose(am[c], res["acc"], rtol=RTOL, atol=1e-12, err_msg=what)
        if res["failed"]:                                # the stay: x0 bit for bit, acceptance 0
            assert np.array_equal(x1[i], inp.x[i]) and am[c] == 0.0, what
        elif res["moved"]:
            assert not np.array_equal(x1[i], inp.x[i]), what
        stayed_at_zero += int(np.array_equal(x1[i], inp.x[i]) and am[c] == 0.0)
        moved += int(not np.array_equal(x1[i], inp.x[i]))
        worst_x = max(worst_x, _rel(x1[i], res["x"]))
        worst_acc = max(worst_acc, abs(am[c] - res["acc"]))
    worst_ref = _check_reference_chain(case, inp, x1, r1, stats)
    print("%s: %d moved, %d stayed with acceptance 0; steps %d; device against restatement: state %.1e relative, acceptance %.1e, reference chain %.1e"
          % (case.id, moved, stayed_at_zero, int(sum(ss[1:])), worst_x, worst_acc, worst_ref))
    assert int(sum(ss[1:])) == case.steps                # the counts of tests/test_aaps_blocks_cpu.py, on the device's output
    if case.kind == "parity":
        assert stayed_at_zero == 0 and moved >= 5, (case, stayed_at_zero, moved)
    else:
        assert stayed_at_zero >= 1 and moved >= 1, (case, stayed_at_zero, moved)


@pytest.mark.parametrize("case", B.CAP_CASES, ids=[c.id for c in B.CAP_CASES])
def test_step_cap(P, case):
    """PTE_AAPS_MAX_LEAPFROGS: at a step of 1e-6 or 1e-7 neither pass leaves its segment; the transition ends at 4096 steps, stays, and has
    drawn the preconditioner's uniforms, d normals, the range draw and 4096 candidate uniforms"""
    inp, x1, r1, stats = _explore_once(P, case)
    am, an, ss, sn = stats
    ref = B.reference(case)
    assert len(ref) == case.N - 1
    for i, res in ref.items():
        c = int(inp.chain[i])
        what = "%s replica %d chain %d" % (case.id, i, c)
        assert res["failed"] and res["steps"] == B.A.MAX_LEAPFROGS == 4096, what
        assert np.array_equal(x1[i], inp.x[i]), what
        assert an[c] == 1 and sn[c] == 1 and ss[c] == 4096 and am[c] == 0.0, (what, ss[c], am[c])
        assert (int(r1[i, 0]), int(r1[i, 1])) == tuple(res["words"]), what
    _check_reference_chain(case, inp, x1, r1, stats)


def _explore_and_swap(P, case, scan):
    _, eng = _engine(P, case, record=[P.traces, P.log_sum_ratio, P.swap_acceptance_pr], extended_traces=True)
    eng.explore(1)
    x1, c1, _ = eng.states()
    eng.swap(scan)                                # scan 1: the pairs (0, 1), (2, 3), ...; scan 2: (1, 2), (3, 4), ... (DEO)
    eng.reduce()
    return x1, c1, eng.traces(), eng.log_sum_ratio(), eng.swap_acceptance()


@pytest.mark.parametrize("case", B.STATISTICS_CASES, ids=[c.id for c in B.STATISTICS_CASES])
def test_statistics_left_for_the_swap(P, case):
    """suff, suff2 (the funnel's log density) and suff3 (the GaussianReference's) at the selected point.  The registers' copy: the extended
    trace's log density of every chain against the restatement's at the state the device returned.  The copy in memory: one swap after
    one explore, so that log_sum_ratio's sums hold one term a pair -- logaddexp(-inf, lr) is lr -- and are the two log ratios
    themselves; one engine per DEO parity, from the same states.  With a GaussianReference the flagged chains take its log density
    as their reference end and the others the fixed reference's, in the density and in both ends of a ratio."""
    inp, N, d = B.inputs(case), case.N, case.d
    worst_lp = worst_lr = 0.0
    states = []
    for scan in (1, 2):
        x1, c1, tr, (up, un, dn, dnn), (sm, sn) = _explore_and_swap(P, case, scan)
        assert np.array_equal(c1, inp.chain) and tr.shape == (1, N, d + 1)
        states.append(x1)
        at = {int(c1[i]): x1[i] for i in range(N)}                     # chain -> the state its replica holds after explore
        lp = lambda c, x: B.log_density(case, inp, c, x)
        for c in range(N):
            assert np.array_equal(tr[0, c, :d], at[c]), (case, c)
            want = lp(c, at[c])
            worst_lp = max(worst_lp, abs(tr[0, c, d] - want) / max(abs(want), 1.0))
            assert math.isclose(tr[0, c, d], want, rel_tol=LP_RTOL, abs_tol=1e-11), (case.id, c, inp.betas[c], tr[0, c, d], want)
        lower = [c for c in range(N - 1) if c % 2 == (0 if scan % 2 == 1 else 1)]
        for c in range(N - 1):
            if c not in lower:
                assert un[c] == 0 and dnn[c] == 0 and sn[c] == 0, (case, scan, c)
                continue
            assert un[c] == 1 and dnn[c] == 1 and sn[c] == 1, (case, scan, c)
            for got, x, num, den in ((up[c], at[c], c + 1, c), (dn[c], at[c + 1], c, c + 1)):
                a, b = lp(num, x), lp(den, x)
                worst_lr = max(worst_lr, abs(got - (a - b)) / (abs(a) + abs(b)))
                assert abs(got - (a - b)) <= LP_RTOL * (abs(a) + abs(b)) + 1e-11, (case.id, scan, c, got, a - b, a, b)
            assert math.isclose(sm[c], min(1.0, math.exp(up[c] + dn[c])), rel_tol=RTOL, abs_tol=1e-300), (case.id, scan, c, sm[c], up[c], dn[c])
    assert np.array_equal(states[0], states[1])
    if case.vref:
        assert 0 < int(np.sum(inp.uses)) < N
    print("%s: device against restatement: log density %.1e relative, log ratio %.1e of |lp| + |lp|" % (case.id, worst_lp, worst_lr))


def test_sharded_funnel_equals_single_engine(P):
    """four chain-shards of two chains against one engine on Funnel(130), two rounds: the payload that crosses a shard boundary carries
    suff2 as well (tests/test_gpu_aaps.py's sharded case is the MVN path at d = 20)"""
    d = 130
    rec = [P.round_trip, P.index_process, P.log_sum_ratio, P.energy_ac1, P.traces]
    mk = lambda: P.Inputs(target=P.Funnel(d), reference=P.ScaledPrecisionNormalLogPotential(B.FUNNEL_REF_PREC, d), n_chains=8, n_rounds=2,
                          explorer=P.AAPS(step_size=0.1, K=3), record=rec, show_report=False)
    one, many = P.PT(mk()), P.PT(mk(), n_shards=4, device_messages=True)
    assert one.replicas.kernel_name() == "k_explore_aaps"
    for _ in range(2):
        assert P.next_round(one) and P.next_round(many)
        ra = P.run_one_round(one); P.adapt(one, ra)
        rb = P.run_one_round(many); P.adapt(many, rb)
        assert np.array_equal(ra.index_process, rb.index_process) and np.array_equal(ra.traces, rb.traces)
        assert np.all(np.isfinite(ra.traces)) and np.any(ra.traces[:, :d] != 0.0)
        for a, b in zip(ra.energy_ac1 + ra.explorer_acceptance_pr + ra.explorer_n_steps, rb.energy_ac1 + rb.explorer_acceptance_pr + rb.explorer_n_steps):
            assert np.array_equal(a, b, equal_nan=True)
    xa, ca, ga = one.replicas.states(); xb, cb, gb = many.shards.states()
    assert np.array_equal(xa, xb) and np.array_equal(ca, cb) and np.array_equal(ga, gb)
    shard = ra.index_process // 2                        # [replica][scan] -> the shard that held it
    assert np.any(shard != shard[:, :1])                 # a replica did cross a shard boundary
