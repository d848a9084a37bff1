"""The checks that the GPU tests of the interpolated-path families share, held once: tests/test_gpu_glm.py, _hier, _ar1, _dense, _mixture,
_mixture_model, _varsel and _changepoint build their data and their PT, name their shapes, and call these with the restatement's
`lambda beta: R.<Family>Chain(model, beta, prec).path_lp`.  Wherever those files differ in a number it is an argument here, and each call
site passes its own: nothing in this module chooses a tolerance, a scale or a recorder for a family.

Tolerances.  RNG words are compared exactly; states and recorders to RTOL = 1e-9 relative, log densities to LP_RTOL = 1e-11 relative -- the
device's exp / log1p differ from libm by an ulp, and its fused multiply-adds from the restatement's twice-rounded ones in rare ties.  (A
family whose arithmetic differs from its restatement's in less says so in its own file and passes the tighter figure: the Gaussian mixture
1e-12, the change points 1e-13.)

Nothing here touches the device at import: pigeons_amd is imported by the P fixture, when a test first asks for it."""
import dataclasses
import math

import numpy as np
import pytest

import aaps_ref
import mixture_ref
import oracle as O

RTOL = 1e-9
LP_RTOL = 1e-11

PRECONDITIONERS = {"identity": (0, "IdentityPreconditioner"), "diagonal": (1, "DiagonalPreconditioner"), "mix": (2, "MixDiagonalPreconditioner")}


@pytest.fixture(scope="module")
def P():
    import pigeons_amd
    return pigeons_amd


# ---- one step from random states ---------------------------------------------------------------------------------------------------------
def random_states(pt, N, d, seed, scale):
    """a sorted-uniform ladder from 0 to 1, states N(0, scale^2), a random chain permutation; the streams stay the engine's"""
    eng = pt.replicas
    g = np.random.default_rng(seed)
    betas = np.concatenate([[0.0], np.sort(g.uniform(0.0, 1.0, N - 2)), [1.0]])
    eng.set_schedule(betas)
    x = g.normal(0.0, scale, (N, d))
    chain = g.permutation(N).astype(np.int64)
    _, _, rng = eng.states()
    eng.set_states(x, chain, rng)
    return betas, x, chain, rng


def log_densities(pt, N, d):
    """[chain][d + 1]: the state one explore step left and the device's log density at it (extended traces)"""
    eng = pt.replicas
    eng.explore(1)
    eng.swap(1)                                   # (a scan ends at its swap: the traces count it from there)
    eng.reduce()
    tr = eng.traces()
    assert tr.shape == (1, N, d + 1)
    return tr[0]


def assert_log_density_at_every_beta(tr, betas, d, path_lp_of, lp_rtol, abs_tol):
    """tr[c, d] against path_lp_of(betas[c]) at tr[c, :d], every chain; returns the restatement's values"""
    wants = []
    for c in range(len(betas)):
        want = path_lp_of(betas[c])(tr[c, :d])
        assert math.isclose(tr[c, d], want, rel_tol=lp_rtol, abs_tol=abs_tol), (c, betas[c], tr[c, d], want)
        wants.append(want)
    return wants


def assert_log_density_is_not(tr, betas, d, path_lp_of):
    """off the reference chain tr[c, d] is away from path_lp_of(betas[c]) (the data that was replaced) by more than 1e-6 relative"""
    for c in range(len(betas)):
        if betas[c] > 0:
            assert not math.isclose(tr[c, d], path_lp_of(betas[c])(tr[c, :d]), rel_tol=1e-6), (c, betas[c], tr[c, d])


def _oracle_rng(rng, i):
    return O.OracleRng(state=(int(rng[i, 0]), int(rng[i, 1])))


def assert_slice_transition(eng, betas, x, chain, rng, path_lp_of, kinds=None, **sampler_kw):
    """one explore step of the engine against oracle.MixedSliceSampler (kinds: all Float64 unless given; sampler_kw: w, p, n_passes where
    the engine's SliceSampler has them) from the same state and RNG words, every replica off the reference chain: both RNG words equal, the
    state within RTOL (1e-12 absolute), acc_n, steps_n and steps_sum equal, acc_mean within RTOL"""
    N, d = x.shape
    eng.explore(1)
    x1, c1, r1 = eng.states()
    eng.reduce()
    am, an, ss, sn = eng.explorer_stats()
    assert np.array_equal(c1, chain)
    kinds = np.zeros(d, dtype=np.int32) if kinds is None else kinds
    for i in range(N):
        c = int(chain[i])
        if c == 0:
            continue
        r = _oracle_rng(rng, i)
        s = O.MixedSliceSampler(path_lp_of(betas[c]), kinds, **sampler_kw)
        yv = x[i].copy()
        s.step(r, yv)
        assert int(r1[i, 0]) == r.state[0] and int(r1[i, 1]) == r.state[1], (i, c)
        np.testing.assert_allclose(x1[i], yv, rtol=RTOL, atol=1e-12, err_msg="replica %d chain %d" % (i, c))
        assert an[c] == s.stats.acc_n and sn[c] == s.stats.steps_n and ss[c] == s.stats.steps_sum, (i, c)
        np.testing.assert_allclose(am[c], s.stats.acc_mean, rtol=RTOL)


def mala_explorer(P, step, precond):
    return P.MALA(step_size=step, preconditioner=getattr(P, PRECONDITIONERS[precond][1])())


def assert_mala_transition(eng, ex, precond, betas, x, chain, rng, chain_of, std_range, form, label=None):
    """scan 2 of the engine under ex = mala_explorer(P, step, precond), its standard deviations uniform on std_range, against
    aaps_ref.build_preconditioner and mixture_ref.mala_transition on chain_of(beta) from the same state and RNG words, every replica off the
    reference chain: both RNG words equal, the state within RTOL (1e-12 absolute), the recorders' counts equal and the mean acceptance
    within RTOL.  form says how the restatement runs and what the test sees of it:
      "whole"       one call for the n_refresh refreshments; some replica's state has changed;
      "by_refresh"  a call per refreshment; over all replicas some proposals are accepted and some rejected (printed under label)"""
    assert form in ("whole", "by_refresh")
    N, d = x.shape
    step, mode = ex.step_size, PRECONDITIONERS[precond][0]
    std = np.random.default_rng(d).uniform(*std_range, d)
    eng.set_explorer_adaptation(step, std)
    eng.explore(2)
    x1, c1, r1 = eng.states()
    eng.reduce()
    am, an, ss, sn = eng.explorer_stats()
    n_refresh = ex.base_n_refresh * int(math.ceil(d ** ex.exponent_n_refresh))
    moved = accepted = rejected = 0
    for i in range(N):
        c = int(chain[i])
        if c == 0:
            continue
        r = _oracle_rng(rng, i)
        Mv = aaps_ref.build_preconditioner(r, d, mode, 1.0 / 3.0, 1.0 / 3.0, std)
        ch = chain_of(betas[c])
        if form == "whole":
            res = mixture_ref.mala_transition(x[i], r, ch, step, n_refresh, Mv)
            xc, acc_n, steps, acc_mean = res["x"], res["acc_n"], res["steps"], res["acc_sum"] / res["acc_n"]
            moved += int(not np.array_equal(xc, x[i]))
        else:
            xc, acc_sum = x[i].copy(), 0.0
            for _ in range(n_refresh):                             # (the density and gradient at the start are pure functions of the state: the same bits)
                res = mixture_ref.mala_transition(xc, r, ch, step, 1, Mv)
                took = not np.array_equal(res["x"], xc)
                accepted += int(took); rejected += int(not took)
                xc, acc_sum = res["x"], acc_sum + res["acc_sum"]
            acc_n, steps, acc_mean = n_refresh, n_refresh, acc_sum / n_refresh
        assert int(r1[i, 0]) == r.state[0] and int(r1[i, 1]) == r.state[1], (i, c)
        np.testing.assert_allclose(x1[i], xc, rtol=RTOL, atol=1e-12, err_msg="replica %d chain %d" % (i, c))
        assert an[c] == acc_n and sn[c] == n_refresh and ss[c] == steps, (i, c)
        np.testing.assert_allclose(am[c], acc_mean, rtol=RTOL, atol=1e-12)
    if form == "whole":
        assert moved > 0
    else:
        print("%s: %d proposals accepted, %d rejected" % (label, accepted, rejected))
        assert accepted > 0 and rejected > 0


# ---- whole runs ------------------------------------------------------------------------------------------------------------------------
def run_rounds(P, target, prec, seed, n_rounds, explorer, n_chains, record, ref_dim=None):
    """pigeons' round loop by hand: the schedule the last round ran with is kept (adapt replaces it after the round).  record: the
    recorders' names in pigeons_amd; ref_dim: the reference's dimension where it is not target.dim"""
    pt = P.PT(P.Inputs(target=target, reference=P.ScaledPrecisionNormalLogPotential(prec, target.dim if ref_dim is None else ref_dim),
                       n_chains=n_chains, n_rounds=n_rounds, seed=seed, explorer=explorer, extended_traces=True, show_report=False,
                       record=[getattr(P, name) for name in record]))
    grids = None
    while P.next_round(pt):
        grids = np.array(pt.shared.tempering.schedule.grids)
        red = P.run_one_round(pt)
        pt = P.adapt(pt, red)
    return pt, grids


def batches(a, B):
    T = a.shape[0] // B * B
    return a[:T].reshape(B, T // B, *a.shape[1:])


def stepping_stone_se(delta, betas, B=8):
    """Monte Carlo standard error of stepping_stone by batch means.  delta[scan][chain] is (target - reference)(x) of the last round's scans
    (extended traces, every chain), which each family computes its own way; they are cut into B consecutive batches, the estimator --
    (forward + backward) / 2 of sum_k log mean_t exp(+-(beta_k+1 - beta_k) delta_t) -- is taken on each, se = sd(batch estimates) / sqrt(B).
    (Shorter batches make each estimate noisier, never less: se is not understated.)"""
    db = batches(delta, B)                                        # [B][t][chain]
    dbeta = np.diff(betas)

    def lme(a):
        m = a.max(axis=1, keepdims=True)
        return (m + np.log(np.mean(np.exp(a - m), axis=1, keepdims=True)))[:, 0]
    fw = lme(db[:, :, :-1] * dbeta).sum(-1)
    bw = -lme(-db[:, :, 1:] * dbeta).sum(-1)
    return float(np.std((fw + bw) / 2.0, ddof=1) / math.sqrt(B))


def assert_same_states(a, b):
    """a, b: engines or shard sets -- states, chain labels and RNG words equal bit for bit"""
    xa, ca, ga = a.states(); xb, cb, gb = b.states()
    assert np.array_equal(xa, xb) and np.array_equal(ca, cb) and np.array_equal(ga, gb)


def assert_two_runs_equal(P, make_inputs):
    """two runs of make_inputs(): states, traces, schedule and stepping_stone equal bit for bit; returns the first"""
    a, b = P.pigeons(P.PT(make_inputs())), P.pigeons(P.PT(make_inputs()))
    assert_same_states(a.replicas, b.replicas)
    assert np.array_equal(a.reduced_recorders.traces, b.reduced_recorders.traces)
    assert np.array_equal(a.shared.tempering.schedule.grids, b.shared.tempering.schedule.grids)
    assert P.stepping_stone(a) == P.stepping_stone(b)
    return a


def assert_compose_runs(P, inputs, kernel_name):
    """a run under Compose(SliceSampler, AutoMALA): the first explorer's kernel, finite traces and evidence, and both explorers recorded
    on every tempered chain; returns the run"""
    pt = P.pigeons(P.PT(inputs))
    assert pt.replicas.kernel_name() == kernel_name
    assert np.all(np.isfinite(pt.reduced_recorders.traces)) and np.isfinite(P.stepping_stone(pt))
    m, n = pt.reduced_recorders.explorer_acceptance_pr
    assert np.all(n[1:] > 0)
    return pt


def with_recorders(P, inputs, *names):
    """inputs with the recorders `names` (pigeons_amd's builders) added where its record list lacks them"""
    have = {b() for b in inputs.record}
    return dataclasses.replace(inputs, record=list(inputs.record) + [getattr(P, n) for n in names if n not in have])


def _same(a, b):
    """np.array_equal of two recorders (arrays, or tuples of arrays and counts); an entry that is NaN in both is equal"""
    if isinstance(a, (tuple, list)):
        return isinstance(b, (tuple, list)) and len(a) == len(b) and all(_same(u, v) for u, v in zip(a, b))
    a, b = np.asarray(a), np.asarray(b)
    return np.array_equal(a, b, equal_nan=a.dtype.kind == "f" and b.dtype.kind == "f")


def boundary_swap_counts(index_process, final_chain, K):
    """accepted swaps of each pair (gK - 1, gK), g = 1 .. N / K - 1, read off one engine's index process: index_process[replica][scan] is the
    chain a replica was on when scan's swap began (the rounds' arrays side by side), final_chain[replica] the chain it ended on.  Only the
    swap of that pair takes a replica from gK - 1 to gK between two scans"""
    ip = np.asarray(index_process)
    nxt = np.concatenate([ip[:, 1:], np.asarray(final_chain)[:, None]], axis=1)
    return [int(np.sum((ip == b - 1) & (nxt == b))) for b in range(K, ip.shape[0], K)]


def assert_sharded_equals_single(P, make_inputs, n_shards, **pt_kw):
    """every round of make_inputs() on one engine and on n_shards (pt_kw: device_messages=True or transport="group", the drivers of the
    message kernels; neither: the host two-phase driver).  Round by round and bit for bit: index process, round trips, traces and online where
    recorded, swap acceptance, log_sum_ratio, the explorer's two recorders, energy_ac1's three arrays, the adapted schedule; then the final
    states.  Every shard boundary's pair has accepted swaps in the single engine's index process -- a condition on make_inputs(): choose the
    seed so -- and the shards applied exactly that many, per boundary and side where the device counts them.  Returns the counts"""
    one, many = P.PT(make_inputs()), P.PT(make_inputs(), n_shards=n_shards, **pt_kw)
    names = {b() for b in one.inputs.record}
    assert "index_process" in names, "the boundary swaps are counted from the index process"
    ips = []
    for rnd in range(one.inputs.n_rounds):
        assert P.next_round(one) and P.next_round(many)
        ra, rb = P.run_one_round(one), P.run_one_round(many)
        for name in ("index_process", "round_trip", "traces", "online"):
            if name in names:
                assert _same(getattr(ra, name), getattr(rb, name)), (rnd, name, getattr(ra, name), getattr(rb, name))
        for name in ("swap_acceptance_pr", "log_sum_ratio", "explorer_acceptance_pr", "explorer_n_steps", "energy_ac1"):
            assert _same(getattr(ra, name), getattr(rb, name)), (rnd, name, getattr(ra, name), getattr(rb, name))
        P.adapt(one, ra); P.adapt(many, rb)
        assert np.array_equal(one.shared.tempering.schedule.grids, many.shared.tempering.schedule.grids), rnd
        ips.append(ra.index_process)
    assert_same_states(one.replicas, many.shards)
    G, K = n_shards, one.inputs.n_chains // n_shards
    counts = boundary_swap_counts(np.concatenate(ips, axis=1), one.replicas.states()[1], K)
    assert len(counts) == G - 1 and min(counts) >= 1, counts
    if pt_kw.get("device_messages") or pt_kw.get("transport") == "group":
        for g, e in enumerate(many.shards.engines):      # side 0: the pair below the shard's first chain, side 1: the pair above its last
            want = [counts[g - 1] if g > 0 else 0, counts[g] if g < G - 1 else 0]
            assert list(e.shard_sync()) == want and list(e.comm_info()[2]) == want, (g, want, e.shard_sync(), e.comm_info()[2])
    else:
        assert many.shards.n_boundary_swaps == sum(counts), (many.shards.n_boundary_swaps, counts)
    return counts


def assert_checkpoint_resume(P, make_inputs, tmp_path):
    """make_inputs(n_rounds=6) straight through against make_inputs(n_rounds=3, checkpoint=True) resumed for three more: index process,
    traces, schedule and states equal bit for bit; returns the resumed run"""
    straight = P.pigeons(P.PT(make_inputs(n_rounds=6)))
    folder = str(tmp_path / "exec")
    P.pigeons(P.PT(make_inputs(n_rounds=3, checkpoint=True)), exec_folder=folder)
    resumed = P.pigeons(P.load_checkpoint(folder, n_rounds_increment=3))
    ra, rb = straight.reduced_recorders, resumed.reduced_recorders
    assert np.array_equal(ra.index_process, rb.index_process) and np.array_equal(ra.traces, rb.traces)
    assert np.array_equal(straight.shared.tempering.schedule.grids, resumed.shared.tempering.schedule.grids)
    assert_same_states(straight.replicas, resumed.replicas)
    return resumed
