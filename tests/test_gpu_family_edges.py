"""The device at the edge battery of tests/family_edges.py: the nine families of the interpolated path at the states where their kernels
hold hand-written special cases, against the 60-digit evaluation of each model's definition (tests/family_mp.py) and, for transitions, the
restatements (tests/<family>_ref.py) -- which tests/test_family_edges_cpu.py holds to the same definition at the same states.

One chain per battery state of a shape (at most 16; longer lists are split), the schedule 0, sorted uniforms, 1, a fixed chain permutation,
RNG words made here on the CPU (splits of one oracle stream), so that everything the device is compared with is known before it runs.

(a) the refresh kernel: pte_set_state runs k_refresh_*_stats on the battery state; energy_ac1's `before` of the next explore step is
    chain_lp of those statistics.  (b) the explorer's epilogue: the extended trace row of the same step, [state after; lp].  Both against
    family_mp, |d| <= 1e-11 |mp| + 1e-11.  SliceSampler(w = 0.25, p = 3, n_passes = 1) keeps the state near the edge; the change point's
    Integer coordinates need an integral width (pte_create refuses another), there it is w = 1, p = 1.  The traces count a scan at its swap,
    so the step is explore(1); swap(1); reduce().
(c) one SliceSampler pass from every battery state against oracle.MixedSliceSampler on the restatement's path_lp: RNG words equal, Integer
    and Bool coordinates equal, Float64 ones to 1e-9 relative + 1e-12, explorer statistics equal; (w, p) = (10, 20) and (0.25, 3) -- the
    change point (2, 2), and both of its evaluation forms.  n_passes = 1: the pass that starts at the edge.
(d) one MALA transition of AR(1) and the hierarchical family from their battery states with |lp| <= 1e6, against mixture_ref.mala_transition.
(f) one AutoMALA transition of every family that has a gradient (the funnel too) from the same states as (d), against
    automala_ref.automala_transition: RNG words, the counting recorders, the sum of the step-size factors and the number of reversibility
    checks passed equal, states and mean acceptance to 1e-9 relative.
(e) one swap from the battery states: each active pair's two log ratios against family_mp, the acceptance against them, the labels
    afterwards against u < alpha with the lower chain's uniform."""
import math

import numpy as np
import pytest
from mpmath import mp, mpf

import aaps_ref as A
import automala_ref as R
import family_edges as E
import mixture_ref as M
import oracle as O

pytestmark = pytest.mark.gpu

RTOL = 1e-9
LP_RTOL, LP_ATOL = 1e-11, 1e-11
RNG_SEED = 2024          # chosen on the CPU: with it no pair of test_one_swap has |u - alpha| < 1e-6 (the test asserts it before it runs the device)

GROUPS = [(s, a, st) for s in E.SHAPES for a, st in E.groups(s)]
GROUP_IDS = ["%s@%d" % (s.id, a) for s, a, _ in GROUPS]


@pytest.fixture(scope="module")
def P():
    import pigeons_amd
    return pigeons_amd


def layout(key, shape, states):
    """(betas, x, chain, rng) of one engine: replica i holds battery state i on chain chain[i]"""
    N = len(states)
    assert 2 <= N <= 16
    g = np.random.default_rng(500 + key)
    betas = np.concatenate([[0.0], np.sort(g.uniform(0.0, 1.0, N - 2)), [1.0]])
    chain = g.permutation(N).astype(np.int64)
    x = np.array([v for _, v in states], dtype=np.float64)
    root = O.OracleRng(seed=RNG_SEED + key)
    rng = np.array([root.split().state for _ in range(N)], dtype=np.uint64)
    return betas, x, chain, rng


def _pt(P, shape, N, explorer, **kw):
    target, ref_dim = E.device_target(P, shape)
    return P.PT(P.Inputs(target=target, reference=P.ScaledPrecisionNormalLogPotential(shape.ref_prec, ref_dim), n_chains=N, n_rounds=2,
                         explorer=explorer, show_report=False, **kw))


def _engine(P, shape, explorer, betas, x, chain, rng, **kw):
    eng = _pt(P, shape, len(chain), explorer, **kw).replicas
    eng.set_schedule(betas)
    eng.set_states(x, chain, rng)
    return eng


def _lp_close(got, want, what):
    assert math.isfinite(got), what
    assert abs(mpf(float(got)) - want) <= LP_RTOL * abs(want) + LP_ATOL, what + (float(got), float(want))


# ---- (a), (b) --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gi", range(len(GROUPS)), ids=GROUP_IDS)
def test_refresh_kernel_and_epilogue_against_the_definition(P, gi):
    shape, _, states = GROUPS[gi]
    betas, x, chain, rng = layout(gi, shape, states)
    N, d = len(states), shape.dim
    ex = P.SliceSampler(w=1.0, p=1, n_passes=1) if shape.family == "changepoint" else P.SliceSampler(w=0.25, p=3, n_passes=1)
    eng = _engine(P, shape, ex, betas, x, chain, rng, record=[P.traces, P.energy_ac1], extended_traces=True)
    eng.explore(1)
    eng.swap(1)
    eng.reduce()
    _, n, mom = eng.energy_ac1()
    tr = eng.traces()
    assert tr.shape == (1, N, d + 1)
    for i in range(N):
        c = int(chain[i])
        assert n[c] == 1
        _lp_close(mom[c, 0], E.mp_lp(shape, betas[c], x[i]), ("refresh", shape.id, states[i][0], betas[c]))
        after = tr[0, c, :d]
        assert np.all(np.isfinite(after))
        assert mom[c, 1] == tr[0, c, d]
        _lp_close(tr[0, c, d], E.mp_lp(shape, betas[c], after), ("epilogue", shape.id, states[i][0], betas[c]))


# ---- (c) -------------------------------------------------------------------------------------------------------------------------------
def _slice_cases():
    out = []
    for gi, (shape, _, _) in enumerate(GROUPS):
        cp = shape.family == "changepoint"
        for w, p in ((10.0, 20), (2.0, 2) if cp else (0.25, 3)):
            for form in (("full", "cached") if cp else (None,)):
                out.append(pytest.param(gi, w, p, form, id="%s-w%g-p%d%s" % (GROUP_IDS[gi], w, p, "-" + form if form else "")))
    return out


def oracle_slice_step(shape, beta, x, rng_words, w, p):
    """one pass of SliceSampler on the restatement -> (state, RNG words, statistics)"""
    r = O.OracleRng(state=(int(rng_words[0]), int(rng_words[1])))
    sl = O.MixedSliceSampler(E.chain(shape, beta).path_lp, E.kinds(shape), w=w, p=p, n_passes=1)
    y = np.array(x, dtype=np.float64)
    sl.step(r, y)
    return y, r.state, sl.stats


@pytest.mark.parametrize("gi,w,p,form", _slice_cases())
def test_one_slice_transition_parity(P, gi, w, p, form):
    shape, _, states = GROUPS[gi]
    betas, x, chain, rng = layout(gi, shape, states)
    N = len(states)
    pt = _pt(P, shape, N, P.SliceSampler(w=w, p=p, n_passes=1))
    eng = pt.replicas
    if form is not None:
        eng.set_changepoint_form(P._lib.CHANGEPOINT_FORM_FULL if form == "full" else P._lib.CHANGEPOINT_FORM_CACHED)
    eng.set_schedule(betas)
    eng.set_states(x, chain, rng)
    eng.explore(1)
    x1, c1, r1 = eng.states()
    eng.reduce()
    am, an, ss, sn = eng.explorer_stats()
    assert np.array_equal(c1, chain)
    exact = E.kinds(shape) != E.COORD_FLOAT64
    for i in range(N):
        c = int(chain[i])
        if c == 0:                                   # the reference chain draws i.i.d.: the family tests hold that
            continue
        yv, words, stats = oracle_slice_step(shape, betas[c], x[i], rng[i], w, p)
        what = "%s %s chain %d" % (shape.id, states[i][0], c)
        assert (int(r1[i, 0]), int(r1[i, 1])) == words, what
        assert np.array_equal(x1[i][exact], yv[exact]), what
        np.testing.assert_allclose(x1[i], yv, rtol=RTOL, atol=1e-12, err_msg=what)
        assert an[c] == stats.acc_n and sn[c] == stats.steps_n and ss[c] == stats.steps_sum, what
        np.testing.assert_allclose(am[c], stats.acc_mean, rtol=RTOL, err_msg=what)


# ---- (d) -------------------------------------------------------------------------------------------------------------------------------
# by shape: at this step size the restatement's own MALA, from the battery states and these RNG words, leaves some chains moved (a proposal
# accepted) and some where they were (every proposal rejected); found on the CPU with mala_counts below
MALA_STEP = {                                        # (moved, left) on the CPU
    "ar1-T1-sv": 1.0, "ar1-T1-n": 1.0,               # (19, 3) (20, 2)
    "ar1-T8-sv": 0.5, "ar1-T8-n": 1.0,               # (1, 19) (2, 18)
    "ar1-T64-sv": 1.0, "ar1-T64-n": 1.0,             # (1, 20) (1, 21)
    "hier-J1-c": 2.0, "hier-J1-n": 3.0,              # (3, 2) (1, 4)
    "hier-J8-c": 1.0, "hier-J8-n": 1.0,              # (2, 3) (3, 2)
    "hier-J64-c": 1.0, "hier-J64-n": 0.5,            # (1, 4) (1, 4)
}
MALA_SHAPES = [s for s in E.SHAPES if s.family in ("ar1", "hier")]


def mala_groups(shape):
    """the battery states of |lp| <= 1e6 at both ends of the path (so at every beta), in groups of at most 16"""
    keep = [(n, v) for n, v in shape.states if abs(E.ref_lp(shape, 0.0, v)) <= 1e6 and abs(E.ref_lp(shape, 1.0, v)) <= 1e6]
    k = -(-len(keep) // 16)
    cuts = [round(i * len(keep) / k) for i in range(k + 1)]
    return [keep[a:b] for a, b in zip(cuts[:-1], cuts[1:])]


def mala_expected(P, shape, key, states, step):
    """(layout, std, n_refresh, the restatement's transition of every replica off the reference chain)"""
    betas, x, chain, rng = layout(key, shape, states)
    d = shape.dim
    ex = P.MALA(step_size=step)
    n_refresh = ex.base_n_refresh * int(math.ceil(d ** ex.exponent_n_refresh))
    std = np.random.default_rng(d).uniform(0.5, 2.0, d)
    res = {}
    for i in range(len(states)):
        c = int(chain[i])
        if c == 0:
            continue
        r = O.OracleRng(state=(int(rng[i, 0]), int(rng[i, 1])))
        Mv = A.build_preconditioner(r, d, 2, 1.0 / 3.0, 1.0 / 3.0, std)
        res[i] = (M.mala_transition(x[i], r, E.chain(shape, betas[c]), step, n_refresh, Mv), r.state)
    return (betas, x, chain, rng), std, n_refresh, res


def mala_counts(P, shape, step):
    """(chains moved, chains left where they were) over the shape's groups"""
    moved = stuck = 0
    for k, states in enumerate(mala_groups(shape)):
        (_, x, _, _), _, _, res = mala_expected(P, shape, 7000 + 10 * E.SHAPES.index(shape) + k, states, step)
        for i, (r, _) in res.items():
            same = np.array_equal(r["x"], x[i])
            moved += int(not same)
            stuck += int(same)
    return moved, stuck


@pytest.mark.parametrize("shape", MALA_SHAPES, ids=[s.id for s in MALA_SHAPES])
def test_one_mala_transition_parity(P, shape):
    step = MALA_STEP[shape.id]
    d = shape.dim
    moved = stuck = 0
    for k, states in enumerate(mala_groups(shape)):
        (betas, x, chain, rng), std, n_refresh, res = mala_expected(P, shape, 7000 + 10 * E.SHAPES.index(shape) + k, states, step)
        ex = P.MALA(step_size=step, preconditioner=P.MixDiagonalPreconditioner())
        eng = _engine(P, shape, ex, betas, x, chain, rng)
        eng.set_explorer_adaptation(step, std)
        eng.explore(2)
        x1, c1, r1 = eng.states()
        eng.reduce()
        am, an, ss, sn = eng.explorer_stats()
        assert np.array_equal(c1, chain)
        for i, (r, words) in res.items():
            c = int(chain[i])
            what = "%s %s chain %d" % (shape.id, states[i][0], c)
            assert (int(r1[i, 0]), int(r1[i, 1])) == words, what
            np.testing.assert_allclose(x1[i], r["x"], rtol=RTOL, atol=1e-12, err_msg=what)
            assert an[c] == r["acc_n"] and sn[c] == n_refresh and ss[c] == r["steps"], what
            np.testing.assert_allclose(am[c], r["acc_sum"] / r["acc_n"], rtol=RTOL, atol=1e-12, err_msg=what)
            same = np.array_equal(r["x"], x[i])
            moved += int(not same)
            stuck += int(same)
    assert moved > 0 and stuck > 0, (moved, stuck)


# ---- (f) -------------------------------------------------------------------------------------------------------------------------------
# One AutoMALA transition (base_n_refresh = 1, mix preconditioner, scan 2: with the MH step) from the same states as (d), of every family
# that has a gradient.  The step is 1 unless the shape is listed; KEPT is (states of |lp| <= 1e6 at both ends, states) by shape -- no state
# is left out silently.  tests/test_family_edges_cpu.py holds the restatement alone to the conditions that make the comparison meaningful.
AUTOMALA_SHAPES = [s for s in E.SHAPES if s.family in E.HAS_GRADIENT]
AUTOMALA_STEP = {}
AUTOMALA_KEPT = {
    "ar1-T1-sv": (24, 25), "ar1-T1-n": (24, 25), "ar1-T8-sv": (22, 25), "ar1-T8-n": (22, 25), "ar1-T64-sv": (23, 25), "ar1-T64-n": (24, 25),
    "hier-J1-c": (6, 10), "hier-J1-n": (6, 10), "hier-J8-c": (6, 10), "hier-J8-n": (6, 10), "hier-J64-c": (6, 10), "hier-J64-n": (6, 10),
    "glm-n1-d1-b": (6, 7), "glm-n1-d1-n": (3, 5), "glm-n65-d3-b": (6, 7), "glm-n65-d3-n": (3, 5), "glm-n130-d67-b": (6, 7), "glm-n130-d67-n": (3, 5),
    "mixture-K1-d1": (2, 4), "mixture-K3-d65": (3, 5), "mixture-K8-d64": (3, 5),
    "mixture_model-n1-K1": (3, 3), "mixture_model-n65-K3": (4, 4), "mixture_model-n200-K8": (4, 4),
    "dense-d1": (3, 4), "dense-d64": (3, 4), "dense-d65": (3, 4), "funnel-d2": (5, 6), "funnel-d65": (3, 6),
}


def automala_n_refresh(d):
    """AutoMALA's exponent_n_refresh = 0.35 at base_n_refresh = 1"""
    return int(math.ceil(d ** 0.35))


def automala_groups(shape):
    """[(key of layout(), states)]: mala_groups with a key range of its own"""
    return [(9000 + 10 * E.SHAPES.index(shape) + k, states) for k, states in enumerate(mala_groups(shape))]


def automala_expected(shape, key, states):
    """(layout, std, {replica off the reference chain: automala_ref.automala_transition's dict + words})"""
    betas, x, chain, rng = layout(key, shape, states)
    d, step = shape.dim, AUTOMALA_STEP.get(shape.id, 1.0)
    std = np.random.default_rng(d).uniform(0.5, 2.0, d)
    res = {}
    for i in range(len(states)):
        c = int(chain[i])
        if c == 0:
            continue
        r = O.OracleRng(state=(int(rng[i, 0]), int(rng[i, 1])))
        Mv = A.build_preconditioner(r, d, 2, 1.0 / 3.0, 1.0 / 3.0, std)
        res[i] = R.automala_transition(x[i], r, E.chain(shape, betas[c]), step, automala_n_refresh(d), Mv, True)
        res[i]["words"] = r.state
    return (betas, x, chain, rng), std, res


@pytest.mark.parametrize("shape", AUTOMALA_SHAPES, ids=[s.id for s in AUTOMALA_SHAPES])
def test_one_automala_transition_parity(P, shape):
    step = AUTOMALA_STEP.get(shape.id, 1.0)
    for key, states in automala_groups(shape):
        (betas, x, chain, rng), std, res = automala_expected(shape, key, states)
        ex = P.AutoMALA(base_n_refresh=1, step_size=step, preconditioner=P.MixDiagonalPreconditioner())
        eng = _engine(P, shape, ex, betas, x, chain, rng)
        eng.set_explorer_adaptation(step, std)
        eng.explore(2)
        R.assert_engine_matches(eng, chain, res, RTOL, lambda i: "%s %s" % (shape.id, states[i][0]))


# ---- (e) -------------------------------------------------------------------------------------------------------------------------------
def swap_expected(gi):
    """per scan in (1, 2): {lower chain c: (num_up, den_up, num_dn, den_dn, alpha, u)} from family_mp and the oracle's stream -- DEO pairs
    (c, c + 1) with c even on the odd scan, c odd on the even one"""
    shape, _, states = GROUPS[gi]
    betas, x, chain, rng = layout(gi, shape, states)
    N = len(states)
    slot = {int(chain[i]): i for i in range(N)}
    out = {}
    for scan in (1, 2):
        pairs = {}
        for c in range(scan % 2 == 0, N - 1, 2):
            i, j = slot[c], slot[c + 1]
            nu, du = E.mp_lp(shape, betas[c + 1], x[i]), E.mp_lp(shape, betas[c], x[i])
            nd, dd = E.mp_lp(shape, betas[c], x[j]), E.mp_lp(shape, betas[c + 1], x[j])
            alpha = min(mpf(1), mp.exp((nu - du) + (nd - dd)))
            u = O.OracleRng(state=(int(rng[i, 0]), int(rng[i, 1]))).rand()
            pairs[c] = (nu, du, nd, dd, alpha, u)
        out[scan] = pairs
    return (betas, x, chain, rng), out


@pytest.mark.parametrize("gi", range(len(GROUPS)), ids=GROUP_IDS)
def test_one_swap(P, gi):
    shape, _, states = GROUPS[gi]
    (betas, x, chain, rng), want = swap_expected(gi)
    N = len(states)
    assert sorted(list(want[1]) + list(want[2])) == list(range(N - 1))          # the two scans cover every pair
    for scan in (1, 2):
        for c, (_, _, _, _, alpha, u) in want[scan].items():
            assert abs(mpf(u) - alpha) >= 1e-6, (shape.id, scan, c, u, float(alpha))
    ex = P.SliceSampler(w=1.0, p=1, n_passes=1) if shape.family == "changepoint" else P.SliceSampler(w=0.25, p=3, n_passes=1)
    for scan in (1, 2):
        eng = _engine(P, shape, ex, betas, x, chain, rng, record=[P.log_sum_ratio, P.swap_acceptance_pr])
        eng.swap(scan)
        _, c1, _ = eng.states()
        eng.reduce()
        up, un, dn, dnn = eng.log_sum_ratio()
        acc, acc_n = eng.swap_acceptance()
        expect = chain.copy()
        for c in range(N - 1):
            if c not in want[scan]:
                assert un[c] == 0 and dnn[c] == 0 and acc_n[c] == 0, (shape.id, scan, c)
                continue
            nu, du, nd, dd, alpha, u = want[scan][c]
            what = (shape.id, scan, c)
            assert un[c] == 1 and dnn[c] == 1 and acc_n[c] == 1, what
            assert math.isfinite(up[c]) and math.isfinite(dn[c]), what
            assert abs(mpf(float(up[c])) - (nu - du)) <= LP_RTOL * (abs(nu) + abs(du)) + LP_ATOL, what + (up[c], float(nu - du))
            assert abs(mpf(float(dn[c])) - (nd - dd)) <= LP_RTOL * (abs(nd) + abs(dd)) + LP_ATOL, what + (dn[c], float(nd - dd))
            with np.errstate(over="ignore"):
                assert math.isclose(acc[c], min(1.0, float(np.exp(up[c] + dn[c]))), rel_tol=1e-9, abs_tol=1e-300), what
            if u < alpha:
                i, j = (int(np.flatnonzero(chain == k)[0]) for k in (c, c + 1))
                expect[i], expect[j] = c + 1, c
        assert np.array_equal(c1, expect), (shape.id, scan, c1, expect)
