"""The restatements tests/<family>_ref.py at the edge battery (tests/family_edges.py) against the 60-digit evaluation of each model's
definition (tests/family_mp.py).  The restatements follow the kernels' operations in the kernels' order, so a formula that is wrong in
both -- a cancellation, a special case that misses its case -- shows here, on the CPU, before the device is held to the same battery
(tests/test_gpu_family_edges.py).

Log densities: every battery state at beta in {0, 0.37, 1}, |restatement - mp| <= 1e-11 |mp| + 1e-11 (LP_RTOL and abs_tol of
tests/test_gpu_hier.py), the restatement never NaN, the 60-digit value always finite.

Gradients (the families that have one): lp_grad at beta = 0.37 -- the AD form has no short-circuit, so one beta inside (0, 1) runs both end
points' gradients -- against mp.diff of the 60-digit density, coordinate by coordinate: |d_i| <= 1e-9 |g_i| + floor ||g||_inf.  The floor is
10 x the largest error of the restatement against mp.diff, relative to ||g||_inf, measured on two N(0, 1.5^2) states (default_rng(99)) of
every shape of the battery at beta = 0.37 -- the states of the existing tests, where nothing cancels; the factor 10 covers libm's ulps from
one platform to the next.  Measured:
    mixture 1.4e-16   glm 7.7e-16   mixture_model 5.9e-16   hier 4.6e-16   ar1 3.1e-16   dense 4.5e-16   funnel 5.0e-16
test_the_measured_ratios_hold repeats the measurement on the small shapes.

Before AmTarget::ar1_and_sqr_norm and Ar1.leaves took 1 - phi^2, its root, its log and 1 - phi from exp(-2 |a|), the AR(1) cases failed:
om = 1 - tanh(a)^2 cancels, the log density was off by 5.5e-9 at |a| = 10, 1.6e-7 at 12, 8.3e-5 at 15, 2.2e-2 at 18 and -inf from
|a| = 19.07 (19.5, 25), whatever T and the observation model, and d/dmu (through (1 - phi) / sigma) failed from a = 10.

AutoMALA (part (f) of tests/test_gpu_family_edges.py): the restatement's transition (tests/automala_ref.py) from the battery states, alone:
it must not raise, no decision of it may be closer than 1e-6 to going the other way (the floor of test_one_swap's |u - alpha|; at
|lp| + |ke| <= ~1e3 it is 100 x the log-density tolerance above) -- otherwise a device that differs in the last bits could rightly decide
otherwise --, and over each family it must move some chains and leave others, pass and fail the reversibility check, and on AR(1), the
hierarchical family and the funnel meet non-finite trials.  Measured (kept states, chains moved / left, checks passed / failed, non-finite
trials, exponents, least margin):
    ar1 139 of 150, 47 / 80, 104 / 319, 87, -7 .. 1, 6.7e-5       hier 36 of 60, 19 / 11, 36 / 64, 5, -6 .. 1, 1.2e-3
    glm 27 of 36, 6 / 15, 15 / 41, 0, -9 .. 1, 1.8e-4             mixture 8 of 14, 2 / 3, 10 / 11, 0, -12 .. -5, 1.1e-2
    mixture_model 11 of 11, 1 / 7, 6 / 19, 0, -43 .. 1, 3.1e-2    dense 9 of 12, 3 / 3, 9 / 13, 0, -3 .. 1, 3.2e-2
    funnel 8 of 12, 2 / 4, 5 / 13, 12, -25 .. 2, 2.4e-3"""
import math

import numpy as np
import pytest
from mpmath import mp, mpf

import family_edges as E
import test_gpu_family_edges as G                   # part (f)'s states, layout and restatement: the very ones the device is compared with

LP_RTOL, LP_ATOL = 1e-11, 1e-11
G_RTOL = 1e-9
BETAS = (0.0, 0.37, 1.0)
G_BETA = 0.37
G_RATIO = {"mixture": 1.4e-16, "glm": 7.7e-16, "mixture_model": 5.9e-16, "hier": 4.6e-16, "ar1": 3.1e-16, "dense": 4.5e-16, "funnel": 5.0e-16}


def mp_gradient(shape, beta, x):
    """mp.diff of the 60-digit path density, one coordinate at a time: the one-sided rule (its step is 2^-210: the truncation error is far
    below the 60 digits), so that the value at the state itself is computed once and serves every coordinate"""
    v = [mpf(float(c)) for c in x]
    at_x = {}
    out = []
    for i in range(len(v)):
        def f(t, i=i):
            if t == v[i]:
                if mp.prec not in at_x:
                    at_x[mp.prec] = E.mp_lp(shape, beta, v)
                return at_x[mp.prec]
            w = list(v)
            w[i] = t
            return E.mp_lp(shape, beta, w)
        out.append(mp.diff(f, v[i], direction=1))
    return out


def _gradient_error(shape, x):
    """(|restatement - mp| per coordinate, |mp| per coordinate) as mpf"""
    _, got = E.chain(shape, G_BETA).lp_grad(np.array(x, dtype=np.float64))
    want = mp_gradient(shape, G_BETA, x)
    assert not np.any(np.isnan(got)), (shape, got)
    return [abs(mpf(float(a)) - w) if math.isfinite(a) else mp.inf for a, w in zip(got, want)], [abs(w) for w in want]


def test_the_battery_covers_every_family():
    assert sorted(set(s.family for s in E.SHAPES)) == sorted(E.FAMILIES) and len(E.FAMILIES) == 9
    assert len(set(s.id for s in E.SHAPES)) == len(E.SHAPES)
    for s in E.SHAPES:
        assert all(np.all(np.isfinite(x)) for _, x in s.states), s


@pytest.mark.parametrize("shape", E.SHAPES, ids=[s.id for s in E.SHAPES])
def test_log_density_against_the_definition(shape):
    bad = []
    for name, x in shape.states:
        for beta in BETAS:
            want = E.mp_lp(shape, beta, x)
            assert mp.isfinite(want), (shape, name, beta)
            got = E.ref_lp(shape, beta, x)
            assert not math.isnan(got), (shape, name, beta)
            err = abs(mpf(got) - want) if math.isfinite(got) else mp.inf
            if not err <= LP_RTOL * abs(want) + LP_ATOL:
                bad.append((name, beta, got, float(want), float(err)))
    assert not bad, bad


@pytest.mark.parametrize("shape", [s for s in E.SHAPES if s.family in E.HAS_GRADIENT],
                         ids=[s.id for s in E.SHAPES if s.family in E.HAS_GRADIENT])
def test_gradient_against_the_definition(shape):
    bad = []
    for name, x in shape.states:
        err, mag = _gradient_error(shape, x)
        floor = 10.0 * G_RATIO[shape.family] * max(mag)
        for i, (e, m) in enumerate(zip(err, mag)):
            if not e <= G_RTOL * m + floor:
                bad.append((name, i, float(e), float(m), float(floor)))
    assert not bad, bad


@pytest.mark.parametrize("shape", [s for s in E.SHAPES if s.family in E.HAS_GRADIENT and s.dim <= 12],
                         ids=[s.id for s in E.SHAPES if s.family in E.HAS_GRADIENT and s.dim <= 12])
def test_the_measured_ratios_hold(shape):
    """the measurement behind G_RATIO, on the shapes small enough to repeat here: within the factor 10 that the floor allows"""
    g = np.random.default_rng(99)
    for _ in range(2):
        err, mag = _gradient_error(shape, g.normal(0.0, 1.5, shape.dim))
        assert max(err) <= 10.0 * G_RATIO[shape.family] * max(mag), (shape, float(max(err) / max(mag)))


# ---- AutoMALA from the battery states: the restatement alone -----------------------------------------------------------------------------
MARGIN_FLOOR = 1e-6
_AUTOMALA = {}


def automala_summary(shape):
    """the restatement's transitions of part (f) of the shape (run once): dict(kept, moved, left, passed, failed, nonfinite, margin)"""
    if shape.id not in _AUTOMALA:
        out = dict(kept=0, moved=0, left=0, passed=0, failed=0, nonfinite=0, margin=math.inf)
        for key, states in G.automala_groups(shape):
            out["kept"] += len(states)
            (_, x, chain, _), _, res = G.automala_expected(shape, key, states)           # (raises where a state has no density or no step)
            assert len(res) == len(states) - 1 and all(np.all(np.isfinite(w["x"])) for w in res.values())
            for i, w in res.items():
                same = np.array_equal(w["x"], x[i])
                out["moved"] += int(not same)
                out["left"] += int(same)
                out["passed"] += w["rev_sum"]
                out["failed"] += w["rev_n"] - w["rev_sum"]
                out["nonfinite"] += w["nonfinite"]
                out["margin"] = min(out["margin"], min(w["margins"]))
        _AUTOMALA[shape.id] = out
    return _AUTOMALA[shape.id]


def test_automala_covers_every_gradient_shape():
    assert [s.id for s in G.AUTOMALA_SHAPES] == [s.id for s in E.SHAPES if s.family not in ("varsel", "changepoint")]
    assert sorted(G.AUTOMALA_KEPT) == sorted(s.id for s in G.AUTOMALA_SHAPES) and len(G.AUTOMALA_SHAPES) == 29


@pytest.mark.parametrize("shape", G.AUTOMALA_SHAPES, ids=[s.id for s in G.AUTOMALA_SHAPES])
def test_automala_from_the_battery_states(shape):
    got = automala_summary(shape)
    print(shape.id, got)
    assert (got["kept"], len(shape.states)) == G.AUTOMALA_KEPT[shape.id]
    assert got["margin"] >= MARGIN_FLOOR, got


@pytest.mark.parametrize("family", E.HAS_GRADIENT)
def test_automala_decides_both_ways_in_every_family(family):
    tot = {}
    for s in G.AUTOMALA_SHAPES:
        if s.family == family:
            for k, v in automala_summary(s).items():
                tot[k] = tot.get(k, 0) + v if k != "margin" else min(tot.get(k, math.inf), v)
    print(family, tot)
    assert tot["moved"] > 0 and tot["left"] > 0 and tot["passed"] > 0 and tot["failed"] > 0, tot
    if family in ("ar1", "hier", "funnel"):
        assert tot["nonfinite"] > 0, tot
