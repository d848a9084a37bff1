"""A NumPy restatement of one AutoMALA transition (src/explorers/AutoMALA.jl as pigeons.jl_amd/csrc/pte_automala.hpp cites it) as the
device runs it.  The test files use it as their reference; tests/test_automala_ref_cpu.py holds it to the C oracle.

It is written the way the reference is, not the way the kernel is: auto_step_size returns an exponent, and the proposal is the leapfrog
from the start point at step_size * 2^exponent.  The kernel keeps one of the search's own trials instead (the log density and the gradient
are pure functions of the state); here every trial of a search is remembered under its step, so the proposal is looked up, whichever
trial the kernel chose to keep.  The target is a chain with lp_grad(x) -> (log density, gradient) (tests/<family>_ref.py, aaps_ref.py);
the draws come from tests/oracle.py::OracleRng in the reference's order: per refresh d normals of the momentum, the two uniforms of the
acceptance window, and -- with the MH step -- one uniform, drawn whether the reversibility check passed or not.  The preconditioner M
is drawn already (aaps_ref.build_preconditioner: its uniforms come first).  Every |p|^2 follows the fixed tree of DESIGN 3."""
import math

import numpy as np

from mixture_ref import tree_sum


class AutoMalaError(ValueError):
    pass


def _leap_frog(chain, M, x, p, g0, eps):
    """hamiltonian_dynamics! with n_steps = 1 from (x, p), g0 the conditioned gradient at x -> (x, p, conditioned gradient, log density,
    kinetic energy of the momentum it leaves).  It returns at the first non-finite lp - ke, without the second half step"""
    half = eps / 2
    p = p + half * g0
    x = x + eps * (p / M)
    lp, g = chain.lp_grad(x)
    g = g / M
    ke = 0.5 * tree_sum(p * p)
    if math.isfinite(lp - ke):
        p = p + half * g
        ke = 0.5 * tree_sum(p * p)
    return x, p, g, lp, ke


def automala_transition(x0, rng, chain, step_size, n_refresh, M, use_mh):
    """explore! with AutoMALA (AutoMALA.jl:84-182) as automala_body runs it: n_refresh refreshes of momentum, each a forward step-size
    search, the proposal and -- with use_mh (every scan but the first of a round) -- the reversed search and the MH step.
    -> dict(x, acc_sum, acc_n, steps_sum, steps_n, fac_sum, fac_n, rev_sum, rev_n, accepted, exponents, nonfinite, margins): the recorders
    as the engine sums them; accepted the number of proposals the MH step took; exponents of every search in order (forward, reversed,
    forward, ...); nonfinite the number of trials whose difference of log joints was not finite; margins every finite
    |difference - bound| that a comparison looked at and |u - probability| where 0 < probability < 1 -- how far each decision was from
    going the other way"""
    x = np.asarray(x0, dtype=np.float64).copy()
    d = x.size
    out = dict(acc_sum=0.0, acc_n=0, steps_sum=0, steps_n=0, fac_sum=0.0, fac_n=0, rev_sum=0, rev_n=0, accepted=0, exponents=[], nonfinite=0, margins=[])

    def beyond(diff, bound, above):
        """diff > bound (above) or diff < bound, noting the margin"""
        if math.isfinite(diff):
            out["margins"].append(abs(diff - bound))
        return diff > bound if above else diff < bound

    def auto_step_size(x, p, g0, h_before, lower, upper):
        """auto_step_size (:184-214) -> (exponent, {step: its trial leapfrog})"""
        trials = {}

        def difference(eps):
            trials[eps] = t = _leap_frog(chain, M, x, p, g0, eps)
            diff = (t[3] - t[4]) - h_before
            out["nonfinite"] += int(not math.isfinite(diff))
            return diff

        eps = step_size
        diff = difference(eps)
        n_steps = exponent = 0
        if not math.isfinite(diff) or beyond(diff, lower, False):
            n = 1
            while True:                                          # shrink_step_size (:233-248)
                eps /= 2.0
                diff = difference(eps)
                if eps == 0.0:
                    raise AutoMalaError("AutoMALA: could not find a positive step size")
                if beyond(diff, lower, True):
                    n_steps, exponent = n, -n
                    break
                n += 1
        elif beyond(diff, upper, True):
            n = 1
            while True:                                          # grow_step_size (:216-231): one step back from the first that went too far
                eps *= 2.0
                diff = difference(eps)
                if not math.isfinite(diff) or beyond(diff, upper, False):
                    n_steps, exponent = n, n - 1
                    break
                n += 1
        out["steps_sum"] += 1 + n_steps
        out["steps_n"] += 1
        out["fac_sum"] += math.ldexp(1.0, exponent)
        out["fac_n"] += 1
        out["exponents"].append(exponent)
        return exponent, trials

    with np.errstate(all="ignore"):
        lp0, g0 = chain.lp_grad(x)
        g0 = g0 / M
        for _ in range(n_refresh):
            p = np.array([rng.randn() for _ in range(d)])
            init_joint = lp0 - 0.5 * tree_sum(p * p)
            if not math.isfinite(init_joint):
                raise AutoMalaError("AutoMALA can only be called on a configuration of positive density")
            ua, ub = rng.rand(), rng.rand()
            lower, upper = math.log(min(ua, ub)), math.log(max(ua, ub))
            proposed, trials = auto_step_size(x, p, g0, init_joint, lower, upper)
            eps = step_size * math.ldexp(1.0, proposed)
            xn, pn, gn, lpn, _ = trials[eps] if eps in trials else _leap_frog(chain, M, x, p, g0, eps)
            if not use_mh:                                       # the first scan of a round: the chain stays where the proposal ended
                x, lp0, g0 = xn, lpn, gn
                continue
            pn = pn * -1.0
            h_rev = lpn - 0.5 * tree_sum(pn * pn)                # log_joint at the proposed point: the reversed search's start, and final_joint_log
            reversed_, _ = auto_step_size(xn, pn, gn, h_rev, lower, upper)
            passed = reversed_ == proposed
            out["rev_sum"] += int(passed)
            out["rev_n"] += 1
            probability = 0.0
            if passed:
                ex = float(np.exp(h_rev - init_joint))
                probability = ex if ex < 1.0 else (ex if math.isnan(ex) else 1.0)
            out["acc_sum"] += probability
            out["acc_n"] += 1
            u = rng.rand()                                       # drawn always
            if 0.0 < probability < 1.0:
                out["margins"].append(abs(u - probability))
            if u < probability:
                out["accepted"] += 1
                x, lp0, g0 = xn, lpn, gn
    out["x"] = x
    return out


def assert_engine_matches(eng, chain, res, rtol, what):
    """the device tests' comparison: a pigeons_amd engine after one explore against {replica: automala_transition's dict + words}.  RNG words
    and counting recorders equal -- the sum of the step-size factors too: a sum of powers of two --, states and mean acceptance within
    rtol (states: + 1e-12); the chain permutation unchanged.  what(replica) names the replica in a failure"""
    x1, c1, r1 = eng.states()
    eng.reduce()
    am, an, ss, sn = eng.explorer_stats()
    fm, fn, rm, rn = eng.automala_stats()
    assert np.array_equal(c1, chain)
    for i, w in res.items():
        c = int(chain[i])
        at = "%s replica %d chain %d" % (what(i), i, c)
        assert (int(r1[i, 0]), int(r1[i, 1])) == tuple(w["words"]), at
        np.testing.assert_allclose(x1[i], w["x"], rtol=rtol, atol=1e-12, err_msg=at)
        assert (an[c], sn[c], ss[c]) == (w["acc_n"], w["steps_n"], w["steps_sum"]), at
        assert (fn[c], rn[c]) == (w["fac_n"], w["rev_n"]), at
        assert fm[c] == w["fac_sum"] / w["fac_n"], at                 # the engine reports sum / n: the same division of the same sum
        assert rm[c] == (w["rev_sum"] / w["rev_n"] if w["rev_n"] else 0.0), at
        if w["acc_n"]:
            np.testing.assert_allclose(am[c], w["acc_sum"] / w["acc_n"], rtol=rtol, atol=1e-12, err_msg=at)
