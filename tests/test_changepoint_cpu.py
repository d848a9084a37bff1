"""The Poisson change-point family without a GPU: pte_create accepts it (a valid configuration reaches the device check) and refuses -- before
any device work -- what the device does not run; the Python and Julia surfaces map PoissonChangePoint onto pte_config and
pte_set_target_changepoint; the NumPy restatement (tests/changepoint_ref.py) agrees with the textbook density, and the oracle's
MixedSliceSampler -- Float64 and Integer coordinates -- on the restatement's call-back samples the enumerated posterior."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import changepoint_ref as R
import family_cpu as F
import oracle as O
from family_cpu import ROOT, P  # noqa: F401  (P: the module's fixture)


def test_enum_and_export_mirrors(P):
    import __graft_entry__ as g
    from pigeons_amd import _lib
    assert _lib.TARGET_CHANGE_POINT == 8
    assert "pte_set_target_changepoint" in _lib.EXPORTS and "pte_set_changepoint_form" in _lib.EXPORTS
    assert hasattr(_lib.load(), "pte_set_target_changepoint")
    hdr = F.HEADER
    assert "PTE_TARGET_CHANGE_POINT = 8" in hdr and "int pte_set_target_changepoint(pte_engine *h, const double *y" in hdr
    jl = F.JULIA
    assert "const TARGET_CHANGE_POINT = Int32(8)\n" in jl
    assert "struct DevicePoissonChangePoint" in jl and "device_family(t::DevicePoissonChangePoint, inputs)" in jl
    assert ":pte_set_target_changepoint" in jl
    assert "PoissonChangePoint" in P.__dict__
    assert ("pte_changepoint.hip", []) in g.UNITS and len(g.UNITS) == 8
    params = open(os.path.join(ROOT, "pigeons.jl_amd", "csrc", "pte_automala_params.hpp")).read()
    assert "X(changepoint)" in params and "EIGHT translation units" in params


@pytest.mark.parametrize("dim", [3, 9, 63, 65, 127])
def test_accepted_config_reaches_the_device_check(P, dim):
    """fails on the code before the family existed ("target 8 has no device log-potential"): a valid configuration now passes validation"""
    F.no_device()
    from pigeons_amd import _lib
    F.assert_reaches_the_device_check(P, n_chains=4, target=8, dim=dim, explorer=2, target_params=[1.0])
    F.assert_reaches_the_device_check(P, n_chains=4, target=8, dim=dim, explorer=2, slice_w=3.0)
    for dk in (0x1000, 0x2000):                         # the scan-loop flags (PTE_KERNEL_FLAG_BITS) are allowed
        if dk & _lib.KERNEL_FLAG_BITS:
            F.assert_reaches_the_device_check(P, n_chains=4, target=8, dim=dim, explorer=2, debug_kernel=dk)


_CP = dict(target=8, dim=7, explorer=2, n_chains=4)


@pytest.mark.parametrize("kw,msg", [
    (dict(explorer=3), "change-point path is explored by SliceSampler only"),                  # AutoMALA
    (dict(explorer=5), "change-point path is explored by SliceSampler only"),                  # MALA
    (dict(explorer=1), "change-point path is explored by SliceSampler only"),                  # ToyExplorer
    (dict(explorer=4), "change-point path is explored by SliceSampler only"),                  # IsingMetropolis
    (dict(explorer=0), "change-point path is explored by SliceSampler only"),                  # none
    (dict(explorer=2, explorer2=3), "change-point path is explored by SliceSampler only"),     # Compose(SliceSampler, AutoMALA)
    (dict(explorer=5, explorer2=2), "change-point path is explored by SliceSampler only"),     # Compose(MALA, SliceSampler)
    (dict(explorer=2, explorer2=2), "change-point path is explored by SliceSampler only"),
    (dict(explorer=6), "AAPS is implemented on the scaled-precision MVN and funnel paths only"),      # AAPS keeps its refusal
    (dict(dim=8), r"dim = 2 K \+ 1 must be odd \(got 8\)"),
    (dict(dim=2), r"dim = 2 K \+ 1 must be odd \(got 2\)"),
    (dict(dim=128), r"dim = 2 K \+ 1 must be odd \(got 128\)"),
    (dict(dim=1), r"K = \(dim - 1\) / 2 must be in 1\.\.63 \(got dim 1\)"),
    (dict(dim=129), r"K = \(dim - 1\) / 2 must be in 1\.\.63 \(got dim 129\)"),
    (dict(dim=4095), r"K = \(dim - 1\) / 2 must be in 1\.\.63"),
    (dict(debug_kernel=1), "debug_kernel 1 is not available on the change-point path"),
    (dict(debug_kernel=8), "debug_kernel 8 is not available on the change-point path"),
    (dict(n_chains_variational=4), "two-leg tempering"),
    (dict(slice_w=2.5), r"for integer variables, the width should be an integer\. Got: 2\.5"),
    (dict(slice_w=float("inf")), r"for integer variables, the width should be an integer\. Got: inf"),
])
def test_pte_create_refusals(P, kw, msg):
    F.assert_create_refused(P, _CP, kw, msg)


def test_the_setters_refusals_are_in_the_library():
    """pte_set_target_changepoint needs an engine, so a machine without a device cannot reach these; their text is pinned here and they are
    raised on the device in tests/test_gpu_changepoint.py"""
    src = open(os.path.join(ROOT, "pigeons.jl_amd", "csrc", "pte.hip")).read()
    for msg in ("pte_set_target_changepoint: the device holds 1..65536 observations (got %lld)",
                "pte_set_target_changepoint: y[%lld] must be an integer count in 0..2^20 (got %g)",
                "pte_set_target_changepoint: null argument",
                "pte_set_target_changepoint: this engine's target is %d, not PTE_TARGET_CHANGE_POINT",
                "pte_set_changepoint_form: form must be PTE_CHANGEPOINT_FORM_AUTO (0), _FULL (1) or _CACHED (2) (got %d)",
                "only the interpolated (funnel) path has a replaceable reference"):
        assert msg in src, msg


_Y = [1, 0, 2, 1, 0, 2, 3, 5, 2, 4, 6, 3]


def _captured(P, target, **kw):
    return F.captured(P, target, ref_dim=target.n_rates, **kw)               # the reference has K + 1 coordinates, not 2 K + 1


def test_python_mapping(P):
    from pigeons_amd import _lib
    t = P.PoissonChangePoint(_Y, 3)
    kw = _captured(P, t)
    assert kw["target"] == _lib.TARGET_CHANGE_POINT and kw["dim"] == 7 and list(kw["target_params"]) == [0.5]
    assert kw["explorer"] == _lib.EXPLORER_SLICE and "explorer2" not in kw          # default explorer: SliceSampler (target.jl:20)
    assert kw["slice_w"] == 10.0
    (ys,), = kw["set_target_changepoint"]                                           # set after create, once per engine
    np.testing.assert_array_equal(ys, np.array(_Y, dtype=np.float64))
    kw = _captured(P, t, explorer=P.SliceSampler(n_passes=2, w=4.0))
    assert kw["slice_n_passes"] == 2 and kw["slice_w"] == 4.0
    for ex in (P.AutoMALA(), P.MALA(), P.AAPS(), P.Compose(P.SliceSampler(), P.AutoMALA()), P.Compose(P.SliceSampler(), P.SliceSampler())):
        with pytest.raises(NotImplementedError, match="explored by SliceSampler only"):
            _captured(P, t, explorer=ex)
    F.assert_reference_refusals(P, t, wrong_dim=7, ref_dim=t.n_rates)               # (a reference of 2 K + 1 coordinates is the wrong one)


def test_every_shard_gets_the_data(P):
    F.assert_every_shard_gets_the_data(P, P.PoissonChangePoint(_Y, 2), P.ScaledPrecisionNormalLogPotential(1.0, 3), N=4, d=5,
                                       setter="set_target_changepoint")


@pytest.mark.parametrize("args,msg", [
    (([], 1), r"1\.\.65536 observations"),
    ((np.zeros(65537), 1), r"1\.\.65536 observations"),
    ((np.zeros((3, 2)), 1), r"1\.\.65536 observations"),
    (([1.0, 0.5], 1), "integer count"),
    (([1.0, -1.0], 1), "integer count"),
    (([1.0, np.nan], 1), "integer count"),
    (([1.0, np.inf], 1), "integer count"),
    (([1.0, 2.0 ** 20 + 1], 1), "integer count"),
    (([1.0, 2.0], 0), r"n_changepoints must be in 1\.\.63"),
    (([1.0, 2.0], 64), r"n_changepoints must be in 1\.\.63"),
    (([1.0, 2.0], 1.5), r"n_changepoints must be in 1\.\.63"),
])
def test_python_validation(P, args, msg):
    with pytest.raises(ValueError, match=msg):
        P.PoissonChangePoint(*args)


def test_change_point_surface(P):
    t = P.PoissonChangePoint(_Y, 2)
    assert t.n_obs == 12 and t.n_changepoints == 2 and t.n_rates == 3 and t.dim == 5
    assert P.PoissonChangePoint(np.full(65536, 2.0 ** 20), 63).dim == 127             # the limits themselves are accepted
    assert P.PoissonChangePoint([0], 1).dim == 3
    want = -1.5 * math.log(2 * math.pi / 0.5) - 2 * math.log(13.0)
    assert math.isclose(t.evidence_offset(0.5), want, rel_tol=1e-15)
    assert math.isclose(t.evidence_offset(0.5), R.ChangePoint(_Y, 2, 0.5).evidence_offset(), rel_tol=1e-15)
    assert "evidence_offset" in P.PoissonChangePoint.__doc__ and "K log(n + 1)" in P.PoissonChangePoint.__doc__


def test_set_target_changepoint_is_bound(P):
    from pigeons_amd import _lib
    L = _lib.load()
    F.assert_null_engine_refused(L.pte_set_target_changepoint, (None, None, 2), {2: C.c_int64}, n_args=3)
    assert L.pte_set_changepoint_form(None, 1) == 1


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------
def _textbook(y, K, p, state):
    """sum of Poisson log-pmfs per observation + N(0, I / p) on the rates + uniform on the (n + 1)^K placements"""
    n = len(y)
    r, tau = np.asarray(state[:K + 1]), np.asarray(state[K + 1:])
    b = [0] + sorted(int(t) for t in tau) + [n]
    ll = 0.0
    for j in range(K + 1):
        for i in range(b[j], b[j + 1]):
            ll += y[i] * r[j] - math.exp(r[j]) - math.lgamma(y[i] + 1.0)
    prior = sum(-0.5 * math.log(2 * math.pi / p) - 0.5 * p * v * v for v in r) - K * math.log(n + 1.0)
    return prior + ll


def test_restatement_against_the_textbook_density():
    g = np.random.default_rng(5)
    n, K, p = 40, 4, 0.7
    y = g.poisson(np.repeat([1.0, 6.0, 0.5, 9.0, 3.0], 8)).astype(float)
    cp = R.ChangePoint(y, K, p)
    states = [np.concatenate([g.normal(0.0, 1.0, K + 1), g.integers(0, n + 1, K).astype(float)]) for _ in range(20)]
    states.append(np.concatenate([g.normal(0.0, 1.0, K + 1), [7.0, 7.0, 30.0, 7.0]]))          # ties
    states.append(np.concatenate([g.normal(0.0, 1.0, K + 1), [0.0, float(n), 0.0, float(n)]]))  # taus at 0 and n: empty first and last segments
    states.append(np.concatenate([g.normal(0.0, 1.0, K + 1), [float(n), 3.0, 0.0, 3.0]]))
    states.append(np.zeros(2 * K + 1))                                                          # the initial state
    for s in states:
        assert cp.inside(s)
        assert math.isclose(cp.lp(s), _textbook(y, K, p, s), rel_tol=1e-12), s
        assert R.ChangePointChain(cp, 1.0, p).path_lp(s) == cp.lp(s)
        assert math.isclose(R.ChangePointChain(cp, 0.0, p).path_lp(s), -0.5 * p * float(np.sum(np.square(s[:K + 1]))), rel_tol=1e-14, abs_tol=1e-300)
    # an empty segment with a rate whose exp overflows contributes exactly 0: the result is finite and is the textbook's without that rate's likelihood
    s = np.concatenate([[0.3, 800.0, -0.2, 0.1, 0.4], [5.0, 5.0, 20.0, 31.0]])
    assert math.isfinite(cp.lp(s)) and math.isclose(cp.lp(s), _textbook(y, K, p, s), rel_tol=1e-12)
    s[1] = 710.0
    assert math.isfinite(cp.lp(s))
    # one tau outside the support: -inf at every beta, the reference's included
    for bad in (-1.0, n + 1.0):
        s = np.concatenate([g.normal(0.0, 1.0, K + 1), [3.0, bad, 9.0, 12.0]])
        assert cp.lp(s) == -math.inf
        for beta in (0.0, 0.3, 1.0):
            assert R.ChangePointChain(cp, beta, p).path_lp(s) == -math.inf


def test_path_interpolates_and_the_taus_are_exchangeable():
    g = np.random.default_rng(8)
    y = g.poisson(4.0, 30).astype(float)
    cp = R.ChangePoint(y, 3, 0.5)
    s = np.concatenate([g.normal(0.0, 1.0, 4), [20.0, 4.0, 11.0]])
    S, ls = cp.sums(s)
    ref, tgt = (-0.25) * S, cp.lp(s)
    assert R.ChangePointChain(cp, 0.0, 0.5).path_lp(s) == ref and R.ChangePointChain(cp, 1.0, 0.5).path_lp(s) == tgt
    assert R.ChangePointChain(cp, 0.25, 0.5).path_lp(s) == 0.75 * ref + 0.25 * tgt
    for perm in ([4.0, 11.0, 20.0], [11.0, 20.0, 4.0]):                              # K! relabellings, one density
        assert cp.lp(np.concatenate([s[:4], perm])) == tgt
    assert math.isclose(cp.c_obs, -sum(math.lgamma(v + 1.0) for v in y), rel_tol=1e-14)


def test_enumeration_integrates_to_the_evidence_of_a_one_segment_model():
    """K = 1 on one observation: the two placements tau = 0, 1 put y_0 in segment 1 or segment 0, so p(y) is the one-segment evidence,
    here against a brute-force Riemann sum of Poisson(y; exp(r)) N(r; 0, 1 / p)"""
    p, y0 = 0.8, 3.0
    cp = R.ChangePoint([y0], 1, p)
    log_ev, post = cp.exact()
    r = np.linspace(-30.0, 12.0, 400001)
    f = np.exp(y0 * r - np.exp(r) - math.lgamma(y0 + 1.0) - 0.5 * p * r * r - 0.5 * math.log(2 * math.pi / p))
    assert math.isclose(log_ev, math.log(f.sum() * (r[1] - r[0])), abs_tol=1e-9)
    assert math.isclose(post[(0,)], 0.5, rel_tol=1e-12) and math.isclose(post[(1,)], 0.5, rel_tol=1e-12)


def test_mixed_slice_sampler_samples_the_enumerated_posterior():
    """the oracle's MixedSliceSampler (Float64 method on the two rates, Integer method on tau) on ChangePointChain.path_lp at beta = 1,
    K = 1, n = 12: the pmf of tau over 3000 steps against the enumeration, every value within 5 standard errors -- the batch-means error
    over 30 batches, and never less than the binomial error sqrt(q (1 - q) / T) of as many independent draws, which bounds it from below
    (a value the walk visited in no batch or in one has no batch-means error to speak of)"""
    p, K, T, B = 0.5, 1, 3000, 30
    y = np.array(_Y, dtype=np.float64)
    n = y.size
    cp = R.ChangePoint(y, K, p)
    _, post = cp.exact()
    q = np.array([post[(t,)] for t in range(n + 1)])
    assert math.isclose(q.sum(), 1.0, rel_tol=1e-12) and np.sum(q > 0.05) >= 3 and q.max() < 0.8       # a posterior with some spread
    ch = R.ChangePointChain(cp, 1.0, p)
    kinds = np.array([O.COORD_FLOAT64] * (K + 1) + [O.COORD_INTEGER] * K, dtype=np.int32)
    s = O.MixedSliceSampler(ch.path_lp, kinds, n_passes=1)
    rng = O.OracleRng(seed=17)
    state = np.zeros(2 * K + 1)
    taus = np.empty(T)
    for t in range(T):
        s.step(rng, state)
        taus[t] = state[2]
    assert np.all(taus == np.floor(taus)) and taus.min() >= 0 and taus.max() <= n
    ind = (taus[:, None] == np.arange(n + 1)[None, :]).astype(float)
    phat = ind.mean(axis=0)
    se_bm = ind.reshape(B, T // B, n + 1).mean(axis=1).std(axis=0, ddof=1) / math.sqrt(B)
    se = np.maximum(se_bm, np.sqrt(q * (1.0 - q) / T))
    dev = (phat - q) / se
    print("pmf of tau: deviations / se", np.round(dev, 2))
    assert np.all(np.abs(dev) < 5.0), (phat, q, se)
    assert s.stats.steps_n == 2 * T * (2 * K + 1)          # both methods record two step counts per visit
