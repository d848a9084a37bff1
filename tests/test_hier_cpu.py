"""The hierarchical normal-means family without a GPU: pte_create accepts it (a valid configuration reaches the device check) and refuses --
before any device work -- what the device does not run; the Python and Julia surfaces map HierarchicalNormalMeans onto pte_config and
pte_set_target_hier; the NumPy restatement (tests/hier_ref.py) has the right gradient, its two parameterisations are one density under the
change of variables, its quadrature agrees with a 2-D grid integration and with the eight-schools numbers of DESIGN 4.14, and the oracle's
slice sampler on the restated density lands on the quadrature's posterior means."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import family_cpu as F
import hier_ref as R
from family_cpu import P  # noqa: F401  (P: the module's fixture)

SCHOOLS_Y = (28.0, 8.0, -3.0, 7.0, -1.0, 1.0, 18.0, 12.0)
SCHOOLS_SIGMA = (15.0, 10.0, 16.0, 11.0, 9.0, 11.0, 10.0, 18.0)


def test_enum_and_export_mirrors(P):
    from pigeons_amd import _lib
    import __graft_entry__ as g
    assert _lib.TARGET_HIERARCHICAL_NORMAL == 9
    assert (_lib.HIER_CENTERED, _lib.HIER_NONCENTERED) == (0, 1)
    assert "pte_set_target_hier" in _lib.EXPORTS
    assert hasattr(_lib.load(), "pte_set_target_hier")
    hdr = F.HEADER
    assert "PTE_TARGET_HIERARCHICAL_NORMAL = 9" in hdr and "int pte_set_target_hier(pte_engine *h, int32_t parameterization, int64_t n_groups" in hdr
    assert "PTE_HIER_CENTERED = 0" in hdr and "PTE_HIER_NONCENTERED = 1" in hdr
    jl = F.JULIA
    assert "const TARGET_HIERARCHICAL_NORMAL = Int32(9)\n" in jl
    assert "struct DeviceHierarchicalNormalMeans" in jl and "device_family(t::DeviceHierarchicalNormalMeans, inputs)" in jl
    assert ":pte_set_target_hier" in jl
    assert "HierarchicalNormalMeans" in P.__dict__
    # the kernels live in an existing translation unit: no ninth one, no RNG-policy setter of their own
    assert len(g.UNITS) == 8
    params = open(os.path.join(g.CSRC, "pte_automala_params.hpp")).read()
    assert "EIGHT translation units" in params and "TGT_HIER = 9" in params and "X(hier)" not in params
    assert '#include "pte_hier.hpp"' in open(os.path.join(g.CSRC, "pte_glm.hip")).read()
    assert "PTE_DEFINE_RNG_POLICY_SETTER" not in open(os.path.join(g.CSRC, "pte_hier.hpp")).read()


@pytest.mark.parametrize("dim", [3, 10, 64, 65, 512])
@pytest.mark.parametrize("explorer,explorer2", [(2, 0), (3, 0), (5, 0), (2, 3)])
def test_accepted_config_reaches_the_device_check(P, explorer, explorer2, dim):
    """fails on the code before the family existed ("target 9 has no device log-potential"): a valid configuration now passes validation"""
    F.no_device()
    F.assert_reaches_the_device_check(P, n_chains=4, target=9, dim=dim, explorer=explorer, explorer2=explorer2, target_params=[1.0])


_HIER = dict(target=9, dim=10, explorer=2, n_chains=4)


@pytest.mark.parametrize("kw,msg", [
    (dict(dim=2), r"hierarchical-normal path holds \[mu, log tau\] and 1\.\.510 group coordinates, dim must be in 3\.\.512 \(got 2\)"),
    (dict(dim=513), r"hierarchical-normal path holds \[mu, log tau\] and 1\.\.510 group coordinates, dim must be in 3\.\.512 \(got 513\)"),
    (dict(explorer=0), "hierarchical-normal path is implemented for SliceSampler / AutoMALA / MALA"),       # none
    (dict(explorer=1), "hierarchical-normal path is implemented for SliceSampler / AutoMALA / MALA"),       # ToyExplorer
    (dict(explorer=4), "hierarchical-normal path is implemented for SliceSampler / AutoMALA / MALA"),       # IsingMetropolis
    (dict(explorer=2, explorer2=1), "hierarchical-normal path is implemented for SliceSampler / AutoMALA / MALA"),
    (dict(explorer=6), "AAPS is implemented on the scaled-precision MVN and funnel paths only"),            # AAPS keeps its refusal
    (dict(debug_kernel=1), "debug_kernel 1 is not available on the hierarchical-normal path"),
    (dict(debug_kernel=8), "debug_kernel 8 is not available on the hierarchical-normal path"),
    (dict(n_chains_variational=4), "two-leg tempering"),
])
def test_pte_create_refusals(P, kw, msg):
    F.assert_create_refused(P, _HIER, kw, msg)


def test_python_mapping(P):
    from pigeons_amd import _lib
    t = P.HierarchicalNormalMeans(SCHOOLS_Y, SCHOOLS_SIGMA, mu_sd=4.0, tau_scale=3.0, parameterization="noncentered")
    kw = F.captured(P, t)
    assert kw["target"] == _lib.TARGET_HIERARCHICAL_NORMAL and kw["dim"] == 10 and list(kw["target_params"]) == [0.5]
    assert kw["explorer"] == _lib.EXPLORER_SLICE                      # default explorer: SliceSampler (target.jl:20)
    (param, ys, ss, mu_sd, tau_scale), = kw["set_target_hier"]       # set after create, once per engine
    assert param == _lib.HIER_NONCENTERED and (mu_sd, tau_scale) == (4.0, 3.0)
    np.testing.assert_array_equal(ys, SCHOOLS_Y); np.testing.assert_array_equal(ss, SCHOOLS_SIGMA)
    t = P.HierarchicalNormalMeans(SCHOOLS_Y, SCHOOLS_SIGMA)
    kw = F.captured(P, t, explorer=P.AutoMALA())
    call = kw["set_target_hier"][0]
    assert kw["explorer"] == _lib.EXPLORER_AUTOMALA and call[0] == _lib.HIER_CENTERED and call[3:] == (5.0, 5.0)
    kw = F.captured(P, t, explorer=P.Compose(P.SliceSampler(), P.MALA()))
    assert kw["explorer"] == _lib.EXPLORER_SLICE and kw["explorer2"] == _lib.EXPLORER_MALA
    F.assert_reference_refusals(P, t, wrong_dim=8)
    with pytest.raises((ValueError, AttributeError, TypeError)):
        P.analytic_lognormalization(t, P.ScaledPrecisionNormalLogPotential(1.0, 10))          # not defined for this family


def test_every_shard_gets_the_data(P):
    F.assert_every_shard_gets_the_data(P, P.HierarchicalNormalMeans(SCHOOLS_Y, SCHOOLS_SIGMA), P.ScaledPrecisionNormalLogPotential(1.0, 10),
                                       N=4, d=10, setter="set_target_hier")


@pytest.mark.parametrize("args,kw,msg", [
    (([1.0, 2.0], [1.0, 1.0]), dict(parameterization="whitened"), "parameterization must be"),
    (([], []), {}, r"1\.\.510 group estimates"),
    ((np.zeros(511), np.ones(511)), {}, r"1\.\.510 group estimates"),
    ((np.zeros((2, 2)), np.ones((2, 2))), {}, r"1\.\.510 group estimates"),
    (([1.0, 2.0], [1.0]), {}, "one standard error per group, 2 of them"),
    (([1.0, np.nan], [1.0, 1.0]), {}, r"y\[1\] must be finite"),
    (([np.inf, 0.0], [1.0, 1.0]), {}, r"y\[0\] must be finite"),
    (([1.0, 2.0], [1.0, 0.0]), {}, r"sigma\[1\] must be positive and finite"),
    (([1.0, 2.0], [-1.0, 1.0]), {}, r"sigma\[0\] must be positive and finite"),
    (([1.0, 2.0], [1.0, np.inf]), {}, r"sigma\[1\] must be positive and finite"),
    (([1.0, 2.0], [1.0, np.nan]), {}, r"sigma\[1\] must be positive and finite"),
    (([1.0, 2.0], [1.0, 1.0]), dict(mu_sd=0.0), "mu_sd must be positive and finite"),
    (([1.0, 2.0], [1.0, 1.0]), dict(mu_sd=np.inf), "mu_sd must be positive and finite"),
    (([1.0, 2.0], [1.0, 1.0]), dict(tau_scale=-2.0), "tau_scale must be positive and finite"),
    (([1.0, 2.0], [1.0, 1.0]), dict(tau_scale=np.nan), "tau_scale must be positive and finite"),
])
def test_python_validation(P, args, kw, msg):
    with pytest.raises(ValueError, match=msg):
        P.HierarchicalNormalMeans(*args, **kw)


def test_hierarchical_normal_means_surface(P):
    t = P.HierarchicalNormalMeans(SCHOOLS_Y, SCHOOLS_SIGMA)
    assert t.n_groups == 8 and t.dim == 10 and t.parameterization == "centered" and t.y.dtype == np.float64
    assert (t.mu_sd, t.tau_scale) == (5.0, 5.0)
    assert repr(t) == "HierarchicalNormalMeans(centered, J=8, dim=10)"
    assert P.HierarchicalNormalMeans(np.zeros(510), np.ones(510), parameterization="noncentered").dim == 512     # the limits are accepted
    assert P.HierarchicalNormalMeans([0.5], [2.0]).dim == 3
    assert math.isclose(t.evidence_offset(0.25), -5.0 * math.log(2.0 * math.pi / 0.25), rel_tol=1e-15)
    assert math.isclose(t.evidence_offset(0.25), R.Hier(SCHOOLS_Y, SCHOOLS_SIGMA).evidence_offset(0.25), rel_tol=1e-15)
    from pigeons_amd.pt import default_explorer
    assert isinstance(default_explorer(t), P.SliceSampler)


def test_set_target_hier_is_bound(P):
    from pigeons_amd import _lib
    F.assert_null_engine_refused(_lib.load().pte_set_target_hier, (None, 0, 2, None, None, 5.0, 5.0),
                                 {1: C.c_int32, 2: C.c_int64, 5: C.c_double, 6: C.c_double})


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------
def _groups(J, seed):
    g = np.random.default_rng(seed)
    return g.normal(0.0, 3.0, J), g.uniform(0.5, 3.0, J)


@pytest.mark.parametrize("param", ["centered", "noncentered"])
def test_gradient_against_central_differences(param):
    """20 random states (J = 1, 5, 70: one block and a ragged second one), the target alone and on the path"""
    g = np.random.default_rng(7)
    n = 0
    for J in (1, 5, 70):
        y, s = _groups(J, J)
        hier = R.Hier(y, s, 2.0, 1.5, param)
        for k in range(8 if J == 5 else 6):
            x = g.normal(0.0, 0.7, J + 2)
            ch = R.HierChain(hier, (1.0, 0.3)[k % 2], 0.6)
            _, grad = ch.lp_grad(x)
            h = 1e-6
            num = np.array([(ch.lp_grad(x + h * e)[0] - ch.lp_grad(x - h * e)[0]) / (2 * h) for e in np.eye(J + 2)])
            np.testing.assert_allclose(grad, num, rtol=2e-6, atol=2e-6)
            assert math.isclose(ch.path_lp(x), ch.lp_grad(x)[0], rel_tol=1e-14, abs_tol=1e-14)
            n += 1
    assert n == 20


def test_the_parameterisations_are_one_density_under_the_change_of_variables():
    """lp_nc(mu, lt, eta) = lp_c(mu, lt, mu + tau eta) + J lt: the Jacobian tau^J of theta = mu + tau eta"""
    g = np.random.default_rng(3)
    for J in (1, 8, 40):
        y, s = _groups(J, 10 + J)
        c, nc = R.Hier(y, s, 5.0, 5.0, "centered"), R.Hier(y, s, 5.0, 5.0, "noncentered")
        for _ in range(5):
            x = g.normal(0.0, 1.0, J + 2)
            xc = x.copy()
            xc[2:] = nc.theta(x)
            want = c.lp(xc) + J * x[1]
            assert math.isclose(nc.lp(x), want, rel_tol=1e-12, abs_tol=1e-12), (J, nc.lp(x), want)


def test_restatement_against_the_textbook_density():
    y, s = _groups(6, 2)
    hier = R.Hier(y, s, 2.5, 0.7, "centered")
    x = np.random.default_rng(4).normal(0.0, 1.0, 8)
    mu, lt, th = x[0], x[1], x[2:]
    tau = math.exp(lt)
    norm = lambda v, m, sd: -0.5 * math.log(2 * math.pi * sd * sd) - (v - m) ** 2 / (2 * sd * sd)
    want = (norm(mu, 0.0, 2.5) + math.log(2.0 / (math.pi * 0.7 * (1.0 + (tau / 0.7) ** 2))) + lt
            + sum(norm(th[j], mu, tau) + norm(y[j], th[j], s[j]) for j in range(6)))
    assert math.isclose(hier.lp(x), want, rel_tol=1e-12)


def test_eight_schools_quadrature():
    """the numbers of DESIGN 4.14"""
    hier = R.Hier(SCHOOLS_Y, SCHOOLS_SIGMA, 5.0, 5.0)
    assert abs(hier.log_evidence() - (-31.3113474)) < 1e-6
    m = hier.posterior_means()
    assert abs(m[0] - 4.39682) < 1e-6 and abs(m[1] - 0.802139) < 1e-6
    np.testing.assert_allclose(m[2:], (6.2119, 4.9402, 3.9270, 4.7571, 3.6155, 4.0426, 6.2967, 4.8543), rtol=0, atol=5e-5)
    # ... and to 1e-6 against the rule at twice the resolution (the figures above are printed to fewer digits)
    np.testing.assert_allclose(m, hier.posterior_means(80001), rtol=0, atol=1e-6)
    np.testing.assert_allclose(hier.posterior_sds(), hier.posterior_sds(80001), rtol=0, atol=1e-6)
    assert abs(hier.log_evidence() - hier.log_evidence(80001)) < 1e-6


def test_quadrature_against_a_two_dimensional_grid():
    """J = 2: the 1-D rule over lt (mu integrated analytically) against a 2-D (mu, lt) trapezoid of prod_j N(y_j; mu, sigma_j^2 + tau^2) x priors"""
    y, s = np.array([1.3, -0.4]), np.array([0.9, 1.7])
    hier = R.Hier(y, s, 2.0, 1.5)
    mu = np.linspace(-30.0, 30.0, 6001)
    lt = np.linspace(-25.0, 12.0, 4001)
    M, L = np.meshgrid(mu, lt, indexing="ij")
    V = s[None, None, :] ** 2 + np.exp(2.0 * L)[..., None]
    logf = (-0.5 * np.log(2 * np.pi * V) - (y - M[..., None]) ** 2 / (2 * V)).sum(-1)
    logf += -0.5 * np.log(2 * np.pi * 4.0) - M ** 2 / 8.0
    logf += hier.c_tau - np.log1p(np.exp(2.0 * L) / 1.5 ** 2) + L
    mx = logf.max()
    wm = np.full(mu.size, mu[1] - mu[0]); wm[0] *= 0.5; wm[-1] *= 0.5
    wl = np.full(lt.size, lt[1] - lt[0]); wl[0] *= 0.5; wl[-1] *= 0.5
    Z = wm @ np.exp(logf - mx) @ wl
    assert math.isclose(hier.log_evidence(), mx + math.log(Z), rel_tol=0, abs_tol=1e-8)


@pytest.mark.parametrize("param", ["centered", "noncentered"])
def test_oracle_slice_sampler_on_the_restatement_lands_on_the_quadrature(param):
    """MixedSliceSampler (every coordinate Float64), seed 1, 2500 steps, the first 500 dropped, 20 batches: every posterior mean (mu, log tau,
    theta_j -- reconstructed per sample in the non-centred form) within 5 batch-means standard errors of the quadrature, every standard error
    below a quarter of the quadrature posterior sd"""
    import oracle as O
    O.build()
    hier = R.Hier(SCHOOLS_Y, SCHOOLS_SIGMA, 5.0, 5.0, param)
    s = O.MixedSliceSampler(hier.lp, np.zeros(10, dtype=np.int32))
    rng = O.OracleRng(seed=1)
    x = np.zeros(10)
    out = np.empty((2500, 10))
    for t in range(2500):
        s.step(rng, x)
        out[t] = x
    kept = out[500:]
    q = np.concatenate([kept[:, :2], hier.theta(kept)], axis=1)
    bm = q.reshape(20, 100, 10).mean(axis=1)
    se = bm.std(axis=0, ddof=1) / math.sqrt(20.0)
    want, sd = hier.posterior_means(), hier.posterior_sds()
    z = np.abs(q.mean(axis=0) - want) / se
    print("slice on the restatement (%s): max |z| %.2f, max se / sd %.3f" % (param, z.max(), (se / sd).max()))
    assert np.all(z < 5.0), (z, q.mean(axis=0), want)
    assert np.all(se < 0.25 * sd), se / sd
