"""The latent-AR(1) state-space family without a GPU: pte_create accepts it (a valid configuration reaches the device check) and refuses --
before any device work -- what the device does not run; the Python and Julia surfaces map LatentAR1 onto pte_config and pte_set_target_ar1;
the NumPy restatement (tests/ar1_ref.py) has the right gradient, its tree sum is its plain sum, its prior part is normalised, its quadrature
of the normal model agrees with itself at twice the resolution and with the numbers of DESIGN 4.15, and the oracle's slice sampler on the
restated density lands on the quadrature's posterior means."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import ar1_ref as R
import family_cpu as F
from family_cpu import P  # noqa: F401  (P: the module's fixture)

TRUTH_Y = (0.3, 0.9, 1.4, 0.8, 0.2, -0.5, -1.1, -0.6, 0.1, 0.7, 1.2, 0.9)
TRUTH_KW = dict(obs_sd=0.5, mu_sd=2.0, phi_loc=0.0, phi_scale=1.0, sigma_scale=1.0)


def test_enum_and_export_mirrors(P):
    from pigeons_amd import _lib
    import __graft_entry__ as g
    assert _lib.TARGET_LATENT_AR1 == 10
    assert (_lib.AR1_STOCHASTIC_VOLATILITY, _lib.AR1_NORMAL_IDENTITY) == (0, 1)
    assert "pte_set_target_ar1" in _lib.EXPORTS
    assert hasattr(_lib.load(), "pte_set_target_ar1")
    hdr = F.HEADER
    assert "PTE_TARGET_LATENT_AR1 = 10" in hdr and "int pte_set_target_ar1(pte_engine *h, int32_t likelihood, int64_t n_obs" in hdr
    assert "PTE_AR1_STOCHASTIC_VOLATILITY = 0" in hdr and "PTE_AR1_NORMAL_IDENTITY = 1" in hdr
    jl = F.JULIA
    assert "const TARGET_LATENT_AR1 = Int32(10)\n" in jl
    assert "struct DeviceLatentAR1" in jl and "device_family(t::DeviceLatentAR1, inputs)" in jl
    assert ":pte_set_target_ar1" in jl
    assert "LatentAR1" in P.__dict__
    # the kernels live in an existing translation unit: no ninth one, no RNG-policy setter of their own
    assert len(g.UNITS) == 8
    params = open(os.path.join(g.CSRC, "pte_automala_params.hpp")).read()
    assert "TGT_AR1 = 10" in params and "X(ar1)" not in params
    assert '#include "pte_ar1.hpp"' in open(os.path.join(g.CSRC, "pte_glm.hip")).read()
    assert "PTE_DEFINE_RNG_POLICY_SETTER" not in open(os.path.join(g.CSRC, "pte_ar1.hpp")).read()


@pytest.mark.parametrize("dim", [4, 64, 65, 512])
@pytest.mark.parametrize("explorer,explorer2", [(2, 0), (3, 0), (5, 0), (2, 3)])
def test_accepted_config_reaches_the_device_check(P, explorer, explorer2, dim):
    """fails on the code before the family existed ("target 10 has no device log-potential"): a valid configuration now passes validation"""
    F.no_device()
    F.assert_reaches_the_device_check(P, n_chains=4, target=10, dim=dim, explorer=explorer, explorer2=explorer2, target_params=[1.0])


_AR1 = dict(target=10, dim=15, explorer=2, n_chains=4)


@pytest.mark.parametrize("kw,msg", [
    (dict(explorer=0), r"latent-AR\(1\) path is implemented for SliceSampler / AutoMALA / MALA"),       # none
    (dict(explorer=1), r"latent-AR\(1\) path is implemented for SliceSampler / AutoMALA / MALA"),       # ToyExplorer
    (dict(explorer=4), r"latent-AR\(1\) path is implemented for SliceSampler / AutoMALA / MALA"),       # IsingMetropolis
    (dict(explorer=2, explorer2=1), r"latent-AR\(1\) path is implemented for SliceSampler / AutoMALA / MALA"),
    (dict(explorer=6), r"AAPS is implemented on the scaled-precision MVN and funnel paths only \(got target 10\)"),
    (dict(explorer=2, explorer2=6), "AAPS is not available as half of a Compose on the device"),
    (dict(dim=3), r"latent-AR\(1\) path holds \[mu, a, ls\] and 1\.\.509 latent states, dim must be in 4\.\.512 \(got 3\)"),
    (dict(dim=513), r"latent-AR\(1\) path holds \[mu, a, ls\] and 1\.\.509 latent states, dim must be in 4\.\.512 \(got 513\)"),
    (dict(debug_kernel=1), r"debug_kernel 1 is not available on the latent-AR\(1\) path"),
    (dict(debug_kernel=8), r"debug_kernel 8 is not available on the latent-AR\(1\) path"),
    (dict(n_chains_variational=4), r"two-leg tempering \(n_chains_variational > 0\) is not available on the latent-AR\(1\) path"),
    # a doubly-wrong configuration gets the earlier message
    (dict(explorer=1, dim=3), r"latent-AR\(1\) path is implemented for SliceSampler / AutoMALA / MALA"),
    (dict(dim=3, debug_kernel=1), r"dim must be in 4\.\.512 \(got 3\)"),
    (dict(debug_kernel=1, n_chains_variational=4), r"debug_kernel 1 is not available on the latent-AR\(1\) path"),
])
def test_pte_create_refusals(P, kw, msg):
    F.assert_create_refused(P, _AR1, kw, msg)


def test_python_mapping(P):
    from pigeons_amd import _lib
    t = P.LatentAR1(TRUTH_Y, likelihood="normal_identity", obs_sd=0.5, mu_sd=2.0, phi_loc=0.25, phi_scale=0.75, sigma_scale=1.5)
    kw = F.captured(P, t)
    assert kw["target"] == _lib.TARGET_LATENT_AR1 and kw["dim"] == 15 and list(kw["target_params"]) == [0.5]
    assert kw["explorer"] == _lib.EXPLORER_SLICE                      # default explorer: SliceSampler (target.jl:20)
    (lik, ys, *rest), = kw["set_target_ar1"]                         # set after create, once per engine
    assert lik == _lib.AR1_NORMAL_IDENTITY and tuple(rest) == (0.5, 2.0, 0.25, 0.75, 1.5)
    np.testing.assert_array_equal(ys, TRUTH_Y)
    t = P.LatentAR1(TRUTH_Y)
    kw = F.captured(P, t, explorer=P.AutoMALA())
    assert kw["explorer"] == _lib.EXPLORER_AUTOMALA and kw["set_target_ar1"][0][0] == _lib.AR1_STOCHASTIC_VOLATILITY
    assert tuple(kw["set_target_ar1"][0][2:]) == (1.0, 5.0, 0.0, 1.0, 1.0)
    kw = F.captured(P, t, explorer=P.Compose(P.SliceSampler(), P.MALA()))
    assert kw["explorer"] == _lib.EXPLORER_SLICE and kw["explorer2"] == _lib.EXPLORER_MALA
    F.assert_reference_refusals(P, t, wrong_dim=12)


def test_every_shard_gets_the_data(P):
    F.assert_every_shard_gets_the_data(P, P.LatentAR1(TRUTH_Y), P.ScaledPrecisionNormalLogPotential(1.0, 15), N=4, d=15, setter="set_target_ar1")


@pytest.mark.parametrize("args,kw,msg", [
    (([1.0, 2.0],), dict(likelihood="poisson"), "likelihood must be"),
    (([],), {}, r"1\.\.509 observations"),
    ((np.zeros(510),), {}, r"1\.\.509 observations"),
    ((np.zeros((2, 2)),), {}, r"1\.\.509 observations"),
    (([1.0, np.nan],), {}, r"y\[1\] must be finite"),
    (([np.inf, 0.0],), {}, r"y\[0\] must be finite"),
    (([1.0, 2.0],), dict(obs_sd=0.0), "obs_sd must be positive and finite"),
    (([1.0, 2.0],), dict(obs_sd=np.nan), "obs_sd must be positive and finite"),
    (([1.0, 2.0],), dict(mu_sd=0.0), "mu_sd must be positive and finite"),
    (([1.0, 2.0],), dict(mu_sd=np.inf), "mu_sd must be positive and finite"),
    (([1.0, 2.0],), dict(phi_scale=-2.0), "phi_scale must be positive and finite"),
    (([1.0, 2.0],), dict(sigma_scale=np.nan), "sigma_scale must be positive and finite"),
    (([1.0, 2.0],), dict(phi_loc=np.inf), "phi_loc must be finite"),
])
def test_python_validation(P, args, kw, msg):
    with pytest.raises(ValueError, match=msg):
        P.LatentAR1(*args, **kw)


def test_latent_ar1_surface(P):
    t = P.LatentAR1(TRUTH_Y)
    assert t.n_obs == 12 and t.dim == 15 and t.likelihood == "stochastic_volatility" and t.y.dtype == np.float64
    assert (t.obs_sd, t.mu_sd, t.phi_loc, t.phi_scale, t.sigma_scale) == (1.0, 5.0, 0.0, 1.0, 1.0)
    assert repr(t) == "LatentAR1(stochastic_volatility, T=12, dim=15)"
    assert P.LatentAR1(np.zeros(509), likelihood="normal_identity").dim == 512     # the limits are accepted
    assert P.LatentAR1([0.5]).dim == 4
    assert math.isclose(t.evidence_offset(0.25), -7.5 * math.log(2.0 * math.pi / 0.25), rel_tol=1e-15)
    assert math.isclose(t.evidence_offset(0.25), R.Ar1(TRUTH_Y).evidence_offset(0.25), rel_tol=1e-15)
    from pigeons_amd.pt import default_explorer
    assert isinstance(default_explorer(t), P.SliceSampler)


def test_set_target_ar1_is_bound(P):
    from pigeons_amd import _lib
    F.assert_null_engine_refused(_lib.load().pte_set_target_ar1, (None, 0, 2, None, 1.0, 5.0, 0.0, 1.0, 1.0),
                                 {1: C.c_int32, 2: C.c_int64, **{i: C.c_double for i in range(4, 9)}}, n_args=9)


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------
LIKS = ["stochastic_volatility", "normal_identity"]


def _trapz(f, x):
    return float(np.sum((f[1:] + f[:-1]) * np.diff(x)) / 2.0)


def _model(T, lik, seed):
    g = np.random.default_rng(seed)
    return R.Ar1(g.normal(0.0, 1.0, T), lik, obs_sd=0.7, mu_sd=2.0, phi_loc=0.3, phi_scale=0.8, sigma_scale=1.5)


@pytest.mark.parametrize("lik", LIKS)
def test_gradient_against_central_differences(lik):
    """T = 1 (no transition), 2 and 5, six random states each, the target alone and on the path"""
    g = np.random.default_rng(7)
    n = 0
    for T in (1, 2, 5):
        ar1 = _model(T, lik, T)
        for k in range(6):
            x = g.normal(0.0, 0.7, T + 3)
            ch = R.Ar1Chain(ar1, (1.0, 0.3)[k % 2], 0.6)
            _, grad = ch.lp_grad(x)
            h = 1e-6
            num = np.array([(ch.lp_grad(x + h * e)[0] - ch.lp_grad(x - h * e)[0]) / (2 * h) for e in np.eye(T + 3)])
            np.testing.assert_allclose(grad, num, rtol=2e-6, atol=2e-6)
            assert math.isclose(ch.path_lp(x), ch.lp_grad(x)[0], rel_tol=1e-14, abs_tol=1e-14)
            n += 1
    assert n == 18


@pytest.mark.parametrize("lik", LIKS)
def test_tree_sum_against_the_plain_sum_and_the_textbook_density(lik):
    g = np.random.default_rng(11)
    norm = lambda v, m, sd: -0.5 * math.log(2 * math.pi * sd * sd) - (v - m) ** 2 / (2 * sd * sd)
    for T in (1, 5, 70, 200):
        ar1 = _model(T, lik, 20 + T)
        x = g.normal(0.0, 0.8, T + 3)
        assert math.isclose(ar1.lp(x), ar1.lp_plain(x), rel_tol=1e-13, abs_tol=1e-12)
        mu, a, ls, h = x[0], x[1], x[2], x[3:]
        phi, sg = math.tanh(a), math.exp(ls)
        want = norm(mu, 0.0, 2.0) + norm(a, 0.3, 0.8) + math.log(2.0 / (math.pi * 1.5 * (1.0 + (sg / 1.5) ** 2))) + ls
        want += norm(h[0], mu, sg / math.sqrt(1.0 - phi * phi))
        want += sum(norm(h[t], mu + phi * (h[t - 1] - mu), sg) for t in range(1, T))
        if lik == "normal_identity":
            want += sum(norm(ar1.y[t], h[t], 0.7) for t in range(T))
        else:
            want += sum(norm(ar1.y[t], 0.0, math.exp(h[t] / 2.0)) for t in range(T))
        assert math.isclose(ar1.lp(x), want, rel_tol=1e-12), (T, ar1.lp(x), want)


def test_the_first_state_does_not_couple_to_log_sigma_as_a_neighbour():
    """h_0's leaf is the stationary law: d/dh_0 of the T = 1 density has no phi (h_{-1} - mu) term -- with a wrongly coupled predecessor
    (coordinate 2 = ls taken for h_{-1}) the T = 1 density would change with ls through u, beyond isg and the prior"""
    ar1 = R.Ar1([0.4], "normal_identity", obs_sd=0.7)
    x = np.array([0.2, 0.9, -0.3, 0.8])
    phi, sg = math.tanh(0.9), math.exp(-0.3)
    u0 = (0.8 - 0.2) / sg * math.sqrt(1.0 - phi * phi)
    t = ar1.leaves(x, grad=False)[0]
    z = (0.4 - 0.8) / 0.7
    want = -(u0 * u0 + R.LOG2PI) / 2.0 + 0.3 + math.log(1.0 - phi * phi) / 2.0 - (z * z + R.LOG2PI) / 2.0 - math.log(0.7)
    assert math.isclose(t[3], want, rel_tol=1e-13)


def test_prior_part_is_normalised_at_one_observation():
    """T = 1 without its observation term: the density of (mu, a, ls, h_0) integrates to 1.  h_0 and mu integrate out in closed form under the
    grid (N(h_0; mu, .) and N(mu; 0, .) are normalised leaves); the grid is over (a, ls), and h_0 on top of it for a check of the leaf itself."""
    ar1 = R.Ar1([0.0], "normal_identity", obs_sd=1.0, mu_sd=2.0, phi_loc=0.3, phi_scale=0.8, sigma_scale=1.5)
    av, lv = np.linspace(-7.0, 7.6, 293), np.linspace(-40.0, 40.0, 4001)
    hv = np.linspace(-60.0, 60.0, 6001)
    # (a) the leaves of a and ls over their grids
    la = np.array([ar1.leaves(np.array([0.0, a, 0.0, 0.0]), grad=False)[0][1] for a in av])
    ll = np.array([ar1.leaves(np.array([0.0, 0.0, l, 0.0]), grad=False)[0][2] for l in lv])
    assert math.isclose(_trapz(np.exp(la), av), 1.0, abs_tol=1e-9)
    assert math.isclose(_trapz(np.exp(ll), lv), 1.0, abs_tol=1e-6)
    # (b) the transition leaf of h_0 (observation term taken off) over h_0, at several (mu, a, ls)
    for mu, a, ls in ((0.0, 0.0, 0.0), (0.7, 1.2, -0.5), (-1.0, -2.0, 0.8)):
        lh = np.empty(hv.size)
        for i, h in enumerate(hv):
            t = ar1.leaves(np.array([mu, a, ls, h]), grad=False)[0]
            lh[i] = t[3] - (-(h * h + R.LOG2PI) / 2.0)                 # (y = 0, obs_sd = 1: the observation term)
        assert math.isclose(_trapz(np.exp(lh), hv), 1.0, abs_tol=1e-9), (mu, a, ls)
    m = np.linspace(-30.0, 30.0, 3001)
    lm = np.array([ar1.leaves(np.array([v, 0.0, 0.0, 0.0]), grad=False)[0][0] for v in m])
    assert math.isclose(_trapz(np.exp(lm), m), 1.0, abs_tol=1e-9)


# ---- the ground truth of the normal model --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def truth():
    ar1 = R.Ar1(TRUTH_Y, "normal_identity", **TRUTH_KW)
    return ar1, ar1._quadrature()


def test_quadrature_reproduces_the_truth_values(truth):
    """the numbers of DESIGN 4.15, and the rule against itself at twice the resolution"""
    ar1, (log_z, mean, sd) = truth
    assert abs(log_z - (-15.9167885)) < 1e-5
    np.testing.assert_allclose(mean[:3], (0.39954, 0.89064, -0.66230), rtol=0, atol=1e-5)
    np.testing.assert_allclose(mean[3:], (0.45596, 0.76489, 0.97827, 0.65512, 0.21261, -0.26494, -0.58207, -0.32672, 0.13567, 0.57274,
                                          0.87946, 0.79402), rtol=0, atol=1e-5)
    log_z2, mean2, sd2 = ar1._quadrature(641, 801)
    assert abs(log_z - log_z2) < 1e-6
    np.testing.assert_allclose(mean, mean2, rtol=0, atol=1e-6)
    np.testing.assert_allclose(sd, sd2, rtol=0, atol=1e-6)
    assert abs(sd[1] - 0.547) < 1e-3 and 0.36 <= sd[3:].min() and sd[3:].max() <= 0.43


def test_quadrature_marginal_against_the_restated_density():
    """T = 2: the (a, ls) integrand of the quadrature is the restated density with mu and h integrated out -- checked at a few (a, ls) by a
    3-D trapezoid over (mu, h_0, h_1) of exp(lp)"""
    y = np.array([0.6, -0.2])
    ar1 = R.Ar1(y, "normal_identity", obs_sd=0.8, mu_sd=1.0, phi_loc=0.1, phi_scale=0.9, sigma_scale=1.2)
    g = np.linspace(-9.0, 9.0, 121)
    w = np.full(g.size, g[1] - g[0]); w[0] *= 0.5; w[-1] *= 0.5
    for a, ls in ((0.3, -0.2), (-0.8, 0.1)):
        M, H0, H1 = np.meshgrid(g, g, g, indexing="ij")
        phi, sg = math.tanh(a), math.exp(ls)
        om = 1.0 - phi * phi
        u0 = (H0 - M) / sg * math.sqrt(om)
        u1 = ((H1 - M) - phi * (H0 - M)) / sg
        lp = (-(M / 1.0) ** 2 / 2.0 - R.LOG2PI / 2.0 - (u0 ** 2 + u1 ** 2) / 2.0 - R.LOG2PI - 2.0 * ls + math.log(om) / 2.0
              - ((y[0] - H0) / 0.8) ** 2 / 2.0 - ((y[1] - H1) / 0.8) ** 2 / 2.0 - R.LOG2PI - 2.0 * math.log(0.8))
        x = np.array([0.3, a, ls, 0.1, -0.4])
        pri = ar1.leaves(x, grad=False)[0][1] + ar1.leaves(x, grad=False)[0][2]
        # the restatement's own value at one point of the grid pins `lp` above to it
        u0x = (0.1 - 0.3) / sg * math.sqrt(om); u1x = ((-0.4 - 0.3) - phi * (0.1 - 0.3)) / sg
        lpx = (-(0.3) ** 2 / 2.0 - R.LOG2PI / 2.0 - (u0x ** 2 + u1x ** 2) / 2.0 - R.LOG2PI - 2.0 * ls + math.log(om) / 2.0
               - ((y[0] - 0.1) / 0.8) ** 2 / 2.0 - ((y[1] + 0.4) / 0.8) ** 2 / 2.0 - R.LOG2PI - 2.0 * math.log(0.8))
        assert math.isclose(ar1.lp(x), lpx + pri, rel_tol=1e-12)
        integral = np.einsum("ijk,i,j,k->", np.exp(lp), w, w, w)
        C = sg * sg / om * np.array([[1.0, phi], [phi, 1.0]])
        Sig = C + 0.64 * np.eye(2) + 1.0
        want = -0.5 * (np.linalg.slogdet(Sig)[1] + 2 * R.LOG2PI) - 0.5 * y @ np.linalg.solve(Sig, y)
        assert math.isclose(math.log(integral), want, abs_tol=1e-6), (a, ls)


def test_oracle_slice_sampler_on_the_restatement_lands_on_the_quadrature(truth):
    """MixedSliceSampler (every coordinate Float64, three passes a step), seed 1, 2000 steps = 6000 sweeps, the first 400 steps dropped, 20
    batches: every posterior mean within 5 batch-means standard errors of the quadrature, every standard error below a quarter of the
    quadrature's posterior sd"""
    import oracle as O
    O.build()
    ar1, (_, want, sd) = truth
    s = O.MixedSliceSampler(ar1.lp_plain, np.zeros(15, dtype=np.int32))
    rng = O.OracleRng(seed=1)
    x = np.zeros(15)
    out = np.empty((2000, 15))
    for t in range(2000):
        s.step(rng, x)
        out[t] = x
    kept = out[400:]
    bm = kept.reshape(20, 80, 15).mean(axis=1)
    se = bm.std(axis=0, ddof=1) / math.sqrt(20.0)
    z = np.abs(kept.mean(axis=0) - want) / se
    print("slice on the restatement: max |z| %.2f, max se / sd %.3f; sample sd / quadrature sd %s"
          % (z.max(), (se / sd).max(), np.round(kept.std(axis=0) / sd, 2)))
    assert np.all(z < 5.0), (z, kept.mean(axis=0), want)
    assert np.all(se < 0.25 * sd), se / sd
