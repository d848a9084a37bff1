"""The case table of the families' explore kernels at four and eight 64-coordinate blocks per lane, defined once and used by
tests/test_family_blocks_cpu.py (the table's own coverage, the restatements' MALA and AutoMALA alone) and tests/test_gpu_family_blocks.py
(the device against the restatements at one transition).

A Case is (family, variant, mode, d, N, explorer parameters): variant the kernel's LIK or PARAM argument, mode "slice", "mala" or "automala"
(which takes the MALA mode's data, states and standard deviations), d the
STATE dimension (hier: J + 2, ar1: T + 3, varsel: twice the number of columns), N the number of replicas.  The data, the schedule, the
states and the chain permutation of a case are made the way the family's own tests/test_gpu_<family>.py makes them for the same mode (its
_data / _mixture / _target, imported from there; the seeds derived from the dimension by the same expressions; the body of its
_random_states restated in layout()).  The RNG words are the engine's own, read back through eng.states(); init_rng_words restates them
(pte.hip, init_zero_state: an engine on the interpolated path starts at the zero state, replica i holding the i-th split of
SplittableRandom(seed), no draw made), so that the MALA restatement can run before any device does -- the GPU test asserts the two are
equal.

Dimensions: 129 / 130 (four blocks: block 2 holds one or two coordinates, block 3 none), 256 (four whole blocks), 257 (eight blocks: block
4 holds one coordinate, blocks 5 to 7 none; varsel's state is even: 258), 512 (eight whole blocks); varsel also 128 (two whole blocks).
Replicas: 6, but 3 (two off the reference chain) for the SliceSampler cases of dense and glm at 512, where a pass of the restatement
takes several seconds a replica, against well under a second elsewhere."""
import math

import numpy as np

import aaps_ref
import ar1_ref
import automala_ref
import dense_ref
import glm_ref
import hier_ref
import mixture_ref
import oracle as O
import varsel_ref
from test_gpu_ar1 import LIK as AR1_LIK, PRIORS as AR1_PRIORS, _data as ar1_data
from test_gpu_dense import _target as dense_target
from test_gpu_glm import _data as glm_data
from test_gpu_hier import PARAM as HIER_PARAM, _data as hier_data
from test_gpu_mixture import _mixture as mixture_data
from test_gpu_varsel import _data as varsel_data

SLICE = dict(w=10.0, p=20, n_passes=1)
PRECOND_MODE = {"identity": 0, "diagonal": 1, "mix": 2}
ENGINE_SEED = 1                                      # pigeons_amd.Inputs.seed's default: the tests of the families leave it alone
HIER_HYPER = dict(mu_sd=2.0, tau_scale=1.5)          # tests/test_gpu_hier.py, _pt


class Case:
    def __init__(self, family, variant, mode, d, N, **kw):
        self.family, self.variant, self.mode, self.d, self.N, self.kw = family, variant, mode, int(d), int(N), kw
        self.id = "-".join(str(v) for v in (family, variant, mode, "d%d" % d) if v is not None)

    def __repr__(self):
        return self.id


def _slice(family, variant, d, N=6, **kw):
    return Case(family, variant, "slice", d, N, **SLICE, **kw)


def _mala(family, variant, d, precond, step, seen, **kw):
    """seen: (proposals accepted, rejected) by the restatement alone on the CPU at this step, over the N - 1 replicas off the reference"""
    return Case(family, variant, "mala", d, 6, precond=precond, step=step, seen=seen, **kw)


# ---- SliceSampler, one pass ------------------------------------------------------------------------------------------------------------
# glm and varsel: n <= 20 observations (the restatement's cost grows with d, hardly with n)
SLICE_CASES = [
    _slice("glm", "bernoulli_logit", 130, n=20), _slice("glm", "normal_identity", 130, n=17),
    _slice("glm", "bernoulli_logit", 257, n=17), _slice("glm", "normal_identity", 257, n=20),
    _slice("glm", "bernoulli_logit", 512, N=3, n=20),
    _slice("hier", "c", 130), _slice("hier", "nc", 130), _slice("hier", "c", 257), _slice("hier", "nc", 257),
    _slice("hier", "c", 512), _slice("hier", "nc", 512),
    _slice("ar1", "sv", 130), _slice("ar1", "n", 130), _slice("ar1", "sv", 257), _slice("ar1", "n", 257),
    _slice("ar1", "sv", 512), _slice("ar1", "n", 512),
    _slice("mixture", None, 130, K=2), _slice("mixture", None, 257, K=8), _slice("mixture", None, 512, K=4),      # one bucket of K each
    _slice("dense", None, 130), _slice("dense", None, 256), _slice("dense", None, 257), _slice("dense", None, 512, N=3),
    _slice("varsel", "bernoulli_logit", 128, n=20, pi=0.5), _slice("varsel", "normal_identity", 128, n=17, pi=0.3),
    _slice("varsel", "bernoulli_logit", 130, n=17, pi=0.2), _slice("varsel", "normal_identity", 130, n=20, pi=0.5),
    _slice("varsel", "bernoulli_logit", 256, n=20, pi=0.3), _slice("varsel", "normal_identity", 256, n=17, pi=0.2),
    _slice("varsel", "bernoulli_logit", 258, n=17, pi=0.5), _slice("varsel", "normal_identity", 258, n=20, pi=0.3),
    _slice("varsel", "bernoulli_logit", 512, n=20, pi=0.2), _slice("varsel", "normal_identity", 512, n=17, pi=0.5),
]

# ---- MALA ------------------------------------------------------------------------------------------------------------------------------
# the steps were chosen on the restatements alone (tests/test_family_blocks_cpu.py repeats the count): each case accepts some proposals
# and rejects others
MALA_CASES = [
    _mala("glm", "bernoulli_logit", 129, "identity", 0.5, (62, 28), n=20), _mala("glm", "bernoulli_logit", 256, "diagonal", 0.3, (70, 35), n=17),
    _mala("glm", "bernoulli_logit", 257, "mix", 0.5, (33, 72), n=20), _mala("glm", "bernoulli_logit", 512, "diagonal", 0.3, (51, 84), n=17),
    _mala("glm", "normal_identity", 129, "diagonal", 0.3, (74, 16), n=17), _mala("glm", "normal_identity", 256, "mix", 0.5, (21, 84), n=20),
    _mala("glm", "normal_identity", 257, "identity", 0.5, (58, 47), n=17), _mala("glm", "normal_identity", 512, "mix", 0.3, (70, 65), n=20),
    _mala("hier", "c", 129, "mix", 0.1, (39, 51)), _mala("hier", "c", 256, "identity", 0.05, (79, 26)),
    _mala("hier", "c", 257, "diagonal", 0.05, (27, 78)), _mala("hier", "c", 512, "mix", 0.05, (88, 47)),
    _mala("hier", "nc", 129, "identity", 0.15, (76, 14)), _mala("hier", "nc", 256, "diagonal", 0.1, (23, 82)),
    _mala("hier", "nc", 257, "mix", 0.1, (61, 44)), _mala("hier", "nc", 512, "identity", 0.1, (79, 56)),
    _mala("ar1", "sv", 129, "diagonal", 0.1, (23, 67)), _mala("ar1", "sv", 256, "mix", 0.05, (46, 59)),
    _mala("ar1", "sv", 257, "identity", 0.1, (25, 80)), _mala("ar1", "sv", 512, "diagonal", 0.1, (55, 80)),
    _mala("ar1", "n", 129, "mix", 0.1, (38, 52)), _mala("ar1", "n", 256, "identity", 0.1, (16, 89)),
    _mala("ar1", "n", 257, "diagonal", 0.05, (55, 50)), _mala("ar1", "n", 512, "identity", 0.1, (52, 83)),
    _mala("mixture", None, 129, "identity", 0.6, (69, 21), K=2), _mala("mixture", None, 256, "diagonal", 0.3, (81, 24), K=4),
    _mala("mixture", None, 257, "mix", 0.4, (76, 29), K=8), _mala("mixture", None, 512, "diagonal", 0.3, (104, 31), K=3),
    _mala("dense", None, 129, "diagonal", 0.4, (55, 35)), _mala("dense", None, 256, "mix", 0.4, (35, 70)),
    _mala("dense", None, 257, "identity", 0.4, (41, 64)), _mala("dense", None, 512, "mix", 0.4, (32, 103)),
]

# ---- AutoMALA --------------------------------------------------------------------------------------------------------------------------
# The eight (family, variant) pairs of MALA_CASES at d = 129, 256, 257, 512 with the MALA case's data, states, n, K and standard deviations,
# base_n_refresh = 1 (6 refreshes at 129, 7 at 256 and 257, 9 at 512), each in one regime:
#   tuned   the MALA case's step, scan 2        grow    step 2^-12, scan 2: every search grows
#   shrink  step 2^8, scan 2: every search shrinks (hier-c and both ar1: through non-finite trials)
#   scan1   the tuned step, scan 1: no reversed search, no MH step -- the chain stays where the proposal ended
# Every pair meets every regime, every regime every dimension and every preconditioner.  Regime and preconditioner of a cell were chosen on
# the restatement alone, from the engine's own RNG words, among those in which it meets the conditions of tests/test_family_blocks_cpu.py
# (at 256 and 257 the hierarchical and AR(1) cases pass or accept nothing under several of the twelve choices): pair k at the j-th
# dimension takes regime (k + j) mod 4 and the MALA case's preconditioner where that does.
# seen: what the restatement makes of the case over the 5 replicas off the reference chain -- (proposals accepted, rejected, reversibility
# checks passed, failed, least and largest exponent of any search, non-finite trials, replicas moved); margin: the least distance of any
# of its decisions from going the other way (tests/automala_ref.py).  tests/test_family_blocks_cpu.py recomputes both.
AUTOMALA_REGIMES = ("tuned", "grow", "shrink", "scan1")
AUTOMALA_DIMS = (129, 256, 257, 512)
AUTOMALA_BASE_N_REFRESH = 1


def _automala(family, variant, d, regime, precond, seen, margin):
    (m,) = [c for c in MALA_CASES if (c.family, c.variant, c.d) == (family, variant, d)]
    step = {"grow": 2.0 ** -12, "shrink": 2.0 ** 8}.get(regime, m.kw["step"])
    kw = {k: v for k, v in m.kw.items() if k not in ("step", "seen", "precond")}
    return Case(family, variant, "automala", d, 6, regime=regime, precond=precond, step=step, scan=1 if regime == "scan1" else 2, seen=seen,
                margin=margin, **kw)


AUTOMALA_CASES = [
    _automala("glm", "bernoulli_logit", 129, "tuned", "identity", (14, 16, 23, 7, -1, 1, 0, 4), 8.11e-04),
    _automala("glm", "bernoulli_logit", 256, "grow", "diagonal", (9, 26, 15, 20, 9, 11, 0, 4), 3.75e-03),
    _automala("glm", "bernoulli_logit", 257, "shrink", "diagonal", (8, 27, 9, 26, -11, -9, 0, 4), 5.18e-03),
    _automala("glm", "bernoulli_logit", 512, "scan1", "mix", (0, 0, 0, 0, -1, 0, 0, 5), 6.92e-03),
    _automala("glm", "normal_identity", 129, "grow", "diagonal", (15, 15, 16, 14, 9, 11, 0, 5), 5.41e-03),
    _automala("glm", "normal_identity", 256, "shrink", "mix", (8, 27, 17, 18, -11, -8, 0, 5), 2.11e-03),
    _automala("glm", "normal_identity", 257, "scan1", "identity", (0, 0, 0, 0, -1, 0, 0, 5), 4.32e-03),
    _automala("glm", "normal_identity", 512, "tuned", "mix", (12, 33, 21, 24, -1, 1, 0, 4), 6.08e-03),
    _automala("hier", "c", 129, "shrink", "mix", (9, 21, 13, 17, -14, -10, 366, 3), 4.70e-03),
    _automala("hier", "c", 256, "scan1", "diagonal", (0, 0, 0, 0, -2, 0, 0, 5), 4.13e-02),
    _automala("hier", "c", 257, "tuned", "identity", (3, 32, 3, 32, -3, 1, 0, 1), 1.67e-02),
    _automala("hier", "c", 512, "grow", "mix", (4, 41, 4, 41, 4, 10, 0, 2), 4.82e-04),
    _automala("hier", "nc", 129, "tuned", "identity", (5, 25, 6, 24, -2, 2, 0, 2), 8.43e-04),
    _automala("hier", "nc", 256, "scan1", "diagonal", (0, 0, 0, 0, -1, 0, 0, 5), 8.06e-02),
    _automala("hier", "nc", 257, "grow", "mix", (3, 32, 3, 32, 3, 9, 0, 1), 5.07e-04),
    _automala("hier", "nc", 512, "shrink", "identity", (12, 33, 12, 33, -15, -9, 8, 2), 6.65e-02),
    _automala("ar1", "sv", 129, "tuned", "diagonal", (5, 25, 6, 24, -3, 1, 0, 2), 1.83e-02),
    _automala("ar1", "sv", 256, "shrink", "mix", (2, 33, 2, 33, -16, -11, 577, 2), 3.87e-02),
    _automala("ar1", "sv", 257, "scan1", "identity", (0, 0, 0, 0, -1, 0, 0, 5), 4.72e-02),
    _automala("ar1", "sv", 512, "grow", "diagonal", (7, 38, 7, 38, 4, 10, 0, 2), 4.74e-04),
    _automala("ar1", "n", 129, "grow", "mix", (3, 27, 3, 27, 5, 10, 0, 2), 2.57e-03),
    _automala("ar1", "n", 256, "shrink", "mix", (2, 33, 2, 33, -16, -11, 577, 2), 4.14e-02),
    _automala("ar1", "n", 257, "scan1", "diagonal", (0, 0, 0, 0, -1, 1, 0, 5), 1.34e-03),
    _automala("ar1", "n", 512, "tuned", "identity", (7, 38, 7, 38, -4, 2, 0, 2), 3.70e-04),
    _automala("mixture", None, 129, "shrink", "identity", (7, 23, 8, 22, -9, -8, 0, 3), 4.03e-02),
    _automala("mixture", None, 256, "scan1", "diagonal", (0, 0, 0, 0, -1, 1, 0, 5), 2.68e-02),
    _automala("mixture", None, 257, "tuned", "mix", (1, 34, 1, 34, -2, 1, 0, 1), 3.13e-02),
    _automala("mixture", None, 512, "grow", "diagonal", (16, 29, 17, 28, 6, 11, 0, 4), 8.13e-04),
    _automala("dense", None, 129, "scan1", "diagonal", (0, 0, 0, 0, -1, 0, 0, 5), 6.22e-03),
    _automala("dense", None, 256, "tuned", "mix", (8, 27, 12, 23, -3, 0, 0, 3), 4.08e-03),
    _automala("dense", None, 257, "grow", "identity", (1, 34, 1, 34, 8, 11, 0, 1), 3.20e-03),
    _automala("dense", None, 512, "shrink", "mix", (20, 25, 21, 24, -12, -9, 0, 5), 1.83e-02),
]

CASES = SLICE_CASES + MALA_CASES
assert len(set(c.id for c in CASES + AUTOMALA_CASES)) == len(CASES) + len(AUTOMALA_CASES)

# ---- the refresh kernels that no family's test_log_density_at_every_beta visits: (family, variant, state dimension, parameters) ---------
LOG_DENSITY_CASES = [
    Case("glm", "bernoulli_logit", "lp", 100, 8, n=40),              # k_refresh_glm_stats<2>
    Case("glm", "normal_identity", "lp", 200, 8, n=30),              # <4>
    Case("mixture", None, "lp", 200, 8, K=3),                        # k_refresh_mixture_stats<4>
    Case("varsel", "normal_identity", "lp", 200, 8, n=40, pi=0.3),   # k_refresh_varsel_stats<4>
    Case("varsel", "bernoulli_logit", "lp", 400, 8, n=30, pi=0.5),   # <8>, ragged
]


# ---- a case's model --------------------------------------------------------------------------------------------------------------------
class Model:
    """restatement: the family's target of tests/<family>_ref.py; chain(beta): one chain of it; device(P): the pigeons_amd target and the
    dimension of its reference; ref_prec; kinds: oracle.COORD_* per coordinate"""

    def __init__(self, restatement, chain_type, ref_prec, device, kinds):
        self.restatement, self.chain_type, self.ref_prec, self.device, self.kinds = restatement, chain_type, ref_prec, device, kinds

    def chain(self, beta):
        return self.chain_type(self.restatement, float(beta), self.ref_prec)


_MODELS = {}


def model(case):
    """(built once per case) -- data seeds and the reference's precision as the family's own test of this mode: SliceSampler and the log
    density at precision 0.5 (mixture's log density: 0.25), MALA at 1"""
    if case.id in _MODELS:
        return _MODELS[case.id]
    f, v, d, mala, lp = case.family, case.variant, case.d, case.mode in ("mala", "automala"), case.mode == "lp"
    prec = 1.0 if mala else 0.5
    kinds = np.zeros(d, dtype=np.int32)
    if f == "glm":
        n = case.kw["n"]
        sd = 0.8 if lp else 1.0
        X, y = glm_data(n, d, v, seed=(n + d) if lp else (3 * n + d) if mala else 7 * n + d, noise_sd=sd)
        m = Model(glm_ref.Glm(X, y, v, sd, prec), glm_ref.GlmChain, prec, lambda P: (P.BayesianGLM(X, y, likelihood=v, noise_sd=sd), d), kinds)
    elif f == "hier":
        J = d - 2
        y, s = hier_data(J, seed=3 * J if mala else 7 * J)
        m = Model(hier_ref.Hier(y, s, HIER_HYPER["mu_sd"], HIER_HYPER["tau_scale"], HIER_PARAM[v]), hier_ref.HierChain, prec,
                  lambda P: (P.HierarchicalNormalMeans(y, s, parameterization=HIER_PARAM[v], **HIER_HYPER), d), kinds)
    elif f == "ar1":
        y = ar1_data(d - 3, v, seed=3 * d if mala else 7 * d)
        m = Model(ar1_ref.Ar1(y, AR1_LIK[v], **AR1_PRIORS), ar1_ref.Ar1Chain, prec,
                  lambda P: (P.LatentAR1(y, likelihood=AR1_LIK[v], **AR1_PRIORS), d), kinds)
    elif f == "mixture":
        K = case.kw["K"]
        prec = 0.25 if lp else prec
        w, mu, sd = mixture_data(K, d, seed=K + d) if lp else mixture_data(K, d, seed=3 * K + d, spread=1.0) if mala else mixture_data(K, d, seed=7 * K + d)
        m = Model(mixture_ref.Mixture(w, mu, sd), mixture_ref.MixtureChain, prec, lambda P: (P.GaussianMixture(w, mu, sd), d), kinds)
    elif f == "dense":
        mean, Q = dense_target(d, 3 * d if mala else 7 * d)
        mean = 0.3 * mean if mala else mean
        m = Model(dense_ref.Dense(mean, Q), dense_ref.DenseChain, prec, lambda P: (P.DenseNormal(mean, Q), d), kinds)
    elif f == "varsel":
        n, pi, cols = case.kw["n"], case.kw["pi"], d // 2
        sd = 0.8 if lp else 1.0
        X, y = varsel_data(n, cols, v, seed=(n + cols) if lp else 7 * n + cols, noise_sd=sd)
        kinds = np.array([O.COORD_FLOAT64] * cols + [O.COORD_BOOL] * cols, dtype=np.int32)
        m = Model(varsel_ref.VarSel(X, y, v, sd, prec, pi), varsel_ref.VarSelChain, prec,
                  lambda P: (P.SpikeSlabRegression(X, y, likelihood=v, noise_sd=sd, inclusion_prob=pi), cols), kinds)
    else:
        raise KeyError(f)
    _MODELS[case.id] = m
    return m


# the seed and the scale of _random_states in the family's own test of this mode
_STATE_SEED = {
    ("glm", "slice"): lambda c: (c.kw["n"], 1.0), ("glm", "mala"): lambda c: (c.d, 0.5), ("glm", "lp"): lambda c: (c.d, 0.5),
    ("hier", "slice"): lambda c: (c.d - 2, 1.0), ("hier", "mala"): lambda c: (c.d, 0.5),
    ("ar1", "slice"): lambda c: (c.d, 1.0), ("ar1", "mala"): lambda c: (c.d, 0.5),
    ("mixture", "slice"): lambda c: (c.kw["K"], 1.5), ("mixture", "mala"): lambda c: (c.d, 1.0), ("mixture", "lp"): lambda c: (c.d, 1.5),
    ("dense", "slice"): lambda c: (c.d, 1.0), ("dense", "mala"): lambda c: (c.d, 0.5),
    ("varsel", "slice"): lambda c: (c.kw["n"], 1.0), ("varsel", "lp"): lambda c: (c.d // 2, 0.5),
}


def layout(case):
    """(betas, x, chain): _random_states of the families' tests -- the schedule 0, sorted uniforms, 1; states N(0, scale^2) (varsel: the
    thetas, then fair coins); a random chain permutation"""
    seed, scale = _STATE_SEED[(case.family, "mala" if case.mode == "automala" else case.mode)](case)
    N, d = case.N, case.d
    g = np.random.default_rng(seed)
    betas = np.concatenate([[0.0], np.sort(g.uniform(0.0, 1.0, N - 2)), [1.0]])
    if case.family == "varsel":
        x = np.concatenate([g.normal(0.0, scale, (N, d // 2)), (g.uniform(size=(N, d // 2)) < 0.5).astype(float)], axis=1)
    else:
        x = g.normal(0.0, scale, (N, d))
    chain = g.permutation(N).astype(np.int64)
    return betas, x, chain


def init_rng_words(N, seed=ENGINE_SEED):
    """the RNG words of a new engine's replicas on the interpolated path: the i-th split of SplittableRandom(seed)"""
    root = O.OracleRng(seed=seed)
    return np.array([root.split().state for _ in range(N)], dtype=np.uint64)


def target_std(case):
    """set_explorer_adaptation's standard deviations, as the family's MALA test draws them"""
    lo, hi = (0.7, 1.4) if case.family == "dense" else (0.5, 2.0)
    return np.random.default_rng(case.d).uniform(lo, hi, case.d)


def n_refresh(d, base=3, exponent=0.35):
    """MALA's defaults (pigeons_amd.MALA.base_n_refresh, exponent_n_refresh)"""
    return base * int(math.ceil(d ** exponent))


def mala_reference(case, betas, x, chain, rng):
    """the restatement's MALA transition of every replica off the reference chain, refresh by refresh as tests/test_gpu_dense.py runs it
    -> ({replica: dict(x, words, acc_sum)}, proposals accepted, rejected)"""
    m, d, step = model(case), case.d, case.kw["step"]
    std, nr = target_std(case), n_refresh(case.d)
    out, accepted, rejected = {}, 0, 0
    for i in range(case.N):
        c = int(chain[i])
        if c == 0:
            continue
        r = O.OracleRng(state=(int(rng[i, 0]), int(rng[i, 1])))
        Mv = aaps_ref.build_preconditioner(r, d, PRECOND_MODE[case.kw["precond"]], 1.0 / 3.0, 1.0 / 3.0, std)
        ch = m.chain(betas[c])
        xc, acc_sum = x[i].copy(), 0.0
        for _ in range(nr):                              # (the density and gradient at the start are pure functions of the state: the same bits)
            res = mixture_ref.mala_transition(xc, r, ch, step, 1, Mv)
            took = not np.array_equal(res["x"], xc)
            accepted += int(took)
            rejected += int(not took)
            xc, acc_sum = res["x"], acc_sum + res["acc_sum"]
        out[i] = dict(x=xc, words=r.state, acc_sum=acc_sum)
    return out, accepted, rejected


def automala_reference(case, betas, x, chain, rng):
    """the restatement's AutoMALA transition (tests/automala_ref.py) of every replica off the reference chain at the case's step and scan
    -> {replica: automala_transition's dict + words}"""
    m, d = model(case), case.d
    std, nr = target_std(case), n_refresh(d, base=AUTOMALA_BASE_N_REFRESH)
    out = {}
    for i in range(case.N):
        c = int(chain[i])
        if c == 0:
            continue
        r = O.OracleRng(state=(int(rng[i, 0]), int(rng[i, 1])))
        Mv = aaps_ref.build_preconditioner(r, d, PRECOND_MODE[case.kw["precond"]], 1.0 / 3.0, 1.0 / 3.0, std)
        out[i] = automala_ref.automala_transition(x[i], r, m.chain(betas[c]), case.kw["step"], nr, Mv, case.kw["scan"] != 1)
        out[i]["words"] = r.state
    return out


def automala_seen(case, x, res):
    """(the counts that a case's seen= records, the least margin) of automala_reference's result"""
    ex = [e for r in res.values() for e in r["exponents"]]
    acc, n = sum(r["accepted"] for r in res.values()), sum(r["acc_n"] for r in res.values())
    rs, rn = sum(r["rev_sum"] for r in res.values()), sum(r["rev_n"] for r in res.values())
    moved = sum(int(not np.array_equal(r["x"], x[i])) for i, r in res.items())
    nonfinite = sum(r["nonfinite"] for r in res.values())
    return (acc, n - acc, rs, rn - rs, min(ex), max(ex), nonfinite, moved), min(min(r["margins"]) for r in res.values())


def slice_reference(case, beta, x, words):
    """one SliceSampler step of the oracle on the restatement's path_lp -> (state, RNG words, statistics); a new chain per step (varsel's
    holds the cached predictor)"""
    m = model(case)
    r = O.OracleRng(state=(int(words[0]), int(words[1])))
    sl = O.MixedSliceSampler(m.chain(beta).path_lp, m.kinds, w=case.kw["w"], p=case.kw["p"], n_passes=case.kw["n_passes"])
    y = np.array(x, dtype=np.float64)
    sl.step(r, y)
    return y, r.state, sl.stats
