"""The edge battery of the nine target families on the interpolated path: a fixed, named list of (shape, data, state) per family, defined
once and used by tests/test_family_edges_cpu.py (the restatements against tests/family_mp.py) and tests/test_gpu_family_edges.py (the
device against both).  No random edge values: every listed value is an exact double, the remaining coordinates are default_rng(seed)
N(0, 1) draws.  Every state lies inside its family's declared domain ("where each family's density is held to its definition")
and has a finite density.

A Shape carries the constructor arguments of the family's restatement (and of its family_mp function, in the same order), the reference's
precision, and its named states.  The module also maps a Shape to its restatement, its chains, its 60-digit value, its coordinate kinds
and its device target, so that neither half repeats that per family."""
import math

import numpy as np

import ar1_ref
import changepoint_ref
import dense_ref
import family_mp as MP
import glm_ref
import hier_ref
import mixture_model_ref
import mixture_ref
import varsel_ref
from mixture_ref import tree_sum

LOG2PI = 1.8378770664093453
COORD_FLOAT64, COORD_INTEGER, COORD_BOOL = 0, 1, 2           # oracle.COORD_*


class Shape:
    def __init__(self, family, name, ctor, ref_prec, states):
        self.family, self.name, self.ctor, self.ref_prec, self.states = family, name, ctor, float(ref_prec), states
        self.id = "%s-%s" % (family, name)
        names = [s for s, _ in states]
        assert len(set(names)) == len(names), names
        self.dim = len(states[0][1])
        assert all(np.asarray(x).shape == (self.dim,) for _, x in states)

    def __repr__(self):
        return self.id


# ---- the funnel has a C oracle and no NumPy restatement: this is pt_oracle.c's funnel_lp_grad and the interpolation around it ----------
class Funnel:
    def __init__(self, dim):
        self.d = int(dim)

    def lp(self, z):
        return self.lp_grad(z)[0]

    def lp_grad(self, z):
        z = np.asarray(z, dtype=np.float64)
        with np.errstate(all="ignore"):
            y = z[0]
            zv = y / 3.0
            sigma = np.exp(y / 2.0)
            logsigma = np.log(sigma)
            zi = z[1:] / sigma
            lp = tree_sum(np.concatenate([[-(zv * zv + LOG2PI) / 2.0 - math.log(3.0)], -(zi * zi + LOG2PI) / 2.0 - logsigma]))
            g = np.concatenate([[0.0], -(zi / sigma)])
            g[0] = tree_sum(np.concatenate([[-(y / 9.0)], (zi * zi - 1.0) / 2.0]))
        return lp, g


class FunnelChain:
    def __init__(self, funnel, beta, ref_prec):
        self.funnel, self.beta, self.omb, self.ref_prec = funnel, beta, 1.0 - beta, ref_prec

    def lp_grad(self, x):
        x = np.asarray(x, dtype=np.float64)
        with np.errstate(all="ignore"):
            S = tree_sum(x * x)
            l2, g2 = self.funnel.lp_grad(x)
            l1 = (-0.5 * self.ref_prec) * S
            return 0.0 + l1 * self.omb + l2 * self.beta, ((-self.ref_prec) * x) * self.omb + g2 * self.beta

    def path_lp(self, x):
        x = np.asarray(x, dtype=np.float64)
        with np.errstate(all="ignore"):
            S = tree_sum(x * x)
            if self.beta == 0.0:
                return (-0.5 * self.ref_prec) * S
            l2 = self.funnel.lp(x)
            if self.beta == 1.0:
                return l2
            return self.omb * ((-0.5 * self.ref_prec) * S) + self.beta * l2


# ---- the families ----------------------------------------------------------------------------------------------------------------------
AR1_PRIORS = dict(obs_sd=0.7, mu_sd=2.0, phi_loc=0.3, phi_scale=0.8, sigma_scale=1.5)
AR1_A = [0.0] + [s * v for v in (1.5, 5.0, 8.0, 10.0, 12.0, 15.0, 18.0, 19.5, 25.0) for s in (1.0, -1.0)]


def _ar1_shapes():
    out = []
    for T in (1, 8, 64):
        for lik in ("stochastic_volatility", "normal_identity"):
            g = np.random.default_rng(1000 + T)
            y = g.normal(0.0, 1.0, T)
            y[0] = 0.0                                              # (an observation that is 0 exactly: its term is -h / 2 whatever h)
            base = g.normal(0.0, 1.0, T + 3)
            st = []
            for a in AR1_A:
                x = base.copy(); x[1] = a
                st.append(("a=%g" % a, x))
            for ls in (-30.0, 30.0):
                x = base.copy(); x[1] = 1.5; x[2] = ls
                st.append(("ls=%g" % ls, x))
            for hv in (600.0, -600.0):
                x = base.copy(); x[3 + T - 1] = hv                  # (the last state: y there is not 0 unless T = 1)
                st.append(("h=%g" % hv, x))
            x = base.copy(); x[3] = -50.0
            st.append(("y=0,h=-50", x))
            x = base.copy(); x[3:] = x[0]
            st.append(("h=mu", x))
            out.append(Shape("ar1", "T%d-%s" % (T, "sv" if lik[0] == "s" else "n"), dict(y=y, likelihood=lik, **AR1_PRIORS), 0.5, st))
    return out


HIER_LT = [-300.0, -30.0, -10.0, 0.0, 10.0, 30.0, 300.0]


def _hier_shapes():
    out = []
    for J in (1, 8, 64):
        for param in ("centered", "noncentered"):
            g = np.random.default_rng(2000 + J)
            y = g.normal(0.0, 1.0, J) * 2.0
            sigma = g.uniform(0.5, 2.0, J)
            base = g.normal(0.0, 1.0, J + 2)
            st = []
            for lt in HIER_LT:
                x = base.copy(); x[1] = lt
                st.append(("lt=%g" % lt, x))
            x = base.copy()
            x[2:] = x[0] if param == "centered" else 0.0            # theta_j = mu exactly (non-centred: eta_j = 0)
            st.append(("theta=mu", x))
            x = base.copy()
            if param == "centered":
                x[2:] = y
            else:
                x[0], x[1], x[2:] = 0.0, 0.0, y                      # mu + exp(0) eta_j = y_j bit for bit
            st.append(("theta=y", x))
            x = _to_1e6(base); x[1] = base[1]                          # (log tau stays inside its own bound)
            st.append(("x1e6", x))
            out.append(Shape("hier", "J%d-%s" % (J, param[0]), dict(y=y, sigma=sigma, mu_sd=2.0, tau_scale=1.5, parameterization=param), 0.5, st))
    return out


ETA_SCALES = [0.0, 1.0, 40.0, 800.0, 1e5]


def _to_1e6(v):
    """v x 1e6, the largest draw brought to 1: no coordinate leaves the declared bound"""
    return v / float(np.max(np.abs(v))) * 1e6


def _scaled(X, theta, target):
    """theta scaled so that max |X theta| is about target"""
    if target == 0.0:
        return np.zeros_like(theta)
    return theta * (target / float(np.max(np.abs(X @ theta))))


def _glm_shapes():
    out = []
    for n, d in ((1, 1), (65, 3), (130, 67)):
        for lik in ("bernoulli_logit", "normal_identity"):
            g = np.random.default_rng(3000 + n)
            X = g.normal(0.0, 1.0, (n, d))
            sep = g.normal(0.0, 1.0, d)                              # the data are separated by this direction
            base = g.normal(0.0, 1.0, d)
            y = (X @ sep > 0.0).astype(np.float64) if lik == "bernoulli_logit" else g.normal(0.0, 1.0, n)
            st = [("eta=%g" % s, _scaled(X, base, s)) for s in ETA_SCALES]
            if lik == "bernoulli_logit":
                x = _scaled(X, sep, 800.0)
                assert np.all((2.0 * y - 1.0) * (X @ x) > 0.0)
                st += [("separating", x), ("anti-separating", -x)]
            out.append(Shape("glm", "n%d-d%d-%s" % (n, d, lik[0]), dict(X=X, y=y, likelihood=lik, noise_sd=0.8, prec=0.5), 0.5, st))
    return out


def _mixture_shapes():
    out = []
    for K, d in ((1, 1), (3, 65), (8, 64)):
        g = np.random.default_rng(4000 + K)
        mu = np.round(g.normal(0.0, 3.0, (K, d)) * 1024.0) / 1024.0
        sd = np.exp(g.uniform(math.log(1e-2), math.log(1e2), (K, d)))
        w = g.uniform(0.2, 1.0, K)
        mu[:, 0] = -np.abs(mu[:, 0]) - 8.0                            # (so that 1e3 standard deviations of 1e3 above it stay within 1e6)
        sd[0, 0], sd[K - 1, d - 1] = 1e3, 1e-3                       # the ends of the declared range
        if K >= 2:
            w[K - 1] = 1e-12
            delta = np.round(g.uniform(0.5, 2.0, d) * 1024.0) / 1024.0
            mu[1], sd[1], w[1] = mu[0] + 2.0 * delta, sd[0], w[0]     # components 0 and 1: equal but for the means, mid exactly between
            mid = mu[0] + delta
            assert np.array_equal(mid - mu[0], mu[1] - mid)
        base = g.normal(0.0, 1.0, d)
        st = [("at-mean", mu[K - 1].copy())]
        if K >= 2:
            st.append(("midway", mid))
        st += [("1e3-sd", mu.max(axis=0) + 1e3 * sd.max(axis=0)), ("zero", np.zeros(d)), ("x1e6", _to_1e6(base))]
        assert all(np.max(np.abs(x)) <= 1e6 for _, x in st)
        out.append(Shape("mixture", "K%d-d%d" % (K, d), dict(weights=w, means=mu, std_devs=sd), 0.25, st))
    return out


def _mixture_model_shapes():
    out = []
    for n, K in ((1, 1), (65, 3), (200, 8)):
        g = np.random.default_rng(5000 + n)
        y = g.normal(0.0, 1.0, n)
        base = g.normal(0.0, 1.0, 3 * K)
        st = []
        x = base.copy(); x[2 * K:] = ([700.0, -700.0] + [0.0] * K)[:K]
        st.append(("alpha=700,-700,0", x))
        x = base.copy(); x[K] = -30.0; x[0] = y[n // 2]
        st.append(("s=-30,mu=y", x))
        x = base.copy(); x[K] = 30.0
        st.append(("s=30", x))
        if K >= 2:
            x = base.copy(); x[1], x[K + 1], x[2 * K + 1] = x[0], x[K], x[2 * K]
            st.append(("twins", x))
        out.append(Shape("mixture_model", "n%d-K%d" % (n, K), dict(y=y, n_components=K, prec=0.5), 0.5, st))
    return out


# inclusion_prob is the target's: each of the three values meets both likelihoods, each shape two of them
VARSEL_PI = {(5, "b"): 0.5, (5, "n"): 1e-6, (32, "b"): 1e-6, (32, "n"): 1.0 - 1e-12, (33, "b"): 1.0 - 1e-12, (33, "n"): 0.5}


def _varsel_shapes():
    out = []
    for n, d in ((5, 1), (65, 32), (65, 33)):
        for lik in ("bernoulli_logit", "normal_identity"):
            g = np.random.default_rng(6000 + d)
            X = g.normal(0.0, 1.0, (n, d))
            base = g.normal(0.0, 1.0, d)
            y = (g.uniform(0.0, 1.0, n) < 0.5).astype(np.float64) if lik == "bernoulli_logit" else g.normal(0.0, 1.0, n)
            st = [("gamma=0,theta=1e6", np.concatenate([np.full(d, 1e6), np.zeros(d)]))]
            for s in ETA_SCALES:
                st.append(("gamma=1,eta=%g" % s, np.concatenate([_scaled(X, base, s), np.ones(d)])))
            j = d // 2
            for s in (1.0, 800.0):
                theta = np.full(d, 1e6)
                theta[j] = s / float(np.max(np.abs(X[:, j])))
                gamma = np.zeros(d); gamma[j] = 1.0
                st.append(("gamma=e%d,eta=%g" % (j, s), np.concatenate([theta, gamma])))
            pi = VARSEL_PI[(n if d == 1 else d, lik[0])]
            out.append(Shape("varsel", "n%d-d%d-%s" % (n, d, lik[0]),
                             dict(X=X, y=y, likelihood=lik, noise_sd=0.8, prec=0.5, inclusion_prob=pi), 0.5, st))
    return out


def _changepoint_shapes():
    out = []
    for n, K, zeros in ((1, 1, True), (50, 3, False), (50, 3, True), (200, 33, False), (200, 63, False)):
        g = np.random.default_rng(7000 + n + K)
        nz = max(1, n // 10)                                         # y[:nz] = 0: a segment [0, nz) has no counts
        y = np.zeros(n) if zeros else g.poisson(4.0, n).astype(np.float64)
        y[:nz] = 0.0
        r = math.log(4.0) + g.normal(0.0, 1.0, K + 1)
        st = []

        def add(name, tau, rr=r):
            st.append((name, np.concatenate([rr, np.asarray(tau, dtype=np.float64)])))
        add("tau=0", np.zeros(K))
        add("tau=n", np.full(K, float(n)))
        add("tau=n/2", np.full(K, float(n // 2)))
        if K >= 2:
            add("descending", np.floor(np.linspace(float(n), 0.0, K)))
            assert np.all(np.diff(st[-1][1][K + 1:]) < 0)
            tau = np.floor(np.linspace(0.0, float(n), K))
            tau[1::2] = tau[0::2][:tau[1::2].size]
            add("duplicates", tau[::-1].copy())
        rr = r.copy(); rr[0] = 600.0
        add("r=600,empty", np.zeros(K), rr)                          # all tau = 0: segments 0 .. K-1 are empty
        rr = r.copy(); rr[0] = -600.0
        add("r=-600,no-counts", np.full(K, float(nz)), rr)           # segment 0 = [0, nz)
        out.append(Shape("changepoint", "n%d-K%d%s" % (n, K, "-y0" if zeros and n > 1 else ""), dict(y=y, n_changepoints=K, prec=0.5), 0.5, st))
    return out


def _dense_shapes():
    out = []
    for d in (1, 64, 65):
        g = np.random.default_rng(8000 + d)
        Q = dense_ref.spectrum_matrix(d, 100.0, seed=d)
        mean = g.normal(0.0, 1.0, d)
        lam, V = np.linalg.eigh(Q)
        st = [("x=mean", mean.copy()), ("largest", mean + 3.0 * V[:, -1]), ("smallest", mean + 3.0 * V[:, 0]),
              ("x1e6", mean + _to_1e6(g.normal(0.0, 1.0, d)))]
        out.append(Shape("dense", "d%d" % d, dict(mean=mean, precision=Q), 0.5, st))
    return out


def _funnel_shapes():
    out = []
    for d in (2, 65):
        st = []
        for y in (-30.0, 0.0, 30.0):
            for other in (0.0, 1e3):
                x = np.full(d, other); x[0] = y
                st.append(("y=%g,x=%g" % (y, other), x))
        out.append(Shape("funnel", "d%d" % d, dict(dim=d), 1.0 / 9.0, st))
    return out


SHAPES = (_ar1_shapes() + _hier_shapes() + _glm_shapes() + _mixture_shapes() + _mixture_model_shapes() + _varsel_shapes()
          + _changepoint_shapes() + _dense_shapes() + _funnel_shapes())
FAMILIES = ["mixture", "glm", "mixture_model", "varsel", "changepoint", "hier", "ar1", "dense", "funnel"]
HAS_GRADIENT = ("mixture", "glm", "mixture_model", "hier", "ar1", "dense", "funnel")
assert sorted(set(s.family for s in SHAPES)) == sorted(FAMILIES)

_TARGET = {"ar1": ar1_ref.Ar1, "hier": hier_ref.Hier, "glm": glm_ref.Glm, "mixture": mixture_ref.Mixture,
           "mixture_model": mixture_model_ref.MixtureModel, "varsel": varsel_ref.VarSel, "changepoint": changepoint_ref.ChangePoint,
           "dense": dense_ref.Dense, "funnel": Funnel}
_CHAIN = {"ar1": ar1_ref.Ar1Chain, "hier": hier_ref.HierChain, "glm": glm_ref.GlmChain, "mixture": mixture_ref.MixtureChain,
          "mixture_model": mixture_model_ref.MixtureModelChain, "varsel": varsel_ref.VarSelChain,
          "changepoint": changepoint_ref.ChangePointChain, "dense": dense_ref.DenseChain, "funnel": FunnelChain}
_RESTATEMENTS = {}


def restatement(shape):
    """the family's restatement of this shape's target (built once)"""
    if shape.id not in _RESTATEMENTS:
        _RESTATEMENTS[shape.id] = _TARGET[shape.family](**shape.ctor)
    return _RESTATEMENTS[shape.id]


def chain(shape, beta):
    """a new chain of the restatement at beta: path_lp is SliceSampler's call-back (variable selection: the cached-predictor form, one chain
    per step), lp_grad the AD form where the family has a gradient"""
    return _CHAIN[shape.family](restatement(shape), float(beta), shape.ref_prec)


def ref_lp(shape, beta, x):
    """the restatement's path log density of a state on its own (variable selection: from the state alone, not from a cached predictor)"""
    c = chain(shape, beta)
    return float(c.lp_full(x) if shape.family == "varsel" else c.path_lp(np.array(x, dtype=np.float64)))


def mp_lp(shape, beta, x):
    """the 60-digit path log density"""
    return getattr(MP, shape.family)(**shape.ctor, beta=float(beta), ref_prec=shape.ref_prec, x=x)


def kinds(shape):
    if shape.family == "varsel":
        d = shape.dim // 2
        return np.array([COORD_FLOAT64] * d + [COORD_BOOL] * d, dtype=np.int32)
    if shape.family == "changepoint":
        K = shape.ctor["n_changepoints"]
        return np.array([COORD_FLOAT64] * (K + 1) + [COORD_INTEGER] * K, dtype=np.int32)
    return np.zeros(shape.dim, dtype=np.int32)


def device_target(P, shape):
    """(target, the reference's dimension) for pigeons_amd.Inputs"""
    c, f = shape.ctor, shape.family
    if f == "ar1":
        return P.LatentAR1(**c), shape.dim
    if f == "hier":
        return P.HierarchicalNormalMeans(**c), shape.dim
    if f == "glm":
        assert c["prec"] == shape.ref_prec
        return P.BayesianGLM(c["X"], c["y"], likelihood=c["likelihood"], noise_sd=c["noise_sd"]), shape.dim
    if f == "mixture":
        return P.GaussianMixture(c["weights"], c["means"], c["std_devs"]), shape.dim
    if f == "mixture_model":
        assert c["prec"] == shape.ref_prec
        return P.MixtureModelPosterior(c["y"], c["n_components"]), shape.dim
    if f == "varsel":
        assert c["prec"] == shape.ref_prec
        return P.SpikeSlabRegression(c["X"], c["y"], likelihood=c["likelihood"], noise_sd=c["noise_sd"], inclusion_prob=c["inclusion_prob"]), shape.dim // 2
    if f == "changepoint":
        assert c["prec"] == shape.ref_prec
        return P.PoissonChangePoint(c["y"], c["n_changepoints"]), c["n_changepoints"] + 1
    if f == "dense":
        return P.DenseNormal(c["mean"], c["precision"]), shape.dim
    if f == "funnel":
        return P.Funnel(c["dim"]), shape.dim
    raise KeyError(f)


def groups(shape, size=16):
    """the shape's states in the fewest groups of at most `size`, of about equal length, one chain per state: [(first index, [(name, x)])]"""
    n = len(shape.states)
    k = -(-n // size)
    cuts = [round(i * n / k) for i in range(k + 1)]
    return [(a, shape.states[a:b]) for a, b in zip(cuts[:-1], cuts[1:])]
