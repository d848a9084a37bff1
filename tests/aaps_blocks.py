"""The case table of k_explore_aaps at every one of its sixteen instantiations (E = 1, 2, 4, 8 blocks per lane x {MVN, funnel} x {ragged,
whole blocks}) and on its failure paths, defined once and used by tests/test_aaps_blocks_cpu.py (the table's own coverage, what the
restatement does on each case, how far its decisions are from ties, its own rounding sensitivity) and tests/test_gpu_aaps_blocks.py (the
device against the restatement at one transition).

A Case is (target, d, N, step, K, preconditioner, vref, kind, seed).  Its inputs are made the way tests/test_gpu_aaps.py::_one_step makes
them from default_rng(seed) -- the schedule 0, squared sorted uniforms, 1; states; a chain permutation; the standard deviations of the
preconditioner; with vref a GaussianReference's mean and std -- with two changes: a funnel case of kind "parity" or "cap" starts near the
typical set (x[0] = 0.5 z0, x[i] = z_i exp(x[0] / 2): the leapfrog is stable there; at _one_step's 0.5 z and step 0.3 most replicas of
d >= 256 fail at once), and vref flags half of the chains (USES: the reference chain among them, and every combination of flagged and
unflagged neighbours), not all.  kind:

  "parity"    no replica fails, at least five of seven move, every replica visits a candidate;
  "unstable"  _one_step's own states at a step too long for the stiffest chains: some replica meets a non-finite point and stays;
  "cap"       a step so short that neither pass leaves its segment within PTE_AAPS_MAX_LEAPFROGS = 4096 steps: every replica stays.

The RNG words are the engine's own; init_rng_words restates them (pte.hip: replica i holds the i-th split of SplittableRandom(seed); on
the MVN path k_init then draws the d normals of the initial state from it, on the funnel path init_zero_state draws nothing), so that the
restatement can run before any device does -- the GPU tests assert the two equal.

reference(case) runs tests/aaps_ref.py::transition on every replica off the reference chain, once per case and process.  probe() is an
instrumented copy of that function: the same arithmetic (the CPU tests hold the two to the same bits), with the state arithmetic in a
dtype of choice, recording the index of the selected candidate and the margins of every decision."""
import math

import numpy as np

import aaps_ref as A
import oracle as O

PRECOND_MODE = {"identity": 0, "diagonal": 1, "mix": 2}
MIX_P0 = MIX_P1 = 1.0 / 3.0                          # MixDiagonalPreconditioner's defaults, as _one_step passes them
FUNNEL_REF_PREC = 1.0 / 9.0
MVN_PATH = (1.0, 10.0)                               # toy_mvn_target: precision 1 at beta = 0, 10 at beta = 1
USES = (1, 1, 0, 1, 0, 0, 1, 0)                      # set_variational_reference's flags by chain


class Case:
    def __init__(self, target, d, step, K=4, precond="mix", vref=False, kind="parity", N=8, seed=3, steps=None):
        """steps: the leapfrog steps of the N - 1 replicas off the reference chain, summed, as the restatement counted them on the CPU"""
        self.target, self.d, self.step, self.K, self.precond, self.vref, self.kind = target, int(d), float(step), int(K), precond, vref, kind
        self.N, self.seed, self.steps = int(N), int(seed), steps
        parts = [target, "d%d" % d] + (["vref"] if vref else []) + ([precond] if precond != "mix" else []) + (["K%d" % K] if K != 4 else [])
        self.id = "-".join(parts + ([kind] if kind != "parity" else []))

    def __repr__(self):
        return self.id


# ---- the table -------------------------------------------------------------------------------------------------------------------------
# steps = ...: the restatement's count on the CPU, summed over the transitions off the reference chain (tests/test_aaps_blocks_cpu.py
# repeats it).  The comment behind a row, as measured on the CPU when the row was written: (fewest, most) steps of one replica; replicas
# moved, and the largest relative distance of a final coordinate from the same transition with np.longdouble state arithmetic (or:
# replicas failed, moved); the margins of the decisions: least |h| / sum |p g~|, least |u - exp(w - L)|, and the distance of the mix
# preconditioner's uniform from its thresholds.  default_rng(3) throughout, but two MVN rows where it moves only four replicas of seven.
# MVN: step 0.25 -- with std in [0.5, 2], step sqrt(10) 2 < 2 keeps every draw of the preconditioner stable.  Funnel: step 0.1, and 0.05
# from d = 511 on.  PARITY_CASES reach all sixteen (E, target, whole) cells; at d = 129 and 257 the last occupied block holds one
# coordinate and the blocks behind it none.
PARITY_CASES = [
    Case("mvn", 33, 0.25, steps=190),                                         # (14, 42), 5 moved, 3.4e-14; margins 2e-03 2e-03 2e-02
    Case("mvn", 64, 0.25, steps=240),                                         # (21, 62), 7 moved, 2.4e-14; margins 4e-04 5e-03 2e-02
    Case("mvn", 100, 0.25, steps=220),                                        # (13, 52), 6 moved, 1.0e-14; margins 1e-03 2e-03 5e-02
    Case("mvn", 128, 0.25, steps=228),                                        # (16, 52), 7 moved, 3.2e-13; margins 4e-04 2e-03 1e-02
    Case("mvn", 129, 0.25, steps=224),                                        # (19, 61), 7 moved, 4.1e-13; margins 4e-04 2e-03 2e-02
    Case("mvn", 193, 0.25, steps=227),                                        # (19, 52), 7 moved, 2.3e-12; margins 6e-04 1e-03 4e-02
    Case("mvn", 255, 0.25, steps=258),                                        # (15, 62), 7 moved, 5.8e-13; margins 8e-04 5e-04 2e-02
    Case("mvn", 256, 0.25, steps=237),                                        # (14, 62), 6 moved, 1.4e-13; margins 7e-04 3e-03 3e-02
    Case("mvn", 257, 0.25, seed=1, steps=195),                                # (15, 40), 7 moved, 1.8e-13; margins 2e-03 3e-03 1e-02
    Case("mvn", 320, 0.25, steps=243),                                        # (21, 51), 6 moved, 6.9e-14; margins 4e-04 8e-04 9e-02
    Case("mvn", 511, 0.25, steps=279),                                        # (14, 62), 7 moved, 1.4e-12; margins 1e-03 4e-04 2e-02
    Case("mvn", 512, 0.25, steps=265),                                        # (17, 62), 7 moved, 2.6e-13; margins 9e-04 1e-04 2e-02
    Case("funnel", 20, 0.1, steps=1679),                                      # (77, 451), 6 moved, 1.7e-14; margins 1e-04 3e-04 2e-02
    Case("funnel", 64, 0.1, steps=1799),                                      # (94, 436), 7 moved, 8.5e-13; margins 4e-04 4e-04 2e-02
    Case("funnel", 65, 0.1, steps=1854),                                      # (112, 449), 7 moved, 1.3e-12; margins 9e-04 1e-03 2e-02
    Case("funnel", 127, 0.1, steps=2111),                                     # (123, 466), 7 moved, 1.9e-13; margins 6e-04 1e-04 2e-02
    Case("funnel", 128, 0.1, steps=1632),                                     # (122, 372), 7 moved, 1.1e-12; margins 3e-05 3e-06 2e-02
    Case("funnel", 129, 0.1, steps=1795),                                     # (115, 367), 7 moved, 8.6e-13; margins 1e-04 6e-04 2e-02
    Case("funnel", 192, 0.1, steps=1828),                                     # (22, 473), 7 moved, 8.7e-13; margins 3e-04 1e-05 2e-02
    Case("funnel", 255, 0.1, steps=1486),                                     # (16, 389), 7 moved, 1.4e-13; margins 8e-05 6e-05 2e-02
    Case("funnel", 256, 0.1, steps=2182),                                     # (64, 461), 7 moved, 1.8e-13; margins 2e-04 2e-05 2e-02
    Case("funnel", 257, 0.1, steps=2032),                                     # (54, 472), 7 moved, 5.1e-13; margins 6e-04 2e-04 2e-02
    Case("funnel", 320, 0.1, steps=1771),                                     # (81, 462), 7 moved, 2.4e-13; margins 3e-04 5e-05 2e-02
    Case("funnel", 511, 0.05, steps=3654),                                    # (192, 948), 7 moved, 3.3e-13; margins 7e-05 6e-05 2e-02
    Case("funnel", 512, 0.05, steps=3913),                                    # (66, 926), 7 moved, 1.3e-12; margins 2e-04 1e-04 2e-02
]
VREF_CASES = [
    Case("funnel", 65, 0.1, vref=True, steps=1345),                           # (83, 335), 7 moved, 1.3e-12; margins 6e-04 1e-03 2e-02
    Case("funnel", 129, 0.1, vref=True, steps=1332),                          # (81, 326), 7 moved, 1.1e-13; margins 1e-04 2e-03 2e-02
    Case("funnel", 256, 0.1, vref=True, steps=1524),                          # (64, 461), 7 moved, 1.8e-13; margins 3e-04 4e-04 2e-02
    Case("funnel", 257, 0.1, vref=True, steps=1569),                          # (37, 471), 7 moved, 5.1e-13; margins 3e-04 2e-04 2e-02
    Case("funnel", 512, 0.05, vref=True, steps=3015),                         # (66, 926), 7 moved, 1.6e-13; margins 5e-04 6e-04 2e-02
]
PRECOND_K_CASES = [
    Case("funnel", 200, 0.1, precond="identity", steps=2001),                 # (94, 473), 7 moved, 7.6e-14; margins 7e-04 3e-05
    Case("funnel", 130, 0.1, precond="diagonal", steps=979),                  # (26, 263), 7 moved, 9.4e-14; margins 7e-05 1e-03
    Case("funnel", 384, 0.1, precond="identity", steps=2298),                 # (11, 471), 7 moved, 3.0e-13; margins 2e-03 3e-04
    Case("funnel", 300, 0.1, precond="diagonal", steps=912),                  # (28, 264), 7 moved, 7.8e-13; margins 1e-03 6e-04
    Case("funnel", 448, 0.1, K=0, steps=478),                                 # (30, 95), 7 moved, 9.7e-14; margins 5e-03 3e-04 2e-02
    Case("mvn", 400, 0.25, K=9, seed=2, steps=417),                           # (27, 94), 7 moved, 4.2e-12; margins 2e-04 1e-03 1e-02
]
UNSTABLE_CASES = [
    Case("mvn", 130, 0.4, kind="unstable", steps=394),                        # (15, 252), 1 failed, 4 moved; margins 7e-03 2e-04 6e-02
    Case("funnel", 130, 0.3, kind="unstable", steps=279),                     # (4, 95), 2 failed, 5 moved; margins 9e-03 3e-03 2e-02
    Case("funnel", 300, 0.3, kind="unstable", steps=417),                     # (2, 157), 2 failed, 5 moved; margins 2e-03 4e-03 2e-02
]
CAP_CASES = [
    Case("mvn", 130, 1e-06, K=2, kind="cap", N=4, steps=12288),               # (4096, 4096), 3 failed, 0 moved; margins 7e-02 6e-05 7e-02
    Case("funnel", 130, 1e-07, K=2, kind="cap", N=4, steps=12288),            # (4096, 4096), 3 failed, 0 moved; margins 1e-01 2e-05 2e-02
]
TRANSITION_CASES = PARITY_CASES + VREF_CASES + PRECOND_K_CASES           # kind "parity"
CASES = TRANSITION_CASES + UNSTABLE_CASES + CAP_CASES
assert len(set(c.id for c in CASES)) == len(CASES)
BY_ID = {c.id: c for c in CASES}
# test_statistics_left_for_the_swap: one case per (target, E >= 2), and the GaussianReference at E = 4 and E = 8
STATISTICS_CASES = [BY_ID[i] for i in ("mvn-d128", "mvn-d129", "mvn-d257", "funnel-d65", "funnel-d129", "funnel-d257",
                                        "funnel-d129-vref", "funnel-d256-vref", "funnel-d257-vref", "funnel-d512-vref")]


# ---- a case's inputs -------------------------------------------------------------------------------------------------------------------
class CaseInputs:
    pass


def init_rng_words(case):
    """the RNG words of a new engine's replicas"""
    root = O.OracleRng(seed=case.seed)
    out = []
    for _ in range(case.N):
        r = root.split()
        if case.target == "mvn":                     # k_init: the initial state's d normals
            for _ in range(case.d):
                r.randn()
        out.append(r.state)
    return np.array(out, dtype=np.uint64)


_INPUTS = {}


def inputs(case):
    """betas, x, chain, std, vm, vs, uses (None without vref), words -- built once per case; do not write to them"""
    if case.id in _INPUTS:
        return _INPUTS[case.id]
    N, d, funnel = case.N, case.d, case.target == "funnel"
    g = np.random.default_rng(case.seed)
    inp = CaseInputs()
    inp.betas = np.concatenate([[0.0], np.sort(g.uniform(0.0, 1.0, N - 2)) ** 2, [1.0]])
    z = g.standard_normal((N, d))
    if funnel and case.kind != "unstable":
        inp.x = z.copy()
        inp.x[:, 0] = 0.5 * z[:, 0]
        inp.x[:, 1:] = z[:, 1:] * np.exp(inp.x[:, 0] / 2.0)[:, None]
    else:
        inp.x = z * (0.5 if funnel else 0.4)
    inp.chain = g.permutation(N).astype(np.int64)
    inp.std = g.uniform(0.5, 2.0, d)
    inp.vm = inp.vs = inp.uses = None
    if case.vref:
        inp.vm, inp.vs = g.normal(0.0, 0.3, d), g.uniform(0.7, 1.5, d)
        inp.uses = np.resize(np.array(USES, dtype=np.int32), N)
    inp.words = init_rng_words(case)
    for a in (inp.betas, inp.x, inp.chain, inp.std, inp.words):
        a.setflags(write=False)
    _INPUTS[case.id] = inp
    return inp


def chain_of(case, inp, c):
    """the restatement's chain c, as the transition sees it"""
    if case.target == "mvn":
        return A.mvn_chain(MVN_PATH[0], MVN_PATH[1], inp.betas[c])
    if case.vref and inp.uses[c]:
        return A.FunnelChain(inp.betas[c], FUNNEL_REF_PREC, inp.vm, inp.vs)
    return A.FunnelChain(inp.betas[c], FUNNEL_REF_PREC)


def log_density(case, inp, c, x):
    """log_potentials[c](x) as the swap and the traces use it (chain_lp, pte_kernels.hpp): on the funnel InterpolatedLogPotential with
    its short-circuits at beta = 0 and 1, the reference end the GaussianReference's where the chain is flagged"""
    x, b = np.asarray(x, dtype=np.float64), float(inp.betas[c])
    if case.target == "mvn":
        return chain_of(case, inp, c).lp_grad(x)[0]
    v = (inp.vm, inp.vs) if case.vref and inp.uses[c] else (None, None)
    ref = A.FunnelChain(0.0, FUNNEL_REF_PREC, *v).lp_grad(x)[0]          # l1 * 1 + l2 * 0
    tgt = A.FunnelChain(1.0, FUNNEL_REF_PREC).lp_grad(x)[0]              # l1 * 0 + l2 * 1
    return ref if b == 0.0 else tgt if b == 1.0 else (1.0 - b) * ref + b * tgt


def preconditioner(case, inp, rng):
    return A.build_preconditioner(rng, case.d, PRECOND_MODE[case.precond], MIX_P0, MIX_P1, inp.std)


def reference_chain_draw(case, inp, words):
    """sample_iid! at the reference chain: d normals in draw order, scaled by the reference's sd, or by the GaussianReference's std and
    shifted by its mean where the chain is flagged -> (state, RNG words)"""
    r = O.OracleRng(state=(int(words[0]), int(words[1])))
    z = np.array([r.randn() for _ in range(case.d)])
    if case.vref and inp.uses[0]:
        return z * inp.vs + inp.vm, r.state
    return z * (1.0 / math.sqrt(FUNNEL_REF_PREC if case.target == "funnel" else MVN_PATH[0])), r.state


_REFERENCE = {}


def reference(case):
    """{replica: dict(x, acc, steps, Kf, failed, words, moved)} of aaps_ref.transition on every replica off the reference chain -- run once
    per case; do not write to it"""
    if case.id in _REFERENCE:
        return _REFERENCE[case.id]
    inp, out = inputs(case), {}
    for i in range(case.N):
        c = int(inp.chain[i])
        if c == 0:
            continue
        r = O.OracleRng(state=(int(inp.words[i, 0]), int(inp.words[i, 1])))
        M = preconditioner(case, inp, r)
        res = A.transition(inp.x[i], r, chain_of(case, inp, c), case.step, case.K, M)
        res["words"], res["moved"] = r.state, not np.array_equal(res["x"], inp.x[i])
        res["x"].setflags(write=False)
        out[i] = res
    _REFERENCE[case.id] = out
    return out


def census(results):
    """(replicas failed, moved, fewest and most steps, steps summed) of {replica: dict(failed, moved, steps)}"""
    st = [r["steps"] for r in results.values()]
    return (sum(int(r["failed"]) for r in results.values()), sum(int(r["moved"]) for r in results.values()), min(st), max(st), sum(st))


# ---- the instrumented copy ---------------------------------------------------------------------------------------------------------------
def _lp_grad(chain, x, ft):
    """chain.lp_grad(x) with the arithmetic in ft (np.float64: the expressions of aaps_ref, to the same bits)"""
    if isinstance(chain, A.MvnChain):
        return ft(chain.nhp) * np.sum(x * x), ft(chain.nprec) * x
    two, nine, three = ft(2.0), ft(9.0), ft(3.0)
    y = x[0]
    sigma = np.exp(y / two)
    logsigma = np.log(sigma)
    z = x[1:] / sigma
    l2 = np.sum(-(z * z + ft(A.LOG2PI)) / two - logsigma) + (-((y / three) * (y / three) + ft(A.LOG2PI)) / two - ft(math.log(3.0)))
    g2 = np.empty_like(x)
    g2[1:] = -(z / sigma)
    g2[0] = np.sum((z * z - ft(1.0)) / two) + (-(y / nine))
    if chain.v is None:
        l1 = ft(-0.5 * chain.ref_prec) * np.sum(x * x)
        g1 = ft(-chain.ref_prec) * x
    else:
        m, c0, i2, gf = (a.astype(ft) for a in chain.v)
        dx = x - m
        l1 = np.sum(c0 - i2 * (dx * dx))
        g1 = gf * dx
    return l1 * ft(chain.omb) + l2 * ft(chain.beta), g1 * ft(chain.omb) + g2 * ft(chain.beta)


def probe(x0, rng, chain, step_size, K, M, ft=np.float64, max_leapfrogs=A.MAX_LEAPFROGS):
    """aaps_ref.transition statement by statement, with x, p, g~, M and the density's sums in ft; the draws, logaddexp and the exp of the
    choice stay in float64.  -> dict(x, acc, steps, Kf, failed, selected, n_candidates, h_margin, u_margin): selected the index in visit
    order of the chosen candidate (-1: x0); h_margin the least |h| / sum |p_i g~_i| over every computed point with finite h (a sign of h
    decides where segments end), u_margin the least |u - exp(w - L)| over the candidates (it decides the choice)"""
    x0 = np.asarray(x0, dtype=np.float64).astype(ft)
    M = np.asarray(M, dtype=np.float64).astype(ft)
    d = x0.size
    p0 = np.array([rng.randn() for _ in range(d)]).astype(ft)
    Kf = rng.rand_range(0, K)
    Kb = K - Kf
    eps, half = ft(step_size), ft(step_size) / ft(2.0)
    st = dict(steps=0, failed=False, visited=0, selected=-1, h_margin=math.inf, u_margin=math.inf)

    def margin_h(p, g):
        h, scale = float(np.sum(p * g)), float(np.sum(np.abs(p * g)))
        if math.isfinite(h) and math.isfinite(scale) and scale > 0.0:
            st["h_margin"] = min(st["h_margin"], abs(h) / scale)

    with np.errstate(all="ignore"):
        lp0, g0 = _lp_grad(chain, x0, ft)
        g0 = g0 / M
        w0 = float(lp0 - ft(0.5) * np.sum(p0 * p0))
        if not math.isfinite(w0):
            raise A.AapsDensityError("AAPS can only be called on a configuration of positive density")
        h0 = float(np.sum(p0 * g0))
        margin_h(p0, g0)
    st["L"], st["sel"] = w0, x0.copy()

    def run(direction, stop_at):
        x, p, g = x0.copy(), ft(direction) * p0, g0.copy()
        s_prev, seg = h0 >= 0.0, 0
        while True:
            if st["steps"] == max_leapfrogs:
                st["failed"] = True
                return
            st["steps"] += 1
            p = p + half * g
            x = x + eps * (p / M)
            lp, gr = _lp_grad(chain, x, ft)
            g = gr / M
            if not math.isfinite(float(lp - ft(0.5) * np.sum(p * p))):
                st["failed"] = True
                return
            p = p + half * g
            pp = np.sum(p * p)
            w = float(lp - ft(0.5) * pp)
            if not math.isfinite(float(pp)) or not math.isfinite(w):
                st["failed"] = True
                return
            margin_h(p, g)
            s = direction * float(np.sum(p * g)) >= 0.0
            if direction > 0:
                seg += 1 if (not s_prev and s) else 0
            else:
                seg -= 1 if (not s and s_prev) else 0
            if seg == stop_at:
                return
            st["L"] = A.logaddexp(st["L"], w)
            u, pr = rng.rand(), math.exp(w - st["L"])
            st["u_margin"] = min(st["u_margin"], abs(u - pr))
            if u < pr:
                st["sel"], st["selected"] = x.copy(), st["visited"]
            st["visited"] += 1
            s_prev = s

    with np.errstate(all="ignore"):
        run(1.0, Kf + 1)
        if not st["failed"]:
            run(-1.0, -(Kb + 1))
    out = dict(steps=st["steps"], Kf=Kf, failed=st["failed"], n_candidates=st["visited"], h_margin=st["h_margin"], u_margin=st["u_margin"])
    if st["failed"]:
        return dict(out, x=x0.copy(), acc=0.0, selected=-1)
    return dict(out, x=st["sel"], acc=1.0 - math.exp(w0 - st["L"]), selected=st["selected"])


def preconditioner_margin(case, words):
    """the distance of the mix preconditioner's first uniform from its two thresholds (inf for the other preconditioners)"""
    if case.precond != "mix":
        return math.inf
    u = O.OracleRng(state=(int(words[0]), int(words[1]))).rand()
    return min(abs(u - MIX_P0), abs(u - (MIX_P0 + MIX_P1)))


_PROBES = {}


def probes(case, ft=np.float64):
    """{replica: probe's dict + words, moved} of every replica off the reference chain -- run once per (case, ft)"""
    key = (case.id, ft)
    if key in _PROBES:
        return _PROBES[key]
    inp, out = inputs(case), {}
    for i in range(case.N):
        c = int(inp.chain[i])
        if c == 0:
            continue
        r = O.OracleRng(state=(int(inp.words[i, 0]), int(inp.words[i, 1])))
        M = preconditioner(case, inp, r)
        res = probe(inp.x[i], r, chain_of(case, inp, c), case.step, case.K, M, ft)
        res["words"], res["moved"] = r.state, not np.array_equal(res["x"].astype(np.float64), inp.x[i])
        out[i] = res
    _PROBES[key] = out
    return out
