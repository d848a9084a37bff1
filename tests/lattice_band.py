"""Inputs that put chosen draws of an IsingMetropolis sweep at chosen distances from their acceptance thresholds.
TEST INFRASTRUCTURE ONLY; nothing here touches a device.

The lattice kernels decide `rand > accept_ratio` against guard-banded thresholds (lattice_thresholds, csrc/pte_ising.hpp) and fall back to the
reference's own arithmetic inside the band.  A draw's uniform u_k depends only on the replica's (seed, gamma) and on k, and the schedule
takes any doubles, so   beta = -ln(u_k / (1 + eps)) / (|delta| beta_target)   puts r = exp(-|delta| beta beta_target) at u_k / (1 + eps):
the k-th draw sits at the relative distance eps ABOVE its threshold (eps > 0: rejected, eps < 0: accepted).  Earlier decisions move with
beta, so a candidate is kept only if the replayed sweep's k-th draw really has that delta.

    thresholds / classify     lattice_thresholds restated, operation for operation, and the class of one decision
    banded_sweep              the kernels' three-way decision restated over tests/spinglass_ref.py's sweep, its in-band rule behind a hook
    search / search_gap       one (state, stream, k, eps) -> beta, the logged draw, its class; draw 1 between two ratios
    build                     the cases of one shape, their coverage bins, the share of discarded tries
    ladders                   cases -> (betas, x, chain, rng) of at most `max_cases` + 2 chains each
"""
import math
import struct

import numpy as np

import spinglass_ref as R
from checkerboard_ref import mix64, uniform_of_draw

BAND = 1e-9                      # the guard band's relative half-width
FILTER_MIN = 1e-13               # PTE_ISING_FILTER_MIN
M64 = (1 << 64) - 1
CLASSES = ("certain_reject", "certain_accept", "window_reject", "window_accept", "band")
# eps of every kind of case: fractions 0.3 and 0.9 of the band's half-width, the window outside the band, far outside
KINDS = (("band", 0.3 * BAND), ("band", -0.3 * BAND), ("band", 0.9 * BAND), ("band", -0.9 * BAND),
         ("window", 3e-9), ("window", -3e-9), ("certain", 1e-5), ("certain", -1e-5))
BETWEEN_MARGIN = 16              # ulps of u kept free on each side of a "between" draw


def pattern(v):
    """the 64-bit pattern of a double (patterns of positive doubles are ordered like the doubles)"""
    return struct.unpack("<Q", struct.pack("<d", v))[0]


class Stream:
    """the (seed, gamma) stream of tests/oracle.py's generator in plain Python: rand() is draw 1, 2, ... of uniform_of_draw"""

    def __init__(self, seed, gamma):
        self.seed, self.gamma = int(seed) & M64, int(gamma) & M64

    def rand(self):
        self.seed = (self.seed + self.gamma) & M64
        return float(mix64(self.seed) & ((1 << 52) - 1)) * 2.0 ** -52

    @property
    def state(self):
        return (self.seed, self.gamma)


def thresholds(bb):
    """lattice_thresholds(bb = beta * beta_target): the four doubles, their high words (_h), their patterns (_b), filter_ok"""
    r4, r8 = math.exp(-4.0 * bb), math.exp(-8.0 * bb)
    t = {"r4lo": r4 * (1.0 - 1e-9), "r4hi": r4 * (1.0 + 1e-9), "r8lo": r8 * (1.0 - 1e-9), "r8hi": r8 * (1.0 + 1e-9)}
    for name in ("r4lo", "r4hi", "r8lo", "r8hi"):
        t[name + "_b"] = pattern(t[name])
        t[name + "_h"] = t[name + "_b"] >> 32
    t["filter_ok"] = bb > FILTER_MIN
    return t


def classify(u, delta, beta, bt, th=None):
    """which of the kernels' paths decides `u > accept_ratio` for a proposal with delta = -4 or -8: the high words first (the vector pass of
    the speculative kernels), the whole patterns next (their scalar procedure), the band last.  The byte kernels compare doubles: for them
    the two window classes are simply certain."""
    assert delta in (-4, -8)
    th = thresholds(beta * bt) if th is None else th
    if not th["filter_ok"]:
        return "band"
    n = "r4" if delta == -4 else "r8"
    ub = pattern(u)
    uh = ub >> 32
    if uh > th[n + "hi_h"]:
        return "certain_reject"
    if uh < th[n + "lo_h"]:
        return "certain_accept"
    if ub > th[n + "hi_b"]:
        return "window_reject"
    if ub < th[n + "lo_b"]:
        return "window_accept"
    return "band"


def exact_rule(u, delta, beta, bt, S, S_stale, th):
    """the reference's arithmetic with the current S: what every kernel must do in the band"""
    ratio = math.exp(R.ising_lp(beta, bt, S + delta) - R.ising_lp(beta, bt, S))
    return ratio < 1 and u > ratio


# the four wrong in-band rules of the discrimination test
WRONG_RULES = {
    "plain threshold": lambda u, delta, beta, bt, S, S_stale, th: u > math.exp(delta * (beta * bt)),
    "always accept": lambda u, delta, beta, bt, S, S_stale, th: False,
    "always reject": lambda u, delta, beta, bt, S, S_stale, th: True,
    "stale S": lambda u, delta, beta, bt, S, S_stale, th: exact_rule(u, delta, beta, bt, S_stale, S_stale, th),
}


def banded_sweep(bits, jr, jd, beta, beta_target, S, rng, n_steps, band_rule=exact_rule):
    """IsingMetropolis(n_steps) the way the lattice kernels decide it: certain and window decisions against the thresholds, band decisions by
    band_rule(u, delta, beta, bt, S, S_stale, th) -> rejected, S_stale = S as it was when the sweep entered the row's current 32-site word
    (the row, where L is no multiple of 32).  With exact_rule this is spinglass_ref.sweep.  Returns the new S."""
    L = int(np.asarray(jr).shape[0])
    jrf = [int(v) for v in np.asarray(jr).ravel()]
    jdf = [int(v) for v in np.asarray(jd).ravel()]
    d, wl = L * L, (32 if L % 32 == 0 else L)
    th = thresholds(beta * beta_target)
    S_stale = S
    for _ in range(n_steps):
        for s in range(d):
            if s % wl == 0:
                S_stale = S
            delta = R.site_delta(bits, jrf, jdf, L, s)
            if delta < 0:
                if not th["filter_ok"]:
                    ratio = math.exp(R.ising_lp(beta, beta_target, S + delta) - R.ising_lp(beta, beta_target, S))
                    if ratio < 1 and rng.rand() > ratio:
                        continue
                else:
                    u = rng.rand()
                    cls = classify(u, delta, beta, beta_target, th)
                    if cls in ("certain_reject", "window_reject") or (cls == "band" and band_rule(u, delta, beta, beta_target, S, S_stale, th)):
                        continue
            bits[s] ^= 1
            S += delta
    return S


class _Reached(Exception):
    pass


class _LogUpTo(list):
    def __init__(self, k):
        super().__init__()
        self.k = k

    def append(self, item):
        super().append(item)
        if item[0] >= self.k:
            raise _Reached()


def replay(bits, jr, jd, seed, gamma, beta, bt, k, n_steps):
    """the draws 1 .. k of the exact sweep from `bits` at beta, or None if it takes fewer than k"""
    log = _LogUpTo(k)
    b = list(bits)
    try:
        R.sweep(b, jr, jd, beta, bt, R.pair_sum(b, jr, jd), Stream(seed, gamma), n_steps, log=log)
    except _Reached:
        return list(log)
    return None


def _beta_for(u, eps, ad, bt):
    beta = -math.log(u / (1.0 + eps)) / (ad * bt)
    return beta if (0.0 < beta < 1.0 and beta * bt > FILTER_MIN) else None


def search(bits, jr, jd, seed, gamma, k, n_steps, eps, bt=1.0, prefer=4):
    """-> (beta, log of draws 1 .. k, class of draw k) for the first of |delta| = 4, 8 whose beta is admissible (inside (0, 1), beta bt above
    the filter's limit) and whose replayed k-th draw has that delta; None if neither is"""
    u = uniform_of_draw(seed, gamma, k)
    for ad in (prefer, 12 - prefer):                 # (the delta the caller aimed at first)
        beta = _beta_for(u, eps, ad, bt)
        if beta is None:
            continue
        log = replay(bits, jr, jd, seed, gamma, beta, bt, k, n_steps)
        if log is not None and log[-1][3] == -ad:
            assert log[-1][5] == u
            return beta, log, classify(u, -ad, beta, bt)
    return None


def first_draw(bits, jr, jd):
    """the sweep up to its first draw, which no beta moves: every site with delta >= 0 flips, the first with delta < 0 draws.
    -> (site, delta, S at the draw, S when the sweep entered the site's 32-site word or row) or None if the first step draws nothing"""
    L = int(np.asarray(jr).shape[0])
    jrf = [int(v) for v in np.asarray(jr).ravel()]
    jdf = [int(v) for v in np.asarray(jd).ravel()]
    b, wl = list(bits), (32 if L % 32 == 0 else L)
    S = S_stale = R.pair_sum(b, jr, jd)
    for s in range(L * L):
        if s % wl == 0:
            S_stale = S
        delta = R.site_delta(b, jrf, jdf, L, s)
        if delta < 0:
            return s, delta, S, S_stale
        b[s] ^= 1
        S += delta
    return None


def search_gap(bits, jr, jd, seed, gamma, n_steps, alt, margin, bt=1.0, max_ulps=4000):
    """draw 1 (no earlier decision: its site, delta and S do not move with beta) placed strictly between the exact ratio and what the wrong
    rule `alt` compares with -- "plain threshold": exp(delta beta bt), "stale S": the exact ratio of the pair sum the word was entered with --
    `margin` ulps of u free on each side: beta stepped ulp by ulp around the eps = 0 value, the widest margin kept.
    -> (beta, log, "band", margin in ulps, exact rule rejects) or None"""
    fd = first_draw(bits, jr, jd)
    if fd is None or (alt == "stale S" and fd[2] == fd[3]):
        return None
    site, delta, S, S_stale = fd
    u = uniform_of_draw(seed, gamma, 1)
    beta0 = _beta_for(u, 0.0, -delta, bt)
    if beta0 is None:
        return None
    ulp, best = math.ulp(u), None
    for direction in (math.inf, -math.inf):
        beta = beta0
        for _ in range(max_ulps):
            ratio = math.exp(R.ising_lp(beta, bt, S + delta) - R.ising_lp(beta, bt, S))
            other = (math.exp(delta * (beta * bt)) if alt == "plain threshold" else
                     math.exp(R.ising_lp(beta, bt, S_stale + delta) - R.ising_lp(beta, bt, S_stale)))
            m = min(u - min(other, ratio), max(other, ratio) - u) / ulp
            if m >= margin and ratio < 1 and (best is None or m > best[0]) and classify(u, delta, beta, bt) == "band":
                best = (m, beta, ratio)
            beta = math.nextafter(beta, direction)
    if best is None:
        return None
    m, beta, ratio = best
    log = replay(bits, jr, jd, seed, gamma, beta, bt, 1, n_steps)
    assert log[0][2:5] == (site, delta, S) and log[0][6] == ratio
    return beta, log, "band", m, u > ratio


# ---- coverage bins -------------------------------------------------------------------------------------------------------------------------
def all_bins(log, L, jr, bonds):
    """the coverage bins of every draw of a log that starts at draw 1.  The byte kernels hold draw k at place (k - 1) % 64 of their buffer of
    64 uniforms; the speculative kernels refill at the start of a 16-site chunk that finds more than 48 consumed (spec_ bins)."""
    d = L * L
    p, cnt, chunk, fresh = 0, 0, None, False         # fresh: refilled and nothing consumed since
    res = []
    for (k, step, site, delta, *_rest) in log:
        i, j = divmod(site, L)
        out = {"delta%d" % delta}
        if i == 0:
            out.add("row0")
        if i == L - 1:
            out.add("rowlast")
        if (k - 1) % 64 >= 48:
            out.add("buf48")
        if k > 1 and (k - 1) % 64 == 0:
            out.add("refill")
        if step == 1:
            out.add("step2")
        if L % 32 == 0:
            out.add("quad%d" % ((j % 16) // 4))
            if j % 32 in (0, 15, 16, 31):
                out.add("bit%d" % (j % 32))
            if j % 32 == 31:
                out.add("bit31_last" if j == L - 1 else "bit31_inner")
            ch = (step * d + site) // 16
            if ch != chunk:
                p, cnt, chunk = p + cnt, 0, ch
                if p + 16 > 64:
                    p, fresh = 0, True
            if p + cnt >= 48:
                out.add("spec_buf48")
            if fresh:
                out.add("spec_refill")
            fresh = False
            cnt += 1
        if bonds:
            out.add("leftbond%+d" % int(np.asarray(jr)[i][(j - 1) % L]))
        res.append(out)
    return res


def bins_of(log, L, jr, bonds):
    """the coverage bins of the log's last draw"""
    return all_bins(log, L, jr, bonds)[-1]


def applicable_bins(L, family, n_steps):
    """the bins a shape can fill: word and quad bins on the bit-packed lattices, bit 31 of an inner word from two words per row, the buffer
    bins where a sweep can take 65 draws, the bond bins with bonds"""
    out = {"delta-4", "delta-8", "row0", "rowlast"}
    if n_steps == 2:
        out.add("step2")
    if L % 32 == 0:
        out |= {"quad0", "quad1", "quad2", "quad3", "bit0", "bit15", "bit16", "bit31", "bit31_last", "buf48", "refill", "spec_buf48", "spec_refill"}
        if L > 32:
            out.add("bit31_inner")
    elif family == "ising" and n_steps * L * L > 65:
        out |= {"buf48", "refill"}
    if family == "ea":
        out |= {"leftbond-1", "leftbond+1"}
    return out


# ---- the cases of one shape -----------------------------------------------------------------------------------------------------------------
def ea_bonds(L, seed):
    """SpinGlassLogPotential.edwards_anderson's planes"""
    g = np.random.default_rng(seed)
    return (2 * g.integers(0, 2, size=(L, L)) - 1).astype(np.int8), (2 * g.integers(0, 2, size=(L, L)) - 1).astype(np.int8)


def _stream_with_small_u(g, k, n_scan, floor):
    """a fresh stream; of n_scan candidates the one whose k-th uniform is the smallest above `floor` (a small accept ratio keeps the sweep
    before a late target near the state it started from).  A choice among streams, made before any beta is formed."""
    best, n = None, 0
    while best is None or n < n_scan:
        n += 1
        seed, gamma = int(g.integers(0, 1 << 63)) * 2 + 1, int(g.integers(0, 1 << 63)) * 2 + 1
        u = uniform_of_draw(seed, gamma, k)
        if u > floor and (best is None or u < best[0]):
            best = (u, seed, gamma)
    return best[1], best[2]


def _ising_targets(L, n_steps):
    """(site, step, delta wanted, defects) of the steered Ising cases: an ordered lattice minus `defects` draws once at every other site,
    so the draw at site t is number t + 1 - (defects before t); a defect to the right of t makes its delta -4"""
    d = L * L
    T = [(0, 0, -8, ()), (15, 0, -4, (16,)), (L + 16, 0, -8, ()), (d - 1, 0, -8, ())]
    if L % 32 == 0:
        if L > 32:
            T.append((L + 31, 0, -4, (L + 32,)))
        T += [(52, 0, -4, (53,)), (72, 0, -8, (2, 6, 10, 14, 18, 22, 26, 30)), (64, 0, -4, (65,))]
    else:
        T += [(2, 0, -4, (3,))]
    if n_steps == 2:
        T.append((12, 1, -8, ()))
        if L % 32 != 0 and 2 * d > 65:
            T += [(50 - d, 1, -8, ()), (64 - d, 1, -8, ())]
    return T


def build(L, family, n_steps, seed, bt=1.0):
    """the cases of one shape with fixed seeds.  family "ising": every bond +1, near-ordered states, steered targets; "ea": +-J bonds, random
    or quenched states, targets aimed through a provisional sweep.  L >= 64 Ising: eight "between" cases on ordered states minus three
    defects and four "between stale"; every other shape: four narrow cases (one ulp free), returned apart and never in a ladder.
    tried / discarded count (state, stream, k) triples: one per probe of a target (its eight kinds follow or not), one per gap search.
    -> dict(L, family, n_steps, jr, jd, cases, coverage {class: bins}, tried, discarded, between_margins, stale_margins, narrow);  a case is
    a dict(kind, eps, cls, beta, bits, seed, gamma, k, draw = the logged k-th draw, bins)"""
    g = np.random.default_rng(seed)
    d = L * L
    bonds = family == "ea"
    jr, jd = ea_bonds(L, 1000 + L) if bonds else (np.ones((L, L), dtype=np.int8), np.ones((L, L), dtype=np.int8))
    cases, tried, discarded = [], 0, 0

    def add(bits, sd, gm, k, kind, eps, found):
        beta, log, cls = found[:3]
        cases.append(dict(kind=kind, eps=eps, cls=cls, beta=beta, bits=list(bits), seed=sd, gamma=gm, k=k, draw=log[-1],
                          bins=bins_of(log, L, jr, bonds)))

    def one(bits, sd, gm, k, kind, eps, ok=None, prefer=4):
        found = search(bits, jr, jd, sd, gm, k, n_steps, eps, bt, prefer)
        want = {"band": ("band",), "window": ("window_reject", "window_accept"), "certain": ("certain_reject", "certain_accept")}[kind]
        if found is None or found[2] not in want or (ok is not None and not ok(found[1])):
            return False
        add(bits, sd, gm, k, kind, eps, found)
        return True

    def all_kinds(bits, sd, gm, k, ok, prefer=4):
        """one try of the triple (state, stream, k): the first kind probes it, the other seven follow only if its draw is where `ok` wants
        it (a kind that then misses its class, say a window case across a high-word boundary, is dropped: the triple is kept)"""
        nonlocal tried, discarded
        tried += 1
        if not one(bits, sd, gm, k, *KINDS[0], ok=ok, prefer=prefer):
            discarded += 1
            return False
        for kind, eps in KINDS[1:]:
            one(bits, sd, gm, k, kind, eps, prefer=-cases[-1]["draw"][3])
        return True

    def gap_cases(kind, alt, margin, want, make_state, into):
        """`want` cases of draw 1 between the exact ratio and `alt`'s; make_state() -> bits whose first draw can show the difference
        (chosen from the state alone, before any beta is formed).  One try per (state, stream)."""
        nonlocal tried, discarded
        n = 0
        while n < want and tried < 2000:
            bits = make_state()
            delta = first_draw(bits, jr, jd)[1]
            sd, gm = _stream_with_small_u(g, 1, 1 if margin > 1 else 16, math.exp(delta * 0.98))
            tried += 1
            found = search_gap(bits, jr, jd, sd, gm, n_steps, alt, margin, bt)
            if found is None:
                discarded += 1
                continue
            into.append(dict(kind=kind, eps=0.0, cls="band", beta=found[0], bits=list(bits), seed=sd, gamma=gm, k=1, draw=found[1][-1],
                             bins=bins_of(found[1], L, jr, bonds), rejected=found[4], margin=found[3]))
            n += 1

    def covered(b):
        return all(any(b in c["bins"] for c in cases if c["cls"] == cl) for cl in CLASSES)

    def quenched():
        """a random lattice brought to a local maximum of S (no site with delta > 0): |S| large, so the two log potentials round visibly"""
        bits = [int(v) for v in g.integers(0, 2, size=d)]
        jrf, jdf = [int(v) for v in jr.ravel()], [int(v) for v in jd.ravel()]
        for _ in range(64):
            moved = False
            for s in range(d):
                if R.site_delta(bits, jrf, jdf, L, s) > 0:
                    bits[s] ^= 1
                    moved = True
            if not moved:
                break
        return bits

    def ordered(lead, extra):
        """every spin +1 but `lead` defects from site 0 on (they flip without a draw ahead of draw 1, in its word) and `extra` elsewhere"""
        bits = [1] * d
        for s in list(range(lead)) + [int(v) for v in g.choice(np.arange(3 * L, d - L), size=extra, replace=False)]:
            bits[s] = 0
        return bits

    def stale_state(make):
        """a state of make() whose first draw sees a pair sum that moved since its word was entered"""
        while True:
            bits = make()
            fd = first_draw(bits, jr, jd)
            if fd is not None and fd[2] != fd[3]:
                return bits

    if bonds:
        # the rare bins first: a probe that misses its bin is still kept while its draw fills a bin that some class lacks
        want = applicable_bins(L, family, n_steps)
        rare = ["rowlast", "bit31_inner", "bit31_last", "bit15", "bit16", "bit0", "bit31", "refill", "spec_refill", "spec_buf48", "buf48", "step2"]
        for b in [r for r in rare if r in want] + sorted(want - set(rare)):
            for _ in range(24):
                if covered(b):
                    break
                if b in rare[:7]:
                    # a bin that names a place: many decisions lie ahead of it.  From a quenched lattice at a large beta nearly all of them
                    # reject, whatever the beta, and the draw numbers hardly move.  The stream is chosen (before any beta is formed)
                    # for a draw in the bin whose own beta is large as well
                    bits = quenched()
                    for _ in range(60):
                        sd, gm = _stream_with_small_u(g, 1, 1, 0.0)
                        plog = []
                        R.sweep(list(bits), jr, jd, 0.93, bt, R.pair_sum(bits, jr, jd), Stream(sd, gm), n_steps, log=plog)
                        cand = [e for e, bb in zip(plog, all_bins(plog, L, jr, bonds)) if b in bb and 0.88 < -math.log(e[5]) / (-e[3] * bt) < 0.98]
                        if cand:
                            break
                    if cand:
                        e = min(cand, key=lambda e: abs(-math.log(e[5]) / (-e[3] * bt) - 0.93))
                        all_kinds(bits, sd, gm, e[0], lambda log: any(not covered(x) for x in bins_of(log, L, jr, bonds) & want), prefer=-e[3])
                    continue
                bits = [int(v) for v in g.integers(0, 2, size=d)]
                sd, gm = _stream_with_small_u(g, 1, 1, 0.0)
                # a provisional sweep at beta_p shows which draws sit in the bin; of the first 32 take the one whose own beta is nearest
                # to beta_p, so that the replay at that beta drifts least from what the provisional sweep showed
                plog, beta_p = [], float(g.uniform(0.1, 0.9))
                R.sweep(list(bits), jr, jd, beta_p, bt, R.pair_sum(bits, jr, jd), Stream(sd, gm), n_steps, log=plog)
                cand = [e for e, bb in zip(plog, all_bins(plog, L, jr, bonds)) if b in bb][:32]
                cand = [e for e in cand if e[0] <= 0.97 * len(plog)] or cand         # (a replay may take fewer draws than the provisional sweep)
                if cand:
                    e = min(cand, key=lambda e: abs(-math.log(e[5]) / (-e[3] * bt) - beta_p))
                    all_kinds(bits, sd, gm, e[0], lambda log: any(not covered(x) for x in bins_of(log, L, jr, bonds) & want), prefer=-e[3])
    else:
        for t, step, delta, defects in _ising_targets(L, n_steps):
            for _ in range(8):
                bits = [1] * d
                for s in defects:
                    bits[s] = 0
                k = step * (d - len(defects)) + t + 1 - sum(1 for s in defects if s < t)
                sd, gm = _stream_with_small_u(g, k, k // 2, math.exp(delta * 0.98))
                if all_kinds(bits, sd, gm, k, lambda log: log[-1][1] == step and (step == 1 or (log[-1][2] == t and log[-1][3] == delta)), prefer=-delta):
                    break
        if L >= 64:
            # "between": ordered minus three defects, draw 1 at site 0; and between the exact ratio and the one a pair sum stale by the
            # word's earlier flips would give: one to three defects from site 0 on flip without a draw ahead of draw 1
            gap_cases("between", "plain threshold", BETWEEN_MARGIN, 8, lambda: ordered(0, 3), cases)
            gap_cases("between stale", "stale S", BETWEEN_MARGIN, 4, lambda: ordered(int(g.integers(1, 4)), 2), cases)
    # CPU only (never in a ladder), where no "between" case is built: the same two gaps with ONE ulp free on each side -- the discrimination
    # test's evidence at those shapes; glibc's exp on both sides there, so no slack is needed.  From states whose |S| is large.
    narrow = []
    if bonds or L < 64:
        gap_cases("narrow plain threshold", "plain threshold", 1, 2, quenched if bonds else (lambda: ordered(0, min(3, L - 4))), narrow)
        gap_cases("narrow stale S", "stale S", 1, 2,
                  (lambda: stale_state(quenched)) if bonds else (lambda: ordered(int(g.integers(1, 4)), min(2, L - 4))), narrow)
    margins = [c["margin"] for c in cases if c["kind"] == "between"]
    stale_margins = [c["margin"] for c in cases if c["kind"] == "between stale"]
    coverage = {c: set() for c in CLASSES}
    for c in cases:
        coverage[c["cls"]] |= c["bins"]
    return dict(L=L, family=family, n_steps=n_steps, bt=bt, jr=jr, jd=jd, cases=cases, coverage=coverage, tried=tried, discarded=discarded,
                between_margins=margins, stale_margins=stale_margins, narrow=narrow)


def ladders(shape, seed, max_cases=46):
    """the shape's cases as engine inputs, at most max_cases per ladder: every case is one replica with its own state and stream; the cases'
    betas sorted between 0 and 1 are the schedule and the chain labels go out in that order (ties refused); two more replicas with random
    lattices hold the reference chain and the target chain.  -> [dict(cases, betas, x, chain, rng)]"""
    g = np.random.default_rng(seed)
    d = shape["L"] ** 2
    n_lad = -(-len(shape["cases"]) // max_cases)
    out = []
    for a in range(n_lad):
        cs = shape["cases"][a::n_lad]
        order = np.argsort([c["beta"] for c in cs], kind="stable")
        betas = np.concatenate([[0.0], [cs[i]["beta"] for i in order], [1.0]])
        if not np.all(np.diff(betas) > 0):
            raise ValueError("two cases of one ladder tie in beta")
        N = len(cs) + 2
        chain = np.zeros(N, dtype=np.int64)
        chain[order] = 1 + np.arange(len(cs))
        chain[N - 2], chain[N - 1] = 0, N - 1
        x = np.zeros((N, d))
        rng = np.zeros((N, 2), dtype=np.uint64)
        for s, c in enumerate(cs):
            x[s] = c["bits"]
            rng[s] = (c["seed"], c["gamma"])
        for s in (N - 2, N - 1):
            x[s] = g.integers(0, 2, size=d)
            rng[s] = (int(g.integers(0, 1 << 63)) * 2 + 1, int(g.integers(0, 1 << 63)) * 2 + 1)
        out.append(dict(cases=cs, betas=betas, x=x, chain=chain, rng=rng))
    return out


def coverage_table(shape):
    """the printable table: a row per bin that applies, a column per class"""
    rows = ["%-12s %s" % ("bin", " ".join("%-14s" % c for c in CLASSES))]
    for b in sorted(applicable_bins(shape["L"], shape["family"], shape["n_steps"])):
        rows.append("%-12s %s" % (b, " ".join("%-14s" % ("x" if b in shape["coverage"][c] else ".") for c in CLASSES)))
    return "\n".join(rows)
