"""The inputs of tests/test_gpu_lattice_band.py without a GPU: this test is about the case builder (tests/lattice_band.py), not the kernels.
The builder's stream and thresholds are what they restate; with fixed seeds it fills every coverage bin that applies to a shape in each of
the five decision classes and yields the "between" cases, discarding at most half of what it tries; the case list would catch each of four
wrong in-band rules in every shape; and the sign of eps decides the targeted draw."""
import functools
import math
import struct

import numpy as np
import pytest

import lattice_band as B
import oracle as O
import spinglass_ref as R

SEED = 12                        # tests/test_gpu_lattice_band.py builds with the same seed
SHAPES = [("ising", 6), ("ising", 32), ("ising", 64), ("ising", 96), ("ea", 5), ("ea", 32), ("ea", 64)]       # all at beta_target = 1


@functools.lru_cache(maxsize=None)
def _shape(family, L, n_steps=2):
    return B.build(L, family, n_steps, seed=SEED)


def _final(case, sh, rule=B.exact_rule, sweep=None, n_steps=None):
    """(final bits, stream position) of one case's replica under the banded restatement with `rule` in the band, or under `sweep`"""
    n_steps = sh["n_steps"] if n_steps is None else n_steps
    b = list(case["bits"])
    g = B.Stream(case["seed"], case["gamma"])
    S = R.pair_sum(b, sh["jr"], sh["jd"])
    if sweep is None:
        S = B.banded_sweep(b, sh["jr"], sh["jd"], case["beta"], sh["bt"], S, g, n_steps, rule)
    else:
        S = sweep(b, sh["jr"], sh["jd"], case["beta"], sh["bt"], S, g, n_steps)
    assert S == R.pair_sum(b, sh["jr"], sh["jd"])
    return b, g.state


def test_stream_is_the_oracles_generator():
    for seed, gamma in ((1, 0x9e3779b97f4a7c15), (0xdeadbeefcafef00d, 0xbf58476d1ce4e5b9)):
        a, b = B.Stream(seed, gamma), O.OracleRng(state=(seed, gamma))
        for k in range(1, 200):
            assert a.rand() == b.rand() == B.uniform_of_draw(seed, gamma, k)
        assert a.state == b.state


def _double_of(bits):
    return struct.unpack("<d", struct.pack("<Q", bits))[0]


def test_thresholds_and_classes_from_the_bit_patterns():
    """the four doubles are ordered, their high words are the patterns' upper halves, and classify is the ladder the kernels walk: a u whose
    high word is outside [lo_h, hi_h] is certain, one inside is window or band by the full patterns, below the filter's limit all is band"""
    for beta in (1e-12, 3e-7, 0.013, 0.4406867935097715, 0.97):
        th = B.thresholds(beta * 1.0)
        for n, ad in (("r4", 4), ("r8", 8)):
            lo, hi, r = th[n + "lo"], th[n + "hi"], math.exp(-ad * beta)
            assert lo < r < hi and th[n + "lo_b"] < B.pattern(r) < th[n + "hi_b"]
            assert th[n + "lo_h"] == B.pattern(lo) >> 32 and th[n + "hi_h"] == B.pattern(hi) >> 32
            assert B.classify(r, -ad, beta, 1.0) == "band" and B.classify(lo, -ad, beta, 1.0) == "band" and B.classify(hi, -ad, beta, 1.0) == "band"
            assert B.classify(math.nextafter(hi, 2.0), -ad, beta, 1.0) in ("window_reject", "certain_reject")
            assert B.classify(math.nextafter(lo, 0.0), -ad, beta, 1.0) in ("window_accept", "certain_accept")
            assert B.classify(r * (1 + 2.0 ** -19), -ad, beta, 1.0) == "certain_reject"
            assert B.classify(r * (1 - 2.0 ** -19), -ad, beta, 1.0) == "certain_accept"
            # the window's ends from the patterns: the first u with the next high word is certain, the last with this one is not
            edge = _double_of((th[n + "hi_h"] + 1) << 32)
            assert B.classify(edge, -ad, beta, 1.0) == "certain_reject"
            assert B.classify(math.nextafter(edge, 0.0), -ad, beta, 1.0) in ("window_reject", "band")
    assert B.classify(0.5, -4, 1e-14, 1.0) == "band" and not B.thresholds(1e-13)["filter_ok"] and B.thresholds(1.0000001e-13)["filter_ok"]


def test_search_refuses_inadmissible_betas_and_ladders_refuse_ties():
    L = 6
    ones = np.ones((L, L), dtype=np.int8)
    bits = [1] * (L * L)
    # an ordered lattice: draw 1 is site 0 with delta = -8; a stream whose first uniform is below exp(-8) has no beta inside (0, 1)
    g = np.random.default_rng(0)
    while True:
        sd, gm = int(g.integers(0, 1 << 63)) * 2 + 1, int(g.integers(0, 1 << 63)) * 2 + 1
        if B.uniform_of_draw(sd, gm, 1) < math.exp(-8.0):
            break
    assert B.search(bits, ones, ones, sd, gm, 1, 1, 0.0) is None
    assert B._beta_for(1.0 - 1e-14, 0.0, 4, 1.0) is None and B._beta_for(0.5, 0.0, 4, 1.0) == math.log(2.0) / 4
    sh = dict(_shape("ising", 6))
    sh["cases"] = [sh["cases"][0], dict(sh["cases"][0])]
    with pytest.raises(ValueError, match="tie in beta"):
        B.ladders(sh, seed=1)


@pytest.mark.parametrize("n_steps", [1, 2])          # both step counts that tests/test_gpu_lattice_band.py builds
@pytest.mark.parametrize("family,L", SHAPES)
def test_builder_fills_every_bin_in_every_class_within_the_cap(family, L, n_steps):
    """the cap: of the (state, stream, k) triples the builder tries -- one per probe of a target, one per "between" or narrow search -- at
    most half are discarded"""
    sh = _shape(family, L, n_steps)
    print("\n%s L = %d, n_steps = %d: %d cases" % (family, L, n_steps, len(sh["cases"])))
    print(B.coverage_table(sh))
    share = sh["discarded"] / sh["tried"]
    print("discarded %d of %d (state, stream, k) triples tried (%.1f %%), the narrow CPU-only searches included" % (sh["discarded"], sh["tried"], 100 * share))
    if sh["between_margins"]:
        print("between margins (ulps of u): %s, smallest %.0f" % (" ".join("%.0f" % m for m in sorted(sh["between_margins"])), min(sh["between_margins"])))
        print("between (stale S) margins: %s" % " ".join("%.0f" % m for m in sorted(sh["stale_margins"])))
    want = B.applicable_bins(L, family, n_steps)
    for cls in B.CLASSES:
        assert not (want - sh["coverage"][cls]), "%s misses %s" % (cls, sorted(want - sh["coverage"][cls]))
    assert share <= 0.5
    if family == "ising" and L >= 64:
        between = [c for c in sh["cases"] if c["kind"] == "between"]
        assert len(between) >= 8 and min(sh["between_margins"]) >= B.BETWEEN_MARGIN
        for c in between:                            # strictly between the exact ratio and the plain threshold, 16 ulps free on each side
            _, _, _, delta, S, u, ratio, rejected = c["draw"]
            plain = math.exp(delta * c["beta"])
            assert ratio == math.exp(R.ising_lp(c["beta"], 1.0, S + delta) - R.ising_lp(c["beta"], 1.0, S)) and S > 2 * L * L - 40
            assert min(plain, ratio) + 16 * math.ulp(u) <= u <= max(plain, ratio) - 16 * math.ulp(u)
            assert rejected == (u > ratio) != (u > plain)
        stale = [c for c in sh["cases"] if c["kind"] == "between stale"]
        assert len(stale) >= 4 and min(sh["stale_margins"]) >= B.BETWEEN_MARGIN
        for c in stale:                              # 16 ulps from the exact ratio (and from the stale one) as well
            assert abs(c["draw"][5] - c["draw"][6]) >= 16 * math.ulp(c["draw"][5]) and c["cls"] == "band"
    # every case is what its kind says, from the bit patterns of its own thresholds
    for c in sh["cases"]:
        _, _, _, delta, _, u, _, _ = c["draw"]
        th = B.thresholds(c["beta"] * 1.0)
        n = "r4" if delta == -4 else "r8"
        assert 0.0 < c["beta"] < 1.0 and th["filter_ok"] and c["cls"] == B.classify(u, delta, c["beta"], 1.0)
        ub = B.pattern(u)
        if c["kind"] in ("band", "between", "between stale"):
            assert th[n + "lo_b"] <= ub <= th[n + "hi_b"]
        elif c["kind"] == "window":
            assert th[n + "lo_h"] <= ub >> 32 <= th[n + "hi_h"] and not th[n + "lo_b"] <= ub <= th[n + "hi_b"]
        else:
            assert not th[n + "lo_h"] <= ub >> 32 <= th[n + "hi_h"]
    for lad in B.ladders(sh, seed=SEED):
        assert len(lad["chain"]) <= 48 and sorted(lad["chain"]) == list(range(len(lad["chain"])))
        for s, c in enumerate(lad["cases"]):
            assert lad["betas"][lad["chain"][s]] == c["beta"]


@pytest.mark.parametrize("family,L", SHAPES)
def test_sign_of_eps_decides_the_targeted_draw(family, L):
    """eps > 0 inside the band: the exact rule rejects the targeted draw; eps < 0: it accepts; the two final lattices of a (state, stream, k)
    differ at the targeted site when the step that holds the draw ends (the next step sweeps the site again, and in an ordered lattice flips
    it back).  The banded restatement with the exact rule is the plain restatement on these replicas."""
    sh = _shape(family, L)
    band = [c for c in sh["cases"] if c["kind"] == "band"]
    pairs = {}
    for c in band:
        assert c["draw"][7] == (c["eps"] > 0), "eps %+.1e" % c["eps"]
        pairs.setdefault((c["seed"], c["k"], abs(c["eps"])), {})[c["eps"] > 0] = c
    full = [p for p in pairs.values() if len(p) == 2]
    assert full and len(full) == len(pairs)          # every in-band case has its twin of the other sign
    for p in full:
        site = p[True]["draw"][2]
        assert p[False]["draw"][2] == site and p[False]["draw"][1] == p[True]["draw"][1]
        n = p[True]["draw"][1] + 1
        (b_rej, g_rej), (b_acc, _) = _final(p[True], sh, n_steps=n), _final(p[False], sh, n_steps=n)
        assert b_rej[site] != b_acc[site]
        assert _final(p[True], sh, sweep=R.sweep, n_steps=n) == (b_rej, g_rej)


@pytest.mark.parametrize("family,L", SHAPES)
def test_each_wrong_in_band_rule_changes_a_case(family, L):
    """the banded restatement with its in-band rule replaced by the plain threshold, always accept, always reject, and the exact ratio with
    S stale by the sweep so far in the word: each changes the final bits or the stream position of at least one replica of the shape.  The
    ladder cases catch the two constant rules everywhere, the plain threshold and the stale S where "between" cases exist (Ising, L = 64 and
    96); the narrow cases (one ulp free, CPU only) are the evidence for those two at the other shapes."""
    sh = _shape(family, L)
    band = [c for c in sh["cases"] if c["cls"] == "band"]
    between = [c for c in band if c["kind"] == "between"]
    for name, rule in B.WRONG_RULES.items():
        pool = {"plain threshold": between[:3] + [c for c in sh["narrow"] if c["kind"] == "narrow plain threshold"],
                "stale S": [c for c in band if c["kind"] == "between stale"] + [c for c in sh["narrow"] if c["kind"] == "narrow stale S"],
                "always accept": [c for c in band if c["kind"] == "band" and c["eps"] > 0][:2],
                "always reject": [c for c in band if c["kind"] == "band" and c["eps"] < 0][:2]}[name]
        caught = [c for c in pool if _final(c, sh, rule) != _final(c, sh)]
        in_ladder = [c for c in caught if not c["kind"].startswith("narrow")]
        print("%s L = %d: %-15s caught by %d ladder case(s) and %d narrow CPU-only case(s) of %d replicas tried%s"
              % (family, L, name, len(in_ladder), len(caught) - len(in_ladder), len(pool),
                 "" if in_ladder else " -- NOT held by the GPU test at this shape"))
        assert caught, name
        if name == "plain threshold" and between:
            assert all(c in caught for c in between[:3])            # every "between" case on its own catches the plain threshold
        if name == "stale S":                                       # and every "between stale" case the stale pair sum
            assert all(c in caught for c in band if c["kind"] == "between stale")
