"""The replica-overlap recorder as far as a machine without a device gets: the XOR-shift identity the kernel rests on and its
word-level form against the restatement (tests/overlap_ref.py), OverlapRecord.moments() on hand-made histograms, the exports and header
declarations, the Python refusals, and adapt_pair over two engines that record their calls."""
import math
import os

import numpy as np
import pytest

import family_cpu as F
import overlap_ref as R
from family_cpu import P, RecordingEngine  # noqa: F401  (P: the module's fixture)

CUBES, SQUARES = (2, 4, 6, 10), (2, 6, 32, 64)
GEOMETRIES = [(L, True) for L in CUBES] + [(L, False) for L in SQUARES]


def xor_shift(a_bits, b_bits, shape):
    """k = popcount(t), kl = sum_dir popcount(t xor shift_dir(t)), t = a xor b: the form the device computes"""
    t = (np.asarray(a_bits).astype(np.int64) ^ np.asarray(b_bits).astype(np.int64)).reshape(shape)
    return int(t.sum()), sum(int(np.sum(t ^ np.roll(t, -1, axis=ax))) for ax in range(len(shape)))


def pack(bits):
    """the HBM row: site s -> bit s & 31 of word s >> 5, padding bits zero"""
    w = np.zeros((len(bits) + 31) // 32, dtype=np.uint64)
    for s, v in enumerate(bits):
        if v:
            w[s >> 5] |= np.uint64(1) << np.uint64(s & 31)
    return [int(v) for v in w]


def popc(v):
    return bin(v).count("1")


def word_form(a_bits, b_bits, L, cube):
    """k_overlap word by word (pigeons.jl_amd/csrc/pte_overlap.hpp) in Python integers: the rows of the cube by lattice3d_load_row's funnel
    shift, the rows of the square (L % 32 == 0) by the funnel shift across their words"""
    M = 0xFFFFFFFF
    t = [x ^ y for x, y in zip(pack(a_bits), pack(b_bits))]
    k, kl = sum(popc(v) for v in t), 0
    if cube:
        mask = M >> (32 - L)

        def row(r):
            o = r * L
            w, sh = o >> 5, o & 31
            hi = t[w + 1] if sh + L > 32 else 0
            return (((hi << 32) | t[w]) >> sh) & mask
        for r in range(L * L):
            z, y = divmod(r, L)
            cur = row(r)
            rt = ((cur >> 1) | (cur << (L - 1))) & mask
            kl += popc(cur ^ rt) + popc(cur ^ row(z * L + (y + 1) % L)) + popc(cur ^ row(((z + 1) % L) * L + y))
    else:
        W = L // 32
        for w in range(len(t)):
            i, j = divmod(w, W)
            cur, nx, dn = t[w], t[i * W + (j + 1) % W], t[((i + 1) % L) * W + j]
            kl += popc(cur ^ ((cur >> 1) | (nx << 31)) & M) + popc(cur ^ dn)
    return k, kl


@pytest.mark.parametrize("L,cube", GEOMETRIES)
def test_xor_shift_identity_on_random_lattices(L, cube):
    d = L ** 3 if cube else L * L
    shape = R.lattice_shape(d, cube)
    g = np.random.default_rng(7 * L + cube)
    for trial in range(4):
        a = g.integers(0, 2, d)
        b = a ^ (g.random(d) < (0.5, 0.1, 0.9, 0.02)[trial])          # every density of differing sites
        want = R.k_and_kl(a, b, shape)
        assert xor_shift(a, b, shape) == want
        if cube or L % 32 == 0:
            assert word_form(a, b, L, cube) == want
        assert 0 <= want[0] <= d and 0 <= want[1] <= len(shape) * d


@pytest.mark.parametrize("L,cube", GEOMETRIES)
def test_single_site_and_complement(L, cube):
    d = L ** 3 if cube else L * L
    shape = R.lattice_shape(d, cube)
    a = np.random.default_rng(L).integers(0, 2, d)
    assert R.k_and_kl(a, a, shape) == (0, 0) == xor_shift(a, a, shape)
    assert R.k_and_kl(a, 1 - a, shape) == (d, 0) == xor_shift(a, 1 - a, shape)
    for site in (0, d // 2, d - 1):
        b = a.copy(); b[site] ^= 1
        want = (1, 6 if cube else 4)                                    # L = 2 included: the doubled bonds are two terms each
        assert R.k_and_kl(a, b, shape) == want == xor_shift(a, b, shape)
        if cube or L % 32 == 0:
            assert word_form(a, b, L, cube) == want


def _record(P, hist, n_links=0, link=None):
    hist = np.asarray(hist, dtype=np.int64)
    N, d = hist.shape[0], hist.shape[1] - 1
    z = np.zeros(N, dtype=np.int64)
    ln, ls, ls2 = link if link is not None else (z, z, z)
    return P.OverlapRecord(np.linspace(0.0, 1.0, N), d, n_links, hist.sum(axis=1), hist, np.asarray(ln), np.asarray(ls), np.asarray(ls2))


def test_moments_on_hand_made_histograms(P):
    d = 8
    frozen = np.zeros(d + 1, dtype=np.int64); frozen[0] = 17                                  # all mass at k = 0: q = 1
    binom = np.array([math.comb(d, k) for k in range(d + 1)], dtype=np.int64)               # the exact Binomial(8, 1/2) table: two i.i.d. copies
    anti = np.zeros(d + 1, dtype=np.int64); anti[d] = 3                                       # q = -1
    rec = _record(P, [frozen, binom, anti, np.zeros(d + 1, dtype=np.int64)])
    assert np.array_equal(rec.q_values(), 1.0 - 2.0 * np.arange(9) / 8.0) and rec.q_values()[0] == 1.0 and rec.q_values()[-1] == -1.0
    m = rec.moments()
    assert m["q2"][0] == 1.0 and m["q4"][0] == 1.0 and m["binder"][0] == 1.0 and m["q_abs"][0] == 1.0
    assert m["q2"][1] == 1.0 / 8.0
    # <q^4> of the mean of d = 8 fair +-1: (3 d^2 - 2 d) / d^4
    assert abs(m["q4"][1] - (3 * 64 - 16) / 8.0 ** 4) < 1e-15 and abs(m["binder"][1] - 0.5 * (3 - (176 / 4096.0) * 64)) < 1e-13
    assert m["q_abs"][2] == 1.0 and m["q2"][2] == 1.0 and m["binder"][2] == 1.0
    assert all(np.isnan(m[k][3]) for k in ("q_abs", "q2", "q4", "binder"))                    # no record: NaN, not a number made up
    assert m["ql"] is None and m["ql_var"] is None
    # link moments: kl in {0, 6, 6, 12} of 24 bonds -> q_l in {1, .5, .5, 0}: mean 0.5, variance 0.125; a chain without records is NaN
    link = (np.array([4, 0, 4, 4]), np.array([24, 0, 0, 4 * 24]), np.array([216, 0, 0, 4 * 576]))
    ml = _record(P, [frozen, binom, anti, frozen], n_links=24, link=link).moments()
    assert ml["ql"][0] == 0.5 and ml["ql_var"][0] == 0.125 and np.isnan(ml["ql"][1]) and np.isnan(ml["ql_var"][1])
    assert ml["ql"][2] == 1.0 and ml["ql_var"][2] == 0.0 and ml["ql"][3] == -1.0 and ml["ql_var"][3] == 0.0


NAMES = ["pte_overlap_create", "pte_overlap_destroy", "pte_overlap_info", "pte_overlap_record", "pte_overlap_run_scans", "pte_overlap_reduce",
         "pte_overlap_get"]


def test_exports_header_and_units(P):
    import ctypes as C
    import __graft_entry__ as g
    from pigeons_amd import _lib
    L = _lib.load()
    for name in NAMES:
        assert name in _lib.EXPORTS and hasattr(L, name), name
    hdr = F.HEADER
    assert "#define PTE_ABI_VERSION 2\n" in hdr and _lib.ABI_VERSION == 2
    for decl in ("typedef struct pte_overlap pte_overlap;",
                 "int pte_overlap_create(pte_engine *a, pte_engine *b, pte_overlap **out);",
                 "int pte_overlap_destroy(pte_overlap *ov);",
                 "int pte_overlap_info(const pte_overlap *ov, int64_t *n_chains, int64_t *dim, int64_t *n_links);",
                 "int pte_overlap_record(pte_overlap *ov);",
                 "int pte_overlap_run_scans(pte_overlap *ov, int64_t first_scan, int64_t n_scans);",
                 "int pte_overlap_reduce(pte_overlap *ov);",
                 "int pte_overlap_get(const pte_overlap *ov, int64_t *n, int64_t *hist, int64_t *link_n, int64_t *link_sum, int64_t *link_sum2);"):
        assert decl in hdr, decl
    for name in NAMES:
        assert ":%s" % name in F.JULIA, name
    assert "mutable struct DeviceOverlap" in F.JULIA
    # a translation unit of its own, in a list of its own, with pte_lattice3d.hip's flags; the other lists did not grow
    assert g.OVERLAP_UNITS == [("pte_overlap.hip", dict(g.LATTICE3D_UNITS)["pte_lattice3d.hip"])]
    assert len(g.UNITS) == 8 and all(len(u) == 1 for u in (g.LATTICE_UNITS, g.CHECKERBOARD_UNITS, g.LATTICE3D_UNITS))
    for f in ("pte_overlap.hip", "pte_overlap.hpp", "pte_overlap_params.hpp"):
        assert os.path.exists(os.path.join(g.CSRC, f)), f
    # null handles are refused, not dereferenced; create's message names what it got
    out = C.c_void_p()
    assert L.pte_overlap_create(None, None, C.byref(out)) == 1 and out.value is None
    assert "pte_overlap_create: null argument" in L.pte_last_error(None).decode()
    assert L.pte_overlap_record(None) == 1 and L.pte_overlap_run_scans(None, 1, 1) == 1 and L.pte_overlap_reduce(None) == 1
    assert L.pte_overlap_info(None, None, None, None) == 1 and L.pte_overlap_get(None, None, None, None, None, None) == 1
    assert L.pte_overlap_destroy(None) == 0
    for name in ("Overlap", "OverlapRecord", "PTPair", "pigeons_pair", "adapt_pair"):
        assert name in P.__dict__, name


def test_python_refusals_come_before_any_device_work(P):
    t3 = P.SpinGlass3DLogPotential.edwards_anderson(0.5, 2, seed=1)
    ok = dict(target=t3, n_chains=4, n_rounds=2, explorer=P.CheckerboardMetropolis(3), show_report=False)
    with pytest.raises(NotImplementedError, match=r"pigeons_pair: the overlap is recorded on the lattice targets \(IsingLogPotential, SpinGlassLogPotential, "
                                                  r"SpinGlass3DLogPotential\); got "):
        P.pigeons_pair(target=P.toy_mvn_target(4), n_chains=4, n_rounds=2, show_report=False)
    with pytest.raises(NotImplementedError, match=r"n_chains_variational must be 0 \(got 3\)"):
        P.pigeons_pair(**dict(ok, n_chains_variational=3))
    for kw, named in ((dict(n_shards=2), "n_shards"), (dict(rank=1, world=2), "rank, world"), (dict(transport="group"), "transport")):
        with pytest.raises(NotImplementedError, match=r"sharded or multi-GPU pairs are not supported \(got %s\)" % named):
            P.pigeons_pair(**dict(ok, **kw))
    with pytest.raises(NotImplementedError, match=r"checkpoint=True is not supported"):
        P.pigeons_pair(**dict(ok, checkpoint=True))
    with pytest.raises(ValueError, match=r"seed_b must differ from seed \(both 5\): identical runs give q = 1"):
        P.pigeons_pair(seed_b=5, **dict(ok, seed=5))


def test_a_valid_pair_reaches_the_device_check(P):
    F.no_device()
    for target, explorer in ((P.SpinGlass3DLogPotential.edwards_anderson(0.5, 2, seed=1), P.CheckerboardMetropolis(3)),
                             (P.SpinGlassLogPotential.edwards_anderson(1.0, 32), P.IsingMetropolis(3)),
                             (P.IsingLogPotential(1.0, 32), P.IsingMetropolis(3))):
        with pytest.raises(P.PteError, match="no HIP device"):
            P.pigeons_pair(target=target, n_chains=4, n_rounds=2, explorer=explorer, show_report=False)


def test_adapt_pair_gives_both_runs_one_schedule(P):
    from pigeons_amd import overlap as OV
    from pigeons_amd import tempering as T
    from pigeons_amd.pt import ReducedRecorders
    N = 6
    t = P.SpinGlass3DLogPotential.edwards_anderson(0.5, 2, seed=1)
    pts = [P.PT(P.Inputs(target=t, n_chains=N, n_rounds=3, seed=s, explorer=P.CheckerboardMetropolis(3), show_report=False),
                engine_factory=RecordingEngine) for s in (1, 2)]
    pair = P.PTPair(*pts)
    g = np.random.default_rng(3)
    old = pts[0].shared.tempering.schedule.grids.copy()
    for rnd in range(2):
        reds = []
        for _ in pts:
            n = np.full(N - 1, 8, dtype=np.int64)
            n[2] = 0 if rnd == 0 else 8                                   # an absent key: rejection 0.5
            reds.append(ReducedRecorders(swap_acceptance_pr=(g.uniform(0.2, 0.9, N - 1), n)))
        assert OV.adapt_pair(pair, *reds) is pair
        rej = 0.5 * (T.rejections(*reds[0].swap_acceptance_pr) + T.rejections(*reds[1].swap_acceptance_pr))
        want = T.optimal_schedule(rej, old, N)
        ga, gb = (pt.replicas.calls["set_schedule"][-1][0] for pt in pts)
        assert len(pts[0].replicas.calls["set_schedule"]) == rnd + 1 == len(pts[1].replicas.calls["set_schedule"])
        assert ga.tobytes() == gb.tobytes() == want.tobytes()            # bit-identical grids, those of the averaged rejections
        for pt, red in zip(pts, reds):
            assert pt.shared.tempering.schedule.grids.tobytes() == want.tobytes() and pt.reduced_recorders is red
            assert pt.shared.tempering.communication_barriers.globalbarrier == T.CommunicationBarriers(rej, old).globalbarrier
        ba, bb = (pt.shared.tempering.communication_barriers for pt in pts)
        assert ba.globalbarrier == bb.globalbarrier and all(ba.localbarrier(x) == bb.localbarrier(x) for x in (0.0, 0.3, 0.77, 1.0))
        old = want
    assert not np.array_equal(old, np.linspace(0, 1, N))
