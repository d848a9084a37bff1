"""The plane autocorrelation of a lattice pair as far as a machine without a device gets: the kernel's word-level form in Python
integers against the restatement (tests/planes_ref.py), the invariants and the closed forms of the special states, OverlapRecord.chi_sg()
and .correlation_length() on hand-made records, the exports and header declarations, the unit list and the Python refusals."""
import math
import os
import re

import numpy as np
import pytest

import family_cpu as F
import overlap_ref as R
import planes_ref as PR
from family_cpu import P  # noqa: F401  (P: the module's fixture)

CUBES, SQUARES = (2, 4, 6, 10), (32, 64)
GEOMETRIES = [(L, True) for L in CUBES] + [(L, False) for L in SQUARES]
with open(os.path.join(F.ROOT, "pigeons.jl_amd", "csrc", "pte_overlap_planes.hpp")) as _f:
    CS = int(re.search(r"constexpr int PLANES_CS = (\d+);", _f.read()).group(1))      # the planes of a lane's bit-sliced counters


def pack(bits):
    """the HBM row: site s -> bit s & 31 of word s >> 5, padding bits zero"""
    w = [0] * ((len(bits) + 31) // 32)
    for s, v in enumerate(bits):
        if v:
            w[s >> 5] |= 1 << (s & 31)
    return w


def popc(v):
    return bin(v).count("1")


def word_form(a_bits, b_bits, L, cube):
    """k_overlap_planes lane by lane and word by word (pigeons.jl_amd/csrc/pte_overlap_planes.hpp) in Python integers -> C [n_axes][L]: the
    rows of the cube by lattice3d_load_row's funnel shift, the lanes' bit-sliced vertical counters, the staggered hand-over, Q in place of
    the counts, and the outputs r <= L / 2 with their mirrors"""
    M32 = 0xFFFFFFFF
    d = len(a_bits)
    t = [x ^ y for x, y in zip(pack(a_bits), pack(b_bits))]
    NW, n_axes = len(t), 3 if cube else 2
    cnt = [0] * (n_axes * L)
    for lane in range(64):
        cs, col0, n_bits, rows = [0] * CS, 0, 0, 0

        def add(v):
            for i in range(CS):
                cs[i], v = cs[i] ^ v, cs[i] & v
            assert v == 0, "a vertical counter ran over"
        if cube:
            mask, n_bits = M32 >> (32 - L), L
            for r in range(lane, L * L, 64):
                z, y = divmod(r, L)
                o = r * L
                w, sh = o >> 5, o & 31
                hi = t[w + 1] if sh + L > 32 else 0
                row = (((hi << 32) | t[w]) >> sh) & mask
                cnt[L + y] += popc(row)
                cnt[2 * L + z] += popc(row)
                add(row)
                rows += 1
        else:
            W = L >> 5
            stride = (64 // W) * W
            if lane < stride:
                col0, n_bits = (lane % W) << 5, 32
                for w in range(lane, NW, stride):
                    cnt[L + w // W] += popc(t[w])
                    add(t[w])
                    rows += 1
        assert rows <= 32
        for j in range(32):
            p = (lane + j) & 31
            n = sum(((cs[i] >> p) & 1) << i for i in range(CS))
            if p < n_bits and n:
                cnt[col0 + p] += n
    M = d // L
    q = [M - 2 * v for v in cnt]
    H = L >> 1
    C = np.zeros((n_axes, L), dtype=np.int64)
    for o in range(n_axes * (H + 1)):
        axis, r = divmod(o, H + 1)
        s = sum(q[axis * L + p] * q[axis * L + (p + r) % L] for p in range(L))
        assert abs(s) < 2 ** 31
        C[axis, r] += s
        if r != 0 and r != L - r:
            C[axis, L - r] += s
    return C


def _shape(L, cube):
    return R.lattice_shape(L ** 3 if cube else L * L, cube)


@pytest.mark.parametrize("L,cube", GEOMETRIES)
def test_word_form_and_invariants_on_four_densities(L, cube):
    shape = _shape(L, cube)
    d, M = int(np.prod(shape)), int(np.prod(shape)) // L
    g = np.random.default_rng(11 * L + cube)
    for trial in range(4):
        xa, xb = PR.states_of_density(g, 2, d, shape, trial)
        for a, b in zip(xa.astype(np.int64), xb.astype(np.int64)):
            want = PR.plane_corr(a, b, shape)
            assert np.array_equal(word_form(a, b, L, cube), want), trial
            k = int(np.sum(a != b))
            Q = PR.plane_sums(a, b, shape)
            assert Q.shape == (len(shape), L) and np.all(Q.sum(axis=1) == d - 2 * k) and np.all(np.abs(Q) <= M)
            for C in want:
                assert int(C.sum()) == (d - 2 * k) ** 2                               # sum_r C(r) = (sum_p Q[p])^2
                assert all(C[r] == C[(L - r) % L] for r in range(L))                  # C(r) = C(L - r)
                assert np.all(C[0] >= np.abs(C)) and 0 <= C[0] <= L * M * M           # Cauchy-Schwarz; |Q| <= M
    if trial == 3 and L >= 4:
        assert np.abs(Q).max() > M // 2, "the striped state: plane sums near their maximum"


def test_axes_are_the_specification_s(P):
    """one differing PLANE per axis: only that axis sees a Q = -M; the others see every Q lowered by 2 M / L"""
    for L, cube in ((4, True), (32, False)):
        shape = _shape(L, cube)
        d, M, nd = int(np.prod(shape)), int(np.prod(shape)) // L, len(shape)
        a = np.zeros(d, dtype=np.int64)
        for axis in range(nd):
            idx = np.arange(d)
            coord = (idx // L ** axis) % L                                           # axis 0 is the fastest site index
            b = (coord == 1).astype(np.int64)
            Q = PR.plane_sums(a, b, shape)
            for other in range(nd):
                want = [(-M if p == 1 else M) for p in range(L)] if other == axis else [M - 2 * M // L] * L
                assert Q[other].tolist() == want, (L, axis, other)
            assert np.array_equal(word_form(a, b, L, cube), PR.plane_corr(a, b, shape))


@pytest.mark.parametrize("L,cube", GEOMETRIES)
def test_special_states_have_closed_forms(L, cube):
    shape = _shape(L, cube)
    d, M = int(np.prod(shape)), int(np.prod(shape)) // L
    a = np.random.default_rng(L).integers(0, 2, d)
    for b in (a, 1 - a):                                                             # equal copies, the complement: Q = +-M everywhere
        C = PR.plane_corr(a, b, shape)
        assert np.all(C == L * M * M) and np.array_equal(word_form(a, b, L, cube), C)
    for site in (0, d // 2 + 1, d - 1):                                              # one differing site: one Q = M - 2 per axis
        b = a.copy()
        b[site] = 1 - b[site]
        C = PR.plane_corr(a, b, shape)
        assert np.all(C[:, 0] == (L - 1) * M * M + (M - 2) ** 2)
        rest = 2 * M * (M - 2) if L == 2 else (L - 2) * M * M + 2 * M * (M - 2)
        assert np.all(C[:, 1:] == rest)
        assert np.array_equal(word_form(a, b, L, cube), C)


# ---- chi_sg and correlation_length on hand-made records ----------------------------------------------------------------------------------
def _record(P, d, plane_n, plane_corr):
    N = len(plane_n)
    z = np.zeros(N, dtype=np.int64)
    return P.OverlapRecord(np.linspace(0.0, 1.0, N), d, 0, z, np.zeros((N, d + 1), dtype=np.int64), z, z, z, np.asarray(plane_n), np.asarray(plane_corr))


def test_the_record_without_planes(P):
    z = np.zeros(2, dtype=np.int64)
    rec = P.OverlapRecord(np.array([0.0, 1.0]), 8, 24, z, np.zeros((2, 9), dtype=np.int64), z, z, z)    # eight positional arguments, as before
    assert rec.plane_n is None and rec.plane_corr is None and rec.chi_sg() is None and rec.correlation_length() is None
    with_planes = P.OverlapRecord(np.array([0.0, 1.0]), 8, 24, z, np.zeros((2, 9), dtype=np.int64), z, z, z, plane_corr=np.zeros((2, 3, 2)), plane_n=z)
    assert with_planes.plane_n is z and with_planes.plane_corr.shape == (2, 3, 2)


def test_chi_sg_and_correlation_length_on_hand_made_records(P):
    L, n_axes = 16, 3
    d, M = L ** 3, L ** 2
    # chain 0: C(r) = A delta_r0 -> chi flat in m, xi = 0.  chain 1: equal copies at every record -> chi(0) = d, chi(m != 0) = 0 exactly, xi NaN.
    # chain 2: no record -> NaN.  chain 3: chi(0) < chi(k_min) -> xi NaN
    A, n = 7 * d, 5
    delta = np.zeros((n_axes, L), dtype=np.int64); delta[:, 0] = A * n
    equal = np.full((n_axes, L), n * L * M * M, dtype=np.int64)
    rising = np.zeros((n_axes, L), dtype=np.int64); rising[:, 0], rising[:, 1], rising[:, L - 1] = 10 * d, -4 * d, -4 * d
    rec = _record(P, d, [n, n, 0, 1], [delta, equal, np.zeros((n_axes, L), dtype=np.int64), rising])
    for m in range(L):
        chi = rec.chi_sg(m)
        assert chi.shape == (4, n_axes)
        assert chi[0].tolist() == [7.0] * n_axes
        assert chi[1].tolist() == [float(d) if m == 0 else 0.0] * n_axes, m
        assert np.all(np.isnan(chi[2]))
    assert np.array_equal(rec.chi_sg(), rec.chi_sg(1), equal_nan=True) and np.array_equal(rec.chi_sg(L + 1), rec.chi_sg(1), equal_nan=True)
    cl = rec.correlation_length()
    assert sorted(cl) == ["chi0", "chi_kmin", "xi", "xi_over_L"]
    assert cl["xi"][0] == 0.0 and cl["xi_over_L"][0] == 0.0 and cl["chi0"][0] == 7.0 and cl["chi_kmin"][0] == 7.0
    assert cl["chi0"][1] == d and cl["chi_kmin"][1] == 0.0 and np.isnan(cl["xi"][1]) and np.isnan(cl["xi_over_L"][1])
    assert all(np.isnan(cl[k][2]) for k in cl)
    assert cl["chi0"][3] == 2.0 and cl["chi_kmin"][3] > 2.0 and np.isnan(cl["xi"][3])


@pytest.mark.parametrize("L,xi", [(16, 2.7), (32, 1.5), (4, 1.0), (64, 11.0)])
def test_the_estimator_returns_the_xi_of_the_ornstein_zernike_form(P, L, xi):
    """C = the inverse DFT of chi0 / (1 + xi^2 (2 sin(k / 2))^2), scaled by 2^40 and rounded to integers: the estimator is exact for this
    form, so it returns xi up to the rounding -- L 2^-41 against values of 2^40 / L and more, far inside the relative 1e-9 asked here"""
    chi = [1.0 / (1.0 + xi * xi * (2.0 * math.sin(math.pi * m / L)) ** 2) for m in range(L)]
    C = [int(round(2.0 ** 40 / L * math.fsum(chi[m] * math.cos(2.0 * math.pi * m * r / L) for m in range(L)))) for r in range(L)]
    C = [C[min(r, L - r)] for r in range(L)]                                         # the symmetry to the last bit, as the device keeps it
    rec = _record(P, L * L, [1, 3], [[C, C], [[3 * v for v in C]] * 2])
    cl = rec.correlation_length()
    for c in range(2):
        assert abs(cl["xi"][c] - xi) <= 1e-9 * xi, (cl["xi"][c], xi)
        assert cl["xi_over_L"][c] == cl["xi"][c] / L
        assert abs(cl["chi0"][c] / cl["chi_kmin"][c] - 1.0 - xi * xi * (2.0 * math.sin(math.pi / L)) ** 2) < 1e-9
    np.testing.assert_allclose(rec.chi_sg(1)[0], rec.chi_sg(1)[1], rtol=1e-14, atol=0)  # three times the records of three times the sums


# ---- exports, header, units, null handles ---------------------------------------------------------------------------------------------------
NAMES = ["pte_overlap_set_planes", "pte_overlap_planes_info", "pte_overlap_planes_get"]


def test_exports_header_and_units(P):
    import ctypes as C
    import __graft_entry__ as g
    from pigeons_amd import _lib
    L = _lib.load()
    for name in NAMES:
        assert name in _lib.EXPORTS and hasattr(L, name), name
    hdr = F.HEADER
    assert "#define PTE_ABI_VERSION 2\n" in hdr and _lib.ABI_VERSION == 2
    for decl in ("int pte_overlap_set_planes(pte_overlap *ov, int on);",
                 "int pte_overlap_planes_info(const pte_overlap *ov, int64_t *n_axes, int64_t *base_length, int64_t *on);",
                 "int pte_overlap_planes_get(const pte_overlap *ov, int64_t *plane_n, int64_t *plane_corr);"):
        assert decl in hdr, decl
    for name in NAMES:
        assert ":%s" % name in F.JULIA, name
    # a translation unit of its own, in a list of its own, with pte_overlap.hip's flags, and built; the other lists did not grow
    assert g.PLANES_UNITS == [("pte_overlap_planes.hip", dict(g.OVERLAP_UNITS)["pte_overlap.hip"])]
    assert len(g.UNITS) == 8 and all(len(u) == 1 for u in (g.LATTICE_UNITS, g.CHECKERBOARD_UNITS, g.LATTICE3D_UNITS, g.OVERLAP_UNITS, g.CLUSTER_UNITS))
    cmds, link = g._compile_jobs(g.LIB)
    assert sum(cmd[-1].endswith("pte_overlap_planes.hip") for cmd in cmds) == 1 and len(cmds) == 14
    assert any(o.endswith("libpte.pte_overlap_planes.o") for o in link)
    for f in ("pte_overlap_planes.hip", "pte_overlap_planes.hpp", "pte_overlap_planes_params.hpp"):
        assert os.path.exists(os.path.join(g.CSRC, f)), f
    src = open(os.path.join(g.CSRC, "pte_overlap_planes.hpp")).read()
    assert "asm" not in src and "EngineDev" not in src and "__launch_bounds__(64) void k_overlap_planes(" in src
    # null handles are refused, not dereferenced
    assert L.pte_overlap_set_planes(None, 1) == 1 and L.pte_overlap_planes_info(None, None, None, None) == 1
    assert L.pte_overlap_planes_get(None, None, None) == 1
    assert L.pte_overlap_set_planes.argtypes == [C.c_void_p, C.c_int]


# ---- the Python side ----------------------------------------------------------------------------------------------------------------------
def test_python_refusals_come_before_any_device_work(P):
    t3 = P.SpinGlass3DLogPotential.edwards_anderson(0.5, 2, seed=1)
    ok = dict(target=t3, n_chains=4, n_rounds=2, explorer=P.CheckerboardMetropolis(3), show_report=False)
    for target, explorer, L in ((P.SpinGlassLogPotential.edwards_anderson(1.0, 6), P.IsingMetropolis(1), 6), (P.IsingLogPotential(1.0, 48), P.IsingMetropolis(1), 48)):
        with pytest.raises(NotImplementedError, match=r"pigeons_pair: wave_vector=True runs on the cube and on the 2-D lattices whose base_length is a multiple of "
                                                      r"32 \(got base_length %d\)" % L):
            P.pigeons_pair(wave_vector=True, **dict(ok, target=target, explorer=explorer))
    # the pair's own refusals still come first and read as before
    with pytest.raises(ValueError, match=r"seed_b must differ from seed \(both 5\)"):
        P.pigeons_pair(seed_b=5, wave_vector=True, **dict(ok, seed=5))
    with pytest.raises(NotImplementedError, match=r"checkpoint=True is not supported"):
        P.pigeons_pair(wave_vector=True, **dict(ok, checkpoint=True))
    import inspect
    sig = inspect.signature(P.pigeons_pair)
    assert sig.parameters["wave_vector"].default is False and "set_planes" in P.Overlap.__dict__


def test_a_valid_pair_with_the_planes_reaches_the_device_check(P):
    F.no_device()
    for target, explorer in ((P.SpinGlass3DLogPotential.edwards_anderson(0.5, 2, seed=1), P.CheckerboardMetropolis(3)),
                             (P.SpinGlassLogPotential.edwards_anderson(1.0, 32), P.IsingMetropolis(3)),
                             (P.IsingLogPotential(1.0, 32), P.IsingMetropolis(3))):
        with pytest.raises(P.PteError, match="no HIP device"):
            P.pigeons_pair(target=target, n_chains=4, n_rounds=2, explorer=explorer, show_report=False, wave_vector=True)
