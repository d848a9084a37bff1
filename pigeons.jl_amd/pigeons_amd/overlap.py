"""The replica overlap between two runs of a lattice family (the project's own specification -- the reference has no such recorder).

Two PTs over the same target and inputs, with different seeds, hold two independent copies of the system at every temperature.  Per chain c
and per scan the device adds, as exact integers, the site overlap k = #{i : s_i^a != s_i^b} (q = 1 - 2 k / d) to a histogram and the link
overlap kl = #{bonds (i, j) : s_i^a s_j^a != s_i^b s_j^b} (q_l = 1 - 2 kl / n_links) to a sum and a sum of squares: P(q), its moments and
the Binder ratio, which tell the glassy phase from the paramagnet where the magnetisation cannot (it vanishes by gauge symmetry).

  Overlap(eng_a, eng_b)      the ctypes wrapper of pte_overlap_* (include/pte.h)
  OverlapRecord              the reduced accumulators of one round and what is computed from them
  pigeons_pair(...) -> PTPair   the round loop: the two engines kept in step scan by scan, their ladders kept equal round by round

Two copies at one temperature also admit Houdayer's cluster move (Houdayer 2001; with parallel tempering the isoenergetic cluster
move of Zhu, Ochoa and Katzgraber 2015): the connected cluster of disagreeing sites around a drawn one is flipped in both copies, which
leaves the sum of the two energies as it was -- always accepted, and non-local where single-spin flips are frozen.  Off unless asked for.

  HoudayerMove(every, min_beta, seed)   the setting: Overlap.set_cluster_move(move), pigeons_pair(cluster_move=move)
  ClusterRecord                         the reduced accumulators of the move

The scalar overlap is the k = 0 term of the quantity a spin-glass study is built around, the wave-vector-dependent susceptibility
chi_SG(k) = (1 / d) <|sum_i q_i exp(i k . x_i)|^2>, q_i = s_i^a s_i^b, and the finite-size correlation length xi_L derived from it, whose
ratio xi_L / L crosses at the transition.  For k along a lattice axis both follow from the autocorrelation of the plane sums
of q, which the device adds up per chain and per record as exact integers.  Off unless asked for.

  Overlap.set_planes(on), pigeons_pair(wave_vector=True)   the switch
  OverlapRecord.plane_n, .plane_corr                       the reduced accumulators (None when the feature is off)
  OverlapRecord.chi_sg(m), .correlation_length()           chi_SG(2 pi m / L) per chain and axis; xi_L, xi_L / L per chain
"""
import ctypes as C
import dataclasses
import math
import time
from dataclasses import InitVar, dataclass
from typing import Any

import numpy as np

from . import tempering as T
from ._lib import PteError
from .engine import _ip
from .pt import (PT, Inputs, IsingLogPotential, NonReversiblePT, SpinGlass3DLogPotential, SpinGlassLogPotential, adapt_explorer,
                 n_scans_in_round, next_round, reduce_recorders, report)

LATTICE_TARGETS = (IsingLogPotential, SpinGlassLogPotential, SpinGlass3DLogPotential)
SHARDING_ARGUMENTS = ("n_shards", "rank", "world", "dist_device", "device_messages", "transport", "comm_id")


@dataclass
class OverlapRecord:
    """The accumulators of one pte_overlap_reduce, all int64 and keyed by chain, and the schedule in force while they were recorded."""
    betas: Any          # float64 [N]
    dim: int            # d, the number of sites
    n_links: int        # bonds of the lattice the link overlap runs over; 0 = no link overlap recorded (2-D lattices with base_length % 32 != 0)
    n: Any              # [N]        records
    hist: Any           # [N][d + 1] records with k differing sites
    link_n: Any         # [N]        records with a link overlap
    link_sum: Any       # [N]        sum of kl
    link_sum2: Any      # [N]        sum of kl^2
    # the plane autocorrelation, None unless the feature was on.  Init-only: they are set as attributes of the same names, and
    # dataclasses.fields() stays the eight accumulators of 4.20 that code written against it enumerates
    plane_n: InitVar[Any] = None       # [N]              records taken with the feature on
    plane_corr: InitVar[Any] = None    # [N][n_axes][L]   sum over those records of C_axis(r) = sum_p Q_axis[p] Q_axis[(p + r) mod L]

    def __post_init__(self, plane_n, plane_corr):
        self.plane_n, self.plane_corr = plane_n, plane_corr

    def chi_sg(self, m=1):
        """chi_SG at the wave vector 2 pi m / L along every axis, float64 [N][n_axes]:  (1 / (d plane_n)) sum_r plane_corr[c][axis][r]
        cos(2 pi m r / L), from Python integers (the sine part vanishes: C(r) = C(L - r)); chi_sg(0) = d <q^2> on every axis.  None when
        the plane sums were not recorded; NaN where a chain has no record."""
        if self.plane_corr is None:
            return None
        corr = np.asarray(self.plane_corr)
        N, n_axes, L = corr.shape
        w = [_cos_turn((int(m) * r) % L, L) for r in range(L)]
        out = np.full((N, n_axes), np.nan)
        for c in range(N):
            n = int(self.plane_n[c])
            if n <= 0:
                continue
            for ax in range(n_axes):
                vals = [int(v) for v in corr[c, ax]]
                num = float(sum(vals)) if int(m) % L == 0 else math.fsum(v * wr for v, wr in zip(vals, w))
                out[c, ax] = num / (float(self.dim) * n)
        return out

    def correlation_length(self):
        """per chain, float64 [N]: chi0 = chi_SG(0), chi_kmin = the mean over the axes of chi_SG(k_min), k_min = 2 pi / L,
        xi = sqrt(chi0 / chi_kmin - 1) / (2 sin(k_min / 2)) and xi_over_L.  xi is NaN where chi_kmin <= 0, where chi0 / chi_kmin < 1 and
        where a chain has no record.  None when the plane sums were not recorded."""
        if self.plane_corr is None:
            return None
        L = np.asarray(self.plane_corr).shape[2]
        chi0, chi_kmin = self.chi_sg(0).mean(axis=1), self.chi_sg(1).mean(axis=1)
        xi = np.full(len(chi0), np.nan)
        for c in range(len(chi0)):
            if chi_kmin[c] > 0.0 and chi0[c] / chi_kmin[c] >= 1.0:
                xi[c] = math.sqrt(chi0[c] / chi_kmin[c] - 1.0) / (2.0 * math.sin(math.pi / L))
        return dict(xi=xi, xi_over_L=xi / L, chi0=chi0, chi_kmin=chi_kmin)

    def q_values(self):
        """q of every bin: 1 - 2 k / d, k = 0 .. d"""
        return 1.0 - 2.0 * np.arange(self.dim + 1, dtype=np.float64) / float(self.dim)

    def moments(self):
        """per chain, from the integers in float64: q_abs = <|q|>, q2 = <q^2>, q4 = <q^4>, binder = (3 - q4 / q2^2) / 2, ql = <q_l> and ql_var
        (the last two None where no link overlap is recorded); NaN where a chain has no record"""
        q = self.q_values()
        h = np.asarray(self.hist, dtype=np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            tot = h.sum(axis=1)
            q_abs, q2, q4 = (h @ np.abs(q)) / tot, (h @ (q * q)) / tot, (h @ (q * q * q * q)) / tot
            out = dict(q_abs=q_abs, q2=q2, q4=q4, binder=0.5 * (3.0 - q4 / (q2 * q2)), ql=None, ql_var=None)
            if self.n_links > 0:
                ql, ql_var = np.full(len(tot), np.nan), np.full(len(tot), np.nan)
                for c, (m, s1, s2) in enumerate(zip(self.link_n, self.link_sum, self.link_sum2)):
                    m, s1, s2 = int(m), int(s1), int(s2)          # Python integers: m s2 - s1^2 is exact
                    if m > 0:
                        ql[c] = 1.0 - 2.0 * (s1 / m) / self.n_links
                        ql_var[c] = 4.0 * ((m * s2 - s1 * s1) / (m * m)) / (self.n_links * self.n_links)
                out.update(ql=ql, ql_var=ql_var)
        return out


def _cos_turn(j, L):
    """cos(2 pi j / L), 0 <= j < L, folded into the first quarter turn so that the table is symmetric and antisymmetric to the last bit: a
    constant C(r) then sums to exactly 0 at every m != 0"""
    if 2 * j > L:
        j = L - j
    if 4 * j == L:
        return 0.0
    if 4 * j > L and L % 2 == 0:
        return -math.cos(2.0 * math.pi * (L // 2 - j) / L)
    return math.cos(2.0 * math.pi * j / L)


@dataclass
class HoudayerMove:
    """Houdayer's cluster move between the two copies of a pair: made at every scan s with s % every == 0 (0: never), on the chains with
    betas[c] >= min_beta -- in three dimensions the disagreeing sites percolate at high temperature and the move then only relabels the copies
    (ClusterRecord.mean_fraction() shows where) -- from a stream of its own keyed by seed (None: the pair's Inputs.seed)."""
    every: int = 1
    min_beta: float = 0.0
    seed: Any = None

    def __post_init__(self):
        if isinstance(self.every, bool) or not isinstance(self.every, (int, np.integer)) or self.every < 0:
            raise ValueError("HoudayerMove: every must be an integer >= 0 (got %r); 0 turns the move off" % (self.every,))
        if not (isinstance(self.min_beta, (int, float, np.integer, np.floating)) and 0.0 <= float(self.min_beta) <= 1.0):
            raise ValueError("HoudayerMove: min_beta must be in [0, 1] (got %r)" % (self.min_beta,))
        if self.seed is not None and (isinstance(self.seed, bool) or not isinstance(self.seed, (int, np.integer)) or not 0 <= int(self.seed) < 2 ** 64):
            raise ValueError("HoudayerMove: seed must be None or an integer in 0 .. 2^64 - 1 (got %r)" % (self.seed,))


@dataclass
class ClusterRecord:
    """The cluster move's accumulators of one pte_overlap_reduce, all int64 and keyed by chain, and the schedule in force meanwhile."""
    betas: Any          # float64 [N]
    n: Any              # [N] moves made (chains below min_beta: 0)
    empty: Any          # [N] moves that found the two copies equal (k = 0) and wrote nothing
    size_sum: Any       # [N] sum of |C|, the sites flipped
    k_sum: Any          # [N] sum of k, the sites at which the copies differed
    abs_ds_sum: Any     # [N] sum of |delta|, the pair sum handed from one copy to the other
    passes_sum: Any     # [N] sum of the passes of the kernel's fixed-point loop (a cost figure, not part of the specification)
    moves_launched: int = 0   # launches the record covers

    def mean_fraction(self):
        """size_sum / k_sum per chain: the share of the disagreeing sites a move flips.  Near 1 the sites percolate and the move only relabels
        the copies: put min_beta above those chains.  NaN where k_sum == 0."""
        k = np.asarray(self.k_sum, dtype=np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(k > 0, np.asarray(self.size_sum, dtype=np.float64) / k, np.nan)


def cluster_move_geometry(target):
    """None where the move runs on this lattice target (the cube; the 2-D lattices with base_length % 32 == 0), else the refusal's text"""
    if isinstance(target, SpinGlass3DLogPotential) or int(target.base_length) % 32 == 0:
        return None
    return ("HoudayerMove runs on the cube and on the 2-D lattices whose base_length is a multiple of 32 (got base_length %d): the packed "
            "bond planes exist only there" % int(target.base_length))


def planes_geometry(target):
    """None where the plane sums are recorded on this lattice target (the cube; the 2-D lattices with base_length % 32 == 0), else the
    refusal's text"""
    if isinstance(target, SpinGlass3DLogPotential) or int(target.base_length) % 32 == 0:
        return None
    return ("wave_vector=True runs on the cube and on the 2-D lattices whose base_length is a multiple of 32 (got base_length %d): the rows "
            "are whole words only there" % int(target.base_length))


class Overlap:
    """pte_overlap_*: the overlap recorder over two engines.  It holds no state of either engine; close() leaves both usable."""

    def __init__(self, eng_a, eng_b):
        if eng_a.L is not eng_b.L:
            raise ValueError("Overlap: the two engines come from different builds of libpte")
        self.L, self.a, self.b = eng_a.L, eng_a, eng_b
        h = C.c_void_p()
        if self.L.pte_overlap_create(eng_a.h, eng_b.h, C.byref(h)) != 0:
            raise PteError(self.L.pte_last_error(None).decode())
        self.h = h
        info = np.zeros(3, dtype=np.int64)
        self._chk(self.L.pte_overlap_info(h, _ip(info[0:1]), _ip(info[1:2]), _ip(info[2:3])))
        self.N, self.d, self.n_links = int(info[0]), int(info[1]), int(info[2])
        self._chk(self.L.pte_overlap_planes_info(h, _ip(info[0:1]), _ip(info[1:2]), _ip(info[2:3])))
        self.n_axes, self.base_length = int(info[0]), int(info[1])      # n_axes == 0: the plane sums are not recorded on this lattice
        self._planes = False                                           # set_planes(True) was called at some time

    def _chk(self, rc):
        if rc != 0:
            raise PteError(self.L.pte_last_error(self.a.h).decode())

    def close(self):
        if getattr(self, "h", None):
            self.L.pte_overlap_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def record(self):
        """one record of the two engines' states as they are"""
        self._chk(self.L.pte_overlap_record(self.h))

    def run_scans(self, first_scan, n_scans):
        """explore, swap (both engines) and record, for every scan of the call"""
        self._chk(self.L.pte_overlap_run_scans(self.h, first_scan, n_scans))

    def reduce(self):
        """-> OverlapRecord of everything recorded since the last reduce; the device's accumulators start again from zero"""
        betas = self.a.schedule()
        self._chk(self.L.pte_overlap_reduce(self.h))
        n, link_n, link_sum, link_sum2 = (np.zeros(self.N, dtype=np.int64) for _ in range(4))
        hist = np.zeros((self.N, self.d + 1), dtype=np.int64)
        self._chk(self.L.pte_overlap_get(self.h, _ip(n), _ip(hist), _ip(link_n), _ip(link_sum), _ip(link_sum2)))
        self._cluster_betas = betas
        plane_n = plane_corr = None
        if self._planes:
            plane_n, plane_corr = np.zeros(self.N, dtype=np.int64), np.zeros((self.N, self.n_axes, self.base_length), dtype=np.int64)
            self._chk(self.L.pte_overlap_planes_get(self.h, _ip(plane_n), _ip(plane_corr)))
            if not (self.planes_on() or plane_n.any()):                # off, and off at every record of the round
                plane_n = plane_corr = None
        return OverlapRecord(betas, self.d, self.n_links, n, hist, link_n, link_sum, link_sum2, plane_n, plane_corr)

    def set_planes(self, on=True):
        """record the plane autocorrelation (OverlapRecord.plane_n, .plane_corr) at every record from now on, or stop"""
        self._chk(self.L.pte_overlap_set_planes(self.h, 1 if on else 0))
        self._planes = self._planes or bool(on)

    def planes_on(self):
        on = np.zeros(1, dtype=np.int64)
        self._chk(self.L.pte_overlap_planes_info(self.h, None, None, _ip(on)))
        return bool(on[0])

    def set_cluster_move(self, move, seed=None):
        """the setting of Houdayer's cluster move from now on (move.seed None: `seed`); the launch counter of its stream starts again from 0"""
        if not isinstance(move, HoudayerMove):
            raise TypeError("Overlap.set_cluster_move: expected a HoudayerMove (got %r)" % (move,))
        s = move.seed if move.seed is not None else seed
        if s is None:
            raise ValueError("Overlap.set_cluster_move: HoudayerMove(seed=None) needs the seed of the run; pass seed=")
        self._chk(self.L.pte_overlap_set_cluster_move(self.h, int(move.every), float(move.min_beta), int(s)))

    def cluster_move(self):
        """one cluster move on the two engines' states as they are"""
        self._chk(self.L.pte_overlap_cluster_move(self.h))

    def reduce_clusters(self):
        """-> ClusterRecord of the moves covered by the last reduce(): one pte_overlap_reduce snapshots and zeroes the overlap's and the
        move's accumulators together, so a round calls reduce(), then this"""
        betas = getattr(self, "_cluster_betas", None)
        if betas is None:
            betas = self.a.schedule()
        arrays = [np.zeros(self.N, dtype=np.int64) for _ in range(6)]
        launched = np.zeros(1, dtype=np.int64)
        self._chk(self.L.pte_overlap_cluster_get(self.h, *[_ip(v) for v in arrays], _ip(launched)))
        return ClusterRecord(betas, *arrays, moves_launched=int(launched[0]))


class PTPair:
    """Two PTs over one target and an Overlap between their engines.  `a` and `b` stay ordinary PTs (stepping_stone, n_round_trips, ... work
    on each); `overlap` is the OverlapRecord of the last round, `overlaps` holds one per round; with a cluster move, `cluster` and `clusters`
    hold its ClusterRecords the same way."""

    def __init__(self, a, b, recorder=None):
        self.a, self.b, self.recorder = a, b, recorder
        self.overlap, self.overlaps = None, []
        self.cluster_move = None                        # the HoudayerMove in force (pigeons_pair(cluster_move=...)), or None
        self.cluster, self.clusters = None, []          # its ClusterRecord of the last round and of every round


def check_pair_inputs(inputs, seed_b, pt_kwargs=(), cluster_move=None, wave_vector=False):
    """what a pair refuses, before any device work"""
    if cluster_move is not None and not isinstance(cluster_move, HoudayerMove):
        raise TypeError("pigeons_pair: cluster_move must be None or a HoudayerMove (got %r)" % (cluster_move,))
    sharding = [k for k in SHARDING_ARGUMENTS if k in pt_kwargs]
    if sharding:
        raise NotImplementedError("pigeons_pair: sharded or multi-GPU pairs are not supported (got %s)" % ", ".join(sharding))
    if not isinstance(inputs.target, LATTICE_TARGETS):
        raise NotImplementedError("pigeons_pair: the overlap is recorded on the lattice targets (IsingLogPotential, SpinGlassLogPotential, "
                                  "SpinGlass3DLogPotential); got %r" % (inputs.target,))
    if int(inputs.n_chains_variational or 0) > 0:
        raise NotImplementedError("pigeons_pair: n_chains_variational must be 0 (got %d): a two-leg ladder holds every temperature twice"
                                  % int(inputs.n_chains_variational))
    if inputs.checkpoint:
        raise NotImplementedError("pigeons_pair: checkpoint=True is not supported: a pair has no checkpoint format")
    if seed_b == inputs.seed:
        raise ValueError("pigeons_pair: seed_b must differ from seed (both %d): identical runs give q = 1 at every record" % inputs.seed)
    if cluster_move is not None and cluster_move_geometry(inputs.target):
        raise NotImplementedError("pigeons_pair: " + cluster_move_geometry(inputs.target))
    if wave_vector and planes_geometry(inputs.target):
        raise NotImplementedError("pigeons_pair: " + planes_geometry(inputs.target))


def run_pair_round(pair):
    """one round of both runs, scan by scan in step: Overlap.run_scans(1, 2^round), then the reductions of a, of b and of the overlap"""
    n = n_scans_in_round(pair.a.shared.iterators)
    t0 = time.perf_counter()
    pair.recorder.run_scans(1, n)
    elapsed = time.perf_counter() - t0
    pair.a.shared.iterators.scan = pair.b.shared.iterators.scan = 0
    red_a, red_b = reduce_recorders(pair.a, elapsed), reduce_recorders(pair.b, elapsed)
    pair.overlap = pair.recorder.reduce()
    pair.overlaps.append(pair.overlap)
    if pair.cluster_move is not None:
        pair.cluster = pair.recorder.reduce_clusters()
        pair.clusters.append(pair.cluster)
    return red_a, red_b


def adapt_pair(pair, red_a, red_b):
    """adapt (src/pt/pigeons.jl:152-162) for the pair: ONE new schedule, from the mean of the two runs' rejection rates, given to both --
    a chain of the pair must stay one temperature."""
    a, b = pair.a, pair.b
    for pt, red in ((a, red_a), (b, red_b)):
        pt.reduced_recorders = red
        adapt_explorer(pt, red)
    old = a.shared.tempering.schedule.grids
    if len(old) == 1:
        return pair
    rej = 0.5 * (T.rejections(*red_a.swap_acceptance_pr) + T.rejections(*red_b.swap_acceptance_pr))
    new_sched = T.Schedule(T.optimal_schedule(rej, old, len(old)))
    barriers = T.CommunicationBarriers(rej, old)
    for pt in (a, b):
        pt.shared.tempering = NonReversiblePT(pt.shared.tempering.path, new_sched, barriers)
        pt.replicas.set_schedule(new_sched.grids)
    return pair


def pigeons_pair(seed_b=None, cluster_move=None, wave_vector=False, **inputs_kwargs):
    """pigeons(; ...) twice over, in step: two PTs over the same target and inputs with seeds `seed` and `seed_b` (default seed + 1), the
    overlap between them recorded at every scan -> PTPair.  Only the first run prints its report.  cluster_move: None, or the HoudayerMove
    made between the two copies (its accumulators per round in pair.clusters, the last in pair.cluster).  wave_vector=True: every record
    also adds the plane autocorrelation, from which OverlapRecord.chi_sg() and .correlation_length() follow."""
    pt_kwargs = {k: inputs_kwargs.pop(k) for k in SHARDING_ARGUMENTS if k in inputs_kwargs}
    inputs = Inputs(**inputs_kwargs)
    if seed_b is None:
        seed_b = inputs.seed + 1
    check_pair_inputs(inputs, seed_b, pt_kwargs, cluster_move, wave_vector)
    a = PT(inputs)
    b = PT(dataclasses.replace(inputs, seed=seed_b, show_report=False, record=list(inputs.record)))
    pair = PTPair(a, b, Overlap(a.replicas, b.replicas))
    pair.cluster_move = cluster_move
    if cluster_move is not None:
        pair.recorder.set_cluster_move(cluster_move, seed=inputs.seed)
    if wave_vector:
        pair.recorder.set_planes(True)
    while next_round(a) and next_round(b):
        adapt_pair(pair, *run_pair_round(pair))
        report(a)
        report(b)
    return pair
