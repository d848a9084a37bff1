"""The replica overlap between two runs of a lattice family (the project's own specification -- the reference has no such recorder).

Two PTs over the same target and inputs, with different seeds, hold two independent copies of the system at every temperature.  Per chain c
and per scan the device adds, as exact integers, the site overlap k = #{i : s_i^a != s_i^b} (q = 1 - 2 k / d) to a histogram and the link
overlap kl = #{bonds (i, j) : s_i^a s_j^a != s_i^b s_j^b} (q_l = 1 - 2 kl / n_links) to a sum and a sum of squares: P(q), its moments and
the Binder ratio, which tell the glassy phase from the paramagnet where the magnetisation cannot (it vanishes by gauge symmetry).

  Overlap(eng_a, eng_b)      the ctypes wrapper of pte_overlap_* (include/pte.h)
  OverlapRecord              the reduced accumulators of one round and what is computed from them
  pigeons_pair(...) -> PTPair   the round loop: the two engines kept in step scan by scan, their ladders kept equal round by round
"""
import ctypes as C
import dataclasses
import time
from dataclasses import dataclass
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
        return OverlapRecord(betas, self.d, self.n_links, n, hist, link_n, link_sum, link_sum2)


class PTPair:
    """Two PTs over one target and an Overlap between their engines.  `a` and `b` stay ordinary PTs (stepping_stone, n_round_trips, ... work
    on each); `overlap` is the OverlapRecord of the last round, `overlaps` holds one per round."""

    def __init__(self, a, b, recorder=None):
        self.a, self.b, self.recorder = a, b, recorder
        self.overlap, self.overlaps = None, []


def check_pair_inputs(inputs, seed_b, pt_kwargs=()):
    """what a pair refuses, before any device work"""
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


def pigeons_pair(seed_b=None, **inputs_kwargs):
    """pigeons(; ...) twice over, in step: two PTs over the same target and inputs with seeds `seed` and `seed_b` (default seed + 1), the
    overlap between them recorded at every scan -> PTPair.  Only the first run prints its report."""
    pt_kwargs = {k: inputs_kwargs.pop(k) for k in SHARDING_ARGUMENTS if k in inputs_kwargs}
    inputs = Inputs(**inputs_kwargs)
    if seed_b is None:
        seed_b = inputs.seed + 1
    check_pair_inputs(inputs, seed_b, pt_kwargs)
    a = PT(inputs)
    b = PT(dataclasses.replace(inputs, seed=seed_b, show_report=False, record=list(inputs.record)))
    pair = PTPair(a, b, Overlap(a.replicas, b.replicas))
    while next_round(a) and next_round(b):
        adapt_pair(pair, *run_pair_round(pair))
        report(a)
        report(b)
    return pair
