// pte_aaps.hpp -- k_explore_aaps: the apogee-to-apogee path sampler (AAPS; Sherlock, Urbas & Ludkin, JCGS 2023; reference
// src/explorers/AAPS.jl) on the device log-potential families, one wavefront per replica, and aaps_launch / aaps_set_rng_policy
// (pte_aaps_params.hpp).  Included by exactly ONE translation unit: pte_aaps.hip in the product build, pte.hip when it is compiled alone.
//
// One explore! call = one AAPS transition (DESIGN 4.7 holds the specification and tests/aaps_ref.py its restatement):
//   preconditioner M (build_preconditioner!, as AutoMALA), momentum p0 ~ N(0, I), Kf = rand(rng, 0:K), Kb = K - Kf;
//   leapfrog forward from (x0, p0) through the current segment and Kf later ones, backward from (x0, -p0) through the rest of the
//   current segment and Kb earlier ones; a segment boundary lies between time-consecutive points u, v with h(u) < 0 <= h(v), where
//   h = sum p g / M in forward-time orientation; every point between the two stopping points is a candidate, chosen progressively
//   with probability proportional to exp(log density - |p|^2 / 2).
//
// Seven vectors live in registers -- lane l holds elements 64j + l, j < E -- : the position x, momentum p, conditioned gradient g / M,
// the preconditioner M, the start x0, its momentum p0 and the selected point.  The log potential and its gradient are AmTarget's
// (pte_automala.hpp).  On the MVN path the four sums of a leapfrog step (|x|^2 inside the log density, |p|^2 after the half step -- the
// failure test of am_leap_frog -- and after the full step, and h) run as one lockstep tree; on the funnel path the density's own sums and
// the half-step |p|^2 are one tree (AmTarget) and the full-step |p|^2 with h a second one, because the gradient of the funnel coordinate
// is itself a sum.
#pragma once
#include <hip/hip_ext.h>
#include "pte_aaps_params.hpp"
#include "pte_automala.hpp"

namespace pte {

// rand(rng, 0:n-1) on Int64 from the replica's sequential stream
__device__ __forceinline__ int64_t rand_range0(SeqRng &r, uint64_t n) { return rand_range0_from([&]() { return r.next(); }, n); }

template <int E, int TGT, bool FULL = false>
__global__ __launch_bounds__(64) void k_explore_aaps(EngineDev e, AapsParams ap) {
    constexpr int NLU = (E == 1 ? 0 : E == 2 ? 1 : E == 4 ? 2 : 3);
    const int lane = lane_id();
    // the ziggurat tables of the momentum draws, staged once (as k_explore_automala)
    __shared__ double s_wi[256];
    __shared__ unsigned long long s_ki[256];
    __shared__ double s_fi[256];
    for (int i = lane; i < 256; i += 64) { s_wi[i] = ZIG_WI[i]; s_ki[i] = ZIG_KI[i]; s_fi[i] = ZIG_FI[i]; }
    __syncthreads();
    const int64_t cl = am_chain_of_workgroup(e.K, blockIdx.x);
    if (cl >= e.K) return;
    const int64_t c = e.c0 + cl;
    const int slot = e.slot_of_chain[cl];
    const int64_t d = e.d;
    double *xrow = e.x + (int64_t)slot * e.ld;
    AmTarget<E, TGT, FULL> T;
    T.d = d; T.lane = lane;
    T.nhp = e.nhp[c]; T.nprec = e.nprec[c];
    T.beta = e.beta[c]; T.omb = 1.0 - T.beta;
    T.ref_nhp = -0.5 * ap.ref_prec; T.ref_nprec = -ap.ref_prec; T.log3 = ap.log3;
    const bool v_on = (TGT == TGT_FUNNEL) && e.v_use != nullptr;      // a GaussianReference is active on this engine
    if (v_on) { T.load_variational(e); T.vr = e.v_use[c] != 0; }

    double x[E];
    if (is_ref_chain(e, c)) {                    // sample_iid! at the reference (pigeons.jl:104-105): the prologue of k_explore_automala
        const double lp0 = lp_before_explore(e, c, slot);
        double S0;
        if (v_on && T.vr) {
            SeqRng r0{e.rng[2 * slot], e.rng[2 * slot + 1]};
#pragma unroll
            for (int j = 0; j < E; ++j) {
                const int nl = (int)max((int64_t)0, min((int64_t)64, d - 64 * (int64_t)j));
                x[j] = 0.0;
                if (nl > 0) {
                    const double z = wave_randn_block(r0, lane, nl);
                    x[j] = lane < nl ? z * e.v_std[64 * j + lane] + T.VM(j) : 0.0;
                    if (lane < nl) xrow[64 * j + lane] = x[j];
                }
            }
            S0 = sqr_norm_regs<E>(x);
            if (lane == 0) { e.suff[slot] = S0; e.rng[2 * slot] = r0.seed; }
        } else {
            S0 = iid_refresh<NLU>(e, slot, e.sd[c], lane);
            __threadfence_block();
#pragma unroll
            for (int j = 0; j < E; ++j) x[j] = T.valid(j) ? xrow[64 * j + lane] : 0.0;
        }
        double l20 = 0.0, l30 = 0.0;
        if (TGT == TGT_FUNNEL) {
            l20 = T.funnel(x, nullptr);
            if (lane == 0) e.suff2[slot] = l20;
            if (v_on) { l30 = T.variational_lp(x); if (lane == 0) e.suff3[slot] = l30; }
        }
        record_after_explore_impl(e, cl, c, slot, lane, lp0, S0, l20, l30);
        return;
    }
    const double lp_before = lp_before_explore(e, c, slot);
    double x0[E];
#pragma unroll
    for (int j = 0; j < E; ++j) x0[j] = T.valid(j) ? xrow[64 * j + lane] : 0.0;

    SeqRng r{e.rng[2 * slot], e.rng[2 * slot + 1]};
    // build_preconditioner! (Preconditioner.jl:57-77), the draws of am_build_preconditioner
    double M[E];
#pragma unroll
    for (int j = 0; j < E; ++j) M[j] = 1.0;
    if (ap.target_std != nullptr && ap.precond != 0) {
        double sdv[E];
#pragma unroll
        for (int j = 0; j < E; ++j) sdv[j] = T.valid(j) ? ap.target_std[64 * j + lane] : 1.0;
        if (ap.precond == 1) {
#pragma unroll
            for (int j = 0; j < E; ++j) M[j] = sdv[j] == 0.0 ? 1.0 : 1.0 / sdv[j];
        } else {
            const double u = r.rand();
            if (u <= ap.p0) {
#pragma unroll
                for (int j = 0; j < E; ++j) M[j] = sdv[j] == 0.0 ? 1.0 : 1.0 / sdv[j];
            } else if (u <= ap.p0 + ap.p1) {
                // ones
            } else {
                const double mix = r.rand(), rmix = 1.0 - mix;
#pragma unroll
                for (int j = 0; j < E; ++j) M[j] = sdv[j] == 0.0 ? 1.0 : mix + rmix / sdv[j];
            }
        }
    }
    // momentum, in AutoMALA's draw order
    double p0[E];
#pragma unroll
    for (int j = 0; j < E; ++j) {
        const int nl = FULL ? 64 : (int)max((int64_t)0, min((int64_t)64, d - 64 * (int64_t)j));
        p0[j] = 0.0;
        if (nl > 0) { const double v = wave_randn_block(r, lane, nl, s_wi, s_ki, s_fi); p0[j] = lane < nl ? v : 0.0; }
    }
    const int Kf = (int)rand_range0(r, (uint64_t)ap.K + 1), Kb = ap.K - Kf;

    double xx[E], p[E], g[E], sel[E];
    // log density and conditioned gradient at (x, p): the start point of a pass
    auto start = [&](double sign) -> double {
        double pp;
#pragma unroll
        for (int j = 0; j < E; ++j) { xx[j] = x0[j]; p[j] = sign * p0[j]; }
        const double lp = T.template logdensity_and_gradient_q<true>(xx, g, p, pp);
#pragma unroll
        for (int j = 0; j < E; ++j) g[j] = g[j] / M[j];
        return lp - 0.5 * pp;
    };
    const double w0 = start(1.0);
    if (!isfinite(w0)) { if (lane == 0) set_error(e, ERR_AAPS_DENSITY, (int)c, -1); return; }
    double h0;
    {
        double t[E];
#pragma unroll
        for (int j = 0; j < E; ++j) t[j] = p0[j] * g[j];
        h0 = tree_sum_regs<E>(t);
    }
#pragma unroll
    for (int j = 0; j < E; ++j) sel[j] = x0[j];
    const double eps = ap.step_size, half = eps / 2;
    double L = w0;
    int steps = 0;
    bool failed = false;
    // one pass: dir = +1 forward from (x0, p0) until the point that opens segment Kf + 1, dir = -1 backward from (x0, -p0) until the
    // point that opens segment -(Kb + 1); every point before the stopping point is a candidate
    auto pass = [&](int dir, int stop_at) {
        bool s_prev = h0 >= 0.0;
        int seg = 0;
        for (;;) {
            if (steps == PTE_AAPS_MAX_LEAPFROGS) { failed = true; return; }
            ++steps;
            // am_leap_frog: half step, full position step, conditioned gradient, half step
#pragma unroll
            for (int j = 0; j < E; ++j) p[j] = p[j] + half * g[j];
#pragma unroll
            for (int j = 0; j < E; ++j) xx[j] = xx[j] + eps * (p[j] / M[j]);
            double lp, pph, pp, hh;
            if constexpr (TGT == TGT_MVN) {
                double t[4][E], out[4];
#pragma unroll
                for (int j = 0; j < E; ++j) {
                    g[j] = (T.nprec * xx[j]) / M[j];
                    t[0][j] = xx[j] * xx[j];
                    t[1][j] = p[j] * p[j];
                    p[j] = p[j] + half * g[j];
                    t[2][j] = p[j] * p[j];
                    t[3][j] = p[j] * g[j];
                }
                tree_sum_regs_multi<E, 4>(t, out);
                lp = T.nhp * out[0]; pph = out[1]; pp = out[2]; hh = out[3];
            } else {
                lp = T.template logdensity_and_gradient_q<true>(xx, g, p, pph);
                double t[2][E], out[2];
#pragma unroll
                for (int j = 0; j < E; ++j) {
                    g[j] = g[j] / M[j];
                    p[j] = p[j] + half * g[j];
                    t[0][j] = p[j] * p[j];
                    t[1][j] = p[j] * g[j];
                }
                tree_sum_regs_multi<E, 2>(t, out);
                pp = out[0]; hh = out[1];
            }
            const double w = lp - 0.5 * pp;
            if (__builtin_expect(!isfinite(lp - 0.5 * pph) || !isfinite(pp) || !isfinite(w), 0)) { failed = true; return; }
            const bool s = (dir > 0 ? hh : -hh) >= 0.0;
            if (dir > 0) { if (!s_prev && s) ++seg; }
            else { if (!s && s_prev) --seg; }
            if (seg == stop_at) return;
            L = dev_logaddexp(L, w);
            if (r.rand() < exp(w - L)) {
#pragma unroll
                for (int j = 0; j < E; ++j) sel[j] = xx[j];
            }
            s_prev = s;
        }
    };
    pass(1, Kf + 1);
    if (!failed) {
        start(-1.0);
        pass(-1, -(Kb + 1));
    }
    double acc;
    if (failed) {
        acc = 0.0;
#pragma unroll
        for (int j = 0; j < E; ++j) x[j] = x0[j];
    } else {
        acc = 1.0 - exp(w0 - L);
#pragma unroll
        for (int j = 0; j < E; ++j) x[j] = sel[j];
    }
#pragma unroll
    for (int j = 0; j < E; ++j) if (T.valid(j)) xrow[64 * j + lane] = x[j];
    const double S = sqr_norm_regs<E>(x);
    double l2 = 0.0, l3 = 0.0;
    if (TGT == TGT_FUNNEL) l2 = T.funnel(x, nullptr);
    if (v_on) l3 = T.variational_lp(x);
    if (lane == 0) {
        e.suff[slot] = S;
        if (TGT == TGT_FUNNEL) e.suff2[slot] = l2;
        if (v_on) e.suff3[slot] = l3;
        e.rng[2 * slot] = r.seed;
        e.expl_steps_sum[cl] += (double)steps; e.expl_steps_n[cl] += 1;
        e.expl_acc_sum[cl] += acc;             e.expl_acc_n[cl] += 1;
    }
    record_after_explore(e, cl, c, slot, lane, lp_before, S, l2, l3);
}

int aaps_launch(const AapsLaunch &L, const EngineDev &dev, const AapsParams &ap) {
#define AAPS_ONE(EE)                                                                                                 \
    if (L.target == TGT_FUNNEL && L.full) launch_on(L.at, k_explore_aaps<EE, TGT_FUNNEL, true>, 64, 0, dev, ap);         \
    else if (L.target == TGT_FUNNEL) launch_on(L.at, k_explore_aaps<EE, TGT_FUNNEL, false>, 64, 0, dev, ap);             \
    else if (L.full) launch_on(L.at, k_explore_aaps<EE, TGT_MVN, true>, 64, 0, dev, ap);                                 \
    else launch_on(L.at, k_explore_aaps<EE, TGT_MVN, false>, 64, 0, dev, ap);
    switch (L.E) {
    case 1: AAPS_ONE(1) break; case 2: AAPS_ONE(2) break; case 4: AAPS_ONE(4) break; case 8: AAPS_ONE(8) break;
    default: return 1;
    }
#undef AAPS_ONE
    return 0;
}

PTE_DEFINE_RNG_POLICY_SETTER(aaps)

}  // namespace pte
