// pte_dense.hpp -- the dense-precision Gaussian family of the device engine (PTE_TARGET_DENSE_NORMAL): the target N(m, Q^-1) with a
// dense symmetric positive-definite precision matrix Q shared by every replica, 1 <= d <= 512 -- the first log potential that costs O(d^2) per
// evaluation.  The interpolated path (1 - beta) ScaledPrecisionNormal(p) + beta target is explored by
//   k_explore_dense        AutoMALA / MALA: automala_body with AmTarget<E, TGT_DENSE>::dense_and_sqr_norm, a full matrix-vector product per
//                          gradient (pte_automala.hpp);
//   k_explore_dense_slice  SliceSampler: a kernel of its own.  A single-coordinate move of a quadratic form has a closed form, so the sweep
//                          keeps u = Q (x - m), A = (x - m)' u and S = sum x^2 of the committed state, evaluates a proposal in O(1) and reads
//                          ONE matrix row per committed coordinate.
// One wave per replica; lane l holds coordinates 64 j + l.  Compiled inside pte_glm.hip (pte_automala_params.hpp).
#pragma once
#include <hip/hip_ext.h>
#include "pte_automala.hpp"
#include "pte_dense_params.hpp"

namespace pte {

template <int E, bool SLICE, bool FULL>
__global__ __launch_bounds__(64) void k_explore_dense(EngineDev e, AmParams ap, DenseParams dn) {
    static_assert(!SLICE, "SliceSampler on the dense-normal path is k_explore_dense_slice");
    automala_body<E, TGT_DENSE, SLICE, FULL>(e, ap, blockIdx.x, dn);
}

// coordinate idx of v (uniform idx), as a uniform value
template <int E>
__device__ __forceinline__ double dense_get(const double (&v)[E], int idx) {
    double out = 0.0;
#pragma unroll
    for (int j = 0; j < E; ++j) { const double t = readlane_f64(v[j], idx & 63); out = (idx >> 6) == j ? t : out; }
    return out;
}

// One sweep of SliceSampler over the d coordinates in state order, n_passes times (slice_sample! :43-62; slice_coord<double>:
// pte_slice_coord.hpp).  With delta = v - x_k the target's quadratic form at the proposal is A' = A + delta (2 u_k + Q_kk delta) and
// S' = S + (v^2 - x_k^2): every lane evaluates the same O(1) expression on broadcast values.  A commit adds delta times row k to u (E loads,
// E fused multiply-adds).  Row k + 1 is requested while coordinate k is being sampled -- a row is in registers a whole coordinate before
// its commit reads it -- and the diagonal stays in registers, so no proposal waits for memory.  The cached u, A and S never leave the call:
// the epilogue evaluates S and the target's log density of the final state in full, as k_refresh_dense_stats does, so the swap
// statistics are a pure function of the stored state.  All control flow is uniform.
template <int E, bool FULL>
__global__ __launch_bounds__(64) void k_explore_dense_slice(EngineDev e, AmParams ap, DenseParams dn) {
    constexpr int NLU = (E == 1 ? 0 : E == 2 ? 1 : E == 4 ? 2 : 3);
    const int lane = lane_id();
    const int64_t cl = blockIdx.x;
    if (cl >= e.K) return;
    const int64_t c = e.c0 + cl;
    const int slot = e.slot_of_chain[cl];
    const int d = FULL ? 64 * E : (int)e.d;
    double *xrow = e.x + (int64_t)slot * e.ld;
    AmTarget<E, TGT_DENSE, FULL> T;
    T.d = e.d; T.lane = lane; T.dn = dn;
    const double beta = e.beta[c], omb = 1.0 - beta, ref_nhp = -0.5 * ap.ref_prec;
    double x[E], z[E], u[E];

    if (is_ref_chain(e, c)) {
        if (e.compose_phase == 2) return;
        const double lp0 = lp_before_explore(e, c, slot);
        const double S0 = iid_refresh<NLU>(e, slot, e.sd[c], lane);            // sample_iid! at the reference (pigeons.jl:104-105)
        __threadfence_block();
#pragma unroll
        for (int j = 0; j < E; ++j) x[j] = T.valid(j) ? xrow[64 * j + lane] : 0.0;
        const double l20 = T.target(x);
        if (lane == 0) e.suff2[slot] = l20;
        record_after_explore_impl(e, cl, c, slot, lane, lp0, S0, l20);
        return;
    }
    const double lp_before = lp_before_explore(e, c, slot);
#pragma unroll
    for (int j = 0; j < E; ++j) x[j] = T.valid(j) ? xrow[64 * j + lane] : 0.0;
    double A, S, unused;
    T.dense_core(x, z, u);
    T.template dense_sums<false>(x, z, u, A, S, x, unused);

    // the path's log potential from the two sums, with InterpolatedLogPotential's short-circuits (AmTarget::path_lp)
    auto path = [&](double A_, double S_) -> double {
        if (beta == 0.0) return ref_nhp * S_;
        const double l2 = dn.c - 0.5 * A_;
        if (beta == 1.0) return l2;
        return omb * (ref_nhp * S_) + beta * l2;
    };
    WaveDraws dr;
    dr.init(e.rng[2 * slot], e.rng[2 * slot + 1], lane);
    SliceTally tally;
    double lp = path(A, S);                                    // cached_log_potential (:32-41): the expression of eval at delta = 0
    if (lp == -INFINITY) { if (lane == 0) set_error(e, ERR_SLICE_SUPPORT, (int)c, -1); return; }
    const SliceKnobs kn{ap.slice_w, 1.1 * ap.slice_w, ap.slice_p, ap.slice_max_iter};
    double qd[E], rn[E];                                       // the diagonal; the row of the NEXT coordinate
#pragma unroll
    for (int j = 0; j < E; ++j) { qd[j] = dn.diag[64 * j + lane]; rn[j] = dn.q[64 * j + lane]; }
    const int64_t ld = dn.ld;
    for (int pass = 0; pass < ap.slice_n_passes; ++pass) {
        for (int k = 0; k < d; ++k) {
            double rc[E];                                      // row k: requested while coordinate k - 1 was sampled
            const double *nrow = dn.q + (int64_t)(k + 1 < d ? k + 1 : 0) * ld + lane;      // (the last coordinate's: row 0, which the next pass starts with)
#pragma unroll
            for (int j = 0; j < E; ++j) { rc[j] = rn[j]; rn[j] = nrow[64 * j]; }
            struct Coord {
                double (&x)[E]; double (&u)[E]; const double (&rc)[E];
                double &A, &S;
                const decltype(path) &lpf;
                int k, lane;
                double xk, uk, qkk;                            // broadcast once per coordinate
                __device__ __forceinline__ void sums(double v, double &A_, double &S_) const {
                    const double dl = v - xk;
                    A_ = A + dl * (2.0 * uk + qkk * dl);
                    S_ = S + (v * v - xk * xk);
                }
                __device__ __forceinline__ double eval(double v) { double A_, S_; sums(v, A_, S_); return lpf(A_, S_); }
                __device__ __forceinline__ void hold() {}
                __device__ __forceinline__ void commit(double v) {
                    double A_, S_;
                    sums(v, A_, S_);
                    const double dl = v - xk;
#pragma unroll
                    for (int j = 0; j < E; ++j) {
                        u[j] = __builtin_fma(dl, rc[j], u[j]);
                        x[j] = (k >> 6) == j && lane == (k & 63) ? v : x[j];
                    }
                    A = A_; S = S_;
                }
            } coord{x, u, rc, A, S, path, k, lane, dense_get<E>(x, k), dense_get<E>(u, k), dense_get<E>(qd, k)};
            const int err = slice_coord<double>(coord, dr, lane, kn, tally, coord.xk, kn.w, lp);
            if (err) { if (lane == 0) set_error(e, err, (int)c, k); return; }
        }
    }
#pragma unroll
    for (int j = 0; j < E; ++j) if (T.valid(j)) xrow[64 * j + lane] = x[j];
    double A1, S1;
    T.dense_core(x, z, u);                                     // in full from the final x: nothing cached leaves the call
    T.template dense_sums<false>(x, z, u, A1, S1, x, unused);
    const double l2 = dn.c - 0.5 * A1;
    if (lane == 0) {
        e.suff[slot] = S1; e.suff2[slot] = l2;
        e.rng[2 * slot] = dr.final_seed();
        e.expl_steps_sum[cl] += (double)tally.steps_sum; e.expl_steps_n[cl] += tally.steps_n;
        e.expl_acc_sum[cl] += tally.acc_sum;             e.expl_acc_n[cl] += tally.acc_n;
    }
    record_after_explore(e, cl, c, slot, lane, lp_before, S1, l2);
}

// swap statistics of every slot recomputed from the stored states (pte_set_state, pte_set_target_dense): suff = sum x^2, suff2 = the target's
// log density
template <int E>
__global__ __launch_bounds__(64) void k_refresh_dense_stats(EngineDev e, DenseParams dn) {
    const int lane = lane_id();
    const int64_t slot = blockIdx.x;
    if (slot >= e.K) return;
    AmTarget<E, TGT_DENSE, false> T;
    T.d = e.d; T.lane = lane; T.dn = dn;
    const double *xrow = e.x + slot * e.ld;
    double x[E], dummy[E], S, Q;
#pragma unroll
    for (int j = 0; j < E; ++j) x[j] = T.valid(j) ? xrow[64 * j + lane] : 0.0;
    const double l2 = T.template dense_and_sqr_norm<false, false>(x, dummy, S, x, Q);
    if (lane == 0) { e.suff[slot] = S; e.suff2[slot] = l2; }
}

int dense_launch(const DenseLaunch &L, const EngineDev &dev, const AmParams &ap, const DenseParams &dn) {
    return with_blocks_per_lane(L.E, [&](auto e_) {
        constexpr int E = decltype(e_)::value;
        if (L.slice) {
            if (L.full) launch_on(L.at, k_explore_dense_slice<E, true>, 64, 0, dev, ap, dn);
            else launch_on(L.at, k_explore_dense_slice<E, false>, 64, 0, dev, ap, dn);
        } else if (L.full) launch_on(L.at, k_explore_dense<E, false, true>, 64, 0, dev, ap, dn);
        else launch_on(L.at, k_explore_dense<E, false, false>, 64, 0, dev, ap, dn);
    });
}

int dense_refresh_stats(int E, unsigned N, hipStream_t stream, const EngineDev &dev, const DenseParams &dn) {
    return with_blocks_per_lane(E, [&](auto e_) {
        hipLaunchKernelGGL((k_refresh_dense_stats<decltype(e_)::value>), dim3(N), dim3(64), 0, stream, dev, dn);
    });
}

}  // namespace pte
