// pte_varsel.hpp -- the variable-selection family of the device engine (PTE_TARGET_VARIABLE_SELECTION): a spike-and-slab
// regression on the GLM family's data.  The state is [theta_0..theta_{d-1}, gamma_0..gamma_{d-1}], theta Float64 and gamma Bool (0.0 / 1.0),
// the effective coefficients are b_j = gamma_j theta_j, and the path is (1 - beta) ScaledPrecisionNormal(p)(theta) + beta target with
//   target = -(p/2) S + c_prior + G(gamma) + sum_i l_i(eta_i) + c_obs,  S = sum_j theta_j^2,  eta = X b,  G = m log pi + (d - m) log(1 - pi).
// The explorer is SliceSampler alone: its Float64 method on the thetas and its Bool method on the gammas, in state order, one wave per
// replica.  The state sits in registers (lane l holds coordinates 64 j + l); the linear predictor eta sits in the wave's LDS, lane l owning
// observations l, l + 64, ...: a proposal for coordinate j reads one column of X from L2 and costs O(n), not O(n d).
#pragma once
#include <hip/hip_ext.h>
#include "pte_automala.hpp"
#include "pte_varsel_params.hpp"

namespace pte {

// What one wave knows about its replica while it explores: the state in registers, eta in LDS, and the sums of the committed state.
template <int E, int LIK, bool FULL>
struct VarselChain {
    VarselParams vp;
    double *eta, *st;               // LDS: eta [n_pad] (lane l reads and writes entries 64 m + l only), the staged state [64 E]
    int lane, d, nb;                // d columns (the state has 2 d coordinates), nb = n_pad / 64
    double beta, omb, ref_nhp;
    double x[E];                    // the committed state
    double S, m, ls;                // of the committed state: sum theta^2 (fixed tree), sum gamma, sum_i l_i(eta_i) of the eta in LDS

    __device__ __forceinline__ bool valid(int j) const { return FULL || 64 * j + lane < 2 * d; }
    // coordinate idx of v (uniform idx), as a uniform value
    __device__ __forceinline__ double get(const double (&v)[E], int idx) const {
        double out = 0.0;
#pragma unroll
        for (int j = 0; j < E; ++j) { const double t = readlane_f64(v[j], idx & 63); out = (idx >> 6) == j ? t : out; }
        return out;
    }
    __device__ __forceinline__ double lik(double e, double yi) const {
        if constexpr (LIK == GLM_BERNOULLI_LOGIT) {
            const double t = exp(-fabs(e));             // softplus(e) = max(e, 0) + log1p(exp(-|e|)), as DESIGN 4.9
            return yi * e - (fmax(e, 0.0) + log1p(t));
        } else {
            const double res = yi - e;
            return -(res * res) * vp.w2;
        }
    }
    // S = sum theta^2 of v and the 64 lane sums `lsum`, over the fixed tree in lockstep (the lane sums in block 0, as DESIGN 4.9)
    __device__ __forceinline__ void sums(const double (&v)[E], double lsum, double &S_out, double &ls_out) const {
        double t[2][E], out[2];
#pragma unroll
        for (int j = 0; j < E; ++j) {
            t[0][j] = 64 * j + lane < d ? v[j] * v[j] : 0.0;
            t[1][j] = j == 0 ? lsum : 0.0;
        }
        tree_sum_regs_multi<E, 2>(t, out);
        S_out = out[0]; ls_out = out[1];
    }
    // the target's log density and the path's, from the three sums
    __device__ __forceinline__ double target_lp(double S_, double m_, double ls_) const {
        const double G = m_ * vp.log_pi + ((double)d - m_) * vp.log_1mpi;
        return ((((ref_nhp * S_) + vp.c_prior) + G) + ls_) + vp.c_obs;
    }
    __device__ __forceinline__ double path_lp(double S_, double m_, double ls_) const {
        if (beta == 0.0) return ref_nhp * S_;
        const double l2 = target_lp(S_, m_, ls_);
        if (beta == 1.0) return l2;
        return omb * (ref_nhp * S_) + beta * l2;
    }
    // eta of the committed state in full, sequential in j with one fused multiply-add per term, then S, m and ls.  The state goes through
    // LDS so that every lane reads b_j = gamma_j theta_j as a broadcast.  Uniform control flow: the barriers are the one wave's own.
    __device__ __forceinline__ void load_sums() {
        constexpr int CH = 4;                           // blocks of observations per pass over the columns
        __syncthreads();
#pragma unroll
        for (int j = 0; j < E; ++j) st[64 * j + lane] = x[j];
        __syncthreads();
        double lsum = 0.0;
        for (int m0 = 0; m0 < nb; m0 += CH) {
            int off[CH];
            double acc[CH];
#pragma unroll
            for (int c = 0; c < CH; ++c) { off[c] = 64 * min(m0 + c, nb - 1) + lane; acc[c] = 0.0; }
            const double *col = vp.xc;
            for (int j = 0; j < d; ++j, col += vp.n_pad) {
                const double b = st[d + j] * st[j];     // one address each: broadcasts
#pragma unroll
                for (int c = 0; c < CH; ++c) acc[c] = __builtin_fma(col[off[c]], b, acc[c]);
            }
#pragma unroll
            for (int c = 0; c < CH; ++c) {
                if (m0 + c >= nb) break;
                const int i = 64 * (m0 + c) + lane;
                eta[i] = acc[c];
                const double l = lik(acc[c], vp.y[i]);
                if (i < vp.n) lsum = lsum + l;          // padded observations contribute exactly 0
            }
        }
        double gm[E];
#pragma unroll
        for (int j = 0; j < E; ++j) { const int i = 64 * j + lane; gm[j] = (i >= d && i < 2 * d) ? x[j] : 0.0; }
        m = tree_sum_regs<E>(gm);                       // (a sum of zeros and ones: exact in any order)
        sums(x, lsum, S, ls);
    }
    // sum_i l_i of eta' = fma(X_c, b_new, fma(X_c, -b_old, eta)): column c of X from L2, eta from LDS, lanes over observations
    __device__ __forceinline__ double column_pass(int c, double b_old, double b_new) const {
        const double *col = vp.xc + (int64_t)c * vp.n_pad + lane, *yp = vp.y + lane;
        const double *ep = eta + lane;
        const double nbo = -b_old;
        double lsum = 0.0;
#pragma unroll 4
        for (int i0 = 0; i0 < vp.n_pad; i0 += 64) {
            const double xv = col[i0];
            const double e = __builtin_fma(xv, b_new, __builtin_fma(xv, nbo, ep[i0]));
            const double l = lik(e, yp[i0]);
            if (i0 + lane < vp.n) lsum = lsum + l;
        }
        return lsum;
    }
    __device__ __forceinline__ void column_commit(int c, double b_old, double b_new) {
        const double *col = vp.xc + (int64_t)c * vp.n_pad + lane;
        double *ep = eta + lane;
        const double nbo = -b_old;
#pragma unroll 4
        for (int i0 = 0; i0 < vp.n_pad; i0 += 64) {
            const double xv = col[i0];
            ep[i0] = __builtin_fma(xv, b_new, __builtin_fma(xv, nbo, ep[i0]));
        }
    }
};

// One sweep of SliceSampler over the 2 d coordinates in state order, n_passes times (slice_sample! :43-62): the Float64 method on the
// thetas, the Bool method on the gammas (slice_coord<double>, slice_coord_bool: pte_slice_coord.hpp).  The log
// potential of a proposal v for coordinate idx is evaluated from the cached predictor: with column c = idx mod d and b_old, b_new the
// effective coefficient of c before and at the proposal, eta' = fma(X_c, b_new, fma(X_c, -b_old, eta)) -- or eta itself when b_new == b_old
// (a theta whose indicator is off never touches the likelihood) -- and S, m follow the proposal.  When a coordinate is done its final value
// is committed the same way.  All control flow is uniform: every value it branches on comes out of a wave reduction or a uniform draw.
template <int E, int LIK, bool FULL>
__global__ __launch_bounds__(64) void k_explore_varsel(EngineDev e, AmParams ap, VarselParams vp) {
    extern __shared__ __attribute__((aligned(16))) double varsel_lds[];
    const int lane = lane_id();
    const int64_t cl = blockIdx.x;
    if (cl >= e.K) return;
    const int64_t c = e.c0 + cl;
    const int slot = e.slot_of_chain[cl];
    const int d = vp.d;
    double *xrow = e.x + (int64_t)slot * e.ld;
    VarselChain<E, LIK, FULL> T;
    T.vp = vp; T.eta = varsel_lds; T.st = varsel_lds + vp.n_pad;
    T.lane = lane; T.d = d; T.nb = vp.n_pad >> 6;
    T.beta = e.beta[c]; T.omb = 1.0 - T.beta; T.ref_nhp = -0.5 * ap.ref_prec;

    if (is_ref_chain(e, c)) {
        if (e.compose_phase == 2) return;
        const double lp0 = lp_before_explore(e, c, slot);
        // i.i.d. from the reference: d normals at the reference's precision (as iid_refresh draws them), then one rand(rng, Bool) per indicator
        SeqRng r0{e.rng[2 * slot], e.rng[2 * slot + 1]};
        const double sd = e.sd[c];
        for (int b = 0; 64 * b < d; ++b) {
            const int nl = min(64, d - 64 * b);
            const double v = wave_randn_block(r0, lane, nl) / sd;
            if (lane < nl) xrow[64 * b + lane] = v;
        }
        const unsigned bb = rng_bool_bit();              // include/pte_rng_policy.h (default 0: `% Bool`)
        for (int s = lane; s < d; s += 64) xrow[d + s] = (double)((mix64(r0.seed + (uint64_t)(s + 1) * r0.gamma) >> bb) & 1ull);
        r0.seed += (uint64_t)d * r0.gamma;
        __threadfence_block();
#pragma unroll
        for (int j = 0; j < E; ++j) T.x[j] = T.valid(j) ? xrow[64 * j + lane] : 0.0;
        T.load_sums();
        const double l20 = T.target_lp(T.S, T.m, T.ls);
        if (lane == 0) { e.suff[slot] = T.S; e.suff2[slot] = l20; e.rng[2 * slot] = r0.seed; }
        record_after_explore_impl(e, cl, c, slot, lane, lp0, T.S, l20);
        return;
    }
    const double lp_before = lp_before_explore(e, c, slot);
#pragma unroll
    for (int j = 0; j < E; ++j) T.x[j] = T.valid(j) ? xrow[64 * j + lane] : 0.0;
    T.load_sums();

    WaveDraws dr;
    dr.init(e.rng[2 * slot], e.rng[2 * slot + 1], lane);
    SliceTally tally;
    double lp = T.path_lp(T.S, T.m, T.ls);                     // cached_log_potential (:32-41)
    if (lp == -INFINITY) { if (lane == 0) set_error(e, ERR_SLICE_SUPPORT, (int)c, -1); return; }
    const SliceKnobs kn{ap.slice_w, 1.1 * ap.slice_w, ap.slice_p, ap.slice_max_iter};
    // coordinate idx (column col, committed at xold) for slice_coord / slice_coord_bool (pte_slice_coord.hpp)
    struct Coord {
        VarselChain<E, LIK, FULL> &T;
        int idx, col;
        bool is_theta, tempered;                               // beta == 0: the path is the reference alone, eta is never read
        double xold, other, b_old;                             // other: the indicator of a theta, the theta of an indicator
        double S_v, m_v, ls_v;                                 // the sums of the state with the coordinate at the last evaluated v
        double S_h, m_h, ls_h;                                 // those of the proposal
        __device__ __forceinline__ double eval(double v) {
            double xv[E];
#pragma unroll
            for (int j = 0; j < E; ++j) xv[j] = (idx >> 6) == j && T.lane == (idx & 63) ? v : T.x[j];
            const double b_new = is_theta ? other * v : v * other;
            m_v = is_theta ? T.m : (T.m - xold) + v;
            double lsum = 0.0;
            const bool moved = tempered && b_new != b_old;
            if (moved) lsum = T.column_pass(col, b_old, b_new);
            T.sums(xv, lsum, S_v, ls_v);
            if (!moved) ls_v = T.ls;
            return T.path_lp(S_v, m_v, ls_v);
        }
        __device__ __forceinline__ void hold() { S_h = S_v; m_h = m_v; ls_h = ls_v; }
        __device__ __forceinline__ void commit(double v) {
            const double b_new = is_theta ? other * v : v * other;
            if (tempered && b_new != b_old) T.column_commit(col, b_old, b_new);
#pragma unroll
            for (int j = 0; j < E; ++j) T.x[j] = (idx >> 6) == j && T.lane == (idx & 63) ? v : T.x[j];
            T.S = S_h; T.m = m_h; T.ls = ls_h;
        }
    };
    for (int pass = 0; pass < ap.slice_n_passes; ++pass) {
        for (int idx = 0; idx < 2 * d; ++idx) {
            const bool is_theta = idx < d;
            const double xold = T.get(T.x, idx);
            const double other = T.get(T.x, is_theta ? idx + d : idx - d);
            Coord coord{T, idx, is_theta ? idx : idx - d, is_theta, T.beta != 0.0, xold, other, is_theta ? other * xold : xold * other, T.S, T.m, T.ls};
            const int err = is_theta ? slice_coord<double>(coord, dr, lane, kn, tally, xold, kn.w, lp) : slice_coord_bool(coord, dr, lane, xold, lp);
            if (err) { if (lane == 0) set_error(e, err, (int)c, idx); return; }
        }
    }
#pragma unroll
    for (int j = 0; j < E; ++j) if (T.valid(j)) xrow[64 * j + lane] = T.x[j];
    T.load_sums();                                             // the swap statistics as k_refresh_varsel_stats computes them: eta in full
    const double l2 = T.target_lp(T.S, T.m, T.ls);
    if (lane == 0) {
        e.suff[slot] = T.S; e.suff2[slot] = l2;
        e.rng[2 * slot] = dr.final_seed();
        e.expl_steps_sum[cl] += (double)tally.steps_sum; e.expl_steps_n[cl] += tally.steps_n;
        e.expl_acc_sum[cl] += tally.acc_sum;             e.expl_acc_n[cl] += tally.acc_n;
    }
    record_after_explore(e, cl, c, slot, lane, lp_before, T.S, l2);
}

// swap statistics of every slot recomputed from the stored states (pte_set_state, pte_set_target_varsel): suff = sum theta^2, suff2 = the
// target's log density
template <int E, int LIK>
__global__ __launch_bounds__(64) void k_refresh_varsel_stats(EngineDev e, VarselParams vp, double ref_prec) {
    extern __shared__ __attribute__((aligned(16))) double varsel_lds[];
    const int lane = lane_id();
    const int64_t slot = blockIdx.x;
    if (slot >= e.K) return;
    VarselChain<E, LIK, false> T;
    T.vp = vp; T.eta = varsel_lds; T.st = varsel_lds + vp.n_pad;
    T.lane = lane; T.d = vp.d; T.nb = vp.n_pad >> 6;
    T.beta = 1.0; T.omb = 0.0; T.ref_nhp = -0.5 * ref_prec;
    const double *xrow = e.x + slot * e.ld;
#pragma unroll
    for (int j = 0; j < E; ++j) T.x[j] = T.valid(j) ? xrow[64 * j + lane] : 0.0;
    T.load_sums();
    const double l2 = T.target_lp(T.S, T.m, T.ls);
    if (lane == 0) { e.suff[slot] = T.S; e.suff2[slot] = l2; }
}

int varsel_launch(const VarselLaunch &L, const EngineDev &dev, const AmParams &ap, const VarselParams &vp) {
    const size_t lds = varsel_lds_bytes(L.E, vp.n_pad);
    return with_blocks_per_lane(L.E, [&](auto e_) {
        auto go = [&](auto lik_) {
            constexpr int E = decltype(e_)::value, LIK = decltype(lik_)::value;
            if (L.full) launch_on(L.at, k_explore_varsel<E, LIK, true>, 64, lds, dev, ap, vp);
            else launch_on(L.at, k_explore_varsel<E, LIK, false>, 64, lds, dev, ap, vp);
        };
        if (L.lik == GLM_NORMAL_IDENTITY) go(std::integral_constant<int, GLM_NORMAL_IDENTITY>{});
        else go(std::integral_constant<int, GLM_BERNOULLI_LOGIT>{});
    });
}

int varsel_refresh_stats(int E, int lik, unsigned N, hipStream_t stream, const EngineDev &dev, const VarselParams &vp, double ref_prec) {
    const size_t lds = varsel_lds_bytes(E, vp.n_pad);
    return with_blocks_per_lane(E, [&](auto e_) {
        constexpr int EE = decltype(e_)::value;
        if (lik == GLM_NORMAL_IDENTITY) hipLaunchKernelGGL((k_refresh_varsel_stats<EE, GLM_NORMAL_IDENTITY>), dim3(N), dim3(64), lds, stream, dev, vp, ref_prec);
        else hipLaunchKernelGGL((k_refresh_varsel_stats<EE, GLM_BERNOULLI_LOGIT>), dim3(N), dim3(64), lds, stream, dev, vp, ref_prec);
    });
}

PTE_DEFINE_RNG_POLICY_SETTER(varsel)

}  // namespace pte
