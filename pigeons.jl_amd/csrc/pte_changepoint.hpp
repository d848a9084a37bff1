// pte_changepoint.hpp -- the Poisson change-point family of the device engine (PTE_TARGET_CHANGE_POINT): K change points on n
// counts.  The state is [r_0..r_K, tau_1..tau_K], the K + 1 log rates Float64 and the K change points Integer (integral doubles in 0..n,
// unordered); with s_1 <= ... <= s_K the sorted taus, s_0 = 0 and s_{K+1} = n, segment j covers observations [s_j, s_{j+1}) and
//   target = -(p/2) S + c_prior + c_tau + sum_j t_j + c_obs,   S = sum_j r_j^2,   t_j = Y_j r_j - len_j exp(r_j)  (0 when len_j = 0),
// Y_j = C[s_{j+1}] - C[s_j] from the prefix table C.  The path is (1 - beta) ScaledPrecisionNormal(p)(r) + beta target, -inf when a tau
// is outside 0..n.  The explorer is SliceSampler alone: its Float64 method on the rates and its Integer method on the taus, in state order,
// one wave per replica.  Lane j holds segment j: its rate, exp of it, its bounds s_j, s_{j+1} and C at them; lane i < K also holds
// tau_{i+1}.  2 K + 1 <= 127 coordinates sit in two registers per lane whatever the dim is, so the kernels have no blocks-per-lane parameter.
//
// Two evaluation forms, the same bits (every term is a function of (r_j, s_j, s_{j+1}) alone and the tree is fixed):
//   full    every proposal ranks the K taus (K cross-lane compares), scatters them into sorted order, gathers C and takes exp of every rate;
//   cached  the sorted bounds, C at them and exp(r_j) are kept for the committed state.  A rate proposal takes one exp and neither a sort
//           nor a gather.  A tau proposal removes the tau's old value from the sorted sequence and inserts the new one: the insert
//           position is a ballot and a popcount, and the lanes between the two positions take their neighbour's bound.  Which neighbour
//           that is depends on the removed position alone, so the shifted bounds (and C at them) are formed once per coordinate
//           (TauMove: six cross-lane moves); a proposal then costs the ballot, one load of C at the proposed value -- one address for
//           the wave -- and selects.
#pragma once
#include <hip/hip_ext.h>
#include "pte_automala.hpp"
#include "pte_changepoint_params.hpp"

namespace pte {

// What one wave knows about its replica: the committed state and what the evaluation of it left.
template <bool CACHED>
struct ChangepointChain {
    ChangepointParams cp;
    int lane, K, n;
    double beta, omb, ref_nhp;
    double r;                       // lane j <= K: the log rate of segment j (0 above)
    int tau;                        // lane i < K: tau_{i+1} (n above: the sort leaves those lanes where they are)
    // of an evaluated state: exp(r), the segment's bounds (lane j: s_j and s_{j+1}; n from lane K on) from the sorted taus, C there, and the two sums
    struct Eval { double er; int lo, hi; double Clo, Chi; double S, ls; };
    // what a proposal for one tau starts from: the committed bounds without the tau's own value (at sorted position rho), as the lanes below
    // the insert position see them (`below`: position m of that sequence) and as the lanes above it do (`above`: position m - 1), and the
    // same for the lower bounds of the lanes two or more above it (`above2`: position m - 2)
    struct TauMove { int below, above, above2; double Cbelow, Cabove, Cabove2; };
    Eval com;                       // of the committed state

    // lane j: s_{j+1} of the taus tv.  Rank by value, ties by lane; the taus are a permutation of the ranks, so every lane below K receives one.
    __device__ __forceinline__ int sorted(int tv) const {
        int cnt = 0;
        for (int m = 0; m < K; ++m) {
            const int t = __builtin_amdgcn_readlane(tv, m);
            cnt += (t < tv || (t == tv && m < lane)) ? 1 : 0;
        }
        const int rank = lane < K ? cnt : lane;
        return __builtin_amdgcn_ds_permute(rank << 2, tv);
    }
    // t_j of lane j from its rate, exp of it, its bounds and C there
    __device__ __forceinline__ double term(double rv, const Eval &o) const {
        const double len = (double)(o.hi - o.lo), Y = o.Chi - o.Clo;
        const double t = (Y * rv) - (len * o.er);
        return (lane <= K && len != 0.0) ? t : 0.0;      // an empty segment contributes 0 whatever its rate (0 * inf otherwise)
    }
    // the value of the lane below (lane 0: `first`)
    __device__ __forceinline__ int from_below(int v, int first) const { const int t = __shfl_up(v, 1, 64); return lane == 0 ? first : t; }
    __device__ __forceinline__ double from_below(double v, double first) const { const double t = __shfl_up(v, 1, 64); return lane == 0 ? first : t; }
    __device__ __forceinline__ void sums(double rv, double t, double &S_out, double &ls_out) const {
        double v[2][1], out[2];
        v[0][0] = lane <= K ? rv * rv : 0.0;
        v[1][0] = t;
        tree_sum_regs_multi<1, 2>(v, out);
        S_out = out[0]; ls_out = out[1];
    }
    __device__ __forceinline__ double target_lp(double S_, double ls_) const {
        return ((((ref_nhp * S_) + cp.c_prior) + cp.c_tau) + ls_) + cp.c_obs;
    }
    __device__ __forceinline__ double path_lp(double S_, double ls_) const {
        if (beta == 0.0) return ref_nhp * S_;
        const double l2 = target_lp(S_, ls_);
        if (beta == 1.0) return l2;
        return omb * (ref_nhp * S_) + beta * l2;
    }
    // the state (rv, tv) in full; tv in 0..n
    __device__ __forceinline__ void full(double rv, int tv, Eval &o) const {
        o.er = exp(rv);
        o.hi = sorted(tv);
        o.Chi = cp.C[o.hi];
        o.lo = from_below(o.hi, 0);                     // s_0 = 0, C[0] = 0
        o.Clo = from_below(o.Chi, 0.0);
        sums(rv, term(rv, o), o.S, o.ls);
    }
    // the stored state; false (and every tau clamped into the table) if a tau is outside 0..n: the path is -inf there
    __device__ __forceinline__ bool load(const double *xrow) {
        r = lane <= K ? xrow[lane] : 0.0;
        const double t = lane < K ? xrow[K + 1 + lane] : (double)n;
        const bool out = !(t >= 0.0 && t <= (double)n);
        tau = out ? 0 : (int)t;
        full(r, tau, com);
        return ballot64(out) == 0ull;
    }
    // the path at rate idx = v
    __device__ __forceinline__ double eval_rate(int idx, double v, Eval &o) const {
        const double rv = lane == idx ? v : r;
        if constexpr (CACHED) {
            const double ev = exp(v);
            o = com;
            o.er = lane == idx ? ev : com.er;
            sums(rv, term(rv, o), o.S, o.ls);
        } else {
            full(rv, tau, o);
        }
        return path_lp(o.S, o.ls);
    }
    // the committed bounds without the one at sorted position rho (uniform), seen from below and from above the insert position.  With
    // u the sequence without rho, u[m] = hi[m] below rho and hi[m + 1] from rho on; hi[m - 1] is lane m's own lower bound.
    __device__ __forceinline__ TauMove tau_move(int rho) const {
        TauMove t;
        const int up = __shfl_down(com.hi, 1, 64);
        const double Cup = __shfl_down(com.Chi, 1, 64);
        t.below = lane < rho ? com.hi : up;                     t.Cbelow = lane < rho ? com.Chi : Cup;             // u[m]
        t.above = lane - 1 < rho ? com.lo : com.hi;             t.Cabove = lane - 1 < rho ? com.Clo : com.Chi;     // u[m - 1], m >= 1
        const int lo2 = from_below(com.lo, 0);
        const double Clo2 = from_below(com.Clo, 0.0);
        t.above2 = lane - 2 < rho ? lo2 : com.lo;               t.Cabove2 = lane - 2 < rho ? Clo2 : com.Clo;       // u[m - 2], m >= 2
        return t;
    }
    // the path at tau_{i+1} = v (integral); mv: tau_move of a lane whose sorted bound is tau_{i+1}'s committed value
    __device__ __forceinline__ double eval_tau(int i, int rho, const TauMove &mv, double v, Eval &o) const {
        if (!(v >= 0.0 && v <= (double)n)) return -INFINITY;
        const int iv = (int)v;
        if constexpr (CACHED) {
            // the other K - 1 bounds below iv are a prefix of the sequence u without lane rho's: iv goes to position q of it, and the new
            // sorted sequence is u[m] below q, iv at q, u[m - 1] above; a lane's lower bound is that sequence one position down
            const int q = __popcll(ballot64(lane < K && lane != rho && com.hi < iv));
            const double Civ = cp.C[iv];                         // one address: a broadcast
            o.hi = lane < q ? mv.below : (lane == q ? iv : mv.above);
            o.Chi = lane < q ? mv.Cbelow : (lane == q ? Civ : mv.Cabove);
            o.lo = lane - 1 < q ? mv.above : (lane - 1 == q ? iv : mv.above2);
            o.Clo = lane - 1 < q ? mv.Cabove : (lane - 1 == q ? Civ : mv.Cabove2);
            if (lane == 0) { o.lo = 0; o.Clo = 0.0; }
            o.er = com.er;
            o.S = com.S;
            double t[1] = {term(r, o)};
            o.ls = tree_sum_regs<1>(t);
        } else {
            full(r, lane == i ? iv : tau, o);
        }
        return path_lp(o.S, o.ls);
    }
};

// One sweep of SliceSampler over the 2 K + 1 coordinates in state order, n_passes times (slice_sample! :43-62): the Float64 method on the
// rates and the Integer method on the taus (slice_coord<double>, slice_coord<int64_t>: pte_slice_coord.hpp).  All control flow is uniform:
// every value it branches on comes out of a wave reduction or a uniform draw.
template <bool CACHED>
__global__ __launch_bounds__(64) void k_explore_changepoint(EngineDev e, AmParams ap, ChangepointParams cp) {
    const int lane = lane_id();
    const int64_t cl = blockIdx.x;
    if (cl >= e.K) return;
    const int64_t c = e.c0 + cl;
    const int slot = e.slot_of_chain[cl];
    const int K = cp.K, n = cp.n;
    double *xrow = e.x + (int64_t)slot * e.ld;
    using Chain = ChangepointChain<CACHED>;
    Chain T;
    T.cp = cp; T.lane = lane; T.K = K; T.n = n;
    T.beta = e.beta[c]; T.omb = 1.0 - T.beta; T.ref_nhp = -0.5 * ap.ref_prec;

    if (is_ref_chain(e, c)) {
        if (e.compose_phase == 2) return;
        const double lp0 = lp_before_explore(e, c, slot);
        // i.i.d. from the reference: K + 1 normals at the reference's precision (as iid_refresh draws them), then rand(rng, 0:n) per tau
        SeqRng r0{e.rng[2 * slot], e.rng[2 * slot + 1]};
        const double v = wave_randn_block(r0, lane, K + 1) / e.sd[c];
        if (lane <= K) xrow[lane] = v;
        for (int k = 0; k < K; ++k) {
            const int64_t t = rand_range0_from([&]() { return r0.next(); }, (uint64_t)n + 1ull);
            if (lane == k) xrow[K + 1 + k] = (double)t;
        }
        __threadfence_block();
        T.load(xrow);
        const double l20 = T.target_lp(T.com.S, T.com.ls);
        if (lane == 0) { e.suff[slot] = T.com.S; e.suff2[slot] = l20; e.rng[2 * slot] = r0.seed; }
        record_after_explore_impl(e, cl, c, slot, lane, lp0, T.com.S, l20);
        return;
    }
    const double lp_before = lp_before_explore(e, c, slot);
    const bool inside = T.load(xrow);

    WaveDraws dr;
    dr.init(e.rng[2 * slot], e.rng[2 * slot + 1], lane);
    SliceTally tally;
    double lp = inside ? T.path_lp(T.com.S, T.com.ls) : -INFINITY;       // cached_log_potential (:32-41)
    if (lp == -INFINITY) { if (lane == 0) set_error(e, ERR_SLICE_SUPPORT, (int)c, -1); return; }
    const SliceKnobs kn{ap.slice_w, 1.1 * ap.slice_w, ap.slice_p, ap.slice_max_iter};
    // coordinate idx for slice_coord (pte_slice_coord.hpp): rate idx, or the tau of lane ti
    struct Coord {
        Chain &T;
        int idx, ti, rho;
        bool is_rate;
        typename Chain::TauMove mv;
        typename Chain::Eval ev, cand;                           // of the last evaluation, of the proposal
        __device__ __forceinline__ double eval(double v) { return is_rate ? T.eval_rate(idx, v, ev) : T.eval_tau(ti, rho, mv, v, ev); }
        __device__ __forceinline__ void hold() { cand = ev; }
        __device__ __forceinline__ void commit(double v) {
            if (is_rate) T.r = T.lane == idx ? v : T.r; else T.tau = T.lane == ti ? (int)v : T.tau;
            T.com = cand;
        }
    };
    const int64_t width = (int64_t)ceil(kn.w);
    for (int pass = 0; pass < ap.slice_n_passes; ++pass) {
        for (int idx = 0; idx < 2 * K + 1; ++idx) {
            const bool is_rate = idx <= K;
            const int ti = idx - K - 1;                          // the tau's lane
            const double xold = is_rate ? readlane_f64(T.r, idx) : (double)__builtin_amdgcn_readlane(T.tau, max(ti, 0));
            Coord coord{T, idx, ti, 0, is_rate};
            if (CACHED && !is_rate) {
                coord.rho = (int)__builtin_ctzll(ballot64(lane < K && T.com.hi == (int)xold));
                coord.mv = T.tau_move(coord.rho);
            }
            const int err = is_rate ? slice_coord<double>(coord, dr, lane, kn, tally, xold, kn.w, lp)
                                    : slice_coord<int64_t>(coord, dr, lane, kn, tally, (int64_t)xold, width, lp);
            if (err) { if (lane == 0) set_error(e, err, (int)c, idx); return; }
        }
    }
    if (lane <= K) xrow[lane] = T.r;
    if (lane < K) xrow[K + 1 + lane] = (double)T.tau;
    typename Chain::Eval fin;                                  // the swap statistics as k_refresh_changepoint_stats computes them: in full
    T.full(T.r, T.tau, fin);
    const double l2 = T.target_lp(fin.S, fin.ls);
    if (lane == 0) {
        e.suff[slot] = fin.S; e.suff2[slot] = l2;
        e.rng[2 * slot] = dr.final_seed();
        e.expl_steps_sum[cl] += (double)tally.steps_sum; e.expl_steps_n[cl] += tally.steps_n;
        e.expl_acc_sum[cl] += tally.acc_sum;             e.expl_acc_n[cl] += tally.acc_n;
    }
    record_after_explore(e, cl, c, slot, lane, lp_before, fin.S, l2);
}

// swap statistics of every slot recomputed from the stored states (pte_set_state, pte_set_target_changepoint): suff = sum r^2, suff2 = the
// target's log density (-inf with a tau outside 0..n)
__global__ __launch_bounds__(64) void k_refresh_changepoint_stats(EngineDev e, ChangepointParams cp, double ref_prec) {
    const int lane = lane_id();
    const int64_t slot = blockIdx.x;
    if (slot >= e.K) return;
    ChangepointChain<false> T;
    T.cp = cp; T.lane = lane; T.K = cp.K; T.n = cp.n;
    T.beta = 1.0; T.omb = 0.0; T.ref_nhp = -0.5 * ref_prec;
    const bool inside = T.load(e.x + slot * e.ld);
    const double l2 = inside ? T.target_lp(T.com.S, T.com.ls) : -INFINITY;
    if (lane == 0) { e.suff[slot] = T.com.S; e.suff2[slot] = l2; }
}

int changepoint_launch(const ChangepointLaunch &L, const EngineDev &dev, const AmParams &ap, const ChangepointParams &cp) {
    if (L.cached) launch_on(L.at, k_explore_changepoint<true>, 64, 0, dev, ap, cp);
    else launch_on(L.at, k_explore_changepoint<false>, 64, 0, dev, ap, cp);
    return 0;
}

int changepoint_refresh_stats(unsigned N, hipStream_t stream, const EngineDev &dev, const ChangepointParams &cp, double ref_prec) {
    hipLaunchKernelGGL(k_refresh_changepoint_stats, dim3(N), dim3(64), 0, stream, dev, cp, ref_prec);
    return 0;
}

PTE_DEFINE_RNG_POLICY_SETTER(changepoint)

}  // namespace pte
