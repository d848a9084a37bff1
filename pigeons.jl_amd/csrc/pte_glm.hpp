// pte_glm.hpp -- the Bayesian-GLM family of the device engine (PTE_TARGET_BAYESIAN_GLM): the interpolated path
// (1 - beta) ScaledPrecisionNormal(p) + beta (log N(theta; 0, I / p) + sum_i l(y_i | x_i . theta)) explored by AutoMALA / MALA
// (automala_body) and by SliceSampler (its slice mode), one wave per replica, d <= 512.  The body and AmTarget are those of the funnel path
// (pte_automala.hpp); the target's log density and gradient (AmTarget<E, TGT_GLM, FULL, 1, LIK>::glm_and_sqr_norm) read the data, shared by
// every replica, from L2 on every evaluation and pass theta and r_i through the workgroup's dynamic LDS.
#pragma once
#include <hip/hip_ext.h>
#include "pte_automala.hpp"
#include "pte_glm_params.hpp"

namespace pte {

template <int E, int LIK, bool SLICE, bool FULL>
__global__ __launch_bounds__(64) void k_explore_glm(EngineDev e, AmParams ap, GlmParams gp) {
    automala_body<E, TGT_GLM, SLICE, FULL, false, 1, LIK>(e, ap, blockIdx.x, gp);
}

// swap statistics of every slot recomputed from the stored states (pte_set_state, pte_set_target_glm): suff = sum x^2, suff2 = the GLM's
// target log density.  (A body of its own: the target holds the reference's precision, and the data and this wave's LDS are set here, in the
// kernel -- PTE_REFRESH_STATS_BODY's T.load(gp) moved the schedule of these kernels: pte_automala.hpp)
template <int E, int LIK>
__global__ __launch_bounds__(64) void k_refresh_glm_stats(EngineDev e, GlmParams gp, double ref_prec) {
    extern __shared__ __attribute__((aligned(16))) double glm_lds[];
    const int lane = lane_id();
    const int64_t slot = blockIdx.x;
    if (slot >= e.K) return;
    AmTarget<E, TGT_GLM, false, 1, LIK> T;
    T.d = e.d; T.lane = lane;
    T.ref_nhp = -0.5 * ref_prec; T.ref_nprec = -ref_prec;
    T.gl = gp; T.glds = glm_lds;
    const double *xrow = e.x + slot * e.ld;
    double x[E];
#pragma unroll
    for (int j = 0; j < E; ++j) x[j] = T.valid(j) ? xrow[64 * j + lane] : 0.0;
    const double S = sqr_norm_regs<E>(x);
    const double l2 = T.target(x);
    if (lane == 0) { e.suff[slot] = S; e.suff2[slot] = l2; }
}

int glm_launch(const GlmLaunch &L, const EngineDev &dev, const AmParams &ap, const GlmParams &gp) {
    const size_t lds = glm_lds_bytes(L.E, gp.n_pad);
    return with_blocks_per_lane(L.E, [&](auto e_) {
        auto go = [&](auto p_) {
            constexpr int E = decltype(e_)::value, LIK = decltype(p_)::value;
            if (L.slice) launch_on(L.at, k_explore_glm<E, LIK, true, false>, 64, lds, dev, ap, gp);
            else if (L.full) launch_on(L.at, k_explore_glm<E, LIK, false, true>, 64, lds, dev, ap, gp);
            else launch_on(L.at, k_explore_glm<E, LIK, false, false>, 64, lds, dev, ap, gp);
        };
        if (L.lik == GLM_NORMAL_IDENTITY) go(std::integral_constant<int, GLM_NORMAL_IDENTITY>{});
        else go(std::integral_constant<int, GLM_BERNOULLI_LOGIT>{});
    });
}

int glm_refresh_stats(int E, int lik, unsigned N, hipStream_t stream, const EngineDev &dev, const GlmParams &gp, double ref_prec) {
    const size_t lds = glm_lds_bytes(E, gp.n_pad);
    return with_blocks_per_lane(E, [&](auto e_) {
        constexpr int EE = decltype(e_)::value;
        if (lik == GLM_NORMAL_IDENTITY) hipLaunchKernelGGL((k_refresh_glm_stats<EE, GLM_NORMAL_IDENTITY>), dim3(N), dim3(64), lds, stream, dev, gp, ref_prec);
        else hipLaunchKernelGGL((k_refresh_glm_stats<EE, GLM_BERNOULLI_LOGIT>), dim3(N), dim3(64), lds, stream, dev, gp, ref_prec);
    });
}

PTE_DEFINE_RNG_POLICY_SETTER(glm)

}  // namespace pte
