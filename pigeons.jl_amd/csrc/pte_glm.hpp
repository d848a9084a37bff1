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
    automala_body<E, TGT_GLM, SLICE, FULL, false, 1, LIK>(e, ap, blockIdx.x, MixParams{}, gp);
}

// swap statistics of every slot recomputed from the stored states (pte_set_state, pte_set_target_glm): suff = sum x^2, suff2 = the GLM's
// target log density
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
    const double l2 = T.glm(x);
    if (lane == 0) { e.suff[slot] = S; e.suff2[slot] = l2; }
}

int glm_launch(const GlmLaunch &L, const EngineDev &dev, const AmParams &ap, const GlmParams &gp) {
    const size_t lds = glm_lds_bytes(L.E, gp.n_pad);
#define GLM_LIK(EE, LL)                                                                                         \
    if (L.slice) launch_on(L.at, k_explore_glm<EE, LL, true, false>, 64, lds, dev, ap, gp);                            \
    else if (L.full) launch_on(L.at, k_explore_glm<EE, LL, false, true>, 64, lds, dev, ap, gp);                        \
    else launch_on(L.at, k_explore_glm<EE, LL, false, false>, 64, lds, dev, ap, gp);
#define GLM_ONE(EE)                                                                                             \
    if (L.lik == GLM_NORMAL_IDENTITY) { GLM_LIK(EE, GLM_NORMAL_IDENTITY) } else { GLM_LIK(EE, GLM_BERNOULLI_LOGIT) }
    switch (L.E) {
    case 1: GLM_ONE(1) break; case 2: GLM_ONE(2) break; case 4: GLM_ONE(4) break; case 8: GLM_ONE(8) break;
    default: return 1;
    }
#undef GLM_ONE
#undef GLM_LIK
    return 0;
}

int glm_refresh_stats(int E, int lik, unsigned N, hipStream_t stream, const EngineDev &dev, const GlmParams &gp, double ref_prec) {
    const size_t lds = glm_lds_bytes(E, gp.n_pad);
#define GLM_REFRESH(EE)                                                                                                                    \
    if (lik == GLM_NORMAL_IDENTITY) hipLaunchKernelGGL((k_refresh_glm_stats<EE, GLM_NORMAL_IDENTITY>), dim3(N), dim3(64), lds, stream, dev, gp, ref_prec); \
    else hipLaunchKernelGGL((k_refresh_glm_stats<EE, GLM_BERNOULLI_LOGIT>), dim3(N), dim3(64), lds, stream, dev, gp, ref_prec);
    switch (E) {
    case 1: GLM_REFRESH(1) break; case 2: GLM_REFRESH(2) break; case 4: GLM_REFRESH(4) break; case 8: GLM_REFRESH(8) break;
    default: return 1;
    }
#undef GLM_REFRESH
    return 0;
}

PTE_DEFINE_RNG_POLICY_SETTER(glm)

}  // namespace pte
