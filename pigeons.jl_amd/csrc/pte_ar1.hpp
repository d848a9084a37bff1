// pte_ar1.hpp -- the latent-AR(1) state-space family of the device engine (PTE_TARGET_LATENT_AR1): T observations y_t of a latent
// state h_t | h_{t-1} ~ N(mu + phi (h_{t-1} - mu), sigma^2), h_0 from the stationary law, phi = tanh(a), sigma = exp(ls), the state
// x = [mu, a, ls, h_0 .. h_{T-1}], observed as y_t ~ N(0, exp(h_t)) (stochastic volatility) or y_t ~ N(h_t, obs_sd^2).  The interpolated path
// (1 - beta) ScaledPrecisionNormal(p) + beta target is explored by AutoMALA / MALA (automala_body) and by SliceSampler (its slice mode), one
// wave per replica, 4 <= d <= 512.  The body and AmTarget are those of the funnel path (pte_automala.hpp); the target's log density and gradient
// are AmTarget<E, TGT_AR1, FULL, 1, LIK>::ar1_and_sqr_norm, which takes every coordinate's neighbour from the lane next to it with a DPP wave
// shift.  Compiled inside pte_glm.hip (pte_automala_params.hpp).
#pragma once
#include <hip/hip_ext.h>
#include "pte_automala.hpp"
#include "pte_ar1_params.hpp"

namespace pte {

template <int E, int LIK, bool SLICE, bool FULL>
__global__ __launch_bounds__(64) void k_explore_ar1(EngineDev e, AmParams ap, Ar1Params ar) {
    automala_body<E, TGT_AR1, SLICE, FULL, false, 1, LIK>(e, ap, blockIdx.x, MixParams{}, GlmParams{}, MixModelParams{}, HierParams{}, ar);
}

// swap statistics of every slot recomputed from the stored states (pte_set_state, pte_set_target_ar1): suff = sum x^2, suff2 = the target's
// log density
template <int E, int LIK>
__global__ __launch_bounds__(64) void k_refresh_ar1_stats(EngineDev e, Ar1Params ar) {
    const int lane = lane_id();
    const int64_t slot = blockIdx.x;
    if (slot >= e.K) return;
    AmTarget<E, TGT_AR1, false, 1, LIK> T;
    T.d = e.d; T.lane = lane;
    T.load_ar1(ar);
    const double *xrow = e.x + slot * e.ld;
    double x[E];
#pragma unroll
    for (int j = 0; j < E; ++j) x[j] = T.valid(j) ? xrow[64 * j + lane] : 0.0;
    const double S = sqr_norm_regs<E>(x);
    const double l2 = T.ar1(x);
    if (lane == 0) { e.suff[slot] = S; e.suff2[slot] = l2; }
}

int ar1_launch(const Ar1Launch &L, const EngineDev &dev, const AmParams &ap, const Ar1Params &ar) {
#define AR1_LIK(EE, LL)                                                                                         \
    if (L.slice) launch_on(L.at, k_explore_ar1<EE, LL, true, false>, 64, 0, dev, ap, ar);                              \
    else if (L.full) launch_on(L.at, k_explore_ar1<EE, LL, false, true>, 64, 0, dev, ap, ar);                          \
    else launch_on(L.at, k_explore_ar1<EE, LL, false, false>, 64, 0, dev, ap, ar);
#define AR1_ONE(EE)                                                                                             \
    if (L.lik == AR1_NORMAL_IDENTITY) { AR1_LIK(EE, AR1_NORMAL_IDENTITY) } else { AR1_LIK(EE, AR1_STOCHASTIC_VOLATILITY) }
    switch (L.E) {
    case 1: AR1_ONE(1) break; case 2: AR1_ONE(2) break; case 4: AR1_ONE(4) break; case 8: AR1_ONE(8) break;
    default: return 1;
    }
#undef AR1_ONE
#undef AR1_LIK
    return 0;
}

int ar1_refresh_stats(int E, int lik, unsigned N, hipStream_t stream, const EngineDev &dev, const Ar1Params &ar) {
#define AR1_REFRESH(EE)                                                                                                          \
    if (lik == AR1_NORMAL_IDENTITY) hipLaunchKernelGGL((k_refresh_ar1_stats<EE, AR1_NORMAL_IDENTITY>), dim3(N), dim3(64), 0, stream, dev, ar); \
    else hipLaunchKernelGGL((k_refresh_ar1_stats<EE, AR1_STOCHASTIC_VOLATILITY>), dim3(N), dim3(64), 0, stream, dev, ar);
    switch (E) {
    case 1: AR1_REFRESH(1) break; case 2: AR1_REFRESH(2) break; case 4: AR1_REFRESH(4) break; case 8: AR1_REFRESH(8) break;
    default: return 1;
    }
#undef AR1_REFRESH
    return 0;
}

}  // namespace pte
