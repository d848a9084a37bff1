// pte_mixture.hpp -- the Gaussian-mixture family of the device engine (PTE_TARGET_GAUSSIAN_MIXTURE): the interpolated path
// (1 - beta) ScaledPrecisionNormal(p) + beta log(sum_k w_k N(mu_k, diag(sigma_k^2))) explored by AutoMALA / MALA (automala_body) and by
// SliceSampler (its slice mode), one wave per replica, d <= 512.  The body and AmTarget are those of the funnel path (pte_automala.hpp);
// only the target's log density and gradient differ (AmTarget<E, TGT_MIXTURE, FULL, KB>::mixture_and_sqr_norm).
#pragma once
#include <hip/hip_ext.h>
#include "pte_automala.hpp"
#include "pte_mixture_params.hpp"

namespace pte {

template <int E, int KB, bool SLICE, bool FULL>
__global__ __launch_bounds__(64) void k_explore_mixture(EngineDev e, AmParams ap, MixParams mp) {
    automala_body<E, TGT_MIXTURE, SLICE, FULL, false, KB>(e, ap, blockIdx.x, mp);
}

// swap statistics of every slot recomputed from the stored states (pte_set_state, pte_set_target_mixture): suff = sum x^2, suff2 = the
// mixture's log density
template <int E, int KB>
__global__ __launch_bounds__(64) void k_refresh_mixture_stats(EngineDev e, MixParams mp) {
    const int lane = lane_id();
    const int64_t slot = blockIdx.x;
    if (slot >= e.K) return;
    AmTarget<E, TGT_MIXTURE, false, KB> T;
    T.d = e.d; T.lane = lane;
    T.load_mixture(mp);
    const double *xrow = e.x + slot * e.ld;
    double x[E];
#pragma unroll
    for (int j = 0; j < E; ++j) x[j] = T.valid(j) ? xrow[64 * j + lane] : 0.0;
    const double S = sqr_norm_regs<E>(x);
    const double l2 = T.mixture(x);
    if (lane == 0) { e.suff[slot] = S; e.suff2[slot] = l2; }
}

int mixture_launch(const MixtureLaunch &L, const EngineDev &dev, const AmParams &ap, const MixParams &mp) {
#define MIX_KB(EE, KK)                                                                                          \
    if (L.slice) launch_on(L.at, k_explore_mixture<EE, KK, true, false>, 64, 0, dev, ap, mp);                    \
    else if (L.full) launch_on(L.at, k_explore_mixture<EE, KK, false, true>, 64, 0, dev, ap, mp);                \
    else launch_on(L.at, k_explore_mixture<EE, KK, false, false>, 64, 0, dev, ap, mp);
#define MIX_ONE(EE)                                                                                             \
    switch (mixture_bucket(mp.K)) { case 2: MIX_KB(EE, 2) break; case 4: MIX_KB(EE, 4) break; default: MIX_KB(EE, 8) break; }
    switch (L.E) {
    case 1: MIX_ONE(1) break; case 2: MIX_ONE(2) break; case 4: MIX_ONE(4) break; case 8: MIX_ONE(8) break;
    default: return 1;
    }
#undef MIX_ONE
#undef MIX_KB
    return 0;
}

int mixture_refresh_stats(int E, unsigned N, hipStream_t stream, const EngineDev &dev, const MixParams &mp) {
#define MIX_REFRESH(EE)                                                                                                                    \
    switch (mixture_bucket(mp.K)) {                                                                                                      \
    case 2: hipLaunchKernelGGL((k_refresh_mixture_stats<EE, 2>), dim3(N), dim3(64), 0, stream, dev, mp); break;                          \
    case 4: hipLaunchKernelGGL((k_refresh_mixture_stats<EE, 4>), dim3(N), dim3(64), 0, stream, dev, mp); break;                          \
    default: hipLaunchKernelGGL((k_refresh_mixture_stats<EE, 8>), dim3(N), dim3(64), 0, stream, dev, mp); break;                         \
    }
    switch (E) {
    case 1: MIX_REFRESH(1) break; case 2: MIX_REFRESH(2) break; case 4: MIX_REFRESH(4) break; case 8: MIX_REFRESH(8) break;
    default: return 1;
    }
#undef MIX_REFRESH
    return 0;
}

PTE_DEFINE_RNG_POLICY_SETTER(mixture)

}  // namespace pte
