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
    automala_body<E, TGT_AR1, SLICE, FULL, false, 1, LIK>(e, ap, blockIdx.x, ar);
}

// swap statistics of every slot recomputed from the stored states (pte_set_state, pte_set_target_ar1): suff = sum x^2, suff2 = the target's
// log density
template <int E, int LIK>
__global__ __launch_bounds__(64) void k_refresh_ar1_stats(EngineDev e, Ar1Params ar) {
    PTE_REFRESH_STATS_BODY(E, TGT_AR1, 1, LIK, ar)
}

int ar1_launch(const Ar1Launch &L, const EngineDev &dev, const AmParams &ap, const Ar1Params &ar) {
    return with_blocks_per_lane(L.E, [&](auto e_) {
        auto go = [&](auto p_) {
            constexpr int E = decltype(e_)::value, LIK = decltype(p_)::value;
            if (L.slice) launch_on(L.at, k_explore_ar1<E, LIK, true, false>, 64, 0, dev, ap, ar);
            else if (L.full) launch_on(L.at, k_explore_ar1<E, LIK, false, true>, 64, 0, dev, ap, ar);
            else launch_on(L.at, k_explore_ar1<E, LIK, false, false>, 64, 0, dev, ap, ar);
        };
        if (L.lik == AR1_NORMAL_IDENTITY) go(std::integral_constant<int, AR1_NORMAL_IDENTITY>{});
        else go(std::integral_constant<int, AR1_STOCHASTIC_VOLATILITY>{});
    });
}

int ar1_refresh_stats(int E, int lik, unsigned N, hipStream_t stream, const EngineDev &dev, const Ar1Params &ar) {
    return with_blocks_per_lane(E, [&](auto e_) {
        constexpr int EE = decltype(e_)::value;
        if (lik == AR1_NORMAL_IDENTITY) hipLaunchKernelGGL((k_refresh_ar1_stats<EE, AR1_NORMAL_IDENTITY>), dim3(N), dim3(64), 0, stream, dev, ar);
        else hipLaunchKernelGGL((k_refresh_ar1_stats<EE, AR1_STOCHASTIC_VOLATILITY>), dim3(N), dim3(64), 0, stream, dev, ar);
    });
}

}  // namespace pte
