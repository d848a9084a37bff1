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
    PTE_REFRESH_STATS_BODY(E, TGT_MIXTURE, KB, 0, mp)
}

// f(std::integral_constant<int, KB>{}) for the bucket of K components
template <typename F>
static inline void with_mixture_bucket(int K, F &&f) {
    switch (mixture_bucket(K)) {
    case 2: f(std::integral_constant<int, 2>{}); break;
    case 4: f(std::integral_constant<int, 4>{}); break;
    default: f(std::integral_constant<int, 8>{}); break;
    }
}

int mixture_launch(const MixtureLaunch &L, const EngineDev &dev, const AmParams &ap, const MixParams &mp) {
    return with_blocks_per_lane(L.E, [&](auto e_) {
        with_mixture_bucket(mp.K, [&](auto kb_) {
            constexpr int E = decltype(e_)::value, KB = decltype(kb_)::value;
            if (L.slice) launch_on(L.at, k_explore_mixture<E, KB, true, false>, 64, 0, dev, ap, mp);
            else if (L.full) launch_on(L.at, k_explore_mixture<E, KB, false, true>, 64, 0, dev, ap, mp);
            else launch_on(L.at, k_explore_mixture<E, KB, false, false>, 64, 0, dev, ap, mp);
        });
    });
}

int mixture_refresh_stats(int E, unsigned N, hipStream_t stream, const EngineDev &dev, const MixParams &mp) {
    return with_blocks_per_lane(E, [&](auto e_) {
        with_mixture_bucket(mp.K, [&](auto kb_) {
            hipLaunchKernelGGL((k_refresh_mixture_stats<decltype(e_)::value, decltype(kb_)::value>), dim3(N), dim3(64), 0, stream, dev, mp);
        });
    });
}

PTE_DEFINE_RNG_POLICY_SETTER(mixture)

}  // namespace pte
