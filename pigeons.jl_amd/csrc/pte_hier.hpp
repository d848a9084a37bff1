// pte_hier.hpp -- the hierarchical normal-means family of the device engine (PTE_TARGET_HIERARCHICAL_NORMAL): J groups with
// estimates y_j and known standard errors sigma_j, mu ~ N(0, mu_sd^2), tau ~ HalfCauchy(0, tau_scale), the state x = [mu, log tau, one
// coordinate per group] in the centred (theta_j) or the non-centred (eta_j, theta_j = mu + tau eta_j) parameterisation.  The interpolated path
// (1 - beta) ScaledPrecisionNormal(p) + beta target is explored by AutoMALA / MALA (automala_body) and by SliceSampler (its slice mode), one
// wave per replica, 3 <= d <= 512.  The body and AmTarget are those of the funnel path (pte_automala.hpp); the target's log density and gradient
// are AmTarget<E, TGT_HIER, FULL, 1, PARAM>::hier_and_sqr_norm.  Compiled inside pte_glm.hip (pte_automala_params.hpp).
#pragma once
#include <hip/hip_ext.h>
#include "pte_automala.hpp"
#include "pte_hier_params.hpp"

namespace pte {

template <int E, int PARAM, bool SLICE, bool FULL>
__global__ __launch_bounds__(64) void k_explore_hier(EngineDev e, AmParams ap, HierParams hp) {
    automala_body<E, TGT_HIER, SLICE, FULL, false, 1, PARAM>(e, ap, blockIdx.x, hp);
}

// swap statistics of every slot recomputed from the stored states (pte_set_state, pte_set_target_hier): suff = sum x^2, suff2 = the target's
// log density
template <int E, int PARAM>
__global__ __launch_bounds__(64) void k_refresh_hier_stats(EngineDev e, HierParams hp) {
    PTE_REFRESH_STATS_BODY(E, TGT_HIER, 1, PARAM, hp)
}

int hier_launch(const HierLaunch &L, const EngineDev &dev, const AmParams &ap, const HierParams &hp) {
    return with_blocks_per_lane(L.E, [&](auto e_) {
        auto go = [&](auto p_) {
            constexpr int E = decltype(e_)::value, PARAM = decltype(p_)::value;
            if (L.slice) launch_on(L.at, k_explore_hier<E, PARAM, true, false>, 64, 0, dev, ap, hp);
            else if (L.full) launch_on(L.at, k_explore_hier<E, PARAM, false, true>, 64, 0, dev, ap, hp);
            else launch_on(L.at, k_explore_hier<E, PARAM, false, false>, 64, 0, dev, ap, hp);
        };
        if (L.param == HIER_NONCENTERED) go(std::integral_constant<int, HIER_NONCENTERED>{});
        else go(std::integral_constant<int, HIER_CENTERED>{});
    });
}

int hier_refresh_stats(int E, int param, unsigned N, hipStream_t stream, const EngineDev &dev, const HierParams &hp) {
    return with_blocks_per_lane(E, [&](auto e_) {
        constexpr int EE = decltype(e_)::value;
        if (param == HIER_NONCENTERED) hipLaunchKernelGGL((k_refresh_hier_stats<EE, HIER_NONCENTERED>), dim3(N), dim3(64), 0, stream, dev, hp);
        else hipLaunchKernelGGL((k_refresh_hier_stats<EE, HIER_CENTERED>), dim3(N), dim3(64), 0, stream, dev, hp);
    });
}

}  // namespace pte
