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
    automala_body<E, TGT_HIER, SLICE, FULL, false, 1, PARAM>(e, ap, blockIdx.x, MixParams{}, GlmParams{}, MixModelParams{}, hp);
}

// swap statistics of every slot recomputed from the stored states (pte_set_state, pte_set_target_hier): suff = sum x^2, suff2 = the target's
// log density
template <int E, int PARAM>
__global__ __launch_bounds__(64) void k_refresh_hier_stats(EngineDev e, HierParams hp) {
    const int lane = lane_id();
    const int64_t slot = blockIdx.x;
    if (slot >= e.K) return;
    AmTarget<E, TGT_HIER, false, 1, PARAM> T;
    T.d = e.d; T.lane = lane;
    T.load_hier(hp);
    const double *xrow = e.x + slot * e.ld;
    double x[E];
#pragma unroll
    for (int j = 0; j < E; ++j) x[j] = T.valid(j) ? xrow[64 * j + lane] : 0.0;
    const double S = sqr_norm_regs<E>(x);
    const double l2 = T.hier(x);
    if (lane == 0) { e.suff[slot] = S; e.suff2[slot] = l2; }
}

int hier_launch(const HierLaunch &L, const EngineDev &dev, const AmParams &ap, const HierParams &hp) {
#define HIER_PARAM(EE, PP)                                                                                      \
    if (L.slice) launch_on(L.at, k_explore_hier<EE, PP, true, false>, 64, 0, dev, ap, hp);                             \
    else if (L.full) launch_on(L.at, k_explore_hier<EE, PP, false, true>, 64, 0, dev, ap, hp);                         \
    else launch_on(L.at, k_explore_hier<EE, PP, false, false>, 64, 0, dev, ap, hp);
#define HIER_ONE(EE)                                                                                            \
    if (L.param == HIER_NONCENTERED) { HIER_PARAM(EE, HIER_NONCENTERED) } else { HIER_PARAM(EE, HIER_CENTERED) }
    switch (L.E) {
    case 1: HIER_ONE(1) break; case 2: HIER_ONE(2) break; case 4: HIER_ONE(4) break; case 8: HIER_ONE(8) break;
    default: return 1;
    }
#undef HIER_ONE
#undef HIER_PARAM
    return 0;
}

int hier_refresh_stats(int E, int param, unsigned N, hipStream_t stream, const EngineDev &dev, const HierParams &hp) {
#define HIER_REFRESH(EE)                                                                                                         \
    if (param == HIER_NONCENTERED) hipLaunchKernelGGL((k_refresh_hier_stats<EE, HIER_NONCENTERED>), dim3(N), dim3(64), 0, stream, dev, hp); \
    else hipLaunchKernelGGL((k_refresh_hier_stats<EE, HIER_CENTERED>), dim3(N), dim3(64), 0, stream, dev, hp);
    switch (E) {
    case 1: HIER_REFRESH(1) break; case 2: HIER_REFRESH(2) break; case 4: HIER_REFRESH(4) break; case 8: HIER_REFRESH(8) break;
    default: return 1;
    }
#undef HIER_REFRESH
    return 0;
}

}  // namespace pte
