// pte_mixture_model.hpp -- the mixture-model-posterior family of the device engine (PTE_TARGET_MIXTURE_MODEL): the interpolated
// path (1 - beta) ScaledPrecisionNormal(p) + beta (log N(theta; 0, I / p) + sum_i log sum_k w_k N(y_i; mu_k, exp(s_k)^2)) over
// theta = [mu, s, alpha] (d = 3 K, K <= 8), explored by AutoMALA / MALA (automala_body) and by SliceSampler (its slice mode), one wave per
// replica, always one block per lane.  The body and AmTarget are those of the funnel path (pte_automala.hpp); the target's log density and
// gradient (AmTarget<1, TGT_MIXMODEL, false, KB>::mixmodel_and_sqr_norm) run with lanes over observations: the 3 K parameters are read from
// their owning lanes into scalar registers, y comes from L2 on every evaluation.
#pragma once
#include <hip/hip_ext.h>
#include "pte_automala.hpp"
#include "pte_mixture_model_params.hpp"

namespace pte {

// two waves per SIMD at least: the accumulators of KB = 8 (3 KB sums of the gradient) stay within 256 registers
template <int KB, bool SLICE>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 8))) void k_explore_mixture_model(EngineDev e, AmParams ap, MixModelParams mm) {
    automala_body<1, TGT_MIXMODEL, SLICE, false, false, KB>(e, ap, blockIdx.x, mm);
}

// swap statistics of every slot recomputed from the stored states (pte_set_state, pte_set_target_mixture_model): suff = sum x^2, suff2 = the
// posterior's log density.  One kernel, the bucket of eight, for every K: the unused components add exact zeros, so the bits are those of
// the explore kernels' smaller buckets
__global__ __launch_bounds__(64) void k_refresh_mixture_model_stats(EngineDev e, MixModelParams mm, double ref_prec) {
    const int lane = lane_id();
    const int64_t slot = blockIdx.x;
    if (slot >= e.K) return;
    AmTarget<1, TGT_MIXMODEL, false, 8> T;
    T.d = e.d; T.lane = lane;
    T.ref_nhp = -0.5 * ref_prec; T.ref_nprec = -ref_prec;
    T.mm = mm; T.mk = (int)(e.d / 3);
    double x[1];
    x[0] = T.valid(0) ? e.x[slot * e.ld + lane] : 0.0;
    const double S = sqr_norm_regs<1>(x);
    const double l2 = T.target(x);
    if (lane == 0) { e.suff[slot] = S; e.suff2[slot] = l2; }
}

int mixture_model_launch(const MixModelLaunch &L, const EngineDev &dev, const AmParams &ap, const MixModelParams &mm) {
#define MIXMODEL_KB(KK)                                                                                         \
    if (L.slice) launch_on(L.at, k_explore_mixture_model<KK, true>, 64, 0, dev, ap, mm);                        \
    else launch_on(L.at, k_explore_mixture_model<KK, false>, 64, 0, dev, ap, mm);
    if (L.K < 1 || L.K > 8) return 1;
    switch (mixture_model_bucket(L.K)) { case 2: MIXMODEL_KB(2) break; case 4: MIXMODEL_KB(4) break; default: MIXMODEL_KB(8) break; }
#undef MIXMODEL_KB
    return 0;
}

int mixture_model_refresh_stats(int K, unsigned N, hipStream_t stream, const EngineDev &dev, const MixModelParams &mm, double ref_prec) {
    if (K < 1 || K > 8) return 1;
    hipLaunchKernelGGL(k_refresh_mixture_model_stats, dim3(N), dim3(64), 0, stream, dev, mm, ref_prec);
    return 0;
}

PTE_DEFINE_RNG_POLICY_SETTER(mixture_model)

}  // namespace pte
