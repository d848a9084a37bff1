// pte_mixture_model_params.hpp -- what the launcher (pte.hip) and the mixture-model-posterior kernels (pte_mixture_model.hpp) share: the data
// as the kernels read it and the one entry point through which the kernels are launched.  The kernels are a translation unit of their own,
// pte_mixture_model.hip (pte_automala_params.hpp says why).
#pragma once
#include "pte_automala_params.hpp"

namespace pte {

// TGT_MIXMODEL: the observations, shared by every replica.  y: [n_pad], zero-padded; n_pad = n rounded up to a multiple of 64.
struct MixModelParams {
    const double *y = nullptr;
    int n = 0, n_pad = 0;
    double nd = 0.0;                        // n as a double (g_alpha_k = -p alpha_k + (sum_i r_ik - n w_k))
    double c_prior = 0.0, c_obs = 0.0;      // -(d/2) log(2 pi / p), -(n/2) log(2 pi)
};

// the components are bucketed: K = dim / 3 <= KB, KB in {2, 4, 8}; the unused ones carry the weight 0 (alpha = -inf)
inline int mixture_model_bucket(int K) { return K <= 2 ? 2 : K <= 4 ? 4 : 8; }

// one launch of k_explore_mixture_model<KB, slice mode>, one workgroup of one wave per replica
struct MixModelLaunch { int K; bool slice; LaunchSite at; };
int mixture_model_launch(const MixModelLaunch &L, const EngineDev &dev, const AmParams &ap, const MixModelParams &mm);     // 0, or 1 if this build holds no such kernel
int mixture_model_refresh_stats(int K, unsigned N, hipStream_t stream, const EngineDev &dev, const MixModelParams &mm, double ref_prec);   // k_refresh_mixture_model_stats

}  // namespace pte
