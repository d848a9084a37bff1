// pte_glm_params.hpp -- what the launcher (pte.hip) and the Bayesian-GLM kernels (pte_glm.hpp) share: the data as the kernels read it and
// the one entry point through which the kernels are launched.  The kernels are a translation unit of their own, pte_glm.hip
// (pte_automala_params.hpp says why).
#pragma once
#include "pte_automala_params.hpp"

namespace pte {

enum { GLM_BERNOULLI_LOGIT = 0, GLM_NORMAL_IDENTITY = 1 };      // include/pte.h PTE_GLM_*

// TGT_GLM: the data, shared by every replica.  xc: [d][n_pad] column-major (the eta pass: lanes over observations), xr: [n][ld]
// row-major with the state row's stride (the gradient pass: lanes over coordinates) and 512 zeros behind the last row, y: [n_pad]; all
// zero-padded.  n_pad = n rounded up to a multiple of 64.
struct GlmParams {
    const double *xc = nullptr, *xr = nullptr, *y = nullptr;
    int n = 0, n_pad = 0;
    int64_t ld = 0;
    double c_prior = 0.0, c_obs = 0.0;      // -(d/2) log(2 pi / p); 0 (logit) or -n (log sigma + log(2 pi) / 2) (normal)
    double w1 = 0.0, w2 = 0.0;              // normal: 1 / sigma^2, 1 / (2 sigma^2)
};

// dynamic LDS of one workgroup (one wave): theta [64 E] then r [n_pad] doubles
inline size_t glm_lds_bytes(int E, int n_pad) { return sizeof(double) * (size_t)(64 * E + n_pad); }

// one launch of k_explore_glm<E, LIK, slice mode, whole blocks>, one workgroup of one wave per replica
struct GlmLaunch { int E; int lik; bool slice; bool full; LaunchSite at; };
int glm_launch(const GlmLaunch &L, const EngineDev &dev, const AmParams &ap, const GlmParams &gp);               // 0, or 1 if this build holds no such kernel
int glm_refresh_stats(int E, int lik, unsigned N, hipStream_t stream, const EngineDev &dev, const GlmParams &gp, double ref_prec);   // k_refresh_glm_stats<E, LIK>

}  // namespace pte
