// pte_varsel_params.hpp -- what the launcher (pte.hip) and the variable-selection kernels (pte_varsel.hpp) share: the data as the kernels read
// it and the entry points through which the kernels are launched.  The kernels are a translation unit of their own, pte_varsel.hip
// (pte_automala_params.hpp says why).
#pragma once
#include "pte_automala_params.hpp"
#include "pte_glm_params.hpp"

namespace pte {

// PTE_TARGET_VARIABLE_SELECTION: the data, shared by every replica.  xc: [d][n_pad] column-major (lanes over observations),
// y: [n_pad]; zero-padded, n_pad = n rounded up to a multiple of 64.  d = the number of columns: the state holds 2 d coordinates,
// theta_0..theta_{d-1} then gamma_0..gamma_{d-1} (0.0 / 1.0).  The likelihoods are the GLM family's (GLM_*).
struct VarselParams {
    const double *xc = nullptr, *y = nullptr;
    int n = 0, n_pad = 0, d = 0;
    double c_prior = 0.0, c_obs = 0.0;      // -(d/2) log(2 pi / p); 0 (logit) or -n (log sigma + log(2 pi) / 2) (normal)
    double w2 = 0.0;                        // normal: 1 / (2 sigma^2)
    double log_pi = 0.0, log_1mpi = 0.0;    // log(pi), log(1 - pi) of the prior inclusion probability, from the host libm
};

// dynamic LDS of one workgroup (one wave): eta [n_pad], then the staged state [64 E] doubles
inline size_t varsel_lds_bytes(int E, int n_pad) { return sizeof(double) * (size_t)(n_pad + 64 * E); }

// one launch of k_explore_varsel<E, LIK, whole blocks>, one workgroup of one wave per replica; E = blocks of 64 coordinates of the 2 d
struct VarselLaunch { int E; int lik; bool full; LaunchSite at; };
int varsel_launch(const VarselLaunch &L, const EngineDev &dev, const AmParams &ap, const VarselParams &vp);      // 0, or 1 if this build holds no such kernel
int varsel_refresh_stats(int E, int lik, unsigned N, hipStream_t stream, const EngineDev &dev, const VarselParams &vp, double ref_prec);   // k_refresh_varsel_stats<E, LIK>

}  // namespace pte
