// pte_ar1_params.hpp -- what the launcher (pte.hip) and the latent-AR(1) kernels (pte_ar1.hpp) share: the data as the kernels read it and
// the one entry point through which the kernels are launched.  The kernels are compiled inside pte_glm.hip, next to the hierarchical
// normal-means kernels (pte_automala_params.hpp says why there is no unit of their own).
#pragma once
#include "pte_automala_params.hpp"

namespace pte {

enum { AR1_STOCHASTIC_VOLATILITY = 0, AR1_NORMAL_IDENTITY = 1 };      // include/pte.h PTE_AR1_*

// TGT_AR1: the data, shared by every replica.  y and y2 = y^2: [512] each, indexed by STATE coordinate (entries 0..2 -- mu, a
// and ls -- and everything from d on are zero), read lane-coalesced.  n = T observations, 0 until pte_set_target_ar1.
struct Ar1Params {
    const double *y = nullptr, *y2 = nullptr;
    int n = 0;
    double imu = 0.0, lmu = 0.0;                    // 1 / mu_sd, log mu_sd
    double phi_loc = 0.0, ips = 0.0, lps = 0.0;     // the prior of a = atanh(phi): its mean, 1 / phi_scale, log phi_scale
    double c_sigma = 0.0, iss = 0.0;                // log 2 - log pi - log sigma_scale, 1 / sigma_scale
    double iobs = 0.0, lobs = 0.0;                  // AR1_NORMAL_IDENTITY: 1 / obs_sd, log obs_sd
};
enum { AR1_DATA_LEN = 512 };                        // doubles per array: lanes past d read zeros, never past the allocation (E <= 8 blocks of 64)

// one launch of k_explore_ar1<E, LIK, slice mode, whole blocks>, one workgroup of one wave per replica
struct Ar1Launch { int E; int lik; bool slice; bool full; LaunchSite at; };
int ar1_launch(const Ar1Launch &L, const EngineDev &dev, const AmParams &ap, const Ar1Params &ar);                // 0, or 1 if this build holds no such kernel
int ar1_refresh_stats(int E, int lik, unsigned N, hipStream_t stream, const EngineDev &dev, const Ar1Params &ar);  // k_refresh_ar1_stats<E, LIK>

}  // namespace pte
