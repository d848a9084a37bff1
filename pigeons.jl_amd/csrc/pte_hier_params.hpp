// pte_hier_params.hpp -- what the launcher (pte.hip) and the hierarchical normal-means kernels (pte_hier.hpp) share: the data as the kernels
// read it and the one entry point through which the kernels are launched.  The kernels are compiled inside pte_glm.hip, the unit of the other
// data-reading family on automala_body (pte_automala_params.hpp says why there is no unit of their own).
#pragma once
#include "pte_automala_params.hpp"

namespace pte {

enum { HIER_CENTERED = 0, HIER_NONCENTERED = 1 };      // include/pte.h PTE_HIER_*

// TGT_HIER: the data, shared by every replica.  y, isig = 1 / sigma, lsig = log sigma: [512] each, indexed by STATE coordinate
// (entries 0 and 1 -- mu and log tau -- and everything from d on are zero), read lane-coalesced.  n = J groups, 0 until pte_set_target_hier.
struct HierParams {
    const double *y = nullptr, *isig = nullptr, *lsig = nullptr;
    int n = 0;
    double imu = 0.0, lmu = 0.0;            // 1 / mu_sd, log mu_sd
    double c_tau = 0.0, its = 0.0;          // log 2 - log pi - log tau_scale, 1 / tau_scale
};
enum { HIER_DATA_LEN = 512 };               // doubles per array: lanes past d read zeros, never past the allocation (E <= 8 blocks of 64)

// one launch of k_explore_hier<E, PARAM, slice mode, whole blocks>, one workgroup of one wave per replica
struct HierLaunch { int E; int param; bool slice; bool full; LaunchSite at; };
int hier_launch(const HierLaunch &L, const EngineDev &dev, const AmParams &ap, const HierParams &hp);                // 0, or 1 if this build holds no such kernel
int hier_refresh_stats(int E, int param, unsigned N, hipStream_t stream, const EngineDev &dev, const HierParams &hp);  // k_refresh_hier_stats<E, PARAM>

}  // namespace pte
