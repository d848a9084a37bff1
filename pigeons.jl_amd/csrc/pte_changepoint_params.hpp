// pte_changepoint_params.hpp -- what the launcher (pte.hip) and the change-point kernels (pte_changepoint.hpp) share: the data as the kernels
// read it and the entry points through which the kernels are launched.  The kernels are a translation unit of their own, pte_changepoint.hip
// (pte_automala_params.hpp says why).
#pragma once
#include "pte_automala_params.hpp"

namespace pte {

// PTE_TARGET_CHANGE_POINT: the data, shared by every replica.  C: the prefix table C[t] = sum_{i < t} y_i, t = 0..n, exact
// integers in doubles (n <= 65536, y_i <= 2^20: below 2^36).  K change points: the state holds 2 K + 1 coordinates, the K + 1 log rates
// then the K change points as integral doubles in 0..n.
struct ChangepointParams {
    const double *C = nullptr;
    int n = 0, K = 0;
    double c_prior = 0.0, c_tau = 0.0, c_obs = 0.0;     // -((K+1)/2) log(2 pi / p); -K log(n + 1); -sum_i lgamma(y_i + 1)
};

// the two evaluation forms of k_explore_changepoint: the same bits, another amount of work per proposal
enum { CHANGEPOINT_FORM_AUTO = 0, CHANGEPOINT_FORM_FULL = 1, CHANGEPOINT_FORM_CACHED = 2 };

// one launch of k_explore_changepoint<CACHED>, one workgroup of one wave per replica
struct ChangepointLaunch { bool cached; LaunchSite at; };
int changepoint_launch(const ChangepointLaunch &L, const EngineDev &dev, const AmParams &ap, const ChangepointParams &cp);
int changepoint_refresh_stats(unsigned N, hipStream_t stream, const EngineDev &dev, const ChangepointParams &cp, double ref_prec);   // k_refresh_changepoint_stats

}  // namespace pte
