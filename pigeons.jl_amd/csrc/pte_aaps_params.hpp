// pte_aaps_params.hpp -- what the launcher (pte.hip) and the AAPS kernels (pte_aaps.hpp) share: kernel parameters and the one entry point
// through which the kernels are launched.  The kernels are a translation unit of their own, pte_aaps.hip (pte_automala_params.hpp says why).
#pragma once
#include "pte_automala_params.hpp"

// The most leapfrog steps one AAPS transition may take (forward and backward pass together, stopping points included).  A transition that
// needs more leaves the state where it was, with acceptance 0 (unlike the other failures, this one depends on the starting point).
#ifndef PTE_AAPS_MAX_LEAPFROGS
#define PTE_AAPS_MAX_LEAPFROGS 4096
#endif

namespace pte {

enum { ERR_AAPS_DENSITY = 12 };

struct AapsParams {
    double step_size;           // am_step_size (not adapted)
    int K;                      // aaps_K: segments besides the current one
    int precond;                // 0 identity, 1 diagonal, 2 mix-diagonal (am_preconditioner)
    double p0, p1;              // mix proportions
    const double *target_std;   // [d] or nullptr (== `nothing`: identity, no draw)
    double ref_prec;            // funnel: precision of the normal reference
    double log3;                // log(3.0) from the host libm
};

// one launch of k_explore_aaps<E, target, whole blocks>, one workgroup of one wave per replica
struct AapsLaunch { int E; int target; bool full; LaunchSite at; };
int aaps_launch(const AapsLaunch &L, const EngineDev &dev, const AapsParams &ap);      // 0, or 1 if this build holds no such kernel

}  // namespace pte
