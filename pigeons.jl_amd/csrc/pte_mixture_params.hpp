// pte_mixture_params.hpp -- what the launcher (pte.hip) and the Gaussian-mixture kernels (pte_mixture.hpp) share: the one entry point through
// which the kernels are launched.  The kernels are a translation unit of their own, pte_mixture.hip (pte_automala_params.hpp says why).
#pragma once
#include "pte_automala_params.hpp"

namespace pte {

// the mixture's components are bucketed: K <= KB, KB in {2, 4, 8} (the lockstep reduction sums KB + 1 trees; the unused ones are zeros)
inline int mixture_bucket(int K) { return K <= 2 ? 2 : K <= 4 ? 4 : 8; }

// one launch of k_explore_mixture<E, KB, slice mode, whole blocks>, one workgroup of one wave per replica
struct MixtureLaunch { int E; bool slice; bool full; LaunchSite at; };
int mixture_launch(const MixtureLaunch &L, const EngineDev &dev, const AmParams &ap, const MixParams &mp);     // 0, or 1 if this build holds no such kernel
int mixture_refresh_stats(int E, unsigned N, hipStream_t stream, const EngineDev &dev, const MixParams &mp);  // k_refresh_mixture_stats<E, KB>

}  // namespace pte
