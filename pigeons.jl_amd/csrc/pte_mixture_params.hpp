// pte_mixture_params.hpp -- what the launcher (pte.hip) and the Gaussian-mixture kernels (pte_mixture.hpp) share: the one entry point through
// which the kernels are launched.  The kernels are the library's fourth translation unit (pte_mixture.hip, compiled with the flags of
// pte_langevin.hip): a unit of their own leaves the generated code of the shipped kernels exactly as it was.  Tools and development builds
// compile pte.hip alone (no -DPTE_SPLIT_LANGEVIN): it then includes the kernels and this entry point itself.
#pragma once
#include "pte_automala_params.hpp"

namespace pte {

// the mixture's components are bucketed: K <= KB, KB in {2, 4, 8} (the lockstep reduction sums KB + 1 trees; the unused ones are zeros)
inline int mixture_bucket(int K) { return K <= 2 ? 2 : K <= 4 ? 4 : 8; }

// one launch of k_explore_mixture<E, KB, slice mode, whole blocks>: N workgroups of one wave on `stream`; `ext`: the launch carries the
// start / stop events (hipExtLaunchKernelGGL, as LangevinLaunch)
struct MixtureLaunch { int E; bool slice; bool full; unsigned N; hipStream_t stream; bool ext; hipEvent_t ev_a, ev_b; };
int mixture_launch(const MixtureLaunch &L, const EngineDev &dev, const AmParams &ap, const MixParams &mp);     // 0, or 1 if this build holds no such kernel
int mixture_refresh_stats(int E, unsigned N, hipStream_t stream, const EngineDev &dev, const MixParams &mp);  // k_refresh_mixture_stats<E, KB>
int mixture_set_rng_policy(unsigned policy);                                                                   // the translation unit's own copy of g_rng_policy (hipError_t as int)

}  // namespace pte
