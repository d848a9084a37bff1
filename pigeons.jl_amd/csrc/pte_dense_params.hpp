// pte_dense_params.hpp -- what the launcher (pte.hip) and the dense-precision Gaussian kernels (pte_dense.hpp) share: the data as the kernels
// read it and the one entry point through which the kernels are launched.  The kernels are compiled inside pte_glm.hip, next to the
// hierarchical normal-means and latent-AR(1) kernels (pte_automala_params.hpp says why there is no unit of their own).
#pragma once
#include "pte_automala_params.hpp"

namespace pte {

// TGT_DENSE: N(m, Q^-1), shared by every replica.  q: the precision matrix [n][ld], row-major, ld = 64 E (E = the blocks per
// lane of dim n), every row zero-padded from n on -- symmetric, so row k is also column k and lane l reads Q[k][64 j + l] coalesced.
// diag: its diagonal [ld], mean: m [ld], both zero from n on.  c = 1/2 log det Q - (n/2) log 2 pi.  n = dim, 0 until pte_set_target_dense.
struct DenseParams {
    const double *q = nullptr, *diag = nullptr, *mean = nullptr;
    int n = 0, ld = 0;
    double c = 0.0;
};

// one launch of k_explore_dense<E, false, whole blocks> (AutoMALA / MALA) or k_explore_dense_slice<E, whole blocks> (SliceSampler), one
// workgroup of one wave per replica
struct DenseLaunch { int E; bool slice; bool full; LaunchSite at; };
int dense_launch(const DenseLaunch &L, const EngineDev &dev, const AmParams &ap, const DenseParams &dn);                // 0, or 1 if this build holds no such kernel
int dense_refresh_stats(int E, unsigned N, hipStream_t stream, const EngineDev &dev, const DenseParams &dn);            // k_refresh_dense_stats<E>

}  // namespace pte
