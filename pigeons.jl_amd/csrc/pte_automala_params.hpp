// pte_automala_params.hpp -- what the launcher (pte.hip) and the kernel families share: kernel parameters, where a launch goes (LaunchSite,
// launch_on) and, per family, the one entry point through which its kernels are launched.
//
// The product library is built from EIGHT translation units (UNITS in __graft_entry__.py) and three listed beside them (LATTICE_UNITS, CHECKERBOARD_UNITS, LATTICE3D_UNITS):
//   pte.hip           the C ABI, the launcher and every kernel not named below, scheduled with -O2 -amdgpu-sched-strategy=max-ilp: the
//                     one-wave-per-SIMD slice kernels gain 1.3-2.3 %
//   pte_langevin.hip  AutoMALA / MALA and SliceSampler on the funnel path (pte_langevin_launch.hpp) with the default scheduler: max-ilp
//                     costs their d >= 512 instantiations up to 10 %
//   pte_aaps.hip, pte_mixture.hip, pte_glm.hip, pte_mixture_model.hip, pte_varsel.hip, pte_changepoint.hip
//                     the AAPS, Gaussian-mixture, Bayesian-GLM, mixture-model-posterior, variable-selection and change-point kernels with pte_langevin.hip's flags.  A unit each: whatever is added
//                     to an existing unit moves the generated code of the kernels already in it (tests/test_codegen_*.py freeze it).
//                     pte_glm.hip also holds the hierarchical normal-means kernels (pte_hier.hpp): they share automala_body and
//                     the unit's RNG-policy setter with the GLM's, and the assembly of every kernel that was there before stayed identical;
//                     so do the latent-AR(1) kernels (pte_ar1.hpp) and the dense-precision Gaussian kernels (pte_dense.hpp,
//                     DESIGN 4.16), under the same check
//   pte_spinglass.hip the spin-glass kernels (pte_spinglass.hpp) with pte.hip's flags: they are the Ising kernels with bonds
//   pte_checkerboard.hip the CheckerboardMetropolis kernels of both lattice targets (pte_checkerboard.hpp) with pte_spinglass.hip's flags
//   pte_lattice3d.hip the 3-D spin-glass kernels (pte_lattice3d.hpp) with pte_spinglass.hip's flags
//   pte_overlap.hip, pte_cluster.hip, pte_overlap_planes.hip
//                     the kernels of a lattice pair, a unit and a list each (OVERLAP_UNITS, CLUSTER_UNITS, PLANES_UNITS) with
//                     pte_lattice3d.hip's flags: the replica overlap (pte_overlap.hpp), Houdayer's cluster move (pte_cluster.hpp,
//                     DESIGN 4.21) and the plane autocorrelation behind chi_SG(k) and xi_L (pte_overlap_planes.hpp) -- fourteen in all
// Every unit includes pte_kernels.hpp and therefore holds its own copy of the `static __device__` word g_rng_policy: PTE_KERNEL_UNITS below.
// Tools and development builds compile pte.hip alone (no -DPTE_SPLIT_LANGEVIN): it then includes the kernel headers and their entry points itself.
#pragma once
#include <hip/hip_ext.h>
#include <type_traits>
#include "pte_kernels.hpp"

namespace pte {

enum { TGT_MVN = 0, TGT_FUNNEL = 2, TGT_MIXTURE = 4, TGT_GLM = 5, TGT_MIXMODEL = 6, TGT_HIER = 9, TGT_AR1 = 10, TGT_DENSE = 11 };

// TGT_MIXTURE (pte_mixture.hpp): the normalised mixture of K diagonal Gaussians, shared by every replica.  mu / inv: [K][ld]
// (ld = the state row's stride, zero-padded), c: [K]; the kernels read mu and inv as lane-coalesced global loads.
struct MixParams {
    const double *mu = nullptr, *inv = nullptr, *c = nullptr;
    int K = 0;
    int64_t ld = 0;
};
enum { ERR_AM_DENSITY = 5, ERR_AM_STEP = 6 };

struct AmParams {
    double step_size;
    int n_refresh;
    int precond;            // 0 identity, 1 diagonal, 2 mix-diagonal
    double p0, p1;          // mix proportions
    const double *target_std;   // [d] or nullptr (== `nothing`: identity, no draw)
    int use_mh;             // scan != 1
    int mala;               // 1: MALA (src/explorers/MALA.jl:74-97) -- fixed step size, one leapfrog, always MH
    int slice;              // 1: SliceSampler on this path (SliceSampler.jl:24-237) with the full log potential per evaluation
    double slice_w; int slice_p, slice_n_passes, slice_max_iter;
    double ref_prec;        // funnel: precision of the normal reference
    double log3;            // log(3.0) from the host libm
    int pace;               // k_*_langevin_mw: 1 = steer the waves' priorities by the replicas' pace (several workgroups share a compute unit and all are resident)
};

// Where one kernel launch goes: `grid` workgroups on `stream`.  ev_a != nullptr: the launch carries the start / stop events of the timing
// bracket it stands in (hipExtLaunchKernelGGL: they take the kernel's own begin / end timestamps -- what rocprofv3's kernel trace reports --
// instead of bracketing it with two event-record commands, which add the stream's hand-over time around a ~85 us kernel (~7 us)).
struct LaunchSite { dim3 grid; hipStream_t stream; hipEvent_t ev_a = nullptr, ev_b = nullptr; };
template <typename K, typename... Args>
static inline void launch_on(const LaunchSite &at, K kernel, dim3 block, size_t lds_bytes, const Args &...args) {
    if (at.ev_a) hipExtLaunchKernelGGL(kernel, at.grid, block, lds_bytes, at.stream, at.ev_a, at.ev_b, 0, args...);
    else hipLaunchKernelGGL(kernel, at.grid, block, lds_bytes, at.stream, args...);
}
// The run-time blocks per lane E as a compile-time constant: f(std::integral_constant<int, E>{}) for the E the one-wave kernels are built
// for -> 0; any other E -> 1 ("this build holds no such kernel") and f is not called.  The one place the family headers spell the list.
template <typename F>
static inline int with_blocks_per_lane(int E, F &&f) {
    switch (E) {
    case 1: f(std::integral_constant<int, 1>{}); return 0;
    case 2: f(std::integral_constant<int, 2>{}); return 0;
    case 4: f(std::integral_constant<int, 4>{}); return 0;
    case 8: f(std::integral_constant<int, 8>{}); return 0;
    default: return 1;
    }
}

// one launch of k_explore_automala<E, target, slice mode, whole blocks>, one workgroup of one wave per replica
struct LangevinLaunch { int E; int target; bool slice; bool full; LaunchSite at;
                        const ScanLoop *scans = nullptr;        // scans != nullptr: k_scans_automala, all the scans of a pte_run_scans call in one launch
                        int scan_wg = 1;                         // ... > 1: k_scans_automala_wg, that many consecutive chains (waves) per workgroup (must equal langevin_scan_wg(); at.grid counts those workgroups)
                        bool one_wave16 = false; };              // test build only (PTE_KERNEL_TEST_LANGEVIN_ONE_WAVE): 512 < d <= 1024 on the one-wave kernel with sixteen blocks per lane
int langevin_launch(const LangevinLaunch &L, const EngineDev &dev, const AmParams &ap);     // 0, or 1 if this build holds no such kernel
int langevin_scan_loop_blocks_per_cu(int E, int target, bool full, int scan_wg = 1);         // occupancy of k_scans_automala[_wg]<E, target, full> (0: not in this build)
int langevin_scan_wg();                                                                      // PTE_SCAN_WG of the Langevin translation unit
void langevin_refresh_funnel_stats(int E, unsigned N, hipStream_t stream, const EngineDev &dev, double log3);      // k_refresh_funnel_stats<E>

// The translation units besides pte.hip.  Each defines <unit>_set_rng_policy -- its own copy of g_rng_policy (hipError_t as int) -- with
// PTE_DEFINE_RNG_POLICY_SETTER(<unit>), and pte_set_rng_policy walks this list: a unit listed here without the setter does not link.
#define PTE_KERNEL_UNITS(X) X(langevin) X(aaps) X(mixture) X(glm) X(mixture_model) X(varsel) X(changepoint) X(spinglass) X(checkerboard) X(lattice3d)
#define PTE_DECLARE_RNG_POLICY_SETTER(unit) int unit##_set_rng_policy(unsigned policy);
PTE_KERNEL_UNITS(PTE_DECLARE_RNG_POLICY_SETTER)
#define PTE_DEFINE_RNG_POLICY_SETTER(unit)                                                                                        \
    int unit##_set_rng_policy(unsigned policy) { return (int)hipMemcpyToSymbol(HIP_SYMBOL(g_rng_policy), &policy, sizeof policy); }

}  // namespace pte
