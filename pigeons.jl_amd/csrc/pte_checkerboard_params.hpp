// pte_checkerboard_params.hpp -- what the launcher (pte.hip) and the checkerboard kernels (pte_checkerboard.hpp) share: the entry point through
// which the kernels are launched.  The kernels are a translation unit of their own, pte_checkerboard.hip (pte_automala_params.hpp says why).
#pragma once
#include "pte_spinglass_params.hpp"

namespace pte {

// one launch of the CheckerboardMetropolis sweep, one workgroup of one wave per replica: k_explore_checkerboard where
// L % 32 == 0 (unless sites), k_explore_checkerboard_sites otherwise.  The lattice and the bonds travel as SpinGlassParams; the Ising target
// passes null bond pointers (every bond +1) and gets the instantiations without bond planes.
struct CheckerboardLaunch { bool sites; LaunchSite at; };
int checkerboard_launch(const CheckerboardLaunch &L, const EngineDev &dev, const SpinGlassParams &sp);

// The threshold word T = floor(r 2^52) of `u > r` on integers (pte_checkerboard.hpp derives it), 2^52 - 1 where r >= 1 or r is NaN.  Here, not
// beside the 2-D kernels, because the 3-D kernel (pte_lattice3d.hpp, a translation unit of its own) decides with the same words.
__device__ __forceinline__ uint64_t checker_threshold(double r) {
    const double s = r * 4503599627370496.0;                     // r 2^52, exact
    return s < 4503599627370496.0 ? (uint64_t)s : MASK52;        // (the conversion truncates: floor of a non-negative double)
}

}  // namespace pte
