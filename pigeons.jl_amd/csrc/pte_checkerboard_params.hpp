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

}  // namespace pte
