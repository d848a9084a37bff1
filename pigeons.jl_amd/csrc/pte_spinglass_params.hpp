// pte_spinglass_params.hpp -- what the launcher (pte.hip) and the spin-glass kernels (pte_spinglass.hpp) share: the bonds as the kernels read
// them and the entry points through which the kernels are launched.  The kernels are a translation unit of their own, pte_spinglass.hip
// (pte_automala_params.hpp says why).
#pragma once
#include "pte_automala_params.hpp"

namespace pte {

// PTE_TARGET_SPIN_GLASS: the quenched +-1 bonds of the L x L periodic lattice, one device copy shared by every replica.
// A bond is held as ONE BIT, set where the bond is -1 (the all-ferromagnetic instance is all zeros): J_sn s_n is then the neighbour's spin
// bit XOR the bond bit.  JR[i][j] couples (i, j) with (i, j + 1), JD[i][j] couples (i, j) with (i + 1, j).
struct SpinGlassParams {
    int L = 0, n_steps = 0;
    double beta_target = 0.0;
    const unsigned char *jb = nullptr;     // [L * L], site s (row-major): bit 1 = JR[s] is -1, bit 2 = JD[s] is -1 (bit 0 is the spin's place in the LDS byte)
    const unsigned *jw = nullptr;          // L % 32 == 0: the planes bit-packed like the lattice, JR [L * L / 32] then JD [L * L / 32]
};

// one launch of the IsingMetropolis sweep on this target, one workgroup of one wave per replica: k_explore_spinglass_spec where
// L % 32 == 0 (unless bytes), k_explore_spinglass otherwise
struct SpinGlassLaunch { bool bytes; LaunchSite at; };
int spinglass_launch(const SpinGlassLaunch &L, const EngineDev &dev, const SpinGlassParams &sp);
int spinglass_refresh_stats(unsigned N, hipStream_t stream, const EngineDev &dev, const SpinGlassParams &sp);     // k_refresh_spinglass_stats

}  // namespace pte
