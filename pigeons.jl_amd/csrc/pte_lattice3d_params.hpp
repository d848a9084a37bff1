// pte_lattice3d_params.hpp -- what the launcher (pte.hip) and the 3-D spin-glass kernels (pte_lattice3d.hpp) share: the bonds as the kernels
// read them and the entry points through which the kernels are launched.  The kernels are a translation unit of their own, pte_lattice3d.hip
// (pte_automala_params.hpp says why).
#pragma once
#include "pte_automala_params.hpp"

namespace pte {

// PTE_TARGET_SPIN_GLASS_3D: the quenched +-1 bonds of the L x L x L periodic lattice, L even, 2 <= L <= 32, one device copy
// shared by every replica.  A bond is ONE BIT, set where the bond is -1.  Row r = z L + y of a plane is one word, the bond of site (z, y, x)
// in bit x: JX couples (z, y, x) with (z, y, x + 1), JY with (z, y + 1, x), JZ with (z + 1, y, x).
struct SpinGlass3DParams {
    int L = 0, n_steps = 0;
    double beta_target = 0.0;
    const unsigned *jw = nullptr;          // three planes of L * L words: JX, then JY, then JZ
};

// row r of the HBM bit string: bits [r L, r L + L), a funnel shift of the two words it may straddle (the second is read only where the row
// reaches into it: never past the word of the row's last bit).  Here, not in pte_lattice3d.hpp: the overlap kernel (pte_overlap.hpp, a
// unit of its own) takes its rows the same way.
__device__ __forceinline__ unsigned lattice3d_load_row(const unsigned *wrow, int r, int L, unsigned mask) {
    const int o = r * L, w = o >> 5, sh = o & 31;
    const unsigned lo = wrow[w], hi = sh + L > 32 ? wrow[w + 1] : 0u;
    return (unsigned)(((((uint64_t)hi) << 32) | lo) >> sh) & mask;
}

// one launch of the CheckerboardMetropolis sweep on this target (k_explore_checkerboard3d), one workgroup of one wave per replica
int lattice3d_launch(const LaunchSite &at, const EngineDev &dev, const SpinGlass3DParams &gp);
int lattice3d_refresh_stats(unsigned N, hipStream_t stream, const EngineDev &dev, const SpinGlass3DParams &gp);     // k_refresh_lattice3d_stats

}  // namespace pte
