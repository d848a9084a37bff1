// pte_spinglass.hpp -- the +-J spin glass (Edwards-Anderson) under IsingMetropolis: the sweep of pte_ising.hpp with every
// neighbour product multiplied by a quenched bond J_ij in {+1, -1}.  The change of the bond-weighted pair sum at a site is still 0, +-4 or
// +-8, so the two guard-banded thresholds of pte_ising.hpp decide here as they do there, and the swap / recorder / boundary code sees the
// Ising target (EngineDev.target == 3, suff = the bond-weighted pair sum).
//
// A bond is one bit, set where it is -1: J_sn s_n = spin bit of n XOR bond bit (the gauge argument: a site sees its neighbour only through
// that product).  The bonds travel in SpinGlassParams, never in EngineDev.
//   k_explore_spinglass          any L >= 2: the byte-lattice sequential sweep, the site's two bonds riding in its LDS byte
//   k_explore_spinglass_spec     L % 32 == 0: the lane-speculative sweep with the two bond planes bit-packed in LDS
//   k_refresh_spinglass_stats    suff of every slot from the packed rows and the bonds
// The two sweeps are the Ising kernels' bodies with BONDS set (pte_lattice_bytes_body.inc, pte_lattice_spec_body.inc): this header holds
// the kernels' names and arguments, the refresh kernel and the launcher.
#pragma once
#include "pte_ising.hpp"
#include "pte_spinglass_params.hpp"

namespace pte {

// k_explore_ising's sweep (pte_lattice_bytes_body.inc) with the site's two bonds riding in its LDS byte.  Dynamic LDS: L * L bytes.
__global__ __launch_bounds__(64) void k_explore_spinglass(EngineDev e, SpinGlassParams tp) {
    constexpr bool BONDS = true;
    const unsigned char *const jb = tp.jb;
#include "pte_lattice_bytes_body.inc"
}

// k_explore_ising_spec's sweep (pte_lattice_spec_body.inc) with the two bond planes bit-packed in LDS behind the lattice.  Dynamic LDS:
// three planes (lattice, JR, JD) of L * L / 8 bytes + 8 each: 24 KiB + 24 at L = 256.
template <bool ONE_WORD>
__global__ __launch_bounds__(64) void k_explore_spinglass_spec(EngineDev e, SpinGlassParams tp) {
    constexpr bool BONDS = true;
    const unsigned *const jw = tp.jw;
#include "pte_lattice_spec_body.inc"
}

// suff = the bond-weighted pair sum of every slot, from the packed rows in HBM and the byte plane of the bonds (any L): after
// pte_set_target_spin_glass, pte_set_state and for the zero initial state
__global__ __launch_bounds__(64) void k_refresh_spinglass_stats(EngineDev e, SpinGlassParams gp) {
    const int lane = lane_id();
    const int64_t slot = blockIdx.x;
    if (slot >= e.K) return;
    const int L = gp.L, d = L * L;
    const unsigned *wrow = reinterpret_cast<const unsigned *>(e.x + slot * e.ld);
    auto bit = [&](int s) { return (wrow[s >> 5] >> (s & 31)) & 1u; };
    long long acc = 0;
    for (int s = lane; s < d; s += 64) {
        const int i = s / L, j = s - i * L;
        const int dn = (i == L - 1 ? 0 : i + 1) * L + j, rt = i * L + (j == L - 1 ? 0 : j + 1);
        const unsigned c0 = bit(s), jb = gp.jb[s];
        acc += 2 - 2 * (int)((c0 ^ bit(rt) ^ (jb >> 1)) & 1u) - 2 * (int)((c0 ^ bit(dn) ^ (jb >> 2)) & 1u);
    }
    for (int k = 1; k < 64; k <<= 1) acc += __shfl_xor(acc, k, 64);
    if (lane == 0) e.suff[slot] = (double)acc;
}

int spinglass_launch(const SpinGlassLaunch &Ln, const EngineDev &dev, const SpinGlassParams &gp) {
    const size_t d = (size_t)gp.L * (size_t)gp.L;
    if (gp.L % 32 == 0 && !Ln.bytes) {
        if (!gp.jw) return 1;
        const size_t lds = 3 * (d / 8 + 8);
        if (gp.L == 32) launch_on(Ln.at, k_explore_spinglass_spec<true>, 64, lds, dev, gp);
        else            launch_on(Ln.at, k_explore_spinglass_spec<false>, 64, lds, dev, gp);
    } else {
        launch_on(Ln.at, k_explore_spinglass, 64, d, dev, gp);
    }
    return 0;
}

int spinglass_refresh_stats(unsigned N, hipStream_t stream, const EngineDev &dev, const SpinGlassParams &gp) {
    hipLaunchKernelGGL(k_refresh_spinglass_stats, dim3(N), dim3(64), 0, stream, dev, gp);
    return 0;
}

PTE_DEFINE_RNG_POLICY_SETTER(spinglass)

}  // namespace pte
