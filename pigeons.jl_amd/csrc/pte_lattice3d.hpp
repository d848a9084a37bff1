// pte_lattice3d.hpp -- the +-J spin glass on the L x L x L periodic lattice under CheckerboardMetropolis, L even, 2 <= L <= 32.
// Site (z, y, x) has index s = (z L + y) L + x and colour (x + y + z) % 2; the bonds JX, JY, JZ couple it with (z, y, x + 1), (z, y + 1, x) and
// (z + 1, y, x).  The pair sum S = sum s_zyx (JX s_x+1 + JY s_y+1 + JZ s_z+1), ising_lp, the bit order in HBM, the zero initial state, the
// refresh of the reference chain, the two-colour rule, its one uniform per active site and its integer thresholds are those of
// pte_ising.hpp / pte_spinglass.hpp / pte_checkerboard.hpp; the swap / recorder / boundary code sees the Ising target (suff = S).
//
// The rule, per active site: delta = -2 s sum_n J_sn s_n over the SIX neighbours, one of -12, -8, -4, 0, 4, 8, 12; the site owns draw number
// n = h (d / 2) + (z L + y)(L / 2) + (x >> 1) + 1 of the stream at kernel entry, h the half-sweep, and flips iff delta >= 0 or
// !(u > r_|delta|), r4, r8, r12 = exp(ising_lp(beta, bt, -4 / -8 / -12)) taken once per explore step.  The stream leaves at seed + n_steps d gamma.
//
// The geometry packs without carries: a row of L <= 32 sites is ONE word (bits 0 .. L - 1), its +-x neighbours are a rotate inside the word,
// its +-y and +-z neighbours are other rows.  One kernel covers every L.
//   k_explore_checkerboard3d     the sweep: lattice and the three bond planes in LDS, one word per row, the rows dealt round-robin to the lanes
//   k_refresh_lattice3d_stats    suff of every slot from the HBM bits and the bonds
#pragma once
#include "pte_ising.hpp"
#include "pte_checkerboard_params.hpp"
#include "pte_lattice3d_params.hpp"

namespace pte {

struct Checker3DThresholds { uint64_t t4, t8, t12; };
__device__ __forceinline__ Checker3DThresholds checker3d_thresholds(double beta, double bt) {
    auto uniform64 = [](uint64_t v) {
        return ((uint64_t)(unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(v >> 32)) << 32) | (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)v);
    };
    return Checker3DThresholds{uniform64(checker_threshold(exp(ising_lp(beta, bt, -4.0)))), uniform64(checker_threshold(exp(ising_lp(beta, bt, -8.0)))),
                               uniform64(checker_threshold(exp(ising_lp(beta, bt, -12.0))))};
}

// Dynamic LDS: four planes of R = L * L words -- the lattice, JX, JY, JZ -- 16 L^2 bytes (16 KiB at L = 32).  The planes are loaded once per
// launch, the lattice is stored once at the end, the 2 n_steps half-sweeps run in between.  At L <= 6 fewer than 64 lanes have a row, at L = 8
// each has exactly one (DESIGN 4.19 gives the lanes-busy figure per L and says why that is accepted).
__global__ __launch_bounds__(64) void k_explore_checkerboard3d(EngineDev e, SpinGlass3DParams tp) {
    extern __shared__ unsigned rows[];
    const int lane = lane_id();
    const int64_t cl = blockIdx.x;
    if (cl >= e.K) return;
    const int64_t c = e.c0 + cl;
    const int slot = e.slot_of_chain[cl];
    const int L = tp.L, R = L * L, d = R * L, NW = (d + 31) >> 5;
    const unsigned mask = 0xFFFFFFFFu >> (32 - L);                                  // L >= 2: a shift of 0 .. 30
    unsigned *const jxp = rows + R, *const jyp = rows + 2 * R, *const jzp = rows + 3 * R;
    unsigned *wrow = reinterpret_cast<unsigned *>(e.x + (int64_t)slot * e.ld);     // the lattice bit-packed in HBM: site s -> bit s & 31 of word s >> 5
    uint64_t seed = e.rng[2 * slot];
    const uint64_t gamma = e.rng[2 * slot + 1];
    const double lp_before = lp_before_explore(e, c, slot);
    const bool refresh = is_ref_chain(e, c);

    for (int r = lane; r < R; r += 64) {
        unsigned v = 0;
        if (refresh) { const unsigned bb = rng_bool_bit(); for (int t = 0; t < L; ++t) v |= (unsigned)((mix64(seed + (uint64_t)(r * L + t + 1) * gamma) >> bb) & 1ull) << t; }
        else         { v = lattice3d_load_row(wrow, r, L, mask); }
        rows[r] = v;
        jxp[r] = tp.jw[r]; jyp[r] = tp.jw[R + r]; jzp[r] = tp.jw[2 * R + r];
    }
    __syncthreads();
    const unsigned zmul = (65536u + (unsigned)L - 1u) / (unsigned)L;                // r / L = (r * zmul) >> 16 for r < 1024, L <= 32
    long long spp;
    if (refresh) {
        seed += (uint64_t)d * gamma;
        // the bond-weighted pair sum of the fresh lattice: every bond once, the +x, +y and +z neighbour products of every row
        long long acc = 0;
        for (int r = lane; r < R; r += 64) {
            const int z = (int)(((unsigned)r * zmul) >> 16), y = r - z * L;
            const unsigned cur = rows[r], rt = ((cur >> 1) | (cur << (L - 1))) & mask;
            const unsigned yp = rows[z * L + (y == L - 1 ? 0 : y + 1)], zp = rows[(z == L - 1 ? 0 : z + 1) * L + y];
            acc += 3 * L - 2 * ((int)__popc(cur ^ rt ^ jxp[r]) + (int)__popc(cur ^ yp ^ jyp[r]) + (int)__popc(cur ^ zp ^ jzp[r]));
        }
        for (int k = 1; k < 64; k <<= 1) acc += __shfl_xor(acc, k, 64);
        spp = acc;
    } else {
        const Checker3DThresholds th = checker3d_thresholds(e.beta[c], tp.beta_target);
        const int half = d >> 1, LH = L >> 1;
        long long acc = 0;
        for (int h = 0; h < 2 * tp.n_steps; ++h) {
            // draw number of the first active site of the half-sweep is h (d / 2) + 1: site (z, y, x) reads hseed + (r (L / 2) + (x >> 1)) gamma
            const uint64_t hseed = seed + ((uint64_t)h * (uint64_t)half + 1ull) * gamma;
            int dS = 0;
            for (int r = lane; r < R; r += 64) {
                const int z = (int)(((unsigned)r * zmul) >> 16), y = r - z * L;
                const int rym = z * L + (y == 0 ? L : y) - 1, ryp = z * L + (y == L - 1 ? 0 : y + 1);
                const int rzm = ((z == 0 ? L : z) - 1) * L + y, rzp = (z == L - 1 ? 0 : z + 1) * L + y;
                const unsigned cur = rows[r];
                // the -x / +x neighbours: one-bit rotates within the L bits of the word (L = 32: shifts by 1 and 31, never by 32)
                const unsigned lf = ((cur << 1) | (cur >> (L - 1))) & mask, rt = ((cur >> 1) | (cur << (L - 1))) & mask;
                // x_k: bit t set <=> the term s J s_n of site t with neighbour k is -1 (spin bit 1 = +1, bond bit 1 = -1).  The - directions go
                // through the bond of the neighbour: JY of the row y - 1, JZ of the row z - 1, JX rotated by one site (DESIGN 4.17's gauging)
                const unsigned jx = jxp[r];
                const unsigned x1 = cur ^ lf ^ (((jx << 1) | (jx >> (L - 1))) & mask), x2 = cur ^ rt ^ jx;
                const unsigned x3 = cur ^ rows[rym] ^ jyp[rym], x4 = cur ^ rows[ryp] ^ jyp[r];
                const unsigned x5 = cur ^ rows[rzm] ^ jzp[rzm], x6 = cur ^ rows[rzp] ^ jzp[r];
                // bit-sliced count of the -1 terms: two full adders, then a 2-bit add.  count = b0 + 2 b1 + 4 b2, delta = 4 count - 12
                const unsigned s1 = x1 ^ x2 ^ x3, c1 = (x1 & x2) | (x3 & (x1 ^ x2)), s2 = x4 ^ x5 ^ x6, c2 = (x4 & x5) | (x6 & (x4 ^ x5));
                const unsigned b0 = s1 ^ s2, k0 = s1 & s2, b1 = c1 ^ c2 ^ k0, b2 = (c1 & c2) | (k0 & (c1 ^ c2));
                const unsigned none = ~(b0 | b1 | b2), one = b0 & ~(b1 | b2), three_or_more = b2 | (b1 & b0);
                // sites of this half-sweep's colour: (x + y + z) % 2 == h % 2
                const unsigned colour = (((y ^ z ^ h) & 1) ? 0xAAAAAAAAu : 0x55555555u) & mask;
                // the uniforms of the sites that need one; the others flip
                const uint64_t wseed = hseed + (uint64_t)(unsigned)(r * LH) * gamma;
                unsigned need = colour & ~three_or_more, rej = 0u;
                while (need) {
                    const int t = __builtin_ctz(need);
                    need &= need - 1u;
                    const uint64_t k = mix64(wseed + (uint64_t)(unsigned)(t >> 1) * gamma) & MASK52;
                    if (k > (((none >> t) & 1u) ? th.t12 : ((one >> t) & 1u) ? th.t8 : th.t4)) rej |= 1u << t;
                }
                const unsigned flip = colour & ~rej;
                dS += 4 * ((int)__popc(flip & x1) + (int)__popc(flip & x2) + (int)__popc(flip & x3) + (int)__popc(flip & x4) + (int)__popc(flip & x5) + (int)__popc(flip & x6))
                      - 12 * (int)__popc(flip);
                rows[r] = cur ^ flip;                // own-colour bits only: what the other lanes read of this row in this half-sweep stays
            }
            acc += dS;
            __syncthreads();                         // the next half-sweep reads the bits this one wrote
        }
        for (int k = 1; k < 64; k <<= 1) acc += __shfl_xor(acc, k, 64);
        spp = (long long)e.suff[slot] + acc;
        seed += (uint64_t)tp.n_steps * (uint64_t)d * gamma;
    }
    __syncthreads();
    // the inverse of the load: HBM word w is bits [32 w, 32 w + 32), assembled by its lane from the rows that overlap it; the rows hold no bit
    // at or beyond L and there is no row beyond R - 1, so bits >= d stay 0
    for (int w = lane; w < NW; w += 64) {
        const int first = (32 * w) / L, last = min((32 * w + 31) / L, R - 1);
        unsigned v = 0;
        for (int r = first; r <= last; ++r) {
            const int o = r * L - 32 * w;            // -L < o < 32
            v |= o >= 0 ? rows[r] << o : rows[r] >> -o;
        }
        wrow[w] = v;
    }
    if (lane == 0) { e.suff[slot] = (double)spp; e.rng[2 * slot] = seed; }
    record_after_explore(e, cl, c, slot, lane, lp_before, (double)spp, 0.0);
}

// suff = the bond-weighted pair sum of every slot, from the packed rows in HBM and the bond planes: after pte_set_target_spin_glass_3d
// (which covers the zero initial state) and pte_set_state
__global__ __launch_bounds__(64) void k_refresh_lattice3d_stats(EngineDev e, SpinGlass3DParams gp) {
    const int lane = lane_id();
    const int64_t slot = blockIdx.x;
    if (slot >= e.K) return;
    const int L = gp.L, R = L * L;
    const unsigned mask = 0xFFFFFFFFu >> (32 - L);
    const unsigned *wrow = reinterpret_cast<const unsigned *>(e.x + slot * e.ld);
    long long acc = 0;
    for (int r = lane; r < R; r += 64) {
        const int z = r / L, y = r - z * L;
        const unsigned cur = lattice3d_load_row(wrow, r, L, mask), rt = ((cur >> 1) | (cur << (L - 1))) & mask;
        const unsigned yp = lattice3d_load_row(wrow, z * L + (y == L - 1 ? 0 : y + 1), L, mask);
        const unsigned zp = lattice3d_load_row(wrow, (z == L - 1 ? 0 : z + 1) * L + y, L, mask);
        acc += 3 * L - 2 * ((int)__popc(cur ^ rt ^ gp.jw[r]) + (int)__popc(cur ^ yp ^ gp.jw[R + r]) + (int)__popc(cur ^ zp ^ gp.jw[2 * R + r]));
    }
    for (int k = 1; k < 64; k <<= 1) acc += __shfl_xor(acc, k, 64);
    if (lane == 0) e.suff[slot] = (double)acc;
}

int lattice3d_launch(const LaunchSite &at, const EngineDev &dev, const SpinGlass3DParams &gp) {
    if (gp.L < 2 || gp.L > 32 || gp.L % 2 != 0 || !gp.jw) return 1;
    launch_on(at, k_explore_checkerboard3d, 64, 16 * (size_t)gp.L * (size_t)gp.L, dev, gp);
    return 0;
}

int lattice3d_refresh_stats(unsigned N, hipStream_t stream, const EngineDev &dev, const SpinGlass3DParams &gp) {
    hipLaunchKernelGGL(k_refresh_lattice3d_stats, dim3(N), dim3(64), 0, stream, dev, gp);
    return 0;
}

PTE_DEFINE_RNG_POLICY_SETTER(lattice3d)

}  // namespace pte
