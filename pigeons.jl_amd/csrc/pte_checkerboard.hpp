// pte_checkerboard.hpp -- CheckerboardMetropolis: the two-colour Metropolis sweep of the Ising and the +-J spin-glass lattice.
// On the periodic L x L lattice with L even no two sites of one colour (i + j) % 2 are neighbours, so all sites of a colour are
// conditionally independent given the other colour and are decided at once: one explore step is 2 n_steps half-sweeps, colour 0 then
// colour 1.  Lattice, bit order, bonds, the pair sum S, ising_lp, the zero initial state and the refresh of the reference chain are those of
// pte_ising.hpp / pte_spinglass.hpp; only the sweep of a tempered chain is new.
//
// The rule, per active site: delta = -2 s_s sum_n J_sn s_n (one of -8, -4, 0, 4, 8); the site owns ONE uniform whatever delta is -- draw
// number n = h (d / 2) + i (L / 2) + (j >> 1) + 1 of the stream at kernel entry, h the half-sweep -- and flips iff delta >= 0 or
// !(u > r_|delta|), with r4 = exp(ising_lp(beta, bt, -4)), r8 = exp(ising_lp(beta, bt, -8)) taken once per explore step (they do not depend
// on the current S: in a simultaneous update "the S before this site" has no meaning).  The stream leaves at seed + n_steps d gamma.  A
// draw's number does not depend on whether it is evaluated: the kernels evaluate the uniforms of the sites with delta < 0 only.
//
// `u > r` on integers.  u52_to_unit(m) = (1 + k 2^-52) - 1 = k 2^-52 EXACTLY for k = m & MASK52 (both operations are exact: k < 2^52), and
// r 2^52 is exact too (a power of two; r >= 0, and a subnormal r becomes normal without losing a bit).  So u > r <=> k > r 2^52 <=> k > floor(r 2^52),
// the last step because k is an integer.  The threshold word is T = floor(r 2^52), and T = 2^52 - 1 where r 2^52 >= 2^52 or r is NaN: no k
// exceeds it, as `u > r` is false for every u < 1 there.  The decision `k > T` is the decision `u > r` of the doubles, bit for bit.
//
//   k_explore_checkerboard<BONDS>          L % 32 == 0: the lattice (and the two bond planes) bit-packed in LDS, a lane decides the 16
//                                          active sites of a 32-site word with a bit-sliced neighbour count
//   k_explore_checkerboard_sites<BONDS>    any even L: the byte lattice of pte_lattice_bytes_body.inc, one lane per active site
// BONDS = false is the Ising target (every bond +1, null bond pointers).
#pragma once
#include "pte_ising.hpp"
#include "pte_checkerboard_params.hpp"

namespace pte {

struct CheckerThresholds { uint64_t t4, t8; };        // (checker_threshold: pte_checkerboard_params.hpp, shared with pte_lattice3d.hpp)
__device__ __forceinline__ CheckerThresholds checker_thresholds(double beta, double bt) {
    auto uniform64 = [](uint64_t v) {
        return ((uint64_t)(unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(v >> 32)) << 32) | (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)v);
    };
    return CheckerThresholds{uniform64(checker_threshold(exp(ising_lp(beta, bt, -4.0)))), uniform64(checker_threshold(exp(ising_lp(beta, bt, -8.0))))};
}

// Dynamic LDS: the lattice plane, L * L / 8 bytes; BONDS: the JR and the JD plane behind it (24 KiB at L = 256).  The planes are loaded once
// per launch, the lattice is stored once at the end, the 2 n_steps half-sweeps run in between.  The L * L / 32 words are dealt round-robin
// to the 64 lanes (at L = 32 only 32 lanes have a word: DESIGN 4.18 says why that is accepted).
template <bool BONDS>
__global__ __launch_bounds__(64) void k_explore_checkerboard(EngineDev e, SpinGlassParams tp) {
    extern __shared__ unsigned words[];
    const int lane = lane_id();
    const int64_t cl = blockIdx.x;
    if (cl >= e.K) return;
    const int64_t c = e.c0 + cl;
    const int slot = e.slot_of_chain[cl];
    const int L = tp.L, d = L * L, W = L >> 5, NW = d >> 5;
    unsigned *const jrp = words + NW, *const jdp = words + 2 * NW;                  // BONDS: the bond planes behind the lattice
    unsigned *wrow = reinterpret_cast<unsigned *>(e.x + (int64_t)slot * e.ld);     // bit-packed lattice in HBM, same word layout as the LDS copy
    uint64_t seed = e.rng[2 * slot];
    const uint64_t gamma = e.rng[2 * slot + 1];
    const double lp_before = lp_before_explore(e, c, slot);
    const bool refresh = is_ref_chain(e, c);

    for (int wd = lane; wd < NW; wd += 64) {
        unsigned v = 0;
        if (refresh) { const unsigned bb = rng_bool_bit(); for (int t = 0; t < 32; ++t) v |= (unsigned)((mix64(seed + (uint64_t)(32 * wd + t + 1) * gamma) >> bb) & 1ull) << t; }
        else         { v = wrow[wd]; }
        words[wd] = v;
        if constexpr (BONDS) { jrp[wd] = tp.jw[wd]; jdp[wd] = tp.jw[NW + wd]; }
    }
    __syncthreads();
    const unsigned rowmul = (65536u + (unsigned)W - 1u) / (unsigned)W;               // wd / W = (wd * rowmul) >> 16 for wd < 2048, W <= 8
    long long spp;
    if (refresh) {
        seed += (uint64_t)d * gamma;
        // the (bond-weighted) pair sum of the fresh lattice: every bond once, right + down neighbour products
        long long acc = 0;
        for (int wd = lane; wd < NW; wd += 64) {
            const int i = (int)(((unsigned)wd * rowmul) >> 16), wj = wd - i * W;
            const unsigned cur = words[wd], dn = words[(i == L - 1 ? 0 : i + 1) * W + wj];
            const unsigned nxt = words[i * W + (wj == W - 1 ? 0 : wj + 1)];
            const unsigned right = (cur >> 1) | (nxt << 31);
            acc += 64 - 2 * ((int)__popc(cur ^ right ^ (BONDS ? jrp[wd] : 0u)) + (int)__popc(cur ^ dn ^ (BONDS ? jdp[wd] : 0u)));
        }
        for (int k = 1; k < 64; k <<= 1) acc += __shfl_xor(acc, k, 64);
        spp = acc;
    } else {
        const CheckerThresholds th = checker_thresholds(e.beta[c], tp.beta_target);
        const int half = d >> 1;
        long long acc = 0;
        for (int h = 0; h < 2 * tp.n_steps; ++h) {
            // draw number of the first active site of the half-sweep is h (d / 2) + 1: site (i, j) reads hseed + (i (L / 2) + (j >> 1)) gamma
            const uint64_t hseed = seed + ((uint64_t)h * (uint64_t)half + 1ull) * gamma;
            int dS = 0;
            for (int wd = lane; wd < NW; wd += 64) {
                const int i = (int)(((unsigned)wd * rowmul) >> 16), wj = wd - i * W, row = i * W;
                const int wu = ((i == 0 ? L : i) - 1) * W + wj, wp = row + (wj == 0 ? W : wj) - 1, wn = row + (wj == W - 1 ? 0 : wj + 1);
                const unsigned cur = words[wd], up = words[wu], dn = words[(i == L - 1 ? 0 : i + 1) * W + wj];
                // the left / right neighbour words: one-bit shifts with the carry from the adjacent word of the row, which wraps at the
                // row's ends (L = 32: the adjacent word is the word itself)
                const unsigned lf = (cur << 1) | (words[wp] >> 31), rt = (cur >> 1) | (words[wn] << 31);
                // x_k: bit t set <=> the term s J s_n of site t with neighbour k is -1 (spin bit 1 = +1, bond bit 1 = -1).  The up term goes
                // through JD of the row above, the left term through JR shifted by one site with its own carry (DESIGN 4.17's gauging)
                unsigned x1 = cur ^ up, x2 = cur ^ dn, x3 = cur ^ lf, x4 = cur ^ rt;
                if constexpr (BONDS) {
                    const unsigned jr = jrp[wd];
                    x1 ^= jdp[wu]; x2 ^= jdp[wd]; x3 ^= (jr << 1) | (jrp[wp] >> 31); x4 ^= jr;
                }
                // two-level bit-sliced count of the -1 terms: none (delta = -8), exactly one (delta = -4), two or more (delta >= 0)
                const unsigned c12 = x1 & x2, c34 = x3 & x4, a12 = x1 ^ x2, a34 = x3 ^ x4;
                const unsigned two = c12 | c34 | (a12 & a34), none = ~(x1 | x2 | x3 | x4);
                // sites of this half-sweep's colour: (i + j) % 2 == h % 2, and j = 32 wj + t has the parity of t
                const unsigned colour = ((i ^ h) & 1) ? 0xAAAAAAAAu : 0x55555555u;
                // the uniforms of the sites that need one; the others flip
                const uint64_t wseed = hseed + (uint64_t)(unsigned)(i * (L >> 1) + 16 * wj) * gamma;
                unsigned need = colour & ~two, rej = 0u;
                while (need) {
                    const int t = __builtin_ctz(need);
                    need &= need - 1u;
                    const uint64_t k = mix64(wseed + (uint64_t)(unsigned)(t >> 1) * gamma) & MASK52;
                    if (k > (((none >> t) & 1u) ? th.t8 : th.t4)) rej |= 1u << t;
                }
                const unsigned flip = colour & ~rej;
                dS += 4 * ((int)__popc(flip & x1) + (int)__popc(flip & x2) + (int)__popc(flip & x3) + (int)__popc(flip & x4)) - 8 * (int)__popc(flip);
                words[wd] = cur ^ flip;              // own-colour bits only: what the other lanes read of this word in this half-sweep stays
            }
            acc += dS;
            __syncthreads();                         // the next half-sweep reads the bits this one wrote
        }
        for (int k = 1; k < 64; k <<= 1) acc += __shfl_xor(acc, k, 64);
        spp = (long long)e.suff[slot] + acc;
        seed += (uint64_t)tp.n_steps * (uint64_t)d * gamma;
    }
    __syncthreads();
    for (int wd = lane; wd < NW; wd += 64) wrow[wd] = words[wd];
    if (lane == 0) { e.suff[slot] = (double)spp; e.rng[2 * slot] = seed; }
    record_after_explore(e, cl, c, slot, lane, lp_before, (double)spp, 0.0);
}

// Any even L >= 2 and the cross-check of the packed kernel: the byte lattice of pte_lattice_bytes_body.inc (L * L bytes of LDS, spin in bit 0,
// BONDS: JR in bit 1 and JD in bit 2, set where -1), one lane per active site striding over the d / 2 active sites of a half-sweep.  Active
// site number a of a half-sweep is (i, j) = (a / (L / 2), 2 (a % (L / 2)) + (i + h) % 2) and reads draw h (d / 2) + a + 1.
template <bool BONDS>
__global__ __launch_bounds__(64) void k_explore_checkerboard_sites(EngineDev e, SpinGlassParams tp) {
    extern __shared__ unsigned char spins[];
    const int lane = lane_id();
    const int64_t cl = blockIdx.x;
    if (cl >= e.K) return;
    const int64_t c = e.c0 + cl;
    const int slot = e.slot_of_chain[cl];
    const int L = tp.L, d = L * L, NW = (d + 31) >> 5;
    unsigned *wrow = reinterpret_cast<unsigned *>(e.x + (int64_t)slot * e.ld);     // the lattice bit-packed in HBM: site s -> bit s & 31 of word s >> 5
    uint64_t seed = e.rng[2 * slot];
    const uint64_t gamma = e.rng[2 * slot + 1];
    const double lp_before = lp_before_explore(e, c, slot);
    const bool refresh = is_ref_chain(e, c);
    const unsigned bb = rng_bool_bit();
    for (int s = lane; s < d; s += 64) {
        const unsigned bit = refresh ? (unsigned)((mix64(seed + (uint64_t)(s + 1) * gamma) >> bb) & 1ull) : ((wrow[s >> 5] >> (s & 31)) & 1u);
        spins[s] = (unsigned char)(bit | (BONDS ? tp.jb[s] : 0));
    }
    __syncthreads();
    long long spp;
    if (refresh) {
        seed += (uint64_t)d * gamma;
        spp = BONDS ? spinglass_recompute(spins, L, lane) : ising_recompute(spins, L, lane);
    } else {
        const CheckerThresholds th = checker_thresholds(e.beta[c], tp.beta_target);
        const int half = d >> 1, LH = L >> 1;
        long long acc = 0;
        for (int h = 0; h < 2 * tp.n_steps; ++h) {
            const uint64_t hseed = seed + ((uint64_t)h * (uint64_t)half + 1ull) * gamma;
            for (int a = lane; a < half; a += 64) {
                const int i = a / LH, j = 2 * (a - i * LH) + ((i ^ h) & 1), s = i * L + j;
                const int iu = (i == 0 ? L : i) - 1, id = i == L - 1 ? 0 : i + 1, jl = (j == 0 ? L : j) - 1, jr = j == L - 1 ? 0 : j + 1;
                const unsigned c0 = spins[s], cu = spins[iu * L + j], cd = spins[id * L + j], cf = spins[i * L + jl], cr = spins[i * L + jr];
                // the -1 terms among s J s_n: up through JD of the site above, down through the site's own JD, left through JR of the site
                // to the left, right through its own JR (without BONDS the bond bits are 0)
                const int cnt = (int)((c0 ^ cu ^ (cu >> 2)) & 1u) + (int)((c0 ^ cd ^ (c0 >> 2)) & 1u) + (int)((c0 ^ cf ^ (cf >> 1)) & 1u) + (int)((c0 ^ cr ^ (c0 >> 1)) & 1u);
                bool flip = true;                    // delta = 4 cnt - 8
                if (cnt < 2) flip = !((mix64(hseed + (uint64_t)(unsigned)a * gamma) & MASK52) > (cnt == 0 ? th.t8 : th.t4));
                if (flip) { spins[s] = (unsigned char)(c0 ^ 1u); acc += 4 * cnt - 8; }
            }
            __syncthreads();                         // the next half-sweep reads the spins this one wrote
        }
        for (int k = 1; k < 64; k <<= 1) acc += __shfl_xor(acc, k, 64);
        spp = (long long)e.suff[slot] + acc;
        seed += (uint64_t)tp.n_steps * (uint64_t)d * gamma;
    }
    __syncthreads();
    for (int wd = lane; wd < NW; wd += 64) {         // LDS bytes -> HBM bits
        unsigned v = 0;
        for (int t = 0; t < 32 && 32 * wd + t < d; ++t) v |= (unsigned)(spins[32 * wd + t] & 1u) << t;
        wrow[wd] = v;
    }
    if (lane == 0) { e.suff[slot] = (double)spp; e.rng[2 * slot] = seed; }
    record_after_explore(e, cl, c, slot, lane, lp_before, (double)spp, 0.0);
}

int checkerboard_launch(const CheckerboardLaunch &Ln, const EngineDev &dev, const SpinGlassParams &gp) {
    const size_t d = (size_t)gp.L * (size_t)gp.L;
    if (gp.L < 2 || gp.L % 2 != 0 || d > 65536) return 1;
    const bool bonds = gp.jb != nullptr;
    if (gp.L % 32 == 0 && !Ln.sites) {
        if (bonds && !gp.jw) return 1;
        if (bonds) launch_on(Ln.at, k_explore_checkerboard<true>, 64, 3 * (d / 8), dev, gp);
        else       launch_on(Ln.at, k_explore_checkerboard<false>, 64, d / 8, dev, gp);
    } else {
        if (bonds) launch_on(Ln.at, k_explore_checkerboard_sites<true>, 64, d, dev, gp);
        else       launch_on(Ln.at, k_explore_checkerboard_sites<false>, 64, d, dev, gp);
    }
    return 0;
}

PTE_DEFINE_RNG_POLICY_SETTER(checkerboard)

}  // namespace pte
