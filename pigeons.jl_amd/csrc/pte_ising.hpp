// pte_ising.hpp -- k_explore_ising: single-site Metropolis sweeps of the 2-D Ising model
// (reference examples/ising.jl:96-116) and the Bernoulli(1/2) refresh of the reference chain
// (ising.jl:49-58), one wavefront per replica.
//
// The reference explorer is a SEQUENTIAL raster sweep whose RNG consumption is data dependent
// (a uniform is drawn only when the flip lowers the density), so a replica's L^2 * n_steps site
// updates form one dependency chain: the sweep is uniform integer work (spins staged in LDS, one
// byte per site), the 64 lanes pre-evaluate the next 64 draws of the counter-based stream and
// parallelise the load / store / refresh / energy recomputation.  Acceptance uses a filtered
// predicate: accept_ratio = exp(lp(spp') - lp(spp)) differs from exp(-|delta| beta beta_I) only by
// rounding of the two interpolated log potentials (<= 1e-10 relative), so `rand > accept_ratio` is
// decided against the per-chain constants with a 1e-9 guard band and evaluated exactly in the band.
//
//   k_explore_ising              any L: the byte-lattice sequential sweep                       body: pte_lattice_bytes_body.inc
//   k_explore_ising_spec         L % 32 == 0: the lane-speculative sweep of the bit-packed lattice    body: pte_lattice_spec_body.inc
//   k_explore_ising_bits         L % 32 == 0: the scalar bit-packed sweep (test build only)
// The two bodies are shared with the spin-glass kernels (pte_spinglass.hpp), which set BONDS; lattice_thresholds is the guard band of all five.
#pragma once
#include "pte_slice2.hpp"

#ifndef PTE_ISING_FILTER_MIN
#define PTE_ISING_FILTER_MIN 1e-13          // beta * beta_target above which the thresholds decide (see lattice_thresholds)
#endif
namespace pte {

struct IsingParams { int L; int n_steps; double beta_target; };

// InterpolatedLogPotential between IsingLogPotential(0.0, L) and IsingLogPotential(beta_target, L)
// (examples/ising.jl:74-77, src/paths/InterpolatedLogPotential.jl:9-16) as a function of sum_pair_products
__device__ __forceinline__ double ising_lp(double beta, double beta_target, double spp) {
    const double ref = 0.0 * spp, tgt = beta_target * spp;
    return beta == 0.0 ? ref : (beta == 1.0 ? tgt : (1.0 - beta) * ref + beta * tgt);
}

__device__ __forceinline__ int ising_site(const unsigned char *sp, int s) {       // uniform read of one spin: +1 / -1
    return __builtin_amdgcn_readfirstlane((int)sp[s]) ? 1 : -1;
}

__device__ inline long long ising_recompute(const unsigned char *sp, int L, int lane) {   // ising.jl:27-35
    long long acc = 0;
    const int d = L * L;
    for (int s = lane; s < d; s += 64) {
        const int i = s / L, j = s - i * L;
        const int up = ((i == 0 ? L : i) - 1) * L + j, dn = (i == L - 1 ? 0 : i + 1) * L + j;
        const int lf = i * L + (j == 0 ? L : j) - 1, rt = i * L + (j == L - 1 ? 0 : j + 1);
        const int sg = sp[s] ? 1 : -1;
        acc += sg * ((sp[up] ? 1 : -1) + (sp[dn] ? 1 : -1) + (sp[lf] ? 1 : -1) + (sp[rt] ? 1 : -1));
    }
    for (int k = 1; k < 64; k <<= 1) acc += __shfl_xor(acc, k, 64);
    return acc / 2;
}

// The guard-banded thresholds for `rand > accept_ratio`.  |delta| = 4 or 8, also with +-1 bonds (the bound on the rounding of the exponent
// below uses |S| <= 2 L^2 only, which the bond-weighted sum keeps).
// When may a proposal with delta < 0 be decided by comparing the uniform with the guard-banded thresholds?  The reference evaluates
// exp(lp(S + delta) - lp(S)) with lp(S) = fl(beta * fl(bt * S)): the two roundings put a relative error of <= 2^-51 S / |delta| on the
// exponent (1.5e-11 at 256 x 256, 2.4e-10 at 1024 x 1024: inside the 1e-9 band whatever beta is), and what the filter ALSO assumes --
// that a uniform is drawn at all, i.e. that this ratio is < 1 in floating point -- holds while 4 beta bt is well above 2^-53.  Below the
// limit every decision takes the exact arithmetic (one full recount of the lattice per decision: ~1 us).  (Rounds 3-5 had 1e-6 here,
// and the second chain of a ladder adapted on a handful of scans does get there: 2.6e-7 after round 2 of C5 -- 207 ms per scan for that
// round instead of 3.8, tools/diag_regimes.py.)
// The thresholds as doubles (the byte-lattice sweep) and as integer bit patterns held in scalar registers (the bit-packed sweeps: bit
// patterns of positive doubles are ordered like the doubles): the high words for the filter, the whole patterns for the band.
// (In the band the byte body takes its uniform before it has the ratio, the bit-packed bodies take none when ratio >= 1: the same
// thing, since filter_ok keeps the rounded exponent < 0 and so the ratio < 1.)
struct LatticeThresholds {
    double r4lo, r4hi, r8lo, r8hi;
    unsigned r4lo_h, r4hi_h, r8lo_h, r8hi_h;
    unsigned long long r4lo_b, r4hi_b, r8lo_b, r8hi_b;
    bool filter_ok;
};
__device__ __forceinline__ LatticeThresholds lattice_thresholds(double bb) {         // bb = beta * beta_target
    LatticeThresholds t;
    const double r4 = exp(-4.0 * bb), r8 = exp(-8.0 * bb);
    auto hi32 = [](double v) { return (unsigned)__builtin_amdgcn_readfirstlane(__double2hiint(v)); };
    auto lo32 = [](double v) { return (unsigned)__builtin_amdgcn_readfirstlane(__double2loint(v)); };
    t.r4lo = r4 * (1.0 - 1e-9); t.r4hi = r4 * (1.0 + 1e-9); t.r8lo = r8 * (1.0 - 1e-9); t.r8hi = r8 * (1.0 + 1e-9);
    t.r4lo_h = hi32(t.r4lo); t.r4hi_h = hi32(t.r4hi); t.r8lo_h = hi32(t.r8lo); t.r8hi_h = hi32(t.r8hi);
    t.r4lo_b = ((unsigned long long)t.r4lo_h << 32) | lo32(t.r4lo); t.r4hi_b = ((unsigned long long)t.r4hi_h << 32) | lo32(t.r4hi);
    t.r8lo_b = ((unsigned long long)t.r8lo_h << 32) | lo32(t.r8lo); t.r8hi_b = ((unsigned long long)t.r8hi_h << 32) | lo32(t.r8hi);
    t.filter_ok = bb > PTE_ISING_FILTER_MIN;
    return t;
}

// The byte lattice with bonds (the spin glass, pte_spinglass.hpp): a site's LDS byte holds its spin in bit 0 and its two bonds in bits 1
// (JR) and 2 (JD), set where the bond is -1
__device__ __forceinline__ int sg_byte(const unsigned char *sp, int s) { return __builtin_amdgcn_readfirstlane((int)sp[s]); }   // uniform read of one site's byte
__device__ __forceinline__ int sg_pm(int bit) { return (bit & 1) ? 1 : -1; }

// S = sum_ij s_ij (JR_ij s_i,j+1 + JD_ij s_i+1,j) from the LDS bytes: every bond once.  At L = 2 the two bonds between the same pair of
// sites are distinct terms.
__device__ inline long long spinglass_recompute(const unsigned char *sp, int L, int lane) {
    long long acc = 0;
    const int d = L * L;
    for (int s = lane; s < d; s += 64) {
        const int i = s / L, j = s - i * L;
        const int dn = (i == L - 1 ? 0 : i + 1) * L + j, rt = i * L + (j == L - 1 ? 0 : j + 1);
        const int c0 = sp[s];
        acc += sg_pm(c0 ^ sp[rt] ^ (c0 >> 1) ^ 1) + sg_pm(c0 ^ sp[dn] ^ (c0 >> 2) ^ 1);
    }
    for (int k = 1; k < 64; k <<= 1) acc += __shfl_xor(acc, k, 64);
    return acc;
}

#ifndef PTE_TU_LANGEVIN          // (a non-template kernel: pte.hip holds it; the other units take this header's helpers only)
__global__ __launch_bounds__(64) void k_explore_ising(EngineDev e, IsingParams tp) {       // the byte-lattice sweep, any L
    constexpr bool BONDS = false;
    const unsigned char *const jb = nullptr;
#include "pte_lattice_bytes_body.inc"
}
#endif  // PTE_TU_LANGEVIN

}  // namespace pte

namespace pte {

// ---------------------------------------------------------------------------------------------
// k_explore_ising_bits: same sweep for base_length % 32 == 0 with the lattice bit-packed in LDS
// (L*L/8 bytes) and the current / upper / lower words of the row held in scalar registers: the
// per-site work is ~25 scalar integer instructions; the uniform is compared against the guard-banded
// thresholds in the integer domain (bit patterns of positive doubles are ordered like the doubles).
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned lds_word(const unsigned *w, int i) { return (unsigned)__builtin_amdgcn_readfirstlane((int)w[i]); }

#if defined(PTE_TEST_KERNELS) && !defined(PTE_TU_LANGEVIN)   // scalar bit-packed sweep: dominated by k_explore_ising_spec, kept in libpte_test.so for A/B parity
__global__ __launch_bounds__(64) void k_explore_ising_bits(EngineDev e, IsingParams ip) {
    extern __shared__ unsigned words[];
    const int lane = lane_id();
    const int64_t cl = blockIdx.x;
    if (cl >= e.K) return;
    const int64_t c = e.c0 + cl;
    const int slot = e.slot_of_chain[cl];
    const int L = ip.L, d = L * L, W = L >> 5, NW = d >> 5;
    unsigned *wrow = reinterpret_cast<unsigned *>(e.x + (int64_t)slot * e.ld);     // bit-packed lattice in HBM, same word layout as the LDS copy
    uint64_t seed = e.rng[2 * slot];
    const uint64_t gamma = e.rng[2 * slot + 1];
    const double lp_before = lp_before_explore(e, c, slot);

    if (is_ref_chain(e, c)) {
        for (int wd = lane; wd < NW; wd += 64) {
            unsigned v = 0;
            const unsigned bb = rng_bool_bit();
            for (int t = 0; t < 32; ++t) v |= (unsigned)((mix64(seed + (uint64_t)(32 * wd + t + 1) * gamma) >> bb) & 1ull) << t;
            words[wd] = v;
        }
        seed += (uint64_t)d * gamma;
    } else {
        for (int wd = lane; wd < NW; wd += 64) words[wd] = wrow[wd];
    }
    __syncthreads();
    long long spp;
    if (is_ref_chain(e, c)) {
        // recompute_sum_pair_products: every bond once = sum over sites of (right + down neighbour products)
        long long acc = 0;
        for (int wd = lane; wd < NW; wd += 64) {
            const int i = wd / W, wj = wd - i * W;
            const unsigned cur = words[wd], dn = words[(i == L - 1 ? 0 : i + 1) * W + wj];
            const unsigned nxt = words[i * W + (wj == W - 1 ? 0 : wj + 1)];
            const unsigned right = (cur >> 1) | (nxt << 31);
            acc += 64 - 2 * ((int)__popc(cur ^ right) + (int)__popc(cur ^ dn));     // +1 per equal pair, -1 per unequal pair
        }
        for (int k = 1; k < 64; k <<= 1) acc += __shfl_xor(acc, k, 64);
        spp = acc;
    } else {
        spp = (long long)e.suff[slot];
        const double beta = e.beta[c], bt = ip.beta_target;
        const LatticeThresholds th = lattice_thresholds(beta * bt);
        double unit = u52_to_unit(mix64(seed + (uint64_t)(lane + 1) * gamma));
        int p = 0;
        for (int k = 0; k < ip.n_steps; ++k) {
            for (int i = 0; i < L; ++i) {
                const int rowu = ((i == 0 ? L : i) - 1) * W, rowd = (i == L - 1 ? 0 : i + 1) * W, row = i * W;
                unsigned leftbit = lds_word(words, row + W - 1) >> 31;       // left neighbour of (i, 0): (i, L-1), not yet updated
                unsigned first_updated = 0;
                for (int wj = 0; wj < W; ++wj) {
                    unsigned cur = lds_word(words, row + wj);
                    const unsigned up = lds_word(words, rowu + wj), dn = lds_word(words, rowd + wj);
                    // right neighbour of bit 31: bit 0 of the next word (old value), or of word 0 of this row (updated) at the row end
                    const unsigned rightbit = (wj == W - 1) ? (first_updated & 1u) : (lds_word(words, row + wj + 1) & 1u);
                    const unsigned cur0 = cur;
                    for (int t = 0; t < 32; ++t) {
                        // branch-light scalar code: selects instead of jumps, one rare branch for the guard band
                        const unsigned sgb = (cur >> t) & 1u;
                        const unsigned lf = t == 0 ? leftbit : ((cur >> (t - 1)) & 1u);
                        // at the end of a one-word row the right neighbour of bit 31 is bit 0 of this very word (already updated)
                        const unsigned rt = t == 31 ? (W == 1 ? (cur & 1u) : rightbit) : ((cur >> (t + 1)) & 1u);
                        const int nb = 2 * (int)(((up >> t) & 1u) + ((dn >> t) & 1u) + lf + rt) - 4;
                        const int delta = (1 - 2 * (int)sgb) * 2 * nb;
                        const int need = (delta < 0) ? 1 : 0;
                        if (__builtin_expect(p == 64, 0)) { seed += 64ull * gamma; unit = u52_to_unit(mix64(seed + (uint64_t)(lane + 1) * gamma)); p = 0; }
                        const unsigned uhi = (unsigned)__builtin_amdgcn_readlane(__double2hiint(unit), p);   // read speculatively, consumed iff `need`
                        const unsigned hi_h = delta == -4 ? th.r4hi_h : th.r8hi_h, lo_h = delta == -4 ? th.r4lo_h : th.r8lo_h;
                        int rej = need & (uhi > hi_h ? 1 : 0);
                        const int sure_acc = uhi < lo_h ? 1 : 0;
                        if (__builtin_expect((need & (1 - rej) & (1 - sure_acc)) | (need & (th.filter_ok ? 0 : 1)), 0)) {
                            // guard band (or a chain where the filter is not valid): exact arithmetic of the reference
                            const unsigned ulo = (unsigned)__builtin_amdgcn_readlane(__double2loint(unit), p);
                            const unsigned long long ub = ((unsigned long long)uhi << 32) | ulo;
                            const unsigned long long lo = delta == -4 ? th.r4lo_b : th.r8lo_b, hi = delta == -4 ? th.r4hi_b : th.r8hi_b;
                            if (th.filter_ok && ub > hi) rej = 1;
                            else if (th.filter_ok && ub < lo) rej = 0;
                            else {
                                const double ratio = exp(ising_lp(beta, bt, (double)(spp + delta)) - ising_lp(beta, bt, (double)spp));
                                if (ratio < 1) rej = (__longlong_as_double((long long)ub) > ratio) ? 1 : 0;
                                else { rej = 0; p -= 1; }        // accept_ratio >= 1: the reference draws nothing
                            }
                        }
                        p += need;
                        const int acc = 1 - rej;
                        cur ^= (unsigned)acc << t;
                        spp += acc * delta;
                    }
                    if (cur != cur0 && lane == 0) words[row + wj] = cur;
                    if (wj == 0) first_updated = cur;
                    leftbit = cur >> 31;
                }
            }
        }
        seed += (uint64_t)p * gamma;
    }
    __syncthreads();
    for (int wd = lane; wd < NW; wd += 64) wrow[wd] = words[wd];
    if (lane == 0) { e.suff[slot] = (double)spp; e.rng[2 * slot] = seed; }
    record_after_explore(e, cl, c, slot, lane, lp_before, (double)spp, 0.0);
}

#endif  // PTE_TEST_KERNELS

// ---------------------------------------------------------------------------------------------
// k_explore_ising_spec: the bit-packed sweep with the 64 lanes as hypotheses.  Its body is pte_lattice_spec_body.inc, which says what it
// does; k_explore_spinglass_spec (pte_spinglass.hpp) is the same body with bond planes.  Dynamic LDS: L * L / 8 bytes + 8.
// ---------------------------------------------------------------------------------------------
template <bool ONE_WORD>
__global__ __launch_bounds__(64) void k_explore_ising_spec(EngineDev e, IsingParams tp) {
    constexpr bool BONDS = false;
    const unsigned *const jw = nullptr;
#include "pte_lattice_spec_body.inc"
}

}  // namespace pte
