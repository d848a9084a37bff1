// pte_spinglass.hpp -- the +-J spin glass (Edwards-Anderson) under IsingMetropolis: the sweep of pte_ising.hpp with every
// neighbour product multiplied by a quenched bond J_ij in {+1, -1}.  The change of the bond-weighted pair sum at a site is still 0, +-4 or
// +-8, so the two guard-banded thresholds of pte_ising.hpp decide here as they do there, and the swap / recorder / boundary code sees the
// Ising target (EngineDev.target == 3, suff = the bond-weighted pair sum).
//
// A bond is one bit, set where it is -1: J_sn s_n = spin bit of n XOR bond bit (the gauge argument: a site sees its neighbour only through
// that product).  The bonds travel in SpinGlassParams, never in EngineDev.
//   k_explore_spinglass          any L >= 2: the byte-lattice sequential sweep, the site's two bonds riding in its LDS byte
//   k_explore_spinglass_spec     L % 32 == 0: the lane-speculative sweep of k_explore_ising_spec with the two bond planes bit-packed in LDS
//   k_refresh_spinglass_stats    suff of every slot from the packed rows and the bonds
#pragma once
#include "pte_ising.hpp"
#include "pte_spinglass_params.hpp"

namespace pte {

__device__ __forceinline__ int sg_byte(const unsigned char *sp, int s) { return __builtin_amdgcn_readfirstlane((int)sp[s]); }   // uniform read of one site's byte
__device__ __forceinline__ int sg_pm(int bit) { return (bit & 1) ? 1 : -1; }

// S = sum_ij s_ij (JR_ij s_i,j+1 + JD_ij s_i+1,j) from the LDS bytes (bit 0 spin, bit 1 JR, bit 2 JD): every bond once.  At L = 2 the two
// bonds between the same pair of sites are distinct terms.
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

// k_explore_ising with the neighbour sum weighted by the bonds: statement for statement its draw order.  Dynamic LDS: L * L bytes.
__global__ __launch_bounds__(64) void k_explore_spinglass(EngineDev e, SpinGlassParams gp) {
    extern __shared__ unsigned char spins[];
    const int lane = lane_id();
    const int64_t cl = blockIdx.x;
    if (cl >= e.K) return;
    const int64_t c = e.c0 + cl;
    const int slot = e.slot_of_chain[cl];
    const int L = gp.L, d = L * L, NW = (d + 31) >> 5;
    unsigned *wrow = reinterpret_cast<unsigned *>(e.x + (int64_t)slot * e.ld);     // the lattice bit-packed in HBM: site s -> bit s & 31 of word s >> 5
    auto store_lattice = [&]() {                                                    // LDS bytes -> HBM bits (call after a barrier)
        for (int wd = lane; wd < NW; wd += 64) {
            unsigned v = 0;
            for (int t = 0; t < 32 && 32 * wd + t < d; ++t) v |= (unsigned)(spins[32 * wd + t] & 1u) << t;
            wrow[wd] = v;
        }
    };
    uint64_t seed = e.rng[2 * slot];
    const uint64_t gamma = e.rng[2 * slot + 1];
    const double lp_before = lp_before_explore(e, c, slot);

    if (is_ref_chain(e, c)) {
        // iid_bernoulli!: site s (row-major, i outer / j inner) <- rand(rng, Bool) = low bit of draw s+1
        const unsigned bb = rng_bool_bit();
        for (int s = lane; s < d; s += 64) spins[s] = (unsigned char)(((mix64(seed + (uint64_t)(s + 1) * gamma) >> bb) & 1ull) | gp.jb[s]);
        seed += (uint64_t)d * gamma;
        __syncthreads();
        const long long spp = spinglass_recompute(spins, L, lane);
        store_lattice();
        if (lane == 0) { e.suff[slot] = (double)spp; e.rng[2 * slot] = seed; }
        record_after_explore(e, cl, c, slot, lane, lp_before, (double)spp, 0.0);
        return;
    }
    for (int s = lane; s < d; s += 64) spins[s] = (unsigned char)(((wrow[s >> 5] >> (s & 31)) & 1u) | gp.jb[s]);
    __syncthreads();
    long long spp = (long long)e.suff[slot];
    const double beta = e.beta[c], bt = gp.beta_target;
    const double bb = beta * bt;
    // |delta| = 4 or 8 with +-1 bonds too: the guard-banded thresholds of k_explore_ising (the bound on the rounding of the exponent there
    // uses |S| <= 2 L^2 only, which the bond-weighted sum keeps)
    const double r4 = exp(-4.0 * bb), r8 = exp(-8.0 * bb);
    const double r4lo = r4 * (1.0 - 1e-9), r4hi = r4 * (1.0 + 1e-9), r8lo = r8 * (1.0 - 1e-9), r8hi = r8 * (1.0 + 1e-9);
    const bool filter_ok = bb > PTE_ISING_FILTER_MIN;

    double unit = u52_to_unit(mix64(seed + (uint64_t)(lane + 1) * gamma));
    int p = 0;

    for (int k = 0; k < gp.n_steps; ++k) {
        int s = 0;
        for (int i = 0; i < L; ++i) {
            const int rowu = ((i == 0 ? L : i) - 1) * L, rowd = (i == L - 1 ? 0 : i + 1) * L, row = i * L;
            for (int j = 0; j < L; ++j, ++s) {
                const int c0 = sg_byte(spins, s), cu = sg_byte(spins, rowu + j), cd = sg_byte(spins, rowd + j);
                const int cf = sg_byte(spins, row + (j == 0 ? L : j) - 1), cr = sg_byte(spins, row + (j == L - 1 ? 0 : j + 1));
                const int sg = sg_pm(c0);
                // J_sn s_n: up through JD of the site above, down through the site's own JD, left through JR of the site to the left, right through its own JR
                // (spin bit 1 = +1, bond bit 1 = -1: the product is +1 where the two bits differ)
                const int nb = sg_pm(cu ^ (cu >> 2)) + sg_pm(cd ^ (c0 >> 2)) + sg_pm(cf ^ (cf >> 1)) + sg_pm(cr ^ (c0 >> 1));
                const int delta = -2 * sg * nb;            // bond-weighted pair sum after - before
                bool accept = true;
                if (delta < 0) {
                    bool need_draw = true, decided = false;
                    double ratio = 0.0;
                    if (__builtin_expect(!filter_ok, 0)) {
                        ratio = exp(ising_lp(beta, bt, (double)(spp + delta)) - ising_lp(beta, bt, (double)spp));
                        need_draw = ratio < 1;
                        decided = true;
                    }
                    if (need_draw) {
                        if (p == 64) { seed += 64ull * gamma; unit = u52_to_unit(mix64(seed + (uint64_t)(lane + 1) * gamma)); p = 0; }
                        const double u = readlane_f64(unit, p);
                        p += 1;
                        if (!decided) {
                            const double lo = delta == -4 ? r4lo : r8lo, hi = delta == -4 ? r4hi : r8hi;
                            if (u > hi) accept = false;
                            else if (u < lo) accept = true;
                            else {
                                ratio = exp(ising_lp(beta, bt, (double)(spp + delta)) - ising_lp(beta, bt, (double)spp));
                                accept = !(ratio < 1 && u > ratio);
                            }
                        } else {
                            accept = !(u > ratio);
                        }
                    }
                }
                if (accept) {
                    if (lane == 0) spins[s] = (unsigned char)(c0 ^ 1);
                    spp += delta;
                }
            }
        }
    }
    __syncthreads();
    store_lattice();
    if (lane == 0) { e.suff[slot] = (double)spp; e.rng[2 * slot] = seed + (uint64_t)p * gamma; }
    record_after_explore(e, cl, c, slot, lane, lp_before, (double)spp, 0.0);
}

// ---------------------------------------------------------------------------------------------
// k_explore_spinglass_spec: k_explore_ising_spec (pte_ising.hpp: 16-site chunks, four quads, 56 (quad, consumed, left) hypotheses, a chase
// of four chained v_readlane) with the bonds folded into what the walk is GIVEN, so that the per-site walk, the pack word and the chase are
// what they are there:
//   * the words above / below / to the right enter a chunk only as neighbour nibbles: XOR the bond words into them first
//     (up ^= JD of the row above, dn ^= JD of this row, right ^= JR of this row);
//   * the left neighbour is the one the walk carries (its NEW value).  Its bond is JR shifted by one site -- with the carry across words
//     and, at column 0, bit 31 of the row's last bond word -- and is folded into the statics: NN / II hold each site's answer for
//     left = 0 and for left = 1; where the left bond is -1 the two halves swap.
// The scalar guard-band path and recompute() take the bonds the same way.  Dynamic LDS: three planes (lattice, JR, JD) of L * L / 8 bytes
// + 8 each (the read-ahead runs two words past a row's end): 24 KiB + 24 at L = 256, loaded once per launch.
// A copy of the Ising kernel rather than a BONDS flag on it: its two instantiations in pte.hip stay untouched.
// ---------------------------------------------------------------------------------------------
template <bool ONE_WORD>
__global__ __launch_bounds__(64) void k_explore_spinglass_spec(EngineDev e, SpinGlassParams gp) {
    extern __shared__ unsigned words[];
    const int lane = lane_id();
    const int64_t cl = blockIdx.x;
    if (cl >= e.K) return;
    const int64_t c = e.c0 + cl;
    const int slot = e.slot_of_chain[cl];
    const int L = gp.L, d = L * L, W = ONE_WORD ? 1 : (L >> 5), NW = d >> 5;
    unsigned *const jrp = words + NW + 2, *const jdp = words + 2 * (NW + 2);        // the bond planes behind the lattice, each with its two words of padding
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
        jrp[wd] = gp.jw[wd]; jdp[wd] = gp.jw[NW + wd];
    }
    if (lane < 2) { words[NW + lane] = 0u; jrp[NW + lane] = 0u; jdp[NW + lane] = 0u; }      // (the padding: read ahead, never used)
    if (refresh) seed += (uint64_t)d * gamma;
    __syncthreads();
    // the bond-weighted pair sum from the LDS planes: every bond once (right + down neighbour products)
    auto recompute = [&]() -> long long {
        long long acc = 0;
        for (int wd = lane; wd < NW; wd += 64) {
            const int i = wd / W, wj = wd - i * W;
            const unsigned cur = words[wd], dn = words[(i == L - 1 ? 0 : i + 1) * W + wj];
            const unsigned nxt = words[i * W + (wj == W - 1 ? 0 : wj + 1)];
            const unsigned right = (cur >> 1) | (nxt << 31);
            acc += 64 - 2 * ((int)__popc(cur ^ right ^ jrp[wd]) + (int)__popc(cur ^ dn ^ jdp[wd]));
        }
        for (int k = 1; k < 64; k <<= 1) acc += __shfl_xor(acc, k, 64);
        return acc;
    };
    if (!refresh) {
        const double beta = e.beta[c], bt = gp.beta_target;
        const double bb = beta * bt;
        const double r4 = exp(-4.0 * bb), r8 = exp(-8.0 * bb);
        auto hi32 = [](double v) { return (unsigned)__builtin_amdgcn_readfirstlane(__double2hiint(v)); };
        auto lo32 = [](double v) { return (unsigned)__builtin_amdgcn_readfirstlane(__double2loint(v)); };
        const double r4l = r4 * (1.0 - 1e-9), r4h = r4 * (1.0 + 1e-9), r8l = r8 * (1.0 - 1e-9), r8h = r8 * (1.0 + 1e-9);
        const unsigned r4lo_h = hi32(r4l), r4hi_h = hi32(r4h), r8lo_h = hi32(r8l), r8hi_h = hi32(r8h);
        const unsigned long long r4lo = ((unsigned long long)r4lo_h << 32) | lo32(r4l), r4hi = ((unsigned long long)r4hi_h << 32) | lo32(r4h);
        const unsigned long long r8lo = ((unsigned long long)r8lo_h << 32) | lo32(r8l), r8hi = ((unsigned long long)r8hi_h << 32) | lo32(r8h);
        const bool filter_ok = bb > PTE_ISING_FILTER_MIN;
        // this lane's hypothesis (lk, lc, lb), as in k_explore_ising_spec
        const int lk = (lane >= 2) + (lane >= 12) + (lane >= 30);
        const int lbase = lk == 0 ? 0 : lk == 1 ? 2 : lk == 2 ? 12 : 30;
        const int lidx = lane - lbase;
        const int lc = lidx >> 1;
        const unsigned lb = (unsigned)(lidx & 1);
        const int lnext = (lk == 0 ? 2 : lk == 1 ? 12 : lk == 2 ? 30 : 0) + 2 * lc;
        const int lacc_sh = 7 + 4 * lk;
        double unit = u52_to_unit(mix64(seed + (uint64_t)(lane + 1) * gamma));
        unsigned long long mR4, mA4, mR8, mA8;
        auto classify = [&]() {
            const unsigned uh = (unsigned)__double2hiint(unit);
            mR4 = ballot64(uh > r4hi_h); mR8 = ballot64(uh > r8hi_h);
            mA4 = filter_ok ? ballot64(!(uh > r4hi_h) && !(uh < r4lo_h)) : ~0ull;
            mA8 = filter_ok ? ballot64(!(uh > r8hi_h) && !(uh < r8lo_h)) : ~0ull;
        };
        classify();
        int p = 0;
        // the boolean functions of a chunk (k_explore_ising_spec) from the GAUGED neighbour words, then the swap of the left = 0 / left = 1
        // halves where the left bond (jlw: bit t = the bond between site t - 1 and site t) is -1
        struct ChunkStatics { unsigned NN, II, SN; };
        auto chunk_statics = [&](unsigned upw, unsigned dnw, unsigned curw, unsigned cur_r, unsigned jlw, int T0) -> ChunkStatics {
            const int t0 = T0 + 4 * lk;
            const unsigned U = (upw >> t0) & 15u, D = (dnw >> t0) & 15u, R = (cur_r >> t0) & 15u, S = (curw >> t0) & 15u, Lb = (jlw >> t0) & 15u;
            const unsigned b0 = U ^ D ^ R, b1 = (U & D) | (R & (U ^ D));
            unsigned N0 = (S & b1 & b0) | (~S & ~b1),       I0 = (S & b1 & b0) | (~S & ~b1 & b0);
            unsigned N1 = (S & b1) | (~S & ~b1 & ~b0),      I1 = (S & b1 & ~b0) | (~S & ~b1 & ~b0);
            const unsigned xN = (N0 ^ N1) & Lb, xI = (I0 ^ I1) & Lb;
            N0 ^= xN; N1 ^= xN; I0 ^= xI; I1 ^= xI;
            return ChunkStatics{(N0 & 15u) | ((N1 & 15u) << 4), (I0 & 15u) | ((I1 & 15u) << 4), ~S};      // bit j + 4 left
        };
        for (int k = 0; k < gp.n_steps; ++k) {
            for (int i = 0; i < L; ++i) {
                const int rowu = ((i == 0 ? L : i) - 1) * W, rowd = (i == L - 1 ? 0 : i + 1) * W, row = i * W;
                unsigned b = lds_word(words, row + W - 1) >> 31;             // left neighbour of (i, 0): (i, L-1), not yet updated
                unsigned first_updated = 0;
                // read one iteration ahead, as there; `up` and `dn` are kept GAUGED (spin bit XOR the bond to this row), nothing needs them raw
                unsigned cur = lds_word(words, row);
                unsigned up = lds_word(words, rowu) ^ lds_word(jdp, rowu), dn = lds_word(words, rowd) ^ lds_word(jdp, row);
                unsigned nxt = ONE_WORD ? 0u : lds_word(words, row + 1);
                unsigned jr = lds_word(jrp, row);
                unsigned jl = (jr << 1) | (lds_word(jrp, row + W - 1) >> 31);  // column 0's left bond: bit 31 of the row's last bond word
                ChunkStatics st0 = chunk_statics(up, dn, cur, (cur >> 1) ^ jr, jl, 0), st1 = st0;      // (chunk 0 never looks at bit 31's right neighbour)
                for (int wj = 0; wj < W; ++wj) {
                    // (broadcast reads, unconditional: behind a row's last word nobody uses them)
                    const unsigned pf_up = words[rowu + wj + 1] ^ jdp[rowu + wj + 1], pf_dn = words[rowd + wj + 1] ^ jdp[row + wj + 1];
                    const unsigned pf_nx = words[row + wj + 2], pf_jr = jrp[row + wj + 1];
                    const unsigned rightbit = (wj == W - 1) ? (first_updated & 1u) : (nxt & 1u);
#pragma unroll
                    for (int T0 = 0; T0 < 32; T0 += 16) {
                        if (__builtin_expect(p + 16 > 64, 0)) {
                            seed += (uint64_t)p * gamma; unit = u52_to_unit(mix64(seed + (uint64_t)(lane + 1) * gamma)); p = 0;
                            classify();
                        }
                        const unsigned rt31 = ONE_WORD ? (cur & 1u) : rightbit;
                        // ---- vector pass: every (quad, consumed, left) hypothesis of the chunk walks its four sites
                        const int sh = p + lc;                                   // <= 48 + 12
                        unsigned wR4 = (unsigned)(mR4 >> sh), wA4 = (unsigned)(mA4 >> sh), wR8 = (unsigned)(mR8 >> sh), wA8 = (unsigned)(mA8 >> sh);
                        asm volatile("" : "+v"(wR4), "+v"(wA4), "+v"(wR8), "+v"(wA8));
                        if (T0 == 16 && ONE_WORD) st1 = chunk_statics(up, dn, cur, ((cur >> 1) | (rt31 << 31)) ^ jr, jl, 16);   // (a one-word row: bit 31's right neighbour is bit 0, just swept)
                        const ChunkStatics st = T0 == 0 ? st0 : st1;
                        const unsigned NN = st.NN, II = st.II, SN = st.SN;
                        const unsigned WR = (wR8 & 15u) | ((wR4 & 15u) << 4), WA = (wA8 & 15u) | ((wA4 & 15u) << 4);   // bit dc + 4 [delta == -4]
                        int dc = 0;
                        unsigned left = lb, ambu = 0, rejn = 0;
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            const unsigned shj = (left << 2) + (unsigned)j;
                            const unsigned need = (NN >> shj) & 1u, is4 = (II >> shj) & 1u;
                            const unsigned idx = (is4 << 2) + (unsigned)dc;
                            const unsigned rej = need & (WR >> idx);
                            ambu |= need & (WA >> idx);
                            left = ((SN >> j) ^ rej) & 1u;                       // the site's new spin: flipped unless rejected
                            rejn |= (rej & 1u) << j;
                            dc += (int)need;
                        }
                        const int accbits = (int)(rejn ^ 15u);
                        ambu &= 1u;
                        const int pk = (lnext + 2 * dc + (int)left) | ((int)ambu << 6) | (accbits << lacc_sh);
                        // ---- chase over the four quads: state s2 = 2 c + b; the statics of the chunk AFTER this one between the hops
                        int s2 = (int)b;
                        const unsigned n_up = T0 == 0 ? up : pf_up, n_dn = T0 == 0 ? dn : pf_dn, n_cw = T0 == 0 ? cur : nxt;
                        const unsigned n_cr = T0 == 0 ? (((cur >> 1) | (rightbit << 31)) ^ jr) : ((nxt >> 1) ^ pf_jr);
                        const unsigned n_jl = T0 == 0 ? jl : ((pf_jr << 1) | (jr >> 31));       // the carry of the left bond across words
                        int nt0 = (T0 == 0 ? 16 : 0) + 4 * lk;
                        int q0 = __builtin_amdgcn_readlane(pk, s2);
                        asm volatile("" : "+s"(q0), "+v"(nt0));
                        unsigned sU = n_up >> nt0, sD = n_dn >> nt0, sR = n_cr >> nt0, sS = n_cw >> nt0, sL = n_jl >> nt0;
                        asm volatile("" : "+s"(q0), "+v"(sU), "+v"(sD), "+v"(sR), "+v"(sS), "+v"(sL));
                        int q1 = __builtin_amdgcn_readlane(pk, q0);
                        asm volatile("" : "+s"(q1), "+v"(sU), "+v"(sD), "+v"(sR), "+v"(sS));
                        unsigned sb0 = sU ^ sD ^ sR, sb1 = (sU & sD) | (sR & (sU ^ sD));
                        unsigned sN0 = (sS & sb1 & sb0) | (~sS & ~sb1), sN1 = (sS & sb1) | (~sS & ~sb1 & ~sb0);
                        { const unsigned x = (sN0 ^ sN1) & sL; sN0 ^= x; sN1 ^= x; }
                        asm volatile("" : "+s"(q1), "+v"(sb0), "+v"(sb1), "+v"(sN0), "+v"(sN1));
                        int q2 = __builtin_amdgcn_readlane(pk, q1);
                        asm volatile("" : "+s"(q2), "+v"(sb0), "+v"(sb1), "+v"(sN0), "+v"(sN1));
                        unsigned sI0 = (sS & sb1 & sb0) | (~sS & ~sb1 & sb0), sI1 = (sS & sb1 & ~sb0) | (~sS & ~sb1 & ~sb0);
                        { const unsigned x = (sI0 ^ sI1) & sL; sI0 ^= x; sI1 ^= x; }
                        unsigned sNN = (sN0 & 15u) | ((sN1 & 15u) << 4);
                        asm volatile("" : "+s"(q2), "+v"(sI0), "+v"(sI1), "+v"(sNN));
                        const int q3 = __builtin_amdgcn_readlane(pk, q2);
                        {
                            const ChunkStatics nst{sNN, (sI0 & 15u) | ((sI1 & 15u) << 4), ~sS};
                            if (T0 == 0) st1 = nst; else st0 = nst;          // (T0 == 16: the next word, read ahead)
                        }
                        const int qa = q0 | q1 | q2 | q3;
                        unsigned cur_fast = cur ^ ((((unsigned)qa >> 7) & 0xFFFFu) << T0);
                        int s2_fast = q3 & 63;
                        asm volatile("" : "+s"(cur_fast), "+s"(s2_fast));
                        if (__builtin_expect((qa & 64) != 0, 0)) {
#pragma unroll
                            for (int kq = 0; kq < 4; ++kq) {
                                const int qbase = kq == 0 ? 0 : kq == 1 ? 2 : kq == 2 ? 12 : 30, nbase = kq == 0 ? 2 : kq == 1 ? 12 : kq == 2 ? 30 : 0;
                                const int q = __builtin_amdgcn_readlane(pk, qbase + s2);
                                if (__builtin_expect(q & 64, 0)) {
                                    // a guard-band decision (or a chain whose filter is not valid) inside this quad: its four sites by
                                    // the scalar procedure with the exact arithmetic of the reference where needed
                                    int cc = s2 >> 1;
                                    unsigned bb_ = (unsigned)(s2 & 1);
                                    for (int j = 0; j < 4; ++j) {
                                        const int tt = T0 + 4 * kq + j;
                                        const unsigned sgs = (cur >> tt) & 1u;
                                        const unsigned rts = (tt == 31 ? rt31 : ((cur >> (tt + 1)) & 1u)) ^ ((jr >> tt) & 1u);
                                        const unsigned lfs = bb_ ^ ((jl >> tt) & 1u);
                                        const int nbs = 2 * (int)(((up >> tt) & 1u) + ((dn >> tt) & 1u) + lfs + rts) - 4;
                                        const int dl = (1 - 2 * (int)sgs) * 2 * nbs;
                                        int rj = 0, nd = 0;
                                        if (dl < 0) {
                                            nd = 1;
                                            const unsigned uh = (unsigned)__builtin_amdgcn_readlane(__double2hiint(unit), p + cc);
                                            const unsigned ul = (unsigned)__builtin_amdgcn_readlane(__double2loint(unit), p + cc);
                                            const unsigned long long ub = ((unsigned long long)uh << 32) | ul;
                                            const unsigned long long lo = dl == -4 ? r4lo : r8lo, hi = dl == -4 ? r4hi : r8hi;
                                            if (filter_ok && ub > hi) rj = 1;
                                            else if (filter_ok && ub < lo) rj = 0;
                                            else {
                                                if (lane == 0) words[row + wj] = cur;
                                                __syncthreads();
                                                const long long spp = recompute();
                                                const double ratio = exp(ising_lp(beta, bt, (double)(spp + dl)) - ising_lp(beta, bt, (double)spp));
                                                if (ratio < 1) rj = (__longlong_as_double((long long)ub) > ratio) ? 1 : 0;
                                                else { rj = 0; nd = 0; }          // accept_ratio >= 1: the reference draws nothing
                                            }
                                        }
                                        cur ^= (unsigned)(rj ? 0 : 1) << tt;
                                        bb_ = (cur >> tt) & 1u;
                                        cc += nd;
                                    }
                                    s2 = __builtin_amdgcn_readfirstlane(2 * cc + (int)bb_);
                                    cur = (unsigned)__builtin_amdgcn_readfirstlane((int)cur);
                                } else {
                                    cur ^= (((unsigned)q >> 7) & 0xFFFFu) << T0;
                                    s2 = (q & 63) - nbase;
                                }
                            }
                        } else {
                            cur = cur_fast; s2 = s2_fast;
                        }
                        p += s2 >> 1;
                        b = (unsigned)(s2 & 1);
                    }
                    words[row + wj] = cur;                                      // (every lane the same word to the same address)
                    if (wj == 0) first_updated = cur;
                    cur = nxt;
                    up = (unsigned)__builtin_amdgcn_readfirstlane((int)pf_up); dn = (unsigned)__builtin_amdgcn_readfirstlane((int)pf_dn);
                    nxt = (unsigned)__builtin_amdgcn_readfirstlane((int)pf_nx);
                    const unsigned jr_n = (unsigned)__builtin_amdgcn_readfirstlane((int)pf_jr);
                    jl = (jr_n << 1) | (jr >> 31);
                    jr = jr_n;
                }
            }
        }
        seed += (uint64_t)p * gamma;
    }
    __syncthreads();
    const long long spp = recompute();
    for (int wd = lane; wd < NW; wd += 64) wrow[wd] = words[wd];
    if (lane == 0) { e.suff[slot] = (double)spp; e.rng[2 * slot] = seed; }
    record_after_explore(e, cl, c, slot, lane, lp_before, (double)spp, 0.0);
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
