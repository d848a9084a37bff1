// pte_lattice_spec_body.inc -- the body of the lane-speculative lattice sweep, held once for k_explore_ising_spec<ONE_WORD> (pte_ising.hpp)
// and k_explore_spinglass_spec<ONE_WORD> (pte_spinglass.hpp).  Not a header: it is spliced between the braces of each kernel, which declares
//     EngineDev e;  <the family's parameters> tp;      the kernel's arguments (tp.L, tp.n_steps, tp.beta_target)
//     constexpr bool BONDS;                            whether the lattice has bond planes (the spin glass) or every bond is +1 (Ising)
//     const unsigned *const jw;                        BONDS: the two planes bit-packed like the lattice, JR then JD; nullptr otherwise
// A fragment and not a __device__ function called from both: inlined from a function the walk comes out 2 VALU per word longer in all four
// instantiations, spliced in it reproduces the code each kernel had as a text of its own (DESIGN 4.17).
//
// The bit-packed sweep with the 64 lanes as hypotheses, the way k_explore_slice7/8 break the slice sampler's chain.  The outcome of site t
// depends on the sweep so far only through (b, c): the NEW value b of its left neighbour and the number c of uniforms consumed since the
// chunk started (which picks the uniform it would read).  A 16-site chunk is cut into four quads; quad k can start in 2 (4k + 1) states, 56
// hypotheses in all: each lane walks the four sites of its quad under its (c, b) in one vector pass (neighbour counts, deltas, the filtered
// accept decisions against the integer thresholds), and a scalar chase of four steps per chunk picks the true quads and carries the state
// on.  Guard-band decisions (and chains whose filter is not valid) are taken by the exact arithmetic of the reference, with
// sum_pair_products recomputed on demand; the final sum_pair_products is recomputed from the lattice by popcounts.
//
// BONDS: the bonds are folded into what the walk is GIVEN, so that the per-site walk, the pack word and the chase are the same code:
//   * the words above / below / to the right enter a chunk only as neighbour nibbles: XOR the bond words into them first
//     (up ^= JD of the row above, dn ^= JD of this row, right ^= JR of this row);
//   * the left neighbour is the one the walk carries (its NEW value).  Its bond is JR shifted by one site -- with the carry across words
//     and, at column 0, bit 31 of the row's last bond word -- and is folded into the statics: NN / II hold each site's answer for
//     left = 0 and for left = 1; where the left bond is -1 the two halves swap.
// The scalar guard-band path and recompute() take the bonds the same way.  Without BONDS the bond words are the constant 0 and the
// statements that only move them are compiled out.
//
// ONE_WORD: base_length == 32 (a row is one word: bit 31's right neighbour is bit 0 of the same word, swept in the same iteration) -- its
// own instantiation, so that the wider lattices do not test for it twice per word.  Dynamic LDS: L * L / 8 bytes + 8 (the read-ahead of the
// word to the right runs two words past a row's end); BONDS: three such planes (lattice, JR, JD), loaded once per launch.
    extern __shared__ unsigned words[];
    const int lane = lane_id();
    const int64_t cl = blockIdx.x;
    if (cl >= e.K) return;
    const int64_t c = e.c0 + cl;
    const int slot = e.slot_of_chain[cl];
    const int L = tp.L, d = L * L, W = ONE_WORD ? 1 : (L >> 5), NW = d >> 5;
    unsigned *const jrp = words + NW + 2, *const jdp = words + 2 * (NW + 2);        // BONDS: the bond planes behind the lattice, each with its two words of padding
    unsigned *wrow = reinterpret_cast<unsigned *>(e.x + (int64_t)slot * e.ld);     // bit-packed lattice in HBM, same word layout as the LDS copy
    uint64_t seed = e.rng[2 * slot];
    const uint64_t gamma = e.rng[2 * slot + 1];
    const double lp_before = lp_before_explore(e, c, slot);
    const bool refresh = is_ref_chain(e, c);
#ifdef PTE_PROFILE_WAVES
    const uint64_t wave_t0 = __builtin_amdgcn_s_memrealtime();
#endif
#ifdef PTE_PROFILE_ISING_SECTIONS
    unsigned long long prof_pass = 0, prof_chase = 0, prof_loop = 0;
#endif

    for (int wd = lane; wd < NW; wd += 64) {
        unsigned v = 0;
        if (refresh) { const unsigned bb = rng_bool_bit(); for (int t = 0; t < 32; ++t) v |= (unsigned)((mix64(seed + (uint64_t)(32 * wd + t + 1) * gamma) >> bb) & 1ull) << t; }
        else         { v = wrow[wd]; }
        words[wd] = v;
        if constexpr (BONDS) { jrp[wd] = jw[wd]; jdp[wd] = jw[NW + wd]; }
    }
    if constexpr (BONDS) {
        if (lane < 2) { words[NW + lane] = 0u; jrp[NW + lane] = 0u; jdp[NW + lane] = 0u; }      // (the padding: read ahead, never used)
    }
    if (refresh) seed += (uint64_t)d * gamma;
    __syncthreads();
    // recompute_sum_pair_products from the LDS lattice (BONDS: the bond-weighted pair sum from the LDS planes): every bond once (right + down
    // neighbour products)
    auto recompute = [&]() -> long long {
        long long acc = 0;
        for (int wd = lane; wd < NW; wd += 64) {
            const int i = wd / W, wj = wd - i * W;
            const unsigned cur = words[wd], dn = words[(i == L - 1 ? 0 : i + 1) * W + wj];
            const unsigned nxt = words[i * W + (wj == W - 1 ? 0 : wj + 1)];
            const unsigned right = (cur >> 1) | (nxt << 31);
            acc += 64 - 2 * ((int)__popc(cur ^ right ^ (BONDS ? jrp[wd] : 0u)) + (int)__popc(cur ^ dn ^ (BONDS ? jdp[wd] : 0u)));
        }
        for (int k = 1; k < 64; k <<= 1) acc += __shfl_xor(acc, k, 64);
        return acc;
    };
    if (!refresh) {
        const double beta = e.beta[c], bt = tp.beta_target;
        const LatticeThresholds th = lattice_thresholds(beta * bt);
        // this lane's hypothesis (lk, lc, lb): quad lk of a 16-site chunk (sites 4 lk .. 4 lk + 3), lc uniforms consumed
        // since the chunk started, left neighbour of the quad's first site now lb; 2 (4 lk + 1) hypotheses per quad = 56 lanes
        const int lk = (lane >= 2) + (lane >= 12) + (lane >= 30);
        const int lbase = lk == 0 ? 0 : lk == 1 ? 2 : lk == 2 ? 12 : 30;
        const int lidx = lane - lbase;
        const int lc = lidx >> 1;
        const unsigned lb = (unsigned)(lidx & 1);
        const int lnext = (lk == 0 ? 2 : lk == 1 ? 12 : lk == 2 ? 30 : 0) + 2 * lc;      // lane of the next quad's hypothesis (c, spin) = lnext + 2 dc + spin
        const int lacc_sh = 7 + 4 * lk;
        double unit = u52_to_unit(mix64(seed + (uint64_t)(lane + 1) * gamma));
        // The 64 buffered uniforms enter the vector pass only through four comparisons of their high words with the guard-banded
        // thresholds: taken once per refill for the whole buffer (four ballots, bit i = uniform i), a hypothesis that has consumed
        // lc uniforms reads bit (p + lc + its own count) of the mask its delta selects -- no LDS copy of the buffer, no load on the
        // chain p -> pass -> chase -> p.   R = certainly rejected (u above the band), A = inside the band (or no valid filter).
        unsigned long long mR4, mA4, mR8, mA8;
        auto classify = [&]() {
            const unsigned uh = (unsigned)__double2hiint(unit);
            mR4 = ballot64(uh > th.r4hi_h); mR8 = ballot64(uh > th.r8hi_h);
            mA4 = th.filter_ok ? ballot64(!(uh > th.r4hi_h) && !(uh < th.r4lo_h)) : ~0ull;
            mA8 = th.filter_ok ? ballot64(!(uh > th.r8hi_h) && !(uh < th.r8lo_h)) : ~0ull;
        };
        classify();
        int p = 0;
        // What a chunk's sites need from their surroundings (see the vector pass below) does not depend on the sweep of the chunk BEFORE it:
        // that one flips its own 16 bits only.  So the boolean functions of a chunk are evaluated before the chase of the previous one, in
        // whose wait states they can issue (a chained hop leaves ~20 cycles in which a lone wave issues nothing otherwise).
        // BONDS: from the GAUGED neighbour words, then the swap of the left = 0 / left = 1 halves where the left bond (jlw: bit t = the bond
        // between site t - 1 and site t) is -1
        struct ChunkStatics { unsigned NN, II, SN; };
        auto chunk_statics = [&](unsigned upw, unsigned dnw, unsigned curw, unsigned cur_r, unsigned jlw, int T0) -> ChunkStatics {
            const int t0 = T0 + 4 * lk;
            const unsigned U = (upw >> t0) & 15u, D = (dnw >> t0) & 15u, R = (cur_r >> t0) & 15u, S = (curw >> t0) & 15u;
            const unsigned b0 = U ^ D ^ R, b1 = (U & D) | (R & (U ^ D));
            unsigned N0 = (S & b1 & b0) | (~S & ~b1),       I0 = (S & b1 & b0) | (~S & ~b1 & b0);
            unsigned N1 = (S & b1) | (~S & ~b1 & ~b0),      I1 = (S & b1 & ~b0) | (~S & ~b1 & ~b0);
            if constexpr (BONDS) {
                const unsigned Lb = (jlw >> t0) & 15u;
                const unsigned xN = (N0 ^ N1) & Lb, xI = (I0 ^ I1) & Lb;
                N0 ^= xN; N1 ^= xN; I0 ^= xI; I1 ^= xI;
            }
            return ChunkStatics{(N0 & 15u) | ((N1 & 15u) << 4), (I0 & 15u) | ((I1 & 15u) << 4), ~S};      // bit j + 4 left
        };
#ifdef PTE_PROFILE_ISING_SECTIONS          // debug builds only (with -DPTE_PROFILE_WAVES): shader-clock cycles of the vector pass / the chase, summed over the chunks
        const unsigned long long prof_t0 = __builtin_readcyclecounter();
#endif
        for (int k = 0; k < tp.n_steps; ++k) {
            for (int i = 0; i < L; ++i) {
                const int rowu = ((i == 0 ? L : i) - 1) * W, rowd = (i == L - 1 ? 0 : i + 1) * W, row = i * W;
                unsigned b = lds_word(words, row + W - 1) >> 31;             // left neighbour of (i, 0): (i, L-1), not yet updated
                unsigned first_updated = 0;
                // The words of a row are read one iteration AHEAD (the sweep of word wj writes words[row + wj] only; the rows above and
                // below and the words to its right keep their values while it runs): the LDS round trip of the next word's three reads
                // (~120 cycles of a lone wave, 8 % of a word's time) runs under this word's two passes, and the word to the right --
                // read for its bit 0 -- IS the next word to sweep.
                // BONDS: `up` and `dn` are kept GAUGED (spin bit XOR the bond to this row), nothing needs them raw
                unsigned cur = lds_word(words, row);
                unsigned up = lds_word(words, rowu) ^ (BONDS ? lds_word(jdp, rowu) : 0u), dn = lds_word(words, rowd) ^ (BONDS ? lds_word(jdp, row) : 0u);
                unsigned nxt = ONE_WORD ? 0u : lds_word(words, row + 1);
                unsigned jr = BONDS ? lds_word(jrp, row) : 0u;
                unsigned jl = BONDS ? (jr << 1) | (lds_word(jrp, row + W - 1) >> 31) : 0u;  // column 0's left bond: bit 31 of the row's last bond word
                ChunkStatics st0 = chunk_statics(up, dn, cur, (cur >> 1) ^ jr, jl, 0), st1 = st0;      // (chunk 0 never looks at bit 31's right neighbour)
                for (int wj = 0; wj < W; ++wj) {
                    // (every lane reads the same address: a broadcast.  Unconditional: behind a row's last word these are words of the next
                    // row or of the two words of padding behind the lattice, and nobody uses them -- a branch around three loads costs more)
                    const unsigned pf_up = words[rowu + wj + 1] ^ (BONDS ? jdp[rowu + wj + 1] : 0u), pf_dn = words[rowd + wj + 1] ^ (BONDS ? jdp[row + wj + 1] : 0u);
                    const unsigned pf_nx = words[row + wj + 2], pf_jr = BONDS ? jrp[row + wj + 1] : 0u;
                    const unsigned rightbit = (wj == W - 1) ? (first_updated & 1u) : (nxt & 1u);
#pragma unroll
                    for (int T0 = 0; T0 < 32; T0 += 16) {
#ifdef PTE_PROFILE_ISING_SECTIONS
                        const unsigned long long pa = __builtin_readcyclecounter();
#endif
                        if (__builtin_expect(p + 16 > 64, 0)) {           // (one chunk in ~5: laid out behind the loop, so that the common path falls through -- a lone wave refetches after a taken branch)
                            seed += (uint64_t)p * gamma; unit = u52_to_unit(mix64(seed + (uint64_t)(lane + 1) * gamma)); p = 0;
                            classify();
                        }
                        const unsigned rt31 = ONE_WORD ? (cur & 1u) : rightbit;
                        // ---- vector pass: every (quad, consumed, left) hypothesis of the chunk walks its four sites
                        // (its uniforms are the next <= 4 of the buffer from position p + lc: bits p + lc .. of the masks)
                        const int sh = p + lc;                                   // <= 48 + 12
                        unsigned wR4 = (unsigned)(mR4 >> sh), wA4 = (unsigned)(mA4 >> sh), wR8 = (unsigned)(mR8 >> sh), wA8 = (unsigned)(mA8 >> sh);
                        asm volatile("" : "+v"(wR4), "+v"(wA4), "+v"(wR8), "+v"(wA8));   // (keep the four 64-bit shifts here: hipcc sinks them below the per-site selects, 8 per pass)
                        // What a site needs from its surroundings does not depend on the walk except through its NEW left neighbour: for
                        // the quad's four sites at once (bit j = site j), from the nibbles of the word above, below, to the right (old
                        // values) and of the spins themselves -- cnt = neighbours that are 1 = (U + D + R) + left, delta = (1 - 2 s) 2 (2 cnt - 4):
                        //   a draw is needed iff  s ? cnt > 2 : cnt < 2,   delta == -4 iff  s ? cnt == 3 : cnt == 1
                        // as boolean functions of (b1 b0 = U + D + R, s), once for left = 0 and once for left = 1; the walk then only
                        // picks bits: 12 instead of 19 instructions per site.
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
                            const unsigned rej = need & (WR >> idx);             // (bit 0; the bits above are dropped where it is used)
                            ambu |= need & (WA >> idx);
                            left = ((SN >> j) ^ rej) & 1u;                       // the site's new spin: flipped unless rejected
                            rejn |= (rej & 1u) << j;
                            dc += (int)need;
                        }
                        const int accbits = (int)(rejn ^ 15u);
                        ambu &= 1u;
                        // The word a hypothesis hands to the chase: bits 0-5 = the LANE of the hypothesis that continues it in the next quad
                        // (quad 3: the state 2 c + spin the chunk ends in), bit 6 = a guard-band decision somewhere in the quad, bits 7-22 =
                        // its accepts already at the quad's place in the chunk.  A hop is then ONE v_readlane whose lane select is the word
                        // read before (the hardware takes bits 0-5), and the chunk's flips are the OR of the four words: round 4 priced a hop
                        // with a shift and an add between the reads at 34-42 cycles against 27.5 chained (tools/ubench/round_cost.hip).
                        const int pk = (lnext + 2 * dc + (int)left) | ((int)ambu << 6) | (accbits << lacc_sh);
                        // ---- chase over the four quads: state s2 = 2 c + b
                        int s2 = (int)b;
#ifdef PTE_PROFILE_ISING_SECTIONS
                        asm volatile("" :: "v"(pk));
                        const unsigned long long pb = __builtin_readcyclecounter();
#endif
                        // all four quads at once when none of them met a guard-band decision (the common case): no branches.
                        // The statics of the chunk AFTER this one are evaluated in three pieces of four instructions BETWEEN the hops: the
                        // empty asm statements tie each piece's inputs to the hop before it and its results to the hop after it (pure
                        // data flow: hipcc would otherwise schedule all of it above the first hop and fill the gaps with s_nop).
                        const unsigned n_up = T0 == 0 ? up : pf_up, n_dn = T0 == 0 ? dn : pf_dn, n_cw = T0 == 0 ? cur : nxt;
                        const unsigned n_cr = T0 == 0 ? (((cur >> 1) | (rightbit << 31)) ^ jr) : ((nxt >> 1) ^ pf_jr);
                        const unsigned n_jl = T0 == 0 ? jl : ((pf_jr << 1) | (jr >> 31));       // the carry of the left bond across words
                        int nt0 = (T0 == 0 ? 16 : 0) + 4 * lk;
                        int q0 = __builtin_amdgcn_readlane(pk, s2);
                        asm volatile("" : "+s"(q0), "+v"(nt0));
                        unsigned sU = n_up >> nt0, sD = n_dn >> nt0, sR = n_cr >> nt0, sS = n_cw >> nt0, sL = 0u;
                        if constexpr (BONDS) {
                            sL = n_jl >> nt0;
                            asm volatile("" : "+s"(q0), "+v"(sU), "+v"(sD), "+v"(sR), "+v"(sS), "+v"(sL));
                        } else {                    // (a fence that names sL here would hold a zero in a VGPR)
                            asm volatile("" : "+s"(q0), "+v"(sU), "+v"(sD), "+v"(sR), "+v"(sS));
                        }
                        int q1 = __builtin_amdgcn_readlane(pk, q0);
                        asm volatile("" : "+s"(q1), "+v"(sU), "+v"(sD), "+v"(sR), "+v"(sS));
                        unsigned sb0 = sU ^ sD ^ sR, sb1 = (sU & sD) | (sR & (sU ^ sD));
                        unsigned sN0 = (sS & sb1 & sb0) | (~sS & ~sb1), sN1 = (sS & sb1) | (~sS & ~sb1 & ~sb0);
                        if constexpr (BONDS) { const unsigned x = (sN0 ^ sN1) & sL; sN0 ^= x; sN1 ^= x; }
                        asm volatile("" : "+s"(q1), "+v"(sb0), "+v"(sb1), "+v"(sN0), "+v"(sN1));
                        int q2 = __builtin_amdgcn_readlane(pk, q1);
                        asm volatile("" : "+s"(q2), "+v"(sb0), "+v"(sb1), "+v"(sN0), "+v"(sN1));
                        unsigned sI0 = (sS & sb1 & sb0) | (~sS & ~sb1 & sb0), sI1 = (sS & sb1 & ~sb0) | (~sS & ~sb1 & ~sb0);
                        if constexpr (BONDS) { const unsigned x = (sI0 ^ sI1) & sL; sI0 ^= x; sI1 ^= x; }
                        unsigned sNN = (sN0 & 15u) | ((sN1 & 15u) << 4);
                        asm volatile("" : "+s"(q2), "+v"(sI0), "+v"(sI1), "+v"(sNN));
                        const int q3 = __builtin_amdgcn_readlane(pk, q2);
                        {
                            const ChunkStatics nst{sNN, (sI0 & 15u) | ((sI1 & 15u) << 4), ~sS};
                            if (T0 == 0) st1 = nst; else st0 = nst;          // (T0 == 16: the next word, read ahead; zeros behind the row's last word)
                        }
                        const int qa = q0 | q1 | q2 | q3;
                        // (the result of the common case first, ONE branch around the rest: with an if / else hipcc keeps a "took the fast
                        // side" flag in a scalar pair and tests it again behind the join)
                        unsigned cur_fast = cur ^ ((((unsigned)qa >> 7) & 0xFFFFu) << T0);
                        int s2_fast = q3 & 63;
                        asm volatile("" : "+s"(cur_fast), "+s"(s2_fast));      // (evaluated HERE: hipcc sinks them into an else side otherwise)
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
                                            const unsigned long long lo = dl == -4 ? th.r4lo_b : th.r8lo_b, hi = dl == -4 ? th.r4hi_b : th.r8hi_b;
                                            if (th.filter_ok && ub > hi) rj = 1;
                                            else if (th.filter_ok && ub < lo) rj = 0;
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
                                    // (every lane computed the same values; tell the compiler, so that the chunk loop stays scalar)
                                    s2 = __builtin_amdgcn_readfirstlane(2 * cc + (int)bb_);
                                    cur = (unsigned)__builtin_amdgcn_readfirstlane((int)cur);
                                } else {
                                    cur ^= (((unsigned)q >> 7) & 0xFFFFu) << T0;      // (the accepts sit at the quad's place; the other quads' bits are 0)
                                    s2 = (q & 63) - nbase;
                                }
                            }
                        } else {
                            cur = cur_fast; s2 = s2_fast;
                        }
#ifdef PTE_PROFILE_ISING_SECTIONS
                        asm volatile("" :: "s"(s2), "s"(cur));
                        { const unsigned long long pc = __builtin_readcyclecounter(); prof_pass += pb - pa; prof_chase += pc - pb; }
#endif
                        p += s2 >> 1;
                        b = (unsigned)(s2 & 1);
                    }
                    // every lane the same word to the same address: 4.18 ms per scan at the C5 shard shape, against 4.34 for lane 0 if the
                    // word changed (a compare, two scalar ANDs, an EXEC save / restore) and 4.32 for lane 0 always
                    words[row + wj] = cur;
                    if (wj == 0) first_updated = cur;
                    // (behind the row's last word these are zeros nobody reads: the row loop reloads)
                    cur = nxt;
                    up = (unsigned)__builtin_amdgcn_readfirstlane((int)pf_up); dn = (unsigned)__builtin_amdgcn_readfirstlane((int)pf_dn);
                    nxt = (unsigned)__builtin_amdgcn_readfirstlane((int)pf_nx);
                    if constexpr (BONDS) {
                        const unsigned jr_n = (unsigned)__builtin_amdgcn_readfirstlane((int)pf_jr);
                        jl = (jr_n << 1) | (jr >> 31);
                        jr = jr_n;
                    }
                }
            }
        }
        seed += (uint64_t)p * gamma;
#ifdef PTE_PROFILE_ISING_SECTIONS
        prof_loop = __builtin_readcyclecounter() - prof_t0;
#endif
    }
    __syncthreads();
    const long long spp = recompute();
    for (int wd = lane; wd < NW; wd += 64) wrow[wd] = words[wd];
    if (lane == 0) { e.suff[slot] = (double)spp; e.rng[2 * slot] = seed; }
    record_after_explore(e, cl, c, slot, lane, lp_before, (double)spp, 0.0);
#ifdef PTE_PROFILE_WAVES                   // debug builds only: per-wave start / end on the 100 MHz clock, placement
    if (lane == 0) {
        double *o = e.on_m2 + 2 * (e.d + 1) + 4 * cl;
        o[0] = (double)wave_t0; o[1] = (double)__builtin_amdgcn_s_memrealtime();
        o[2] = (double)__builtin_amdgcn_s_getreg((31 << 11) | 4); o[3] = (double)__builtin_amdgcn_s_getreg((31 << 11) | 20);
#ifdef PTE_PROFILE_ISING_SECTIONS
        o[0] = (double)prof_loop; o[1] = (double)prof_pass; o[2] = (double)prof_chase;
#endif
    }
#endif
