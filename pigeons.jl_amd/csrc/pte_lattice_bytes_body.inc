// pte_lattice_bytes_body.inc -- the body of the byte-lattice sequential sweep, held once for k_explore_ising (pte_ising.hpp) and
// k_explore_spinglass (pte_spinglass.hpp): the same draw order, statement for statement, with the neighbour sum weighted by the bonds in
// the second.  Not a header: it is spliced between the braces of each kernel (pte_lattice_spec_body.inc says why), which declares
//     EngineDev e;  <the family's parameters> tp;      the kernel's arguments (tp.L, tp.n_steps, tp.beta_target)
//     constexpr bool BONDS;                            whether a site's LDS byte carries its two bonds (bit 1 = JR, bit 2 = JD, set where -1)
//     const unsigned char *const jb;                   BONDS: the bonds of site s at their place in the byte; nullptr otherwise
// Any L >= 2; dynamic LDS: L * L bytes.
    extern __shared__ unsigned char spins[];
    const int lane = lane_id();
    const int64_t cl = blockIdx.x;
    if (cl >= e.K) return;
    const int64_t c = e.c0 + cl;
    const int slot = e.slot_of_chain[cl];
    const int L = tp.L, d = L * L, NW = (d + 31) >> 5;
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
        const unsigned bb = rng_bool_bit();              // include/pte_rng_policy.h (default 0: `% Bool`)
        for (int s = lane; s < d; s += 64) spins[s] = (unsigned char)(((mix64(seed + (uint64_t)(s + 1) * gamma) >> bb) & 1ull) | (BONDS ? jb[s] : 0));
        seed += (uint64_t)d * gamma;
        __syncthreads();
        const long long spp = BONDS ? spinglass_recompute(spins, L, lane) : ising_recompute(spins, L, lane);
        store_lattice();
        if (lane == 0) { e.suff[slot] = (double)spp; e.rng[2 * slot] = seed; }
        record_after_explore(e, cl, c, slot, lane, lp_before, (double)spp, 0.0);
        return;
    }
    for (int s = lane; s < d; s += 64) spins[s] = (unsigned char)(((wrow[s >> 5] >> (s & 31)) & 1u) | (BONDS ? jb[s] : 0));
    __syncthreads();
    long long spp = (long long)e.suff[slot];
    const double beta = e.beta[c], bt = tp.beta_target;
    const LatticeThresholds th = lattice_thresholds(beta * bt);

    // 64 buffered uniforms of the replica's stream
    double unit = u52_to_unit(mix64(seed + (uint64_t)(lane + 1) * gamma));
    int p = 0;

    for (int k = 0; k < tp.n_steps; ++k) {
        int s = 0;
        for (int i = 0; i < L; ++i) {
            const int rowu = ((i == 0 ? L : i) - 1) * L, rowd = (i == L - 1 ? 0 : i + 1) * L, row = i * L;
            for (int j = 0; j < L; ++j, ++s) {
                int sg, nb, c0 = 0;
                if constexpr (BONDS) {
                    c0 = sg_byte(spins, s);
                    const int cu = sg_byte(spins, rowu + j), cd = sg_byte(spins, rowd + j);
                    const int cf = sg_byte(spins, row + (j == 0 ? L : j) - 1), cr = sg_byte(spins, row + (j == L - 1 ? 0 : j + 1));
                    sg = sg_pm(c0);
                    // J_sn s_n: up through JD of the site above, down through the site's own JD, left through JR of the site to the left, right through its own JR
                    // (spin bit 1 = +1, bond bit 1 = -1: the product is +1 where the two bits differ)
                    nb = sg_pm(cu ^ (cu >> 2)) + sg_pm(cd ^ (c0 >> 2)) + sg_pm(cf ^ (cf >> 1)) + sg_pm(cr ^ (c0 >> 1));
                } else {
                    sg = ising_site(spins, s);
                    nb = ising_site(spins, rowu + j) + ising_site(spins, rowd + j) +
                         ising_site(spins, row + (j == 0 ? L : j) - 1) + ising_site(spins, row + (j == L - 1 ? 0 : j + 1));
                }
                const int delta = -2 * sg * nb;            // (bond-weighted) sum_pair_products after - before (flip!, ising.jl:38-46)
                bool accept = true;
                if (delta < 0) {
                    bool need_draw = true, decided = false;
                    double ratio = 0.0;
                    if (__builtin_expect(!th.filter_ok, 0)) {
                        ratio = exp(ising_lp(beta, bt, (double)(spp + delta)) - ising_lp(beta, bt, (double)spp));
                        need_draw = ratio < 1;
                        decided = true;
                    }
                    if (need_draw) {
                        if (p == 64) { seed += 64ull * gamma; unit = u52_to_unit(mix64(seed + (uint64_t)(lane + 1) * gamma)); p = 0; }
                        const double u = readlane_f64(unit, p);
                        p += 1;
                        if (!decided) {
                            const double lo = delta == -4 ? th.r4lo : th.r8lo, hi = delta == -4 ? th.r4hi : th.r8hi;
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
                    if (lane == 0) spins[s] = BONDS ? (unsigned char)(c0 ^ 1) : (unsigned char)(sg > 0 ? 0 : 1);
                    spp += delta;
                }
            }
        }
    }
    __syncthreads();
    store_lattice();
    if (lane == 0) { e.suff[slot] = (double)spp; e.rng[2 * slot] = seed + (uint64_t)p * gamma; }
    record_after_explore(e, cl, c, slot, lane, lp_before, (double)spp, 0.0);
