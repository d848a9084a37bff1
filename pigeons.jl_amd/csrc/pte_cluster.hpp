// pte_cluster.hpp -- Houdayer's cluster move between the two copies of a lattice pair (Houdayer 2001; with parallel tempering the
// isoenergetic cluster move of Zhu, Ochoa and Katzgraber 2015).  For chain c: a, b = the bit strings of the slots that hold chain c in engine A
// and in engine B (the HBM bit-packed lattice of pte_ising.hpp / pte_lattice3d.hpp), t = a xor b, k = popcount(t).
//   the draw      u = mix64(seed + (m N + c + 1) gamma), j = ((u >> 32) k) >> 32; the seed site is the j-th set bit of t in increasing site index
//   the cluster   C = the connected component of the seed site among the set bits of t under the lattice's nearest-neighbour links (periodic)
//   the flip      a ^= C, b ^= C: the sum of the two energies is unchanged, the move is always accepted and is its own inverse
//   the swap's    delta = sum_dir (4 popcount(B & x) - 2 popcount(B)), B = C xor shift_dir(C) the bonds with one end in the cluster,
//   statistic     x = a xor shift_dir(a) xor J_dir the bonds whose term is -1 before the flip; suff_a += delta, suff_b -= delta
//   k_cluster_move    one workgroup per chain: t, C and a in LDS, the component as a fixed point C <- C | (neighbours(C) & t)
// One workgroup owns a chain and the launches of a stream are ordered: plain loads and stores, no atomics.
#pragma once
#include "pte_lattice3d_params.hpp"
#include "pte_cluster_params.hpp"

namespace pte {

// w / div for w < 2048, div <= 32 with mul = ceil(65536 / div): exact where w (mul div - 65536) < 65536 -- w < 1024 at div <= 32 (the cube's
// rows), w < 2048 at div <= 8 (the square's words per row)
__device__ __forceinline__ int cluster_div(int w, unsigned mul) { return (int)(((unsigned)w * mul) >> 16); }

// The closure of n, a subset of t, along a row: every run of set bits of t that holds a bit of n, whole.  A log-step fill in both directions:
// after the step s the run is covered 2 s - 1 sites beyond every bit of n, so a run of any length costs log2 steps, not one pass per site.
//   ring   the row is the L <= 32 low bits of the word and closes on itself (the cube: +-x is the L-bit rotate)
//   word   the row goes on in the neighbouring words (the square): nothing wraps inside the word
__device__ __forceinline__ unsigned cluster_fill_ring(unsigned n, unsigned t, int L, unsigned mask) {
    unsigned up = n, pu = t, dn = n, pd = t;
    for (int s = 1; s < L; s <<= 1) {                                              // 1 <= s <= 16 and 1 <= L - s <= 31: no shift by 32
        up |= pu & (((up << s) | (up >> (L - s))) & mask); pu &= ((pu << s) | (pu >> (L - s))) & mask;
        dn |= pd & (((dn >> s) | (dn << (L - s))) & mask); pd &= ((pd >> s) | (pd << (L - s))) & mask;
    }
    return up | dn;
}
__device__ __forceinline__ unsigned cluster_fill_word(unsigned n, unsigned t) {
    unsigned up = n, pu = t, dn = n, pd = t;
#pragma unroll
    for (int s = 1; s < 32; s <<= 1) {
        up |= pu & (up << s); pu &= pu << s;
        dn |= pd & (dn >> s); pd &= pd >> s;
    }
    return up | dn;
}

// the sum of v over the workgroup, uniform: a wave reduction, then the waves' sums through red[] (NT / 64 words of LDS)
template <int NT>
__device__ __forceinline__ int cluster_block_sum(int v, int *red, int tid) {
    for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m, 64);
    if constexpr (NT == 64) return v;
    __syncthreads();                                                               // the readers of the sum before this one are done with red[]
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    int s = 0;
    for (int w = 0; w < NT / 64; ++w) s += red[w];
    return s;
}

// Dynamic LDS, 16-byte aligned: 16 words of scratch (the waves' partial sums, three vote words), then t, C and a, n words each.
//   cube    n = L^2: a row of L bits is one word (lattice3d_load_row), +-x is the rotate inside it, +-y and +-z are the neighbouring rows
//   square  L % 32 == 0, n = d / 32: row i is the words [i W, (i + 1) W), W = L / 32; +-x crosses into the neighbouring word of the row
//           (wrapping to the row's own other end), +-y is the word W away
// The site order of the draw is the order of the words and of the bits inside them in both forms.
__global__ __launch_bounds__(PTE_CLUSTER_THREADS) void k_cluster_move(ClusterSide sa, ClusterSide sb, ClusterMove mv, ClusterAcc acc) {
    extern __shared__ uint4 cluster_lds[];
    constexpr int NT = PTE_CLUSTER_THREADS;
    const int tid = (int)threadIdx.x, lane = tid & 63;
    const int c = blockIdx.x;
    if (c >= mv.N) return;
    if (!(mv.beta[c] >= mv.min_beta)) return;                                      // uniform over the workgroup, as is every exit below
    const bool cube = mv.geom == OVERLAP_GEOM_CUBE;
    const int d = mv.d, L = mv.L, NW = (d + 31) >> 5, W = cube ? 1 : L >> 5;
    const int n = cube ? L * L : NW;
    int *const red = reinterpret_cast<int *>(cluster_lds), *const vote = red + 8;
    unsigned *const T = reinterpret_cast<unsigned *>(cluster_lds) + 16, *const C = T + n, *const A = C + n;
    const int slot_a = sa.slot_of_chain[c], slot_b = sb.slot_of_chain[c];
    unsigned *const wa = reinterpret_cast<unsigned *>(sa.x + (int64_t)slot_a * sa.ld);
    unsigned *const wb = reinterpret_cast<unsigned *>(sb.x + (int64_t)slot_b * sb.ld);
    const unsigned mask = cube ? 0xFFFFFFFFu >> (32 - L) : 0xFFFFFFFFu;           // the cube: L >= 2, a shift of 0 .. 30
    const unsigned mul = (65536u + (unsigned)(cube ? L : W) - 1u) / (unsigned)(cube ? L : W);

    int k = 0;
    for (int w = tid; w < n; w += NT) {
        const unsigned av = cube ? lattice3d_load_row(wa, w, L, mask) : wa[w], bv = cube ? lattice3d_load_row(wb, w, L, mask) : wb[w];
        A[w] = av; T[w] = av ^ bv; C[w] = 0u;
        k += (int)__popc(av ^ bv);
    }
    if (tid < 3) vote[tid] = 0;
    k = cluster_block_sum<NT>(k, red, tid);
    __syncthreads();
    if (k == 0) {
        if (tid == 0) { acc.p[CLUSTER_ACC_N * mv.N + c] += 1; acc.p[CLUSTER_ACC_EMPTY * mv.N + c] += 1; }
        return;
    }

    // the seed site: word by word in chunks of 64, a wave prefix sum of the popcounts, then the bit inside the word.  Every wave does the
    // same search on the same words and arrives at the same answer: nothing to hand over
    const uint64_t u = mix64(mv.stream + ((uint64_t)c + 1ull) * CLUSTER_GAMMA);
    const int j = (int)(((u >> 32) * (uint64_t)k) >> 32);                          // 0 .. k - 1
    int seed_w = -1, run = 0;
    unsigned seed_bit = 0u;
    for (int base = 0; base < n; base += 64) {
        const unsigned v = base + lane < n ? T[base + lane] : 0u;
        const int pc = (int)__popc(v);
        int incl = pc;
        for (int s = 1; s < 64; s <<= 1) { const int o = __shfl_up(incl, s, 64); incl += lane >= s ? o : 0; }
        const int total = __shfl(incl, 63, 64);
        if (j < run + total) {
            const int before = run + incl - pc;                                    // set bits ahead of this lane's word
            const int src = __ffsll((unsigned long long)__ballot(before <= j && j < before + pc)) - 1;      // true in exactly one lane
            unsigned vv = (unsigned)__shfl((int)v, src, 64);                       // that lane's word and rank, uniform from here on
            const int skip = j - __shfl(before, src, 64);                          // 0 .. 31 lower set bits to pass over
            for (int i = 0; i < 31 && i < skip; ++i) vv &= vv - 1u;
            seed_w = base + src;
            seed_bit = vv & (0u - vv);
            break;
        }
        run += total;
    }
    if (seed_w < 0) return;                                                        // j < k: not reached
    if (tid == 0) C[seed_w] = seed_bit;
    __syncthreads();

    // the component: C <- C | (neighbours(C) & t) until a pass adds nothing.  The operator is monotone and only adds bits, so a lane may
    // read a neighbour's old or new word -- the fixed point is the same -- and C is updated in place between the barriers.  Every pass but
    // the last adds a site: at most d + 1 passes, and the loop is written with that bound.  A word that is left as it was found is closed
    // along x (it is 0 or the result of an earlier fill); only pass 0 meets one that is not, the seed's.
    int passes = 0;
    for (int pass = 0, slot = 0; pass <= d; ++pass) {
        bool changed = false;
        for (int w = tid; w < n; w += NT) {
            const unsigned t = T[w];
            if (t == 0u) continue;
            const unsigned cur = C[w];
            const int i = cluster_div(w, mul), jj = w - i * (cube ? L : W);         // cube: (z, y); square: (row, word of the row)
            unsigned nb;
            if (cube) {
                nb = C[i * L + (jj == 0 ? L : jj) - 1] | C[i * L + (jj == L - 1 ? 0 : jj + 1)] | C[((i == 0 ? L : i) - 1) * L + jj] | C[(i == L - 1 ? 0 : i + 1) * L + jj];
            } else {
                nb = C[((i == 0 ? L : i) - 1) * W + jj] | C[(i == L - 1 ? 0 : i + 1) * W + jj]
                     | (C[i * W + (jj == 0 ? W : jj) - 1] >> 31) | (C[i * W + (jj == W - 1 ? 0 : jj + 1)] << 31);
            }
            const unsigned from = (cur | nb) & t;
            if (from == cur && pass != 0) continue;
            const unsigned g = cube ? cluster_fill_ring(from, t, L, mask) : cluster_fill_word(from, t);
            if (g != cur) { C[w] = g; changed = true; }
        }
        ++passes;
        // the vote: three words in turn -- this pass's is raised before the barrier and read behind it, the next pass's is cleared now (its
        // last readers, two passes back, have all passed the previous barrier)
        const int next = slot == 2 ? 0 : slot + 1;
        if (tid == 0) vote[next] = 0;
        if (__any(changed) && lane == 0) vote[slot] = 1;
        __syncthreads();
        if (vote[slot] == 0) break;
        slot = next;
    }

    // |C| and delta: every site owns its + direction bonds
    int size = 0, delta = 0;
    for (int w = tid; w < n; w += NT) {
        const unsigned cw = C[w], aw = A[w];
        const int i = cluster_div(w, mul), jj = w - i * (cube ? L : W);
        unsigned bx, xx, by, xy, bz = 0u, xz = 0u;
        if (cube) {
            const int R = L * L, ry = i * L + (jj == L - 1 ? 0 : jj + 1), rz = (i == L - 1 ? 0 : i + 1) * L + jj;
            bx = cw ^ (((cw >> 1) | (cw << (L - 1))) & mask); xx = aw ^ (((aw >> 1) | (aw << (L - 1))) & mask) ^ mv.jw[w];
            by = cw ^ C[ry]; xy = aw ^ A[ry] ^ mv.jw[R + w];
            bz = cw ^ C[rz]; xz = aw ^ A[rz] ^ mv.jw[2 * R + w];
        } else {
            const int nx = i * W + (jj == W - 1 ? 0 : jj + 1), dn = (i == L - 1 ? 0 : i + 1) * W + jj;
            bx = cw ^ ((cw >> 1) | (C[nx] << 31)); xx = aw ^ ((aw >> 1) | (A[nx] << 31)) ^ (mv.jw ? mv.jw[w] : 0u);
            by = cw ^ C[dn]; xy = aw ^ A[dn] ^ (mv.jw ? mv.jw[NW + w] : 0u);
        }
        size += (int)__popc(cw);
        delta += 4 * ((int)__popc(bx & xx) + (int)__popc(by & xy) + (int)__popc(bz & xz)) - 2 * ((int)__popc(bx) + (int)__popc(by) + (int)__popc(bz));
    }
    size = cluster_block_sum<NT>(size, red, tid);
    delta = cluster_block_sum<NT>(delta, red, tid);

    // the flip, word by word in both engines' rows.  The cube's HBM word w is the bits [32 w, 32 w + 32), assembled from the rows that
    // overlap it (the inverse of the load, as in k_explore_checkerboard3d); C holds no bit at or beyond d, so those bits stay 0
    for (int w = tid; w < NW; w += NT) {
        unsigned v = 0u;
        if (cube) {
            const int first = (32 * w) / L, last = min((32 * w + 31) / L, L * L - 1);
            for (int r = first; r <= last; ++r) {
                const int o = r * L - 32 * w;                                      // -L < o < 32
                v |= o >= 0 ? C[r] << o : C[r] >> -o;
            }
        } else {
            v = C[w];
        }
        if (v != 0u) { wa[w] ^= v; wb[w] ^= v; }
    }
    if (tid == 0) {
        sa.suff[slot_a] = sa.suff[slot_a] + (double)delta;
        sb.suff[slot_b] = sb.suff[slot_b] - (double)delta;
        int64_t *const p = acc.p + c;
        p[CLUSTER_ACC_N * mv.N] += 1;
        p[CLUSTER_ACC_SIZE * mv.N] += size;
        p[CLUSTER_ACC_K * mv.N] += k;
        p[CLUSTER_ACC_ABS_DS * mv.N] += delta < 0 ? -delta : delta;
        p[CLUSTER_ACC_PASSES * mv.N] += passes;
    }
}

int cluster_launch(hipStream_t stream, const ClusterSide &a, const ClusterSide &b, const ClusterMove &mv, const ClusterAcc &acc) {
    const int d = mv.d, L = mv.L;
    if (d < 1 || d > OVERLAP_MAX_DIM || mv.N < 1) return 1;
    if (mv.geom == OVERLAP_GEOM_CUBE ? (L < 2 || L > 32 || L % 2 != 0 || L * L * L != d || !mv.jw) : mv.geom == OVERLAP_GEOM_SQUARE ? (L < 32 || L % 32 != 0 || L * L != d) : true) return 1;
    hipLaunchKernelGGL(k_cluster_move, dim3((unsigned)mv.N), dim3(PTE_CLUSTER_THREADS), cluster_lds_bytes(d, mv.geom, L), stream, a, b, mv, acc);
    return 0;
}

}  // namespace pte
