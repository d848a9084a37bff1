// pte_overlap.hpp -- the replica overlap between two engines that hold the same lattice model at the same temperatures.
// For chain c: a, b = the bit strings of the slots that hold chain c in engine A and in engine B (the HBM bit-packed lattice of
// pte_ising.hpp / pte_lattice3d.hpp: site s -> bit s & 31 of word s >> 5, bits at and beyond d zero), t = a xor b.
//   site overlap   k  = popcount(t)                                  q   = 1 - 2 k / d
//   link overlap   kl = sum_dir popcount(t xor shift_dir(t))         q_l = 1 - 2 kl / n_links
// shift_dir is the periodic shift by one site along a lattice direction: bit i of t xor shift(t) is set where s_i s_j differs between the two
// copies, j the +dir neighbour of i -- every site owns its +dir bond, so at L = 2 the two bonds between the same pair of sites are two terms,
// and the bonds themselves cancel (J^2 = 1): the kernel never reads them.
//   k_overlap      one wave per chain: t to LDS, k and kl by wave reductions, lane 0 adds to its chain's bins
// One wave owns a chain and the launches of a stream are ordered: plain loads and stores, no atomics.
#pragma once
#include "pte_lattice3d_params.hpp"
#include "pte_overlap_params.hpp"

namespace pte {

// Dynamic LDS: t, ceil(d / 32) words (8 KiB at d = 65536).  The words are dealt lane-strided; the link term reads the LDS copy:
//   cube    rows of L bits taken with lattice3d_load_row (masked to L bits, rows 0 .. L^2 - 1 only: no bit at or beyond d enters); +x is the
//           rotate inside the row, +y and +z are the neighbouring rows
//   square  L % 32 == 0, so d % 32 == 0 (no padding bit in any word) and row i is the words [i W, (i + 1) W), W = L / 32; +x is the funnel
//           shift by one bit across the row's words, wrapping to the row's own first word; +y is the word W further on, wrapping to row 0
__global__ __launch_bounds__(64) void k_overlap(const double *xa, int64_t lda, const int32_t *slot_a, const double *xb, int64_t ldb, const int32_t *slot_b,
                                                int d, int N, int geom, int L, OverlapAcc acc) {
    extern __shared__ unsigned t[];
    const int lane = lane_id();
    const int c = blockIdx.x;
    if (c >= N) return;
    const unsigned *a = reinterpret_cast<const unsigned *>(xa + (int64_t)slot_a[c] * lda);
    const unsigned *b = reinterpret_cast<const unsigned *>(xb + (int64_t)slot_b[c] * ldb);
    const int NW = (d + 31) >> 5;
    int k = 0;
    for (int w = lane; w < NW; w += 64) {
        const unsigned v = a[w] ^ b[w];
        t[w] = v;
        k += (int)__popc(v);
    }
    for (int m = 1; m < 64; m <<= 1) k += __shfl_xor(k, m, 64);
    __syncthreads();
    int kl = 0;
    if (geom == OVERLAP_GEOM_CUBE) {
        const int R = L * L;
        const unsigned mask = 0xFFFFFFFFu >> (32 - L);                              // L >= 2: a shift of 0 .. 30
        for (int r = lane; r < R; r += 64) {
            const int z = r / L, y = r - z * L;
            const unsigned cur = lattice3d_load_row(t, r, L, mask), rt = ((cur >> 1) | (cur << (L - 1))) & mask;
            const unsigned yp = lattice3d_load_row(t, z * L + (y == L - 1 ? 0 : y + 1), L, mask);
            const unsigned zp = lattice3d_load_row(t, (z == L - 1 ? 0 : z + 1) * L + y, L, mask);
            kl += (int)__popc(cur ^ rt) + (int)__popc(cur ^ yp) + (int)__popc(cur ^ zp);
        }
    } else if (geom == OVERLAP_GEOM_SQUARE) {
        const int W = L >> 5;
        for (int w = lane; w < NW; w += 64) {
            const int i = w / W, j = w - i * W;
            const unsigned cur = t[w], nx = t[i * W + (j == W - 1 ? 0 : j + 1)], dn = t[(i == L - 1 ? 0 : i + 1) * W + j];
            kl += (int)__popc(cur ^ ((cur >> 1) | (nx << 31))) + (int)__popc(cur ^ dn);
        }
    }
    for (int m = 1; m < 64; m <<= 1) kl += __shfl_xor(kl, m, 64);
    if (lane == 0) {
        acc.hist[(int64_t)c * (d + 1) + k] += 1;
        acc.n[c] += 1;
        if (geom != OVERLAP_GEOM_NONE) {
            acc.link_n[c] += 1;
            acc.link_sum[c] += kl;
            acc.link_sum2[c] += (int64_t)kl * kl;
        }
    }
}

int overlap_launch(hipStream_t stream, const OverlapSide &a, const OverlapSide &b, int d, int N, int geom, int L, const OverlapAcc &acc) {
    if (d < 1 || d > OVERLAP_MAX_DIM || N < 1) return 1;
    if (geom == OVERLAP_GEOM_CUBE ? (L < 2 || L > 32 || L * L * L != d) : geom == OVERLAP_GEOM_SQUARE ? (L < 32 || L % 32 != 0 || L * L != d) : geom != OVERLAP_GEOM_NONE) return 1;
    hipLaunchKernelGGL(k_overlap, dim3((unsigned)N), dim3(64), sizeof(unsigned) * (size_t)((d + 31) >> 5), stream, a.x, a.ld, a.slot_of_chain, b.x, b.ld,
                       b.slot_of_chain, d, N, geom, L, acc);
    return 0;
}

}  // namespace pte
