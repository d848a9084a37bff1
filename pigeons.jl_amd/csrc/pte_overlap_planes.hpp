// pte_overlap_planes.hpp -- the plane autocorrelation of the overlap field of a lattice pair: what the wave-vector-dependent
// spin-glass susceptibility chi_SG(k) along the lattice axes and the correlation length xi_L are computed from on the host.
// For chain c: t = a xor b exactly as k_overlap forms it (pte_overlap.hpp).  With M = d / L sites per plane (2-D: per line), for every axis
// and every coordinate p = 0 .. L - 1
//   P_axis[p] = the set bits of t among the M sites whose coordinate along the axis is p        Q_axis[p] = M - 2 P_axis[p] = sum of q_i
//   C_axis(r) = sum_p Q_axis[p] Q_axis[(p + r) mod L],  r = 0 .. L - 1                           C(r) = C(L - r);  |C| <= L M^2 <= 2^25
//   k_overlap_planes   one wave per chain: t and the plane counts in LDS, lane o owns the output (axis, r <= L / 2) and its mirror
// One wave owns a chain and the launches of a stream are ordered: the global accumulators take plain loads and stores, no atomics.  The
// plane counts are gathered with LDS atomics: all sums are integers, so their order changes no result.
#pragma once
#include "pte_lattice3d_params.hpp"
#include "pte_overlap_planes_params.hpp"

namespace pte {

// The count along axis 0 is a vertical one: bit p over all rows.  A lane keeps it bit-sliced over the rows it holds -- plane i of cs is bit
// i of 32 counters, one per bit position -- and a row word is added to all 32 at once by a ripple of half adders (carry-save): 3 operations
// per plane and row instead of one pass per bit.  Six planes count to 63; a lane holds at most 32 rows (planes_launch)
constexpr int PLANES_CS = 6;

__device__ __forceinline__ void planes_cs_add(unsigned (&cs)[PLANES_CS], unsigned v) {
#pragma unroll
    for (int i = 0; i < PLANES_CS; ++i) {
        const unsigned carry = cs[i] & v;
        cs[i] ^= v;
        v = carry;
    }
}

__device__ __forceinline__ int planes_cs_get(const unsigned (&cs)[PLANES_CS], int p) {
    int n = 0;
#pragma unroll
    for (int i = 0; i < PLANES_CS; ++i) n |= (int)((cs[i] >> p) & 1u) << i;
    return n;
}

// Dynamic LDS: t, ceil(d / 32) words, then cnt, n_axes L words: cnt[axis L + p] holds P_axis[p], then Q_axis[p] in its place.
//   cube    lane l takes the rows l, l + 64, ... (at most 16) with lattice3d_load_row under the L-bit mask, rows 0 .. L^2 - 1 only: no bit at
//           or beyond d is counted.  The row's popcount goes to y and to z, the row itself into the lane's vertical counters
//   square  L % 32 == 0, W = L / 32 words per row, no padding bit.  The first G W lanes, G = 64 / W, take the words l, l + G W, ...: lane l
//           stays in word column l % W of the rows l / W, l / W + G, ... (at most ceil(L / G) <= 32), so its vertical counters are those of
//           the columns 32 (l % W) .. + 31.  W = 1, 2, 4, 8: all 64 lanes; W = 3: 63.  The word's popcount goes to its row
// The vertical counters are handed to cnt bit position by bit position, lane l starting at position l & 31: the lanes of one instruction
// are spread over all the positions.
__global__ __launch_bounds__(64) void k_overlap_planes(const double *xa, int64_t lda, const int32_t *slot_a, const double *xb, int64_t ldb, const int32_t *slot_b,
                                                       int d, int N, int geom, int L, int64_t *plane_n, int64_t *plane_corr) {
    extern __shared__ unsigned t[];
    const int lane = lane_id();
    const int c = blockIdx.x;
    if (c >= N) return;
    const unsigned *a = reinterpret_cast<const unsigned *>(xa + (int64_t)slot_a[c] * lda);
    const unsigned *b = reinterpret_cast<const unsigned *>(xb + (int64_t)slot_b[c] * ldb);
    const int NW = (d + 31) >> 5;
    const int n_axes = planes_axes(geom);
    int *cnt = reinterpret_cast<int *>(t + NW);
    for (int w = lane; w < NW; w += 64) t[w] = a[w] ^ b[w];
    for (int i = lane; i < n_axes * L; i += 64) cnt[i] = 0;
    __syncthreads();
    unsigned cs[PLANES_CS] = {0u, 0u, 0u, 0u, 0u, 0u};
    int col0 = 0, n_bits = 0;                                                           // the lane's counters are the columns col0 .. col0 + n_bits - 1
    if (geom == OVERLAP_GEOM_CUBE) {
        const int R = L * L;
        const unsigned mask = 0xFFFFFFFFu >> (32 - L);                                  // L >= 2: a shift of 0 .. 30
        n_bits = L;
        for (int r = lane; r < R; r += 64) {
            const int z = r / L, y = r - z * L;
            const unsigned row = lattice3d_load_row(t, r, L, mask);
            const int pc = (int)__popc(row);
            atomicAdd(&cnt[L + y], pc);
            atomicAdd(&cnt[2 * L + z], pc);
            planes_cs_add(cs, row);
        }
    } else {
        const int W = L >> 5, stride = (64 / W) * W;
        if (lane < stride) {
            col0 = (lane % W) << 5;
            n_bits = 32;
            for (int w = lane; w < NW; w += stride) {
                const unsigned v = t[w];
                atomicAdd(&cnt[L + w / W], (int)__popc(v));
                planes_cs_add(cs, v);
            }
        }
    }
    for (int j = 0; j < 32; ++j) {
        const int p = (lane + j) & 31;
        const int n = planes_cs_get(cs, p);
        if (p < n_bits && n != 0) atomicAdd(&cnt[col0 + p], n);
    }
    __syncthreads();
    const int M = d / L;
    for (int i = lane; i < n_axes * L; i += 64) cnt[i] = M - 2 * cnt[i];
    __syncthreads();
    // C(r) = C(L - r): the outputs are r = 0 .. L / 2 of every axis (L is even), n_axes L (L / 2 + 1) multiply-adds over the wave
    const int H = L >> 1;
    int64_t *corr = plane_corr + (int64_t)c * n_axes * L;
    for (int o = lane; o < n_axes * (H + 1); o += 64) {
        const int axis = o / (H + 1), r = o - axis * (H + 1);
        const int *q = cnt + axis * L;
        int s = 0;
        for (int p = 0, p2 = r; p < L; ++p) {
            s += q[p] * q[p2];
            p2 = p2 + 1 == L ? 0 : p2 + 1;
        }
        corr[axis * L + r] += s;
        if (r != 0 && r != L - r) corr[axis * L + L - r] += s;
    }
    if (lane == 0) plane_n[c] += 1;
}

int planes_launch(hipStream_t stream, const OverlapSide &a, const OverlapSide &b, int d, int N, int geom, int L, const PlanesAcc &acc) {
    if (d < 1 || d > OVERLAP_MAX_DIM || N < 1) return 1;
    // the shapes of overlap_launch that have a geometry; d <= OVERLAP_MAX_DIM bounds the square at L <= 256: W <= 8, at most 32 rows per lane
    if (geom == OVERLAP_GEOM_CUBE ? (L < 2 || L > 32 || (L & 1) || L * L * L != d) : geom == OVERLAP_GEOM_SQUARE ? (L < 32 || L % 32 != 0 || L * L != d) : true) return 1;
    hipLaunchKernelGGL(k_overlap_planes, dim3((unsigned)N), dim3(64), planes_lds_bytes(d, geom, L), stream, a.x, a.ld, a.slot_of_chain, b.x, b.ld,
                       b.slot_of_chain, d, N, geom, L, acc.n, acc.corr);
    return 0;
}

}  // namespace pte
