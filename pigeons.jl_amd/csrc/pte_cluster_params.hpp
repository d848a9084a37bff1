// pte_cluster_params.hpp -- what the launcher (pte.hip) and Houdayer's cluster move between the two copies of a lattice pair
// (pte_cluster.hpp) share: the two engines as the kernel writes them, the accumulators, the draw, and the entry point through which the
// kernel is launched.  The kernel is a translation unit of its own, pte_cluster.hip (pte_automala_params.hpp says why).  DESIGN 4.21.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "pte_overlap_params.hpp"

namespace pte {

// threads of the workgroup that owns a chain: 256 = four waves (shipped), 64 = one wave (the A/B build of DESIGN 4.21's table)
#ifndef PTE_CLUSTER_THREADS
#define PTE_CLUSTER_THREADS 256
#endif

// one engine as the kernel reads and writes it: the bit-packed rows, their stride in 8-byte words, the chain -> slot map at the time of the
// launch and the swap statistic of every slot (the bond-weighted pair sum, an integer held in a double)
struct ClusterSide { double *x; int64_t ld; const int32_t *slot_of_chain; double *suff; };

// per chain, all int64, zeroed at every pte_overlap_reduce: n moves made, empty moves with k = 0, size_sum += |C|, k_sum += k,
// abs_ds_sum += |delta|, passes_sum += passes of the fixed point (the measurement's, not part of the specification).  One allocation, the
// six arrays of N words one behind the other in this order: the kernel is handed one pointer, not six
struct ClusterAcc { int64_t *p; };
enum { CLUSTER_ACC_N = 0, CLUSTER_ACC_EMPTY, CLUSTER_ACC_SIZE, CLUSTER_ACC_K, CLUSTER_ACC_ABS_DS, CLUSTER_ACC_PASSES, CLUSTER_ACC_ARRAYS };

// one launch: chain c takes part iff beta[c] >= min_beta and draws u = mix64(seed + (m N + c + 1) gamma), gamma = CLUSTER_GAMMA, from a
// stream of its own (no engine's RNG words are read); the launcher hands over stream = seed + m N gamma (mod 2^64), the part all chains
// share.  jw = the bond planes, a set bit where the bond is -1: the cube's three planes of L * L row words (SpinGlass3DParams::jw), the
// square's two planes of L * L / 32 words (SpinGlassParams::jw), null for the Ising family (J = 0 bits)
struct ClusterMove {
    int d, N, geom, L;
    const unsigned *jw;
    const double *beta;
    double min_beta;
    uint64_t stream;
};

constexpr uint64_t CLUSTER_GAMMA = 0x9E3779B97F4A7C15ULL;

// the dynamic LDS of one workgroup: 16 words of scratch, then t, C and a, one word per row (cube) or per 32 sites (square) each -- 64 bytes
// + 24 KiB at the largest d the launcher admits (OVERLAP_MAX_DIM)
constexpr size_t cluster_lds_bytes(int d, int geom, int L) { return 64 + 3 * sizeof(unsigned) * (size_t)(geom == OVERLAP_GEOM_CUBE ? L * L : (d + 31) >> 5); }

// one launch of k_cluster_move on `stream`, one workgroup per chain; 1 if (d, N, geom, L) is not a shape the kernel covers
int cluster_launch(hipStream_t stream, const ClusterSide &a, const ClusterSide &b, const ClusterMove &mv, const ClusterAcc &acc);

}  // namespace pte
