// pte_overlap_params.hpp -- what the launcher (pte.hip) and the replica-overlap kernel (pte_overlap.hpp) share: the accumulators, the lattice
// geometries the link overlap knows, and the entry point through which the kernel is launched.  The kernel is a translation unit of its own,
// pte_overlap.hip (pte_automala_params.hpp says why).  DESIGN 4.20.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pte {

// which periodic lattice the d site bits are, for the link overlap: none (the site overlap alone: 2-D lattices whose rows are not whole
// words), the L x L square with L % 32 == 0 (rows are L / 32 whole words), the L x L x L cube of pte_lattice3d.hpp (a row is L <= 32 bits)
enum { OVERLAP_GEOM_NONE = 0, OVERLAP_GEOM_SQUARE = 2, OVERLAP_GEOM_CUBE = 3 };

// one engine as the kernel reads it: the bit-packed rows, their stride in 8-byte words and the chain -> slot map at the time of the launch
struct OverlapSide { const double *x; int64_t ld; const int32_t *slot_of_chain; };

// per chain, all int64, zeroed at every pte_overlap_reduce: hist [N][d + 1] (bin k = popcount(a xor b)), n [N] records, link_n [N] records
// with a link overlap, link_sum / link_sum2 [N] = sum of kl and of kl^2 (kl <= 3 d <= 98304: kl^2 < 2^34)
struct OverlapAcc { int64_t *hist, *n, *link_n, *link_sum, *link_sum2; };

// the largest d the kernel holds: a xor b of one chain is kept in LDS, d / 32 words = 8 KiB here
constexpr int OVERLAP_MAX_DIM = 65536;

// one launch of k_overlap on `stream`, one workgroup of one wave per chain; 1 if (d, N, geom, L) is not a shape the kernel covers
int overlap_launch(hipStream_t stream, const OverlapSide &a, const OverlapSide &b, int d, int N, int geom, int L, const OverlapAcc &acc);

}  // namespace pte
