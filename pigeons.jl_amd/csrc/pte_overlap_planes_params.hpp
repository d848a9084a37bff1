// pte_overlap_planes_params.hpp -- what the launcher (pte.hip) and the plane-correlation kernel of a lattice pair (pte_overlap_planes.hpp)
// share: the accumulators and the entry point through which the kernel is launched.  The kernel is a translation unit of its own,
// pte_overlap_planes.hip (pte_automala_params.hpp says why).  DESIGN 4.22.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "pte_overlap_params.hpp"

namespace pte {

// the lattice axes a geometry has: 3 on the cube, 2 on the square, 0 where the kernel does not run.  Axis 0 is the fastest site index (the
// bit inside a row word of the cube; the column j of the square), axis 1 the next (y; the row i), axis 2 the cube's z
constexpr int planes_axes(int geom) { return geom == OVERLAP_GEOM_CUBE ? 3 : geom == OVERLAP_GEOM_SQUARE ? 2 : 0; }

// per chain, int64, zeroed at every pte_overlap_reduce: n [N] records taken while the feature was on, corr [N][n_axes][L] += C_axis(r),
// C_axis(r) = sum_p Q[p] Q[(p + r) mod L], Q[p] = the sum of q_i = s_i^a s_i^b over the plane (2-D: the line) at coordinate p of that axis.
// One record has |C| <= L M^2 = d M, M = d / L: 2^25 on the 32^3 cube, 2^24 at 256 x 256 -- an int32 in the kernel
struct PlanesAcc { int64_t *n, *corr; };

// the dynamic LDS of one workgroup: t, ceil(d / 32) words, then the plane counts, n_axes L words -- 4480 B on the 32^3 cube, 10 KiB at
// 256 x 256, the largest d the launcher admits (OVERLAP_MAX_DIM)
constexpr size_t planes_lds_bytes(int d, int geom, int L) { return sizeof(unsigned) * (size_t)((d + 31) >> 5) + sizeof(int) * (size_t)(planes_axes(geom) * L); }

// one launch of k_overlap_planes on `stream`, one workgroup of one wave per chain; 1 if (d, N, geom, L) is not a shape the kernel covers
int planes_launch(hipStream_t stream, const OverlapSide &a, const OverlapSide &b, int d, int N, int geom, int L, const PlanesAcc &acc);

}  // namespace pte
