// pte_overlap_planes.hip -- the fourteenth translation unit of libpte.so: the plane-correlation kernel of a lattice pair
// (pte_overlap_planes.hpp) behind planes_launch.  Compiled with the flags of pte_overlap.hip (-O2, -amdgpu-sched-strategy=max-ilp); a unit of
// its own keeps the generated code of the shipped kernels, k_overlap among them, unchanged.  The kernel draws no random number: the unit
// needs no RNG-policy setter (it is not in PTE_KERNEL_UNITS).
#define PTE_TU_LANGEVIN 1          // pte_kernels.hpp, pte_ising.hpp: leave the engine's non-template kernels to pte.hip
#include "pte_overlap_planes.hpp"
