// pte_cluster.hip -- the thirteenth translation unit of libpte.so: Houdayer's cluster move (pte_cluster.hpp) behind cluster_launch.
// Compiled with the flags of pte_overlap.hip (-O2, -amdgpu-sched-strategy=max-ilp); a unit of its own keeps the generated code of the
// shipped kernels unchanged.  The kernel's one draw is its own mix64 word: the unit needs no RNG-policy setter (it is not in PTE_KERNEL_UNITS).
#define PTE_TU_LANGEVIN 1          // pte_kernels.hpp, pte_ising.hpp: leave the engine's non-template kernels to pte.hip
#include "pte_cluster.hpp"
