// pte_spinglass.hip -- the ninth translation unit of libpte.so: the spin-glass kernels (pte_spinglass.hpp) behind spinglass_launch.
// Compiled with the flags of pte.hip, the unit of the Ising kernels they are made from (-O2, -amdgpu-sched-strategy=max-ilp); a unit of its
// own keeps the generated code of the shipped kernels unchanged.
#define PTE_TU_LANGEVIN 1          // pte_kernels.hpp, pte_ising.hpp: leave the engine's non-template kernels to pte.hip
#include "pte_spinglass.hpp"
