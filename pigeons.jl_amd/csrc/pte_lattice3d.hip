// pte_lattice3d.hip -- the eleventh translation unit of libpte.so: the 3-D spin-glass kernels (pte_lattice3d.hpp) behind lattice3d_launch.
// Compiled with the flags of pte_spinglass.hip (-O2, -amdgpu-sched-strategy=max-ilp); a unit of its own keeps the generated code of the
// shipped kernels unchanged.
#define PTE_TU_LANGEVIN 1          // pte_kernels.hpp, pte_ising.hpp: leave the engine's non-template kernels to pte.hip
#include "pte_lattice3d.hpp"
