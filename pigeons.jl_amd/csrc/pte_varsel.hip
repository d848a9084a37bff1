// pte_varsel.hip -- the seventh translation unit of libpte.so: the variable-selection kernels (pte_varsel.hpp) behind varsel_launch.
// Compiled with the flags of pte_langevin.hip (the default scheduler); a unit of its own keeps the generated code of the shipped kernels
// unchanged -- interprocedural attribute inference over callees the units share could otherwise move it.
#define PTE_TU_LANGEVIN 1          // pte_kernels.hpp: leave the engine's non-template kernels to pte.hip
#include "pte_varsel.hpp"
