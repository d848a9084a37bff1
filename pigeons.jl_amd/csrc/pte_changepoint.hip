// pte_changepoint.hip -- the eighth translation unit of libpte.so: the change-point kernels (pte_changepoint.hpp) behind changepoint_launch.
// Compiled with the flags of pte_langevin.hip (the default scheduler); a unit of its own keeps the generated code of the shipped kernels
// unchanged -- interprocedural attribute inference over callees the units share could otherwise move it.
#define PTE_TU_LANGEVIN 1          // pte_kernels.hpp: leave the engine's non-template kernels to pte.hip
#include "pte_changepoint.hpp"
