// pte_mixture_model.hip -- the sixth translation unit of libpte.so: the mixture-model-posterior kernels (pte_mixture_model.hpp) behind
// mixture_model_launch.  Compiled with the flags of pte_langevin.hip (the default scheduler); a unit of its own keeps the generated code of
// the shipped kernels unchanged -- interprocedural attribute inference over callees the units share could otherwise move it.
#define PTE_TU_LANGEVIN 1          // pte_kernels.hpp: leave the engine's non-template kernels to pte.hip
#include "pte_mixture_model.hpp"
