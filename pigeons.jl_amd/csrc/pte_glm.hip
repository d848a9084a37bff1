// pte_glm.hip -- the fifth translation unit of libpte.so: the Bayesian-GLM kernels (pte_glm.hpp) behind glm_launch, and the hierarchical
// normal-means kernels (pte_hier.hpp) behind hier_launch, the latent-AR(1) kernels (pte_ar1.hpp) behind ar1_launch and the dense-precision
// Gaussian kernels (pte_dense.hpp) behind dense_launch -- the data-reading families on automala_body; they share this unit's RNG-policy word.
// Compiled with the flags of pte_langevin.hip (the default scheduler); a unit of its own keeps the generated code of the shipped kernels
// unchanged -- interprocedural attribute inference over callees the units share could otherwise move it.
#define PTE_TU_LANGEVIN 1          // pte_kernels.hpp: leave the engine's non-template kernels to pte.hip
#include "pte_glm.hpp"
#include "pte_hier.hpp"
#include "pte_ar1.hpp"
#include "pte_dense.hpp"
