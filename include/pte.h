/* pte.h -- C ABI of the MI355X-native parallel-tempering engine ("pte").
 *
 * Drop-in boundary for the explore-then-swap hot path of Pigeons.jl v0.4.10.
 * The reference has NO C ABI on this path (it is Julia multiple dispatch); the
 * entry points below are what a Julia `ccall` glue (INTEGRATION.md,
 * pigeons.jl_amd/julia/PigeonsMI355X.jl) binds at the three dispatch hooks that
 * bracket the hot path, plus construction / adaptation / checkpoint hooks:
 *
 *   create_replicas(inputs, shared, source)      src/replicas/replicas.jl:65-98   -> pte_create
 *   explore!(pt, explorer, ::Val)                src/pt/pigeons.jl:82-132         -> pte_explore
 *   swap!(pair_swapper, replicas, swap_graph)    src/swap/swap.jl:6-39,106-126    -> pte_swap
 *   `while next_scan!(pt)` loop                  src/pt/pigeons.jl:49-52          -> pte_run_scans (fused)
 *   reduce_recorders!(pt, replicas)              src/recorders/recorders.jl:88-120 -> pte_reduce + pte_get_*
 *   adapt_tempering / discretize                 src/tempering/NonReversiblePT.jl:46-66 -> pte_set_schedule
 *   adapt_explorer(::AutoMALA, ...)              src/explorers/AutoMALA.jl:70-79   -> pte_set_explorer_adaptation
 *   checkpoint (Replica fields)                  src/pt/checkpoint.jl:110-145     -> pte_get_state / pte_set_state
 *
 * Conventions (precedent: the reference's only FFI, ext/PigeonsBridgeStanExt/interface.jl:118-183):
 *   - every call returns int: 0 = ok, != 0 = error; message via pte_last_error().
 *   - plain pointers and sizes; caller allocates all output arrays (host memory).
 *   - the engine owns all device memory; handles are freed by pte_destroy.
 *   - all calls on one handle come from one host thread; calls are synchronous at
 *     return (results visible to the host), asynchronous internally (HIP streams).
 *   - indices are 0-based: chain 0 = reference (beta = 0), chain N-1 = target;
 *     replica r = reference `replica_index` r+1.
 *   - floating point is IEEE binary64 throughout ("f64").
 *   - there is NO CPU fallback: on a machine without a HIP device pte_create fails.
 */
#ifndef PTE_H
#define PTE_H

#include <stdint.h>
#include "pte_rng_policy.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PTE_ABI_VERSION 2

/* Device log-potential families (closed set; arbitrary Julia closures cannot run
 * on the GPU -- unsupported combinations make pte_create fail, and the caller
 * keeps the reference CPU path). */
enum {
    PTE_TARGET_MVN_SCALED_PRECISION = 0, /* toy_mvn_target: src/paths/ScaledPrecisionNormalPath.jl:5-48   */
    PTE_TARGET_TEST_SWAPPER         = 1, /* TestSwapper:    src/swap/pair_swapper.jl:100-149               */
    PTE_TARGET_FUNNEL               = 2, /* InterpolatingPath(normal ref, Neal's funnel)                   */
    PTE_TARGET_ISING                = 3, /* InterpolatingPath(Ising(0), Ising(beta)): examples/ising.jl        */
    PTE_TARGET_GAUSSIAN_MIXTURE     = 4, /* InterpolatingPath(normal ref, normalised mixture of K <= 8 diagonal Gaussians;
                                            pte_set_target_mixture): SliceSampler / AutoMALA / MALA / Compose of them, dim <= 512 */
    PTE_TARGET_BAYESIAN_GLM         = 5, /* InterpolatingPath(normal ref = the prior, prior x GLM likelihood of data X, y;
                                            pte_set_target_glm): SliceSampler / AutoMALA / MALA / Compose of them, dim <= 512 */
    PTE_TARGET_MIXTURE_MODEL        = 6, /* InterpolatingPath(normal ref = the prior, prior x likelihood of a K-component normal mixture model
                                            of data y; pte_set_target_mixture_model): theta = [mu, s, alpha], dim = 3 K, K <= 8;
                                            SliceSampler / AutoMALA / MALA / Compose of them */
    PTE_TARGET_VARIABLE_SELECTION = 7,   /* spike-and-slab regression on data X, y (pte_set_target_varsel): the state is [theta, gamma],
                                            d Float64 coefficients then d Bool indicators stored as 0.0 / 1.0, dim = 2 d, d <= 256;
                                            SliceSampler only (its Float64 and Bool coordinate methods) */
    PTE_TARGET_CHANGE_POINT = 8,         /* K Poisson change points on n counts (pte_set_target_changepoint): the state is [r, tau],
                                            K + 1 Float64 log rates then K Integer change points stored as integral doubles in 0..n,
                                            dim = 2 K + 1, K <= 63; SliceSampler only (its Float64 and Integer coordinate methods) */
    PTE_TARGET_HIERARCHICAL_NORMAL = 9,  /* InterpolatingPath(normal ref, hierarchical normal-means posterior of J group estimates;
                                            pte_set_target_hier): the state is [mu, log tau, one coordinate per group], dim = J + 2 in
                                            3..512; SliceSampler / AutoMALA / MALA / Compose of them */
    PTE_TARGET_LATENT_AR1 = 10,          /* InterpolatingPath(normal ref, posterior of a latent AR(1) state-space model of T observations;
                                            pte_set_target_ar1): the state is [mu, atanh phi, log sigma, h_0 .. h_{T-1}], dim = T + 3 in
                                            4..512; SliceSampler / AutoMALA / MALA / Compose of them */
    PTE_TARGET_DENSE_NORMAL = 11,        /* InterpolatingPath(normal ref, N(mean, precision^-1) with a dense precision matrix;
                                            pte_set_target_dense): dim in 1..512; SliceSampler / AutoMALA / MALA / Compose of them */
    PTE_TARGET_SPIN_GLASS = 12,          /* InterpolatingPath(SpinGlass(0), SpinGlass(beta)): the +-J Edwards-Anderson model, PTE_TARGET_ISING with
                                            quenched bonds (pte_set_target_spin_glass): dim = base_length^2, 2 <= base_length, dim <= 65536;
                                            target_params[0] = beta; PTE_EXPLORER_ISING_METROPOLIS or PTE_EXPLORER_CHECKERBOARD_METROPOLIS */
    PTE_TARGET_SPIN_GLASS_3D = 13        /* the same model on the base_length^3 periodic cube (pte_set_target_spin_glass_3d; DESIGN 4.19, the project's
                                            own specification): dim = base_length^3, base_length even and in 2..32 (a row of the lattice is one
                                            32-bit word); target_params[0] = beta; PTE_EXPLORER_CHECKERBOARD_METROPOLIS only, debug_kernel 0 */
};
/* PTE_TARGET_LATENT_AR1: the observation model */
enum {
    PTE_AR1_STOCHASTIC_VOLATILITY = 0,   /* y_t ~ N(0, exp(h_t))                                                                    */
    PTE_AR1_NORMAL_IDENTITY = 1          /* y_t ~ N(h_t, obs_sd^2): linear-Gaussian given (phi, sigma)                              */
};
/* PTE_TARGET_HIERARCHICAL_NORMAL: what the group coordinates are */
enum {
    PTE_HIER_CENTERED = 0,               /* x[2 + j] = theta_j ~ N(mu, tau^2)                                                       */
    PTE_HIER_NONCENTERED = 1             /* x[2 + j] = eta_j ~ N(0, 1), theta_j = mu + tau eta_j                                    */
};
/* PTE_TARGET_BAYESIAN_GLM: the likelihood of each observation */
enum {
    PTE_GLM_BERNOULLI_LOGIT = 0,         /* logistic regression: y_i in {0, 1}, l_i = y_i eta_i - softplus(eta_i)                  */
    PTE_GLM_NORMAL_IDENTITY = 1          /* linear regression with known noise sd sigma: l_i = log N(y_i; eta_i, sigma^2)          */
};
enum {
    PTE_EXPLORER_NONE     = 0,           /* `nothing` (TestSwapper)                                        */
    PTE_EXPLORER_TOY      = 1,           /* ToyExplorer:  src/explorers/ToyExplorer.jl:5-14                */
    PTE_EXPLORER_SLICE    = 2,           /* SliceSampler: src/explorers/SliceSampler.jl:8-237 -- the Float64-coordinate methods, on
                                            the scaled-precision MVN path (closed-form single-coordinate update, the fast kernels)
                                            and on the interpolated funnel path (the log potential evaluated in full per proposal,
                                            as slice_sample! does for any log_potential :105-118; dim <= 1024).  Not on the
                                            device: its Bool / Integer coordinate variants (:65-86,136-142,189) -- no device target
                                            has integer coordinates (Ising has its own explorer) -- and a GaussianReference under it;
                                            pte_create / pte_set_variational_reference refuse those, the caller keeps the CPU path */
    PTE_EXPLORER_AUTOMALA = 3,           /* AutoMALA:     src/explorers/AutoMALA.jl:29-294                 */
    PTE_EXPLORER_ISING_METROPOLIS = 4,   /* IsingMetropolis: examples/ising.jl:91-116 (n_steps in slice_n_passes) */
    PTE_EXPLORER_MALA     = 5,           /* MALA:         src/explorers/MALA.jl:19-105 (am_* fields; step size fixed) */
    PTE_EXPLORER_AAPS     = 6,           /* AAPS:         src/explorers/AAPS.jl (apogee-to-apogee path sampler; am_step_size, am_preconditioner / am_p0 / am_p1,
                                            aaps_K; step size fixed; MVN and funnel paths, dim <= 512, single explorer)      */
    PTE_EXPLORER_CHECKERBOARD_METROPOLIS = 7 /* CheckerboardMetropolis: the two-colour Metropolis sweep of the lattice targets (the project's own
                                            specification, n_steps in slice_n_passes); PTE_TARGET_ISING and PTE_TARGET_SPIN_GLASS with an even
                                            base_length, PTE_TARGET_SPIN_GLASS_3D, single explorer */
};
enum {                                   /* Inputs.record (src/pt/Inputs.jl:57-62)                         */
    PTE_RECORD_ROUND_TRIP    = 1u << 0,  /* round_trip     src/recorders/RoundTripRecorder.jl              */
    PTE_RECORD_INDEX_PROCESS = 1u << 1,  /* index_process  src/recorders/recorder.jl:81                    */
    PTE_RECORD_ONLINE        = 1u << 2,  /* online / _transformed_online (target chain mean, variance)     */
    PTE_RECORD_TRACES        = 1u << 3,  /* traces: [state; log density] of the target chain per scan (src/recorders/recorder.jl:27,39-43; src/pt/pigeons.jl:116-125) */
    PTE_RECORD_TRACES_EXTENDED = 1u << 5, /* with PTE_RECORD_TRACES: inputs.extended_traces, every chain is traced (src/pt/pigeons.jl:116) */
    PTE_RECORD_ENERGY_AC1    = 1u << 4,  /* energy_ac1: per-chain covariance of the log density before / after explore! (recorder.jl:113; pigeons.jl:134-143) */
    PTE_RECORD_REFERENCE_REDUCTION = 1u << 6 /* swap_acceptance_pr / log_sum_ratio reduced the way the reference reduces them instead of by chain-keyed sums on the
                                              * device: every replica's own Mean (mu += (x - mu) / n, src/recorders/recorders.jl:88-130 over OnlineStats) and LogSum
                                              * (src/recorders/LogSum.jl:1-24) fitted in scan order, then merged over the binary tree on the replica index
                                              * (all_reduce_deterministically, src/mpi_utils/Entangler.jl:188-251).  The device logs the two log ratios of every active pair and
                                              * scan ([max_scans_per_round][n_chains][2] doubles); pte_reduce replays the fits and merges on the host, so the adapted schedule
                                              * is the reference's to the last bit instead of to 1e-11.  Needs PTE_RECORD_INDEX_PROCESS (who held the lower chain).  A
                                              * chain-shard replays the pairs whose lower chain it owns (log and index rows are local; the tree runs over the global
                                              * replica index).  With PTE_RECORD_TRACES the online statistics are rebuilt the same way, and AutoMALA's am_factors (the
                                              * exponent of every step-size search is logged: the step size adapts on their mean) always, with its reversibility_rate (the same log).
                                              * With PTE_RECORD_ENERGY_AC1 the pair of log densities around every explore step is logged too (by a launch of its own before and
                                              * after the explorer kernels: such an engine runs the launch-per-scan loop) and energy_ac1's correlation replayed.  Off by default: the values agree to ~1e-12 either way, and a round of 1024 x 1024 chain-scans logs 16 MB. */
};

enum {                                   /* pte_config.debug_kernel: which kernel generation explores (0 = the default)   */
    PTE_KERNEL_DEFAULT          = 0,
    PTE_KERNEL_SLICE_SEQUENTIAL = 1,     /* SliceSampler: the plain sequential kernel (exact fallback of the default one)  */
    /* 2, 5, 7 (and 8 = the default named explicitly): earlier SliceSampler generations, test build libpte_test.so only    */
    PTE_KERNEL_ISING_BITS       = 101,   /* IsingMetropolis: scalar bit-packed sweep, test build only                      */
    PTE_KERNEL_ISING_BYTES      = 102,   /* IsingMetropolis: scalar byte-lattice sweep (the kernel of base_length % 32 != 0);
                                            CheckerboardMetropolis: its byte-lattice kernel k_explore_checkerboard_sites           */
    /* a FLAG, or-ed to any of the above: pte_run_scans launches explore and swap per scan (the loop of rounds 1-4) even where the whole
     * call could run as ONE kernel with pairwise swap hand-shakes (pte_scan_loop_name); for A/B runs and the parity tests of the two forms */
    PTE_KERNEL_TWO_LAUNCHES     = 0x1000,
    /* a FLAG: where the one-kernel scan loop has a form with several consecutive chains per workgroup (their pairs shake hands through
     * LDS; pte_scan_loop_name ends in "_wg"), use the form with one chain per workgroup instead; bit-identical, for A/B runs and tests */
    PTE_KERNEL_SCAN_LOOP_ONE_CHAIN = 0x2000,
    PTE_KERNEL_FLAG_BITS        = 0x3000,
    /* FAULT INJECTION, test build libpte_test.so only (pte_create of the product library refuses them): what the one-kernel scan loop does when
     * its forward-progress assumptions break (tests/test_gpu_scan_loop_progress.py).
     *   DEAD_CHAIN      the wave of chain 7 leaves the loop silently before its third swap of every call: its partner's hand-shake times out after
     *                   3 s, every other wave sees the error word and leaves, pte_run_scans fails, the engine is poisoned (pte_scan_loop_stats)
     *   LATE_WORKGROUP  workgroup 3 of every scan-loop launch reaches the residency gate 80 ms late (as if the device had no room for it): the
     *                   launch aborts with nothing written and the call runs as explore + swap launches -- same results, no error */
    PTE_KERNEL_TEST_DEAD_CHAIN     = 0x4000,
    PTE_KERNEL_TEST_LATE_WORKGROUP = 0x8000,
    /* A/B reference, test build only: AutoMALA / MALA at 512 < dim <= 1024 on the ONE-wave kernel with sixteen blocks per lane (rounds 1-5; it
     * spills 250-300 VGPRs) instead of the four-waves-per-replica kernel k_explore_langevin_mw (round 6) -- bit-identical, tests/test_gpu_langevin_mw.py */
    PTE_KERNEL_TEST_LANGEVIN_ONE_WAVE = 0x10000,
    PTE_KERNEL_TEST_BITS        = 0x1C000
};

/* Mirrors the fields of `Inputs` (src/pt/Inputs.jl:9-102) and of the explorer
 * structs that the hot path reads. */
typedef struct pte_config {
    uint32_t struct_size;        /* = sizeof(pte_config); checked by pte_create                            */
    uint32_t abi_version;        /* = PTE_ABI_VERSION                                                      */
    int32_t  device;             /* HIP device ordinal                                                     */
    int32_t  target;             /* PTE_TARGET_*                                                           */
    int32_t  explorer;           /* PTE_EXPLORER_*                                                         */
    uint32_t record_flags;       /* PTE_RECORD_*                                                           */
    int64_t  n_chains;           /* Inputs.n_chains (global N)                                             */
    int64_t  dim;                /* state dimension d                                                      */
    uint64_t seed;               /* Inputs.seed                                                            */
    int64_t  max_scans_per_round;/* capacity of the index-process buffer, 2^n_rounds                       */
    double   target_params[4];   /* MVN: {precision0, precision1}; TestSwapper: {accept pr};
                                    FUNNEL: {reference precision}; ISING: {beta}, dim = base_length^2; across the ABI
                                    (pte_get_state / pte_set_state / traces / online) a state is 0/1 spins as f64,
                                    row-major matrix[i,j] -> state[i*L + j]; in HBM and in boundary messages the
                                    lattice is bit-packed (8 KiB at base_length 256)                               */
    /* SliceSampler fields (SliceSampler.jl:8-20) */
    double   slice_w;
    int32_t  slice_p;
    int32_t  slice_n_passes;
    int32_t  slice_max_iter;
    /* AutoMALA fields (AutoMALA.jl:29-68) */
    int32_t  am_base_n_refresh;
    double   am_exponent_n_refresh;
    double   am_step_size;
    double   am_p0, am_p1;       /* MixDiagonalPreconditioner(p0, p1), Preconditioner.jl:43-52             */
    int32_t  am_preconditioner;  /* 0 identity, 1 diagonal, 2 mix-diagonal                                 */
    /* chain sharding: this engine owns chains [rank*N/world, (rank+1)*N/world)                           */
    int32_t  rank;
    int32_t  world_size;
    int32_t  explorer2;          /* Compose(explorer, explorer2), src/explorers/Compose.jl:5-19; PTE_EXPLORER_NONE = single explorer */
    /* StabilizedPT with inputs.variational == nothing (src/tempering/StabilizedPT.jl:37-51, src/swap/VariationalDEO.jl):
     * n_chains fixed-leg chains + n_chains_variational variational-leg chains, N = their sum (Inputs.jl:128); global
     * chain order = variational leg reference -> target, then the fixed leg target -> reference; references at both
     * ends, the two targets in the middle.  pte_set_schedule takes the N per-chain betas in that order
     * (concatenate_log_potentials, StabilizedPT.jl:67-69).  0 = one leg (NonReversiblePT).  Single engine only. */
    int64_t  n_chains_variational;
    /* Debug / bisecting: PTE_KERNEL_*.  The kernel is chosen by this field only -- the library never reads the
     * environment -- and pte_create fails on a value this build does not contain.  pte_kernel_name reports the choice. */
    int32_t  debug_kernel;
    int32_t  aaps_K;             /* AAPS: K, the number of segments besides the current one (AAPS.jl; default 5, 0..64)      */
} pte_config;

typedef struct pte_engine pte_engine;

/* Fill `cfg` with the reference defaults (Inputs.jl:14-20, SliceSampler.jl:8-20, AutoMALA.jl:29-68). */
int pte_default_config(pte_config *cfg);

/* create_replicas: split RNG streams, initial states, chain = replica index, equally spaced schedule. */
int pte_create(const pte_config *cfg, pte_engine **out);
int pte_destroy(pte_engine *h);
const char *pte_last_error(const pte_engine *h);   /* h may be NULL: error of the last failed pte_create */

/* Schedule.grids (src/schedules/Schedule.jl) -> log_potentials along the ladder (discretize). */
int pte_set_schedule(pte_engine *h, const double *betas, int64_t n_chains);
int pte_get_schedule(const pte_engine *h, double *betas);

/* adapt_explorer(::AutoMALA): new step size and estimated_target_std_deviations (NULL = nothing). */
int pte_set_explorer_adaptation(pte_engine *h, double step_size, const double *target_std, int64_t dim);

/* One explore! over all local replicas for scan index `scan` (1-based within the round,
 * src/pt/Iterators.jl:37-47; AutoMALA skips the MH step when scan == 1). */
int pte_explore(pte_engine *h, int64_t scan);
/* One communicate!: DEO graph parity = iseven(scan) (src/swap/DEO.jl:12). */
int pte_swap(pte_engine *h, int64_t scan);
/* The fused scan loop: for s = first_scan .. first_scan+n_scans-1: explore!(s); communicate!(s).
 * On a chain-sharded engine (world_size > 1) this needs pte_comm_init and is collective over the ranks. */
int pte_run_scans(pte_engine *h, int64_t first_scan, int64_t n_scans);

/* reduce_recorders!: snapshot the round's accumulators to the host and reset them on the
 * device (incl. the round-trip state machines, RoundTripRecorder.jl:30-34). */
int pte_reduce(pte_engine *h);

/* Reduced recorders of the last pte_reduce. Array lengths in brackets (world_size == 1; a sharded
 * engine returns its local slice: pairs keyed by a local lower chain, chains [c0, c0+K)). */
int pte_get_swap_acceptance(const pte_engine *h, double *mean /*N-1*/, int64_t *n /*N-1*/);
int pte_get_log_sum_ratio(const pte_engine *h, double *up /*N-1*/, int64_t *up_n, double *dn /*N-1*/, int64_t *dn_n);
int pte_get_round_trip(const pte_engine *h, int64_t *n_tempered_restarts, int64_t *n_round_trips);
int pte_get_index_process(const pte_engine *h, int64_t *out /*N * n_scans, [replica][scan]*/, int64_t *n_scans);
int pte_get_explorer_stats(const pte_engine *h, double *acceptance_mean /*N*/, int64_t *acceptance_n /*N*/,
                           double *n_steps_sum /*N*/, int64_t *n_steps_n /*N*/);
int pte_get_automala_stats(const pte_engine *h, double *factor_mean /*N*/, int64_t *factor_n /*N*/,
                           double *reversibility_mean /*N*/, int64_t *reversibility_n /*N*/);
int pte_get_online(const pte_engine *h, double *mean /*d*/, double *variance /*d*/, int64_t *n);   /* two legs: both target chains, merged */
/* the (d+1)-th entry of the `online` sample extract_sample(state::Array, lp) = [state; lp(state)] (src/pt/state.jl:79) */
int pte_get_online_log_density(const pte_engine *h, double *mean, double *variance);
/* energy_ac1s(pt) (src/recorders/recorder.jl:156-173) for the local chains: cor[K] (NaN where n < 2), n[K],
 * moments[5K] = running (mean before, mean after, C_bb, C_ba, C_aa); NULL pointers are skipped. */
int pte_get_energy_ac1(const pte_engine *h, double *cor, int64_t *n, double *moments);
/* traces of the last round, out[scan][d+1] (two legs: out[scan][2][d+1], the variational leg's target first);
 * *n_scans = 0 on shards that do not own the target chain.
 * With PTE_RECORD_TRACES_EXTENDED: out[scan][K][d+1], the K local chains in chain order, on every shard. */
int pte_get_traces(const pte_engine *h, double *out, int64_t *n_scans);

/* Replica fields in replica order (src/replicas/Replica.jl:5-30): state [N*d], chain [N],
 * rng [2N] = (seed, gamma) of each SplittableRandom.  NULL pointers are skipped. */
/* GaussianReference (src/variational/GaussianReference.jl:4-74) taking over the reference end of the interpolated
 * path on the chains with uses[c] != 0 (update_reference! + update_path_variational, src/variational/variational.jl:28-41):
 * log density -0.5 log(2 pi s^2) - (x - m)^2 / (2 s^2) per coordinate, gradient -(x - m) / s^2, sample_iid! = randn * s + m.
 * Funnel target, single engine.  NULL mean / std deactivates. */
int pte_set_variational_reference(pte_engine *h, const double *mean /*d*/, const double *std_dev /*d*/, int64_t dim,
                                  const int32_t *uses /*N*/);
/* PTE_TARGET_GAUSSIAN_MIXTURE: the target MixtureModel([MvNormal(means[k], Diagonal(std_devs[k].^2))], weights) (K components of
 * dimension d, row-major [K][d]; the weights need not sum to 1).  Validates (1 <= K <= 8; weights and std_devs positive and finite; means
 * finite), uploads and refreshes the swap statistics of the current states; may be called again to replace the mixture.  Until the first
 * call pte_explore, pte_swap, pte_run_scans and pte_get_state fail.  DESIGN 4.8. */
int pte_set_target_mixture(pte_engine *h, int64_t n_components, const double *weights /*K*/, const double *means /*K*d*/,
                           const double *std_devs /*K*d*/);
/* PTE_TARGET_BAYESIAN_GLM: the data of the target N(theta; 0, I / p) prod_i p(y_i | eta_i = X[i] . theta) (p = target_params[0], the
 * reference's precision; X row-major [n_obs][d]; noise_sd is read by PTE_GLM_NORMAL_IDENTITY only).  Validates (the likelihood; 1 <= n_obs
 * <= 4096 and n_obs * d <= 131072; X and y finite; y in {0, 1} for the logit; noise_sd positive and finite for the normal), uploads and
 * refreshes the swap statistics of the current states; may be called again to replace the data.  Until the first call pte_explore,
 * pte_swap, pte_run_scans, pte_group_run_scans and pte_get_state fail.  stepping_stone estimates log p(y) - (d/2) log(2 pi / p).  DESIGN 4.9. */
int pte_set_target_glm(pte_engine *h, int32_t likelihood, int64_t n_obs, const double *X /*[n_obs][d]*/, const double *y /*[n_obs]*/,
                       double noise_sd);
/* PTE_TARGET_MIXTURE_MODEL: the observations of the target N(theta; 0, I / p) prod_i sum_k w_k N(y_i; mu_k, exp(s_k)^2) with
 * theta = [mu_1..mu_K, s_1..s_K, alpha_1..alpha_K], w = softmax(alpha), K = dim / 3 (p = target_params[0], the reference's precision).
 * Validates in this order (the engine's target; 1 <= n_obs <= 65536; y not NULL; every y[i] finite), uploads and refreshes the swap
 * statistics of the current states; may be called again to replace the data.  Until the first call pte_explore, pte_swap, pte_run_scans,
 * pte_group_run_scans and pte_get_state fail.  stepping_stone estimates log p(y) - (d/2) log(2 pi / p).  DESIGN 4.11. */
int pte_set_target_mixture_model(pte_engine *h, int64_t n_obs, const double *y /*[n_obs]*/);
/* PTE_TARGET_HIERARCHICAL_NORMAL: the data of the target N(mu; 0, mu_sd^2) HalfCauchy(tau; 0, tau_scale) tau prod_j N(theta_j; mu, tau^2)
 * N(y_j; theta_j, sigma_j^2) in x = [mu, log tau, theta or eta] (parameterization PTE_HIER_*; the density is normalised in x).  Validates in
 * this order (the engine's target; the parameterization; n_groups == dim - 2; y and sigma not NULL; every y[j] finite and sigma[j] positive
 * and finite, in j; mu_sd, then tau_scale, positive and finite), uploads and refreshes the swap statistics of the current states; may be
 * called again to replace the data.  Until the first call pte_explore, pte_swap, pte_run_scans, pte_group_run_scans and pte_get_state fail.
 * stepping_stone estimates log p(y) - (d/2) log(2 pi / p), p = target_params[0] the reference's precision.  DESIGN 4.14. */
int pte_set_target_hier(pte_engine *h, int32_t parameterization, int64_t n_groups, const double *y /*[n_groups]*/,
                        const double *sigma /*[n_groups]*/, double mu_sd, double tau_scale);
/* PTE_TARGET_LATENT_AR1: the data of the target N(mu; 0, mu_sd^2) N(a; phi_loc, phi_scale^2) HalfCauchy(sigma; 0, sigma_scale) sigma
 * N(h_0; mu, sigma^2 / (1 - phi^2)) prod_{t>0} N(h_t; mu + phi (h_{t-1} - mu), sigma^2) prod_t p(y_t | h_t) in x = [mu, a, ls, h], phi = tanh(a),
 * sigma = exp(ls) (likelihood PTE_AR1_*; obs_sd is read by PTE_AR1_NORMAL_IDENTITY only; the density is normalised in x).  Validates in this
 * order (the engine's target; the likelihood; n_obs == dim - 3; y not NULL; every y[t] finite, in t; obs_sd -- the normal model only --, then
 * mu_sd, phi_scale, sigma_scale positive and finite; phi_loc finite), uploads and refreshes the swap statistics of the current states; may be
 * called again to replace the data.  Until the first call pte_explore, pte_swap, pte_run_scans, pte_group_run_scans and pte_get_state fail.
 * stepping_stone estimates log p(y) - (d/2) log(2 pi / p), p = target_params[0] the reference's precision.  DESIGN 4.15. */
int pte_set_target_ar1(pte_engine *h, int32_t likelihood, int64_t n_obs, const double *y /*[n_obs]*/, double obs_sd, double mu_sd,
                       double phi_loc, double phi_scale, double sigma_scale);
/* PTE_TARGET_DENSE_NORMAL: the target N(mean, precision^-1), normalised: log density c - (x - mean)' precision (x - mean) / 2 with
 * c = log det(precision) / 2 - (dim/2) log 2 pi.  precision is row-major dim x dim.  Refuses, in this order: a null argument; an engine of
 * another target; dim != the engine's dim; a non-finite entry of mean, then of precision (named by index); precision[i][j] != precision[j][i]
 * compared bit for bit (the kernels read row k as column k; the first offending pair is named); a matrix that is not positive definite (the
 * first non-positive pivot of a host Cholesky factorisation is named, which also gives c).  A refused call leaves the engine as it was.
 * Otherwise uploads the matrix, its diagonal and the mean ((dim + 2) x 64 ceil-pow2(dim / 64) doubles: 2 MiB + 8 KiB at dim = 512) and
 * refreshes the swap statistics of the current states; may be called again to replace the data.  Until the first call pte_explore,
 * pte_swap, pte_run_scans, pte_group_run_scans and pte_get_state fail.  Every chain of the path is Gaussian, and stepping_stone estimates
 * -(dim/2) log(2 pi / p), p = target_params[0] the reference's precision: the log evidence of the normalised target is 0.  DESIGN 4.16. */
int pte_set_target_dense(pte_engine *h, int64_t dim, const double *mean /*[dim]*/, const double *precision /*[dim][dim]*/);
/* PTE_TARGET_SPIN_GLASS: the quenched bonds of the base_length x base_length periodic lattice, row-major, every entry +1 or -1:
 * bonds_right[i][j] couples site (i, j) with (i, (j + 1) mod L), bonds_down[i][j] couples (i, j) with ((i + 1) mod L, j).  The target is
 * exp(beta S), S = sum_ij s_ij (bonds_right_ij s_i,j+1 + bonds_down_ij s_i+1,j) (at L = 2 the two bonds between the same pair of sites are
 * distinct terms); with every bond +1 the family is PTE_TARGET_ISING bit for bit.  Refuses an engine of another target, a base_length
 * that is not the engine's, a null argument, and the first entry that is not +-1 (by plane and index): +-J is the supported disorder --
 * real-valued or diluted couplings break the two-threshold filter and the bit packing of the sweep.  A refused call leaves the engine as it
 * was.  Otherwise uploads the bonds (one copy shared by all replicas) and recounts the swap statistic of the current states; may be called
 * again to replace the bonds.  Until the first call pte_explore, pte_swap, pte_run_scans, pte_group_run_scans and pte_get_state fail.
 * DESIGN 4.17. */
int pte_set_target_spin_glass(pte_engine *h, int64_t base_length, const int8_t *bonds_right /*[L][L]*/, const int8_t *bonds_down /*[L][L]*/);
/* PTE_TARGET_SPIN_GLASS_3D: the quenched bonds of the base_length^3 periodic lattice, three planes [L][L][L] in C order [z][y][x], every
 * entry +1 or -1: bonds_x[z][y][x] couples site (z, y, x) with (z, y, (x + 1) mod L), bonds_y[z][y][x] with (z, (y + 1) mod L, x),
 * bonds_z[z][y][x] with ((z + 1) mod L, y, x).  Site (z, y, x) is coordinate (z L + y) L + x of the state.  The target is exp(beta S),
 * S = sum s_zyx (bonds_x s_x+1 + bonds_y s_y+1 + bonds_z s_z+1) (at L = 2 the two bonds between the same pair of sites are distinct terms).
 * Refuses an engine of another target, a base_length that is not the engine's, a null argument, and the first entry that is not +-1 (by
 * plane and index).  A refused call leaves the engine as it was.  Otherwise uploads the bonds (one copy shared by all replicas) and recounts
 * the swap statistic of the current states; may be called again to replace the bonds.  Until the first call pte_explore, pte_swap,
 * pte_run_scans, pte_group_run_scans and pte_get_state fail.  DESIGN 4.19. */
int pte_set_target_spin_glass_3d(pte_engine *h, int64_t base_length, const int8_t *bonds_x /*[L][L][L]*/, const int8_t *bonds_y /*[L][L][L]*/,
                                 const int8_t *bonds_z /*[L][L][L]*/);
/* PTE_TARGET_VARIABLE_SELECTION: the data of the target N(theta; 0, I / p) prod_j pi^gamma_j (1 - pi)^(1 - gamma_j)
 * prod_i p(y_i | eta_i = sum_j X[i][j] gamma_j theta_j) (p = target_params[0], the reference's precision; pi = inclusion_prob; X row-major
 * [n_obs][d] with d = dim / 2; likelihood PTE_GLM_*, noise_sd read by PTE_GLM_NORMAL_IDENTITY only).  Validates as pte_set_target_glm does
 * (the likelihood; d == dim / 2; 1 <= n_obs <= 4096 and n_obs * d <= 131072; X and y finite; y in {0, 1} for the logit; noise_sd positive
 * and finite for the normal), then inclusion_prob in (0, 1); uploads and refreshes the swap statistics of the current states; may be called
 * again to replace the data.  Until the first call pte_explore, pte_swap, pte_run_scans, pte_group_run_scans and pte_get_state fail.
 * stepping_stone estimates log p(y) - (d/2) log(2 pi / p) - d log 2 (the reference is uniform on the 2^d indicator vectors).  DESIGN 4.12. */
int pte_set_target_varsel(pte_engine *h, const double *X /*[n_obs][d]*/, const double *y /*[n_obs]*/, int64_t n_obs, int64_t d,
                          int32_t likelihood, double noise_sd, double inclusion_prob);
/* PTE_TARGET_CHANGE_POINT: the data of the target N(r; 0, I / p) (n + 1)^-K prod_j prod_{s_j <= i < s_{j+1}} Poisson(y_i; exp(r_j)), where
 * s_1 <= ... <= s_K are the sorted change points tau (unordered in the state), s_0 = 0, s_{K+1} = n, K = (dim - 1) / 2 and p =
 * target_params[0], the reference's precision.  Validates (1 <= n_obs <= 65536; every y_i finite, integral and in 0..2^20), uploads the
 * prefix sums of y and refreshes the swap statistics of the current states; may be called again to replace the data.  Until the first call
 * pte_explore, pte_swap, pte_run_scans, pte_group_run_scans and pte_get_state fail.  stepping_stone estimates
 * log p(y) - ((K+1)/2) log(2 pi / p) - K log(n + 1) (the reference is uniform on the (n + 1)^K placements).  DESIGN 4.13. */
int pte_set_target_changepoint(pte_engine *h, const double *y /*[n_obs]*/, int64_t n_obs);
/* PTE_TARGET_CHANGE_POINT: the form in which k_explore_changepoint evaluates a proposal -- in full, or from the sorted bounds kept for the
 * committed state.  Both compute the same bits; AUTO is the faster one.  For measurements and tests. */
enum { PTE_CHANGEPOINT_FORM_AUTO = 0, PTE_CHANGEPOINT_FORM_FULL = 1, PTE_CHANGEPOINT_FORM_CACHED = 2 };
int pte_set_changepoint_form(pte_engine *h, int32_t form);
int pte_get_state(const pte_engine *h, double *state, int64_t *chain, uint64_t *rng);
/* NULL leaves a field as it is.  chain must be a permutation of the engine's own chains (of a shard: [c0, c0 + K)); it is judged before
 * anything is copied, so a refused call has changed nothing -- and a poisoned engine (pte_scan_loop_stats) stays poisoned. */
int pte_set_state(pte_engine *h, const double *state, const int64_t *chain, const uint64_t *rng);

/* ---- chain-sharded engines (one engine per GPU; rank g owns chains [g*N/G, (g+1)*N/G)) -----------
 * The reference's distributed swap! (src/swap/swap.jl:79-102) exchanges 16-byte SwapStats with the
 * partner replica's rank and moves chain labels.  Here the shard boundary is between CHAINS, so only
 * the G-1 boundary pairs cross GPUs: their SwapStats are exchanged between the two phases below and,
 * iff the swap is accepted, the two replicas' payloads {state, sum x^2, rng, replica id, round-trip
 * state} trade places.  With these two-phase calls the HOST moves the bytes (any transport; the CPU tests use
 * gloo, loopback tests plain copies); the transport the library itself provides is pte_comm_* below.  side: 0 = pair (c0-1, c0), 1 = pair (c0+K-1, c0+K).
 * With world_size == 1 these calls are valid too (no boundary is ever active) and equal pte_swap. */
int pte_shard_info(const pte_engine *h, int64_t *first_chain, int64_t *n_local_chains, int64_t *n_local_pairs);
/* phase 1: swap_stat of every local chain (one rand per replica), index_process / round_trip records.
 * stats_out[4] = (log_ratio, uniform) of the lowest and of the highest local chain;
 * active_out[2] = whether the boundary pair on that side is a pair of this scan's DEO graph. */
int pte_swap_begin(pte_engine *h, int64_t scan, double *stats_out, int32_t *active_out);
/* phase 2: nbr_stats[4] = SwapStats received from the lower / upper neighbour (ignored where inactive);
 * decisions, recorders, chain relabelling of local pairs; accepted_out[2] = boundary swap accepted. */
int pte_swap_finish(pte_engine *h, int64_t scan, const double *nbr_stats, int32_t *accepted_out);
int64_t pte_boundary_payload_bytes(const pte_engine *h);            /* 8 * (sw + 6), sw = d (f64 coordinates) or ceil(ceil(d/32)/2) (bit-packed Ising lattice) */
int pte_boundary_export(pte_engine *h, int side, void *dst, int dst_is_device);
int pte_boundary_import(pte_engine *h, int side, const void *src, int src_is_device);
/* Device-resident, stream-ordered variant of the two phases (no host round trip per scan): the boundary
 * chain's SwapStat and -- speculatively -- its replica's payload are packed into one message of
 * pte_shard_message_bytes() = 8 (sw + 8) bytes per active side; the caller moves send -> neighbour's recv
 * with stream-ordered transfers (RCCL send/recv enqueued on pte_get_stream(), replacing the reference's
 * MPI transmits, src/mpi_utils/Entangler.jl:118-180) and the receiving engine decides and applies the
 * payload on the device iff the swap is accepted.  All four buffers are caller-owned device memory.
 *   pte_shard_scan_begin : explore!(scan) + phase 1 + pack; active_out[2] as for pte_swap_begin (host-computable)
 *   pte_shard_scan_finish: phase 2 from the received messages + conditional import
 *   pte_shard_sync       : synchronise, raise device errors, boundary_swaps_out[2] = applied swaps per side */
void *pte_get_stream(const pte_engine *h);                          /* hipStream_t of the engine */
int64_t pte_shard_message_bytes(const pte_engine *h);
int pte_shard_set_buffers(pte_engine *h, void *send_lo, void *recv_lo, void *send_hi, void *recv_hi);
int pte_shard_scan_begin(pte_engine *h, int64_t scan, int32_t *active_out);
int pte_shard_scan_finish(pte_engine *h, int64_t scan);
int pte_shard_sync(pte_engine *h, int64_t *boundary_swaps_out);
/* ---- transport behind the ABI -------------------------------------------------------------------
 * The reference keeps its communication inside the package (MPI: src/mpi_utils/Entangler.jl:118-180
 * `transmit!`, :188-251 `all_reduce_deterministically`; distributed swap! src/swap/swap.jl:79-102).  Here the
 * boundary exchange of a chain-sharded engine is RCCL point-to-point (ncclSend / ncclRecv in one group per scan,
 * over xGMI inside a node) enqueued on the engine's own HIP stream between the pack and the decide kernels:
 * no host synchronisation inside the scan loop, no collective on the data path.
 *   one process per GPU : rank 0 calls pte_comm_unique_id, the host hands the 128 bytes to every rank by any
 *                         means it has (MPI.bcast, a socket, a file), every rank calls pte_comm_init; from then
 *                         on pte_run_scans works on the sharded engine exactly as on a single one.
 *   one process, G GPUs : pte_group_run_scans drives G engines (rank g = engines[g]) from one host thread; the
 *                         messages move by stream-ordered device-to-device copies (peer copies over xGMI).
 * Message buffers are engine-owned unless the caller installed its own with pte_shard_set_buffers.
 * RCCL is mapped at run time (dlopen; $PTE_RCCL_LIB overrides the search), libpte.so does not link it. */
#define PTE_COMM_ID_BYTES 128
/* Which library the transport's entry points come from (the file, via dladdr) and what its ncclGetVersion reports -- for the
 * log line of a multi-GPU run.  $PTE_RCCL_LIB can name another library (tests: a stand-in that accepts two ranks on one
 * device); it is honoured only after pte_comm_allow_library_override(1), and a set variable WITHOUT that opt-in makes every
 * pte_comm_* call fail (a stale variable must not silently re-route the boundary traffic). */
int pte_comm_allow_library_override(int32_t allow);
int pte_comm_library(char *path_out, int64_t capacity, int32_t *version_out);
int pte_comm_unique_id(uint8_t *id_out /*PTE_COMM_ID_BYTES*/);
int pte_comm_init(pte_engine *h, const uint8_t *id /*PTE_COMM_ID_BYTES*/);   /* ncclCommInitRank(cfg.world_size, id, cfg.rank); collective */
int pte_comm_destroy(pte_engine *h);
/* kind: 0 none, 1 RCCL; n_ranks_seen: sum over the communicator of 1 (measured, not configured);
 * boundary_swaps[2]: boundary swaps applied on the device since pte_create, per side. NULLs are skipped. */
int pte_comm_info(pte_engine *h, int32_t *kind, int32_t *n_ranks_seen, int64_t *boundary_swaps);
/* Small host-side collectives over the same communicator, so that a host without MPI can bracket a round:
 * barrier; element-wise MAX / SUM of n doubles (op: 0 max, 1 sum); all-gather of `bytes` bytes per rank into
 * recv[world * bytes] in rank order (the per-round recorder slices -- recorders are keyed by chain / pair, so
 * concatenation in rank order is deterministic).  With world_size == 1 they are local no-ops / copies. */
int pte_comm_barrier(pte_engine *h);
int pte_comm_allreduce(pte_engine *h, double *inout, int64_t n, int32_t op);
int pte_comm_allgather(pte_engine *h, const void *send, int64_t bytes, void *recv);
/* G engines of ONE process, engines[g] = rank g of a world of G (same N, d, explorer): the fused scan loop. */
int pte_group_run_scans(pte_engine *const *engines, int32_t n_engines, int64_t first_scan, int64_t n_scans);

/* ---- the replica overlap between two runs of a lattice family (the project's own specification) ----------------
 * Two engines a, b over the same lattice model -- PTE_TARGET_ISING, PTE_TARGET_SPIN_GLASS or PTE_TARGET_SPIN_GLASS_3D, the same
 * bonds, the same N and schedule, different seeds -- hold two independent copies of the system at every temperature.  For chain c,
 * with t = (bits of the replica at chain c in a) XOR (the same in b) over the dim site bits, a record adds
 *   site overlap   k  = popcount(t), 0..dim            q   = 1 - 2 k / dim           to hist[c][k] and n[c]
 *   link overlap   kl = sum_dir popcount(t XOR shift_dir(t)), shift_dir the periodic shift by one site along each lattice direction
 *                  (every site owns its +dir bond; at base_length 2 the two bonds between the same pair of sites are distinct terms;
 *                  the bonds cancel, J^2 = 1)          q_l = 1 - 2 kl / n_links      to link_n[c], link_sum[c], link_sum2[c]
 * All accumulators are exact int64.  The link overlap is recorded on the cube at every base_length (n_links = 3 dim) and on the 2-D
 * lattices where base_length % 32 == 0 (n_links = 2 dim); elsewhere pte_overlap_info reports n_links = 0 and link_n stays 0.
 * The object holds no state of either engine: destroying it leaves both usable.  Errors of pte_overlap_create are read with
 * pte_last_error(NULL), errors of the other calls with pte_last_error(a) (an error of b is copied there).
 *   pte_overlap_create    refuses, naming what it got: a null argument or a == b; engines on different devices; a target that is not a
 *                         lattice; differing target, dim or N; world_size != 1; n_chains_variational > 0; a spin-glass engine without
 *                         bonds; bond planes that differ (both engines' device planes are downloaded and compared); histograms of
 *                         more than 2 GiB (N (dim + 1) 8 bytes)
 *   pte_overlap_record    one record of the states as they are; synchronous
 *   pte_overlap_run_scans for s = first_scan .. first_scan + n_scans - 1: explore!(s) and communicate!(s) of a on a's stream and of b on
 *                         b's, then one record of the post-swap states; each engine ends exactly where pte_run_scans alone would have
 *                         left it unless the cluster move is on.  record and run_scans refuse when the two engines' schedules differ in any bit, and a poisoned engine
 *   pte_overlap_reduce    snapshot the accumulators to the host and zero them on the device
 *   pte_overlap_get       the snapshot: n[N], hist[N][dim + 1], link_n[N], link_sum[N], link_sum2[N]; NULLs are skipped */
typedef struct pte_overlap pte_overlap;
int pte_overlap_create(pte_engine *a, pte_engine *b, pte_overlap **out);
int pte_overlap_destroy(pte_overlap *ov);
int pte_overlap_info(const pte_overlap *ov, int64_t *n_chains, int64_t *dim, int64_t *n_links);
int pte_overlap_record(pte_overlap *ov);
int pte_overlap_run_scans(pte_overlap *ov, int64_t first_scan, int64_t n_scans);
int pte_overlap_reduce(pte_overlap *ov);
int pte_overlap_get(const pte_overlap *ov, int64_t *n, int64_t *hist, int64_t *link_n, int64_t *link_sum, int64_t *link_sum2);

/* ---- Houdayer's cluster move between the two copies (the project's own specification; off after pte_overlap_create) ----
 * For chain c with betas[c] >= min_beta, t = a XOR b as above and k = popcount(t): if k == 0 nothing is written and empty[c] += 1; else
 *   the draw     u = mix64(seed + (uint64)(m N + c + 1) 0x9E3779B97F4A7C15) mod 2^64, m the launch counter (0 at set, +1 per launch);
 *                j = ((u >> 32) k) >> 32; the seed site is the j-th set bit of t in increasing site index.  No engine's RNG word is read
 *   the cluster  C = the connected component of the seed site among the set bits of t under the lattice's nearest-neighbour links with
 *                periodic wrap (4 on the square, 6 on the cube; the bonds' signs play no part; diagonal contact does not connect)
 *   the flip     a ^= C, b ^= C in both engines' rows; S_a + S_b is unchanged, so the move is always accepted, and it is its own inverse
 *   the swap's   delta = sum_dir (4 popcount(B & x) - 2 popcount(B)), B = C XOR shift_dir(C), x = a XOR shift_dir(a) XOR J_dir, every site
 *   statistic    owning its +dir bond: the pair sum of a's replica gains delta, that of b's replica loses it, as exact integers
 * It runs on the cube at every base_length and on the 2-D lattices where base_length % 32 == 0 (the link overlap's condition).
 * Accumulators per chain, int64, zeroed by pte_overlap_reduce with the others: n moves made, empty moves with k == 0, size_sum += |C|,
 * k_sum += k, abs_ds_sum += |delta|, passes_sum += passes of the kernel's fixed-point loop (a measurement, not part of the specification).
 *   pte_overlap_set_cluster_move  every = 0 turns the move off; otherwise pte_overlap_run_scans launches it at every scan s with
 *                                 s % every == 0, after both swaps and before the record (whose values it does not change: t stays).
 *                                 Refuses, naming what it got: every < 0; min_beta outside [0, 1] or NaN; a 2-D lattice whose base_length
 *                                 is not a multiple of 32.  Resets m
 *   pte_overlap_cluster_move      one move on the states as they are; synchronous; the entry checks of pte_overlap_record; refused if the
 *                                 move was never set
 *   pte_overlap_cluster_get       the snapshot taken by pte_overlap_reduce: the six arrays [N] and the number of launches it covers;
 *                                 NULLs are skipped */
int pte_overlap_set_cluster_move(pte_overlap *ov, int64_t every, double min_beta, uint64_t seed);
int pte_overlap_cluster_move(pte_overlap *ov);
int pte_overlap_cluster_get(const pte_overlap *ov, int64_t *n, int64_t *empty, int64_t *size_sum, int64_t *k_sum, int64_t *abs_ds_sum, int64_t *passes_sum,
                            int64_t *moves_launched);

/* ---- the plane autocorrelation of the overlap field (the project's own specification; off after pte_overlap_create) ----
 * What the wave-vector-dependent spin-glass susceptibility chi_SG(k) along the lattice axes and the correlation length xi_L are computed
 * from.  n_axes = 3 on the cube, 2 on the 2-D lattices; axis 0 is the fastest site index (x of site (z, y, x) at (z L + y) L + x; the
 * column j of site (i, j) at i L + j), axis 1 the next (y; the row i), axis 2 the cube's z; L = base_length, M = dim / L.  For chain c, with
 * t = a XOR b as above, a record taken while the feature is on adds, as exact integers,
 *   P_axis[p]  = the set bits of t among the M sites whose coordinate along the axis is p, p = 0 .. L - 1
 *   Q_axis[p]  = M - 2 P_axis[p]                             the sum of q_i = s_i^a s_i^b over that plane (2-D: that line)
 *   C_axis(r)  = sum_p Q_axis[p] Q_axis[(p + r) mod L]       to plane_corr[c][axis][r], r = 0 .. L - 1, and 1 to plane_n[c]
 * C(r) = C(L - r) and |C| <= L M^2.  On the host, along an axis and with k = 2 pi m / L,
 *   chi_SG(m) = (1 / (dim plane_n)) sum_r plane_corr[c][axis][r] cos(2 pi m r / L),   chi_SG(0) = dim <q^2>
 *   xi_L      = 1 / (2 sin(pi / L)) sqrt(chi_SG(0) / chi_SG(1) - 1)
 * and sum_r plane_corr[c][axis][r] == sum_k hist[c][k] (dim - 2 k)^2 on every axis when every record of the round was taken with the
 * feature on.  It runs where the link overlap is recorded: the cube at every base_length, the 2-D lattices where base_length % 32 == 0.
 *   pte_overlap_set_planes    on != 0: pte_overlap_record and pte_overlap_run_scans launch the kernel right after the record's own
 *                             (behind a cluster move of the same scan); 0: they do not.  Refuses, naming the base length, a 2-D lattice
 *                             whose base_length is not a multiple of 32.  The accumulators are allocated at the first on != 0: with the
 *                             feature never on, no call makes a launch, a copy or an allocation on its account
 *   pte_overlap_planes_info   n_axes (0 where the feature cannot run), base_length, on (0 / 1); NULLs are skipped
 *   pte_overlap_planes_get    the snapshot taken by pte_overlap_reduce, which zeroes these accumulators with the others:
 *                             plane_n[N], plane_corr[N][n_axes][base_length] (zeros if the feature was never on); NULLs are skipped */
int pte_overlap_set_planes(pte_overlap *ov, int on);
int pte_overlap_planes_info(const pte_overlap *ov, int64_t *n_axes, int64_t *base_length, int64_t *on);
int pte_overlap_planes_get(const pte_overlap *ov, int64_t *plane_n, int64_t *plane_corr);

/* Name of the kernel that explores on this engine (e.g. "k_explore_slice8"), for profiles and bench.py. */
const char *pte_kernel_name(const pte_engine *h);

/* The form pte_run_scans takes on this engine -- the reference's `while next_scan!(pt)` loop, src/pt/pigeons.jl:46-55: "" = two launches
 * per scan (explore, swap); otherwise the ONE kernel that runs all the scans of a call (e.g. "k_scans_slice8": workgroup c holds chain c,
 * the DEO swap is a hand-shake between the two waves of a pair, no launch boundary and no grid-wide barrier per scan).  Chosen when one GPU
 * holds the whole ladder, every workgroup is resident at once, the explorer has such a kernel and pte_config.debug_kernel does not carry
 * PTE_KERNEL_TWO_LAUNCHES; results are bit-identical either way.  A name ending in "_wg" (AutoMALA / MALA) is the form with several
 * consecutive chains per workgroup, whose inner pairs shake hands through LDS (PTE_KERNEL_SCAN_LOOP_ONE_CHAIN selects the other form);
 * "k_scans_langevin_mw" (AutoMALA / MALA on the scaled-precision MVN path, 512 < dim <= 1024) gives a chain a 256-thread workgroup.
 * pte_timing_get(kernel = 4) times these launches. */
const char *pte_scan_loop_name(const pte_engine *h);
int pte_scan_loop_info(const pte_engine *h, int64_t *resident_limit, int64_t *timed_launches, int64_t *timed_scans);
/* Forward progress of that one kernel (round 6).  Its hand-shakes spin, so all its workgroups must be on the device together.  That is ENFORCED
 * inside the launch: no workgroup touches anything before every workgroup has arrived at a counter; if one is still missing after 50 ms (another
 * engine, stream or process holds compute units) all of them return with nothing written and pte_run_scans runs the same scans as explore + swap
 * launches -- same results, no error, the next 1, 2, 4, ... 256 calls skip the attempt.  So pte_run_scans cannot hang, as the reference's loop
 * cannot (src/pt/pigeons.jl:46-55).  What is left: a wave that dies or stays descheduled for 3 s AFTER all have arrived (the residency of a
 * started workgroup is the hardware's; whole-queue preemption between processes suspends and resumes all of a queue's waves together).  Then the
 * hand-shake times out, every other wave sees the error word and leaves at once, the call fails and the engine is POISONED: its replicas stopped at
 * different scans.  Every pte_* call on it fails with a message saying so, except pte_destroy and pte_set_state with state, chain and rng of all
 * replicas, which restores it (and discards the recorders of the round).
 *   *fused_calls: pte_run_scans calls that ran as one launch; *gate_aborts: launches that found a workgroup missing and fell back;
 *   *poisoned: 0 / 1.  NULLs are skipped. */
int pte_scan_loop_stats(const pte_engine *h, int64_t *fused_calls, int64_t *gate_aborts, int32_t *poisoned);

/* index process of the local slots: replica[scan][K], chain[scan][K] (global ids). */
int pte_get_index_process_shard(const pte_engine *h, int64_t *replica, int64_t *chain, int64_t *n_scans);
int pte_get_replica_ids(const pte_engine *h, int64_t *out /*K*/);

/* Measurement hooks (bench.py): per-kernel HIP-event timing accumulated on the engine's stream
 * over pte_run_scans calls since the last reset.  kernel: 0 = explore, 1 = swap (both empty while pte_run_scans runs as one fused launch:
 * 4 = that launch, pte_scan_loop_info says how many scans it held); 2 = k_init (create_replicas), timed once
 * at pte_create and not touched by pte_timing_reset; 3 = the boundary exchange of a chain-sharded engine (events around
 * ncclGroupStart .. ncclGroupEnd on the engine's stream: from "messages packed" to "messages landed", one sample per even scan).
 * enable: 0 off, 1 every kernel, 2 the explore kernels only (an event pair costs ~10 us of stream time per launch). */
int pte_timing_reset(pte_engine *h, int enable);
int pte_timing_get(const pte_engine *h, int kernel, double *total_ms, int64_t *launches);
/* the individual launch durations behind pte_timing_get (min / median / max of the timed region); out_ms may be NULL */
int pte_timing_get_samples(const pte_engine *h, int kernel, double *out_ms, int64_t capacity, int64_t *n_out);

/* The conventions of Julia's Random stdlib that no fixture from a live Julia pins yet (include/pte_rng_policy.h: the
 * ziggurat tail formula, the bit rand(rng, Bool) takes).  One word per device, read by every engine of this process on
 * that device; the default is PTE_RNG_POLICY_DEFAULT.  Never read from the environment. */
int pte_set_rng_policy(int32_t device, uint32_t policy);
int pte_get_rng_policy(int32_t device, uint32_t *policy);

/* RNG building blocks exposed for parity tests of the device samplers: fill `n` draws from the
 * stream (seed, gamma) on the device, in the reference's sequential order.
 * kind: 0 = rand (Float64 in [0,1)), 1 = randn, 2 = randexp, 3 = rand(rng, Bool) as 0.0 / 1.0.  Returns the advanced stream. */
int pte_test_rng_fill(int32_t device, uint64_t *seed_gamma /*2, in-out*/, int32_t kind, int64_t n, double *out);
/* The quotient procedure of the Langevin-family kernels, element by element (round 6): the preconditioner's diagonal and the funnel's sigma divide
 * thousands of values each, so a / b is evaluated as Markstein's correctly rounded q' = fma(fma(-q, b, a), r, q), q = a r, r = RN(1 / b), and as the
 * division itself wherever the theorem does not apply (quotient estimate outside [2^-900, 2^900], zero, non-finite; divisor with an extreme exponent
 * or an all-ones significand).  out[i] must equal the IEEE quotient a[i] / b[i] the reference computes (src/explorers/hamiltonian_dynamics.jl:60-76,
 * `./ M`) bit for bit; took_division[i] = 1 where the guards chose the division. */
int pte_test_quotient(int32_t device, const double *a, const double *b, int64_t n, double *out, int32_t *took_division);
/* sqr_norm of each row of x [rows][d] with the engine's fixed reduction tree. */
int pte_test_sqr_norm(int32_t device, const double *x, int64_t rows, int64_t d, double *out);

#ifdef __cplusplus
}
#endif
#endif /* PTE_H */
