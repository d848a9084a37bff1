# PigeonsMI355X.jl -- the reference-side binding a Pigeons.jl maintainer would add (a package extension or a small package).
#
# INERT IN THE BUILD IMAGE (no Julia toolchain exists there; never executed).  It binds the dispatch hooks that bracket the
# explore-then-swap hot path of Pigeons.jl v0.4.10, plus construction / adaptation / recorders, to the C ABI of include/pte.h.
# Conventions follow the reference's only FFI precedent, ext/PigeonsBridgeStanExt/interface.jl:118-183 (Cint return code,
# message fetched on error).
#
# How a run reaches the device -- nothing in Pigeons.jl is edited, every hook is reached by ordinary dispatch:
#
#     pt = pigeons(target = on_mi355x(toy_mvn_target(1024)), n_chains = 1024, explorer = SliceSampler(),
#                  record = [round_trip, log_sum_ratio])
#
#   PT(inputs)  (src/pt/PT.jl:49-54)
#     Shared(inputs)                      create_path / default_explorer / default_reference forward to the wrapped target (below)
#     create_replicas(inputs, shared)     `inputs::Inputs{<:OnDevice}`: dispatch on the FIRST type parameter of Inputs (its `target`
#                                          field, src/pt/Inputs.jl:9-11) -- the method PT(inputs) itself calls (src/replicas/replicas.jl:65-68)
#   run_one_round!(pt)  (src/pt/pigeons.jl:46-55), unmodified:
#     explore!(pt, explorer, ::Val)       loops `for replica in locals(pt.replicas)`: locals(::DeviceReplicas) is ONE DeviceBatch, and
#                                          explore!(pt, ::DeviceBatch, explorer) is one ccall for all replicas (dispatch on the replica)
#     communicate!(pt) -> swap!(pair_swapper, pt.replicas, swap_graph)       dispatch on the replicas container
#     reduce_recorders!(pt, pt.replicas)                                     dispatch on the replicas container
#   adapt(pt, reduced_recorders)  (src/pt/pigeons.jl:152-162), unmodified: adapt_tempering runs on the host as always; the new
#     schedule / explorer parameters reach the device from `after_adapt!` (called from the fused run_one_round! below, or by hand).
# The FUSED scan loop (one ccall per round instead of two per scan) needs a method of run_one_round! itself; it dispatches on
# PT's first type parameter (the `inputs` field, src/pt/PT.jl:6-12) and is optional.
module PigeonsMI355X

using Pigeons
using Pigeons: Inputs, Shared, Replica, PT, SliceSampler, AutoMALA, MALA, Compose, ToyExplorer, ScaledPrecisionNormalPath,
               InterpolatingPath, ScaledPrecisionNormalLogPotential, GroupBy, Mean, Sum, Variance, CovMatrix, Group, LogSum,
               RoundTripRecorder, OnlineStateRecorder, EqualWeight
using Random: AbstractRNG

const libpte = "libpte.so"

# ---- include/pte.h mirrored ------------------------------------------------------------------------------------------------
const TARGET_MVN, TARGET_TEST_SWAPPER, TARGET_FUNNEL, TARGET_ISING, TARGET_GAUSSIAN_MIXTURE = Int32(0), Int32(1), Int32(2), Int32(3), Int32(4)
const TARGET_BAYESIAN_GLM = Int32(5)
const TARGET_MIXTURE_MODEL = Int32(6)
const TARGET_VARIABLE_SELECTION = Int32(7)
const TARGET_CHANGE_POINT = Int32(8)
const TARGET_HIERARCHICAL_NORMAL = Int32(9)
const HIER_CENTERED, HIER_NONCENTERED = Int32(0), Int32(1)
const TARGET_LATENT_AR1 = Int32(10)
const AR1_STOCHASTIC_VOLATILITY, AR1_NORMAL_IDENTITY = Int32(0), Int32(1)
const TARGET_DENSE_NORMAL = Int32(11)
const TARGET_SPIN_GLASS = Int32(12)
const TARGET_SPIN_GLASS_3D = Int32(13)      # the +-J spin glass on the L^3 cube, CheckerboardMetropolis only (DESIGN 4.19)
const GLM_BERNOULLI_LOGIT, GLM_NORMAL_IDENTITY = Int32(0), Int32(1)
const EXPLORER_NONE, EXPLORER_TOY, EXPLORER_SLICE, EXPLORER_AUTOMALA, EXPLORER_ISING, EXPLORER_MALA, EXPLORER_AAPS = Int32.((0, 1, 2, 3, 4, 5, 6))
const EXPLORER_CHECKERBOARD_METROPOLIS = Int32(7)      # the two-colour Metropolis sweep of the lattice targets (DESIGN 4.18)
const RECORD_ROUND_TRIP, RECORD_INDEX_PROCESS, RECORD_ONLINE, RECORD_TRACES, RECORD_ENERGY_AC1, RECORD_TRACES_EXTENDED =
    UInt32.((1, 2, 4, 8, 16, 32))
const RECORD_REFERENCE_REDUCTION = UInt32(64)   # swap recorders reduced by per-replica Mean / LogSum fits + tree merge, replayed in pte_reduce (include/pte.h)

# mirror of `pte_config` -- field order and types must match; pte_create checks struct_size and abi_version, so a layout
# mismatch fails loudly instead of corrupting memory
Base.@kwdef mutable struct PteConfig
    struct_size::UInt32 = 0
    abi_version::UInt32 = 2
    device::Int32 = 0
    target::Int32 = TARGET_MVN
    explorer::Int32 = EXPLORER_TOY
    record_flags::UInt32 = 3
    n_chains::Int64 = 10
    dim::Int64 = 1
    seed::UInt64 = 1
    max_scans_per_round::Int64 = 1024
    target_params::NTuple{4,Float64} = (1.0, 10.0, 0.0, 0.0)
    slice_w::Float64 = 10.0
    slice_p::Int32 = 20
    slice_n_passes::Int32 = 3
    slice_max_iter::Int32 = 1024
    am_base_n_refresh::Int32 = 3
    am_exponent_n_refresh::Float64 = 0.35
    am_step_size::Float64 = 1.0
    am_p0::Float64 = 1/3
    am_p1::Float64 = 1/3
    am_preconditioner::Int32 = 2
    rank::Int32 = 0
    world_size::Int32 = 1
    explorer2::Int32 = EXPLORER_NONE      # Compose(explorer, explorer2)
    n_chains_variational::Int64 = 0       # StabilizedPT with variational == nothing
    debug_kernel::Int32 = 0               # PTE_KERNEL_*: 0 = the default kernel of the explorer (never read from the environment)
    aaps_K::Int32 = 5                     # AAPS.K (AAPS.jl)
end

# ---- targets on the device -------------------------------------------------------------------------------------------------
"""`on_mi355x(target; device = 0, rank = 0, world_size = 1, reference_reduction = false)`: run the explore-then-swap loop of `target` on an MI355X.
`reference_reduction = true` (PTE_RECORD_REFERENCE_REDUCTION, include/pte.h): the swap recorders are reduced with the reference's own arithmetic --
per-replica Mean / LogSum fits merged over the binary tree on the replica index -- instead of chain-keyed sums; forces :index_process, logs 16 B per
chain and scan.  An explicit option, like `PT(reference_reduction = ...)` on the Python side: nothing here reads the environment (ADVICE r05)."""
struct OnDevice{T}
    target::T
    device::Int
    rank::Int
    world_size::Int
    reference_reduction::Bool
end
on_mi355x(target; device = 0, rank = 0, world_size = 1, reference_reduction = false) = OnDevice(target, device, rank, world_size, reference_reduction)

# everything Shared(inputs) / preflight ask of a target goes to the wrapped one (src/targets/target.jl informal interface)
Pigeons.create_path(t::OnDevice, inputs::Inputs) = Pigeons.create_path(t.target, inputs)
Pigeons.default_explorer(t::OnDevice) = Pigeons.default_explorer(t.target)
Pigeons.default_reference(t::OnDevice) = Pigeons.default_reference(t.target)
Pigeons.initialization(t::OnDevice, rng::AbstractRNG, i::Int) = Pigeons.initialization(t.target, rng, i)
Pigeons.sample_iid!(t::OnDevice, replica, shared) = Pigeons.sample_iid!(t.target, replica, shared)
Pigeons.sample_names(state, t::OnDevice) = Pigeons.sample_names(state, t.target)

"""Neal's funnel of test/supporting/dimensional-analysis.jl:34-52 (a `LogDensity` defined in user code there): the device family
PTE_TARGET_FUNNEL.  Used as `Inputs(target = on_mi355x(DeviceFunnel(128)), reference = ScaledPrecisionNormalLogPotential(1/9, 128))`."""
struct DeviceFunnel; dim::Int; end
"""The Ising model of examples/ising.jl:13-37 (`IsingLogPotential(beta, base_length)`, defined in user code there):
PTE_TARGET_ISING, explorer = the Metropolis sweeps of examples/ising.jl:91-116 (n_sweeps passes)."""
struct DeviceIsing; beta::Float64; base_length::Int; n_sweeps::Int; end
"""The +-J Edwards-Anderson spin glass, the device family PTE_TARGET_SPIN_GLASS (DESIGN 4.17): examples/ising.jl with every neighbour product
multiplied by a quenched bond.  `bonds_right[i, j]` couples site (i, j) with (i, j + 1), `bonds_down[i, j]` couples (i, j) with (i + 1, j)
(periodic), every entry +1 or -1; explorer = the Metropolis sweeps of examples/ising.jl:91-116 (n_sweeps passes)."""
struct DeviceSpinGlass; beta::Float64; bonds_right::Matrix{Int8}; bonds_down::Matrix{Int8}; n_sweeps::Int; end
"""The +-J Edwards-Anderson spin glass on the L x L x L periodic lattice, the device family PTE_TARGET_SPIN_GLASS_3D (DESIGN 4.19), L even and
in 2..32.  `bonds_x[z, y, x]` couples site (z, y, x) with (z, y, x + 1), `bonds_y[z, y, x]` with (z, y + 1, x), `bonds_z[z, y, x]` with
(z + 1, y, x) (periodic), every entry +1 or -1; explorer = CheckerboardMetropolis, n_sweeps two-colour sweeps per explore step."""
struct DeviceSpinGlass3D; beta::Float64; bonds_x::Array{Int8, 3}; bonds_y::Array{Int8, 3}; bonds_z::Array{Int8, 3}; n_sweeps::Int; end
"""A normalised mixture of K <= 8 diagonal Gaussians, the device family PTE_TARGET_GAUSSIAN_MIXTURE (DESIGN 4.8): the device form of
`DistributionLogPotential(MixtureModel([MvNormal(means[k], Diagonal(std_devs[k] .^ 2)) for k in 1:K], weights))`.  `means` and
`std_devs` are K x dim.  Used as `Inputs(target = on_mi355x(DeviceGaussianMixture(w, m, s)), reference = ScaledPrecisionNormalLogPotential(p, dim))`."""
struct DeviceGaussianMixture; weights::Vector{Float64}; means::Matrix{Float64}; std_devs::Matrix{Float64}; end
"""The posterior of a Bayesian GLM, the device family PTE_TARGET_BAYESIAN_GLM (DESIGN 4.9): prior N(0, I / p) on the d coefficients times
the likelihood of y given eta = X * theta, `likelihood` = :bernoulli_logit (logistic regression, y in {0, 1}) or :normal_identity (linear
regression with known `noise_sd`).  X is n x dim.  Used as `Inputs(target = on_mi355x(DeviceBayesianGLM(X, y, :bernoulli_logit, 1.0)),
reference = ScaledPrecisionNormalLogPotential(p, dim))` -- the reference is the prior.  stepping_stone(pt) + (dim/2) log(2 pi / p) is the
log evidence."""
struct DeviceBayesianGLM; X::Matrix{Float64}; y::Vector{Float64}; likelihood::Symbol; noise_sd::Float64; end
"""The posterior of a finite mixture model given data, the device family PTE_TARGET_MIXTURE_MODEL (DESIGN 4.11): `y` holds n real
observations of a mixture of `n_components` normals (K <= 8); the state is [mu; s; alpha] (dim = 3 K) with standard deviations exp.(s)
and weights softmax(alpha), and the prior N(0, I / p).  Used as `Inputs(target = on_mi355x(DeviceMixtureModelPosterior(y, 2)),
reference = ScaledPrecisionNormalLogPotential(p, 6))` -- the reference is the prior.  stepping_stone(pt) + (dim/2) log(2 pi / p) is the
log evidence."""
struct DeviceMixtureModelPosterior; y::Vector{Float64}; n_components::Int; end
"""Bayesian variable selection, a spike-and-slab regression: the device family PTE_TARGET_VARIABLE_SELECTION (DESIGN 4.12).  The data and
likelihoods of DeviceBayesianGLM (X is n x d) with an inclusion indicator per column: the state is [theta; gamma] (dim = 2 d, gamma stored as
0.0 / 1.0), eta = X * (gamma .* theta), prior N(0, I / p) on theta and Bernoulli(`inclusion_prob`) on every gamma_j.  Used as
`Inputs(target = on_mi355x(DeviceSpikeSlabRegression(X, y, :normal_identity, 1.0, 0.5)), reference = ScaledPrecisionNormalLogPotential(p, d),
explorer = SliceSampler())` -- SliceSampler is the one explorer of this family.  stepping_stone(pt) + (d/2) log(2 pi / p) + d log 2 is the
log evidence."""
struct DeviceSpikeSlabRegression; X::Matrix{Float64}; y::Vector{Float64}; likelihood::Symbol; noise_sd::Float64; inclusion_prob::Float64; end
"""Multiple change-point detection on count data: the device family PTE_TARGET_CHANGE_POINT (DESIGN 4.13).  n counts y, K = n_changepoints
change points; the state is [r; tau] (dim = 2 K + 1): K + 1 log rates, then K Integer change points in 0:n stored as integral Float64,
unordered -- segment j lies between the j-th and (j+1)-th smallest -- with prior N(0, I / p) on r and uniform on every tau.  Used as
`Inputs(target = on_mi355x(DevicePoissonChangePoint(y, K)), reference = ScaledPrecisionNormalLogPotential(p, K + 1), explorer =
SliceSampler())` -- SliceSampler is the one explorer of this family, and its width must be integral.
stepping_stone(pt) + ((K+1)/2) log(2 pi / p) + K log(n + 1) is the log evidence."""
struct DevicePoissonChangePoint; y::Vector{Float64}; n_changepoints::Int; end
"""The posterior of a hierarchical normal-means model ("eight schools"), the device family PTE_TARGET_HIERARCHICAL_NORMAL (DESIGN 4.14):
J group estimates `y` with known standard errors `sigma`, theta_j ~ N(mu, tau^2), mu ~ N(0, mu_sd^2), tau ~ HalfCauchy(0, tau_scale); the
state is [mu; log tau; theta] (`parameterization = :centered`) or [mu; log tau; eta] with theta = mu .+ tau .* eta (`:noncentered`),
dim = J + 2 <= 512.  Used as `Inputs(target = on_mi355x(DeviceHierarchicalNormalMeans(y, sigma, 5.0, 5.0, :noncentered)), reference =
ScaledPrecisionNormalLogPotential(p, J + 2))`.  stepping_stone(pt) + (dim/2) log(2 pi / p) is the log evidence."""
struct DeviceHierarchicalNormalMeans; y::Vector{Float64}; sigma::Vector{Float64}; mu_sd::Float64; tau_scale::Float64; parameterization::Symbol; end
"""The posterior of a latent AR(1) state-space model, the device family PTE_TARGET_LATENT_AR1 (DESIGN 4.15): T observations `y` of a latent
state h_t | h_{t-1} ~ N(mu + phi (h_{t-1} - mu), sigma^2), h_0 from the stationary law, mu ~ N(0, mu_sd^2), atanh(phi) ~ N(phi_loc, phi_scale^2),
sigma ~ HalfCauchy(0, sigma_scale), observed as y_t ~ N(0, exp(h_t)) (`likelihood = :stochastic_volatility`) or y_t ~ N(h_t, obs_sd^2)
(`:normal_identity`); the state is [mu; atanh phi; log sigma; h], dim = T + 3 <= 512.  Used as `Inputs(target =
on_mi355x(DeviceLatentAR1(y, :stochastic_volatility, 1.0, 5.0, 0.0, 1.0, 1.0)), reference = ScaledPrecisionNormalLogPotential(p, T + 3))`.
stepping_stone(pt) + (dim/2) log(2 pi / p) is the log evidence."""
struct DeviceLatentAR1; y::Vector{Float64}; likelihood::Symbol; obs_sd::Float64; mu_sd::Float64; phi_loc::Float64; phi_scale::Float64; sigma_scale::Float64; end
"""The multivariate normal N(mean, precision^-1) with a dense precision matrix, the device family PTE_TARGET_DENSE_NORMAL (DESIGN 4.16):
`precision` is dim x dim, symmetric bit for bit (pass `(Q + Q') / 2`) and positive definite, dim <= 512; the density is normalised.  Used as
`Inputs(target = on_mi355x(DeviceDenseNormal(mean, precision)), reference = ScaledPrecisionNormalLogPotential(p, dim))`.
stepping_stone(pt) + (dim/2) log(2 pi / p) estimates the log evidence, which is 0."""
struct DeviceDenseNormal; mean::Vector{Float64}; precision::Matrix{Float64}; end

# (target code, dim, target_params, reference precision check) of a wrapped target
device_family(t::ScaledPrecisionNormalPath, inputs) = (TARGET_MVN, t.dim, (t.precision0, t.precision1, 0.0, 0.0))
device_family(t::Pigeons.TestSwapper, inputs) = (TARGET_TEST_SWAPPER, 0, (t.constant_swap_accept_pr, 0.0, 0.0, 0.0))
function device_family(t::DeviceFunnel, inputs)
    ref = inputs.reference
    ref isa ScaledPrecisionNormalLogPotential && ref.dim == t.dim ||
        error("the device funnel path needs reference = ScaledPrecisionNormalLogPotential(precision, $(t.dim)); keep the CPU path otherwise")
    return (TARGET_FUNNEL, t.dim, (ref.precision, 0.0, 0.0, 0.0))
end
device_family(t::DeviceIsing, inputs) = (TARGET_ISING, t.base_length^2, (t.beta, 0.0, 0.0, 0.0))
function device_family(t::DeviceSpinGlass, inputs)
    L = size(t.bonds_right, 1)
    size(t.bonds_right) == (L, L) && size(t.bonds_down) == (L, L) && 2 <= L && L^2 <= 65536 ||
        error("DeviceSpinGlass: bonds_right and bonds_down are L x L with 2 <= L and L^2 <= 65536")
    return (TARGET_SPIN_GLASS, L^2, (t.beta, 0.0, 0.0, 0.0))
end
function device_family(t::DeviceSpinGlass3D, inputs)
    L = size(t.bonds_x, 1)
    size(t.bonds_x) == (L, L, L) && size(t.bonds_y) == (L, L, L) && size(t.bonds_z) == (L, L, L) && 2 <= L <= 32 && iseven(L) ||
        error("DeviceSpinGlass3D: bonds_x, bonds_y and bonds_z are L x L x L with L even and in 2..32")
    return (TARGET_SPIN_GLASS_3D, L^3, (t.beta, 0.0, 0.0, 0.0))
end
function device_family(t::DeviceGaussianMixture, inputs)
    K, dim = size(t.means)
    length(t.weights) == K && size(t.std_devs) == (K, dim) || error("DeviceGaussianMixture: weights [K], means and std_devs K x dim")
    ref = inputs.reference
    ref isa ScaledPrecisionNormalLogPotential && ref.dim == dim ||
        error("the device Gaussian-mixture path needs reference = ScaledPrecisionNormalLogPotential(precision, $dim); keep the CPU path otherwise")
    return (TARGET_GAUSSIAN_MIXTURE, dim, (ref.precision, 0.0, 0.0, 0.0))
end
function device_family(t::DeviceBayesianGLM, inputs)
    n, dim = size(t.X)
    length(t.y) == n || error("DeviceBayesianGLM: X is n x dim, y has the n observations")
    t.likelihood in (:bernoulli_logit, :normal_identity) || error("DeviceBayesianGLM: likelihood :bernoulli_logit or :normal_identity")
    ref = inputs.reference
    ref isa ScaledPrecisionNormalLogPotential && ref.dim == dim ||
        error("the device Bayesian-GLM path needs reference = ScaledPrecisionNormalLogPotential(precision, $dim) (the prior); keep the CPU path otherwise")
    return (TARGET_BAYESIAN_GLM, dim, (ref.precision, 0.0, 0.0, 0.0))
end
function device_family(t::DeviceMixtureModelPosterior, inputs)
    1 <= t.n_components <= 8 || error("DeviceMixtureModelPosterior: the device holds 1..8 components")
    1 <= length(t.y) <= 65536 || error("DeviceMixtureModelPosterior: the device holds 1..65536 observations")
    dim = 3 * t.n_components
    ref = inputs.reference
    ref isa ScaledPrecisionNormalLogPotential && ref.dim == dim ||
        error("the device mixture-model path needs reference = ScaledPrecisionNormalLogPotential(precision, $dim) (the prior); keep the CPU path otherwise")
    return (TARGET_MIXTURE_MODEL, dim, (ref.precision, 0.0, 0.0, 0.0))
end
function device_family(t::DeviceHierarchicalNormalMeans, inputs)
    1 <= length(t.y) <= 510 || error("DeviceHierarchicalNormalMeans: the device holds 1..510 groups")
    length(t.sigma) == length(t.y) || error("DeviceHierarchicalNormalMeans: sigma has one standard error per group")
    t.parameterization in (:centered, :noncentered) || error("DeviceHierarchicalNormalMeans: parameterization :centered or :noncentered")
    dim = length(t.y) + 2
    ref = inputs.reference
    ref isa ScaledPrecisionNormalLogPotential && ref.dim == dim ||
        error("the device hierarchical-normal path needs reference = ScaledPrecisionNormalLogPotential(precision, $dim); keep the CPU path otherwise")
    return (TARGET_HIERARCHICAL_NORMAL, dim, (ref.precision, 0.0, 0.0, 0.0))
end
function device_family(t::DeviceLatentAR1, inputs)
    1 <= length(t.y) <= 509 || error("DeviceLatentAR1: the device holds 1..509 observations")
    t.likelihood in (:stochastic_volatility, :normal_identity) || error("DeviceLatentAR1: likelihood :stochastic_volatility or :normal_identity")
    dim = length(t.y) + 3
    ref = inputs.reference
    ref isa ScaledPrecisionNormalLogPotential && ref.dim == dim ||
        error("the device latent-AR(1) path needs reference = ScaledPrecisionNormalLogPotential(precision, $dim); keep the CPU path otherwise")
    return (TARGET_LATENT_AR1, dim, (ref.precision, 0.0, 0.0, 0.0))
end
function device_family(t::DeviceDenseNormal, inputs)
    dim = length(t.mean)
    1 <= dim <= 512 || error("DeviceDenseNormal: the device holds 1..512 coordinates")
    size(t.precision) == (dim, dim) || error("DeviceDenseNormal: precision is dim x dim, mean has the dim entries")
    ref = inputs.reference
    ref isa ScaledPrecisionNormalLogPotential && ref.dim == dim ||
        error("the device dense-normal path needs reference = ScaledPrecisionNormalLogPotential(precision, $dim); keep the CPU path otherwise")
    return (TARGET_DENSE_NORMAL, dim, (ref.precision, 0.0, 0.0, 0.0))
end
function device_family(t::DeviceSpikeSlabRegression, inputs)
    n, d = size(t.X)
    length(t.y) == n || error("DeviceSpikeSlabRegression: X is n x d, y has the n observations")
    t.likelihood in (:bernoulli_logit, :normal_identity) || error("DeviceSpikeSlabRegression: likelihood :bernoulli_logit or :normal_identity")
    1 <= d <= 256 || error("DeviceSpikeSlabRegression: the device holds 1..256 columns")
    0 < t.inclusion_prob < 1 || error("DeviceSpikeSlabRegression: inclusion_prob must be in (0, 1)")
    ref = inputs.reference
    ref isa ScaledPrecisionNormalLogPotential && ref.dim == d ||
        error("the device variable-selection path needs reference = ScaledPrecisionNormalLogPotential(precision, $d) (the prior of the coefficients); keep the CPU path otherwise")
    return (TARGET_VARIABLE_SELECTION, 2 * d, (ref.precision, 0.0, 0.0, 0.0))
end
function device_family(t::DevicePoissonChangePoint, inputs)
    K = t.n_changepoints
    1 <= K <= 63 || error("DevicePoissonChangePoint: the device holds 1..63 change points")
    1 <= length(t.y) <= 65536 || error("DevicePoissonChangePoint: the device holds 1..65536 observations")
    all(v -> isinteger(v) && 0 <= v <= 2^20, t.y) || error("DevicePoissonChangePoint: every y must be an integer count in 0..2^20")
    ref = inputs.reference
    ref isa ScaledPrecisionNormalLogPotential && ref.dim == K + 1 ||
        error("the device change-point path needs reference = ScaledPrecisionNormalLogPotential(precision, $(K + 1)) (the prior of the log rates); keep the CPU path otherwise")
    return (TARGET_CHANGE_POINT, 2 * K + 1, (ref.precision, 0.0, 0.0, 0.0))
end
device_family(t, inputs) = error("target $(typeof(t)) has no device log-potential family (closed set: include/pte.h PTE_TARGET_*); keep the CPU path")

# explorer structs -> pte_config fields (SliceSampler.jl:8-20, AutoMALA.jl:29-68, MALA.jl:19-40, Compose.jl:5-9)
preconditioner_code(::Pigeons.IdentityPreconditioner) = Int32(0)
preconditioner_code(::Pigeons.DiagonalPreconditioner) = Int32(1)
preconditioner_code(p::Pigeons.MixDiagonalPreconditioner) = Int32(2)
function set_explorer!(cfg::PteConfig, ex::SliceSampler, slot)
    cfg.slice_w = ex.w; cfg.slice_p = ex.p; cfg.slice_n_passes = ex.n_passes; cfg.slice_max_iter = ex.max_iter
    return EXPLORER_SLICE
end
set_explorer!(cfg::PteConfig, ::ToyExplorer, slot) = EXPLORER_TOY
function set_explorer!(cfg::PteConfig, ex::AutoMALA, slot)
    cfg.am_base_n_refresh = ex.base_n_refresh; cfg.am_exponent_n_refresh = ex.exponent_n_refresh; cfg.am_step_size = ex.step_size
    cfg.am_preconditioner = preconditioner_code(ex.preconditioner)
    if ex.preconditioner isa Pigeons.MixDiagonalPreconditioner
        cfg.am_p0 = ex.preconditioner.p0; cfg.am_p1 = ex.preconditioner.p1
    end
    return EXPLORER_AUTOMALA
end
function set_explorer!(cfg::PteConfig, ex::MALA, slot)
    cfg.am_base_n_refresh = ex.base_n_refresh; cfg.am_exponent_n_refresh = ex.exponent_n_refresh; cfg.am_step_size = ex.step_size
    cfg.am_preconditioner = preconditioner_code(ex.preconditioner)
    return EXPLORER_MALA
end
function set_explorer!(cfg::PteConfig, ex::Pigeons.AAPS, slot)       # step size fixed; AAPS alone (pte_create refuses it inside a Compose)
    cfg.am_step_size = ex.step_size; cfg.aaps_K = ex.K
    cfg.am_preconditioner = preconditioner_code(ex.preconditioner)
    if ex.preconditioner isa Pigeons.MixDiagonalPreconditioner
        cfg.am_p0 = ex.preconditioner.p0; cfg.am_p1 = ex.preconditioner.p1
    end
    return EXPLORER_AAPS
end
set_explorer!(cfg::PteConfig, ::Nothing, slot) = EXPLORER_NONE
set_explorer!(cfg::PteConfig, ex, slot) = error("explorer $(typeof(ex)) has no device kernel; keep the CPU path")

# Inputs.record (recorder builder functions, src/pt/Inputs.jl:57-62) -> PTE_RECORD_*
function record_flags(inputs::Inputs, shared::Shared)
    names = Set(Symbol(b) for b in Pigeons.recorder_builders(inputs, shared))
    f = UInt32(0)
    :round_trip in names && (f |= RECORD_ROUND_TRIP)
    :index_process in names && (f |= RECORD_INDEX_PROCESS)
    (:online in names || :_transformed_online in names) && (f |= RECORD_ONLINE)
    :traces in names && (f |= RECORD_TRACES)
    (:traces in names && inputs.extended_traces) && (f |= RECORD_TRACES_EXTENDED)
    :energy_ac1 in names && (f |= RECORD_ENERGY_AC1)
    :disk in names && error("the disk recorder is not served by the device path (SURVEY.md 2: out of scope)")
    # on_mi355x(target; reference_reduction = true): the reference's own reduction arithmetic for the swap recorders (and :online when :traces is recorded)
    (inputs.target isa OnDevice && inputs.target.reference_reduction) && (f |= RECORD_REFERENCE_REDUCTION | RECORD_INDEX_PROCESS)
    return f
end

# ---- replicas (informal interface src/replicas/replicas.jl:11-40) ------------------------------------------------------------
"""Device-resident `replicas`.  `host_recorders` receives what the host itself records (timing, allocations)."""
mutable struct DeviceReplicas
    handle::Ptr{Cvoid}
    n_chains::Int          # all chains (both legs of a StabilizedPT)
    dim::Int
    first_chain::Int       # 0-based, this rank's shard
    n_local::Int
    world_size::Int
    record_flags::UInt32
    host_recorders
end
"""What `locals(replicas)` iterates over: ALL local replicas as one unit of work (explore! is one launch, not a loop)."""
struct DeviceBatch
    replicas::DeviceReplicas
end
Base.getproperty(b::DeviceBatch, s::Symbol) =          # the two fields generic code reads off `locals(pt.replicas)[1]`
    s === :recorders ? getfield(b, :replicas).host_recorders :
    s === :state ? replica_state(getfield(b, :replicas), 1) : getfield(b, s)

Pigeons.locals(r::DeviceReplicas) = (DeviceBatch(r),)
Pigeons.load(r::DeviceReplicas) = Pigeons.single_process_load(r.n_chains)
Pigeons.entangler(r::DeviceReplicas) = Pigeons.Entangler(r.n_chains; parent_communicator = nothing)   # (only `.load` is read off it)

function check(r::DeviceReplicas, rc::Cint)
    rc == 0 && return
    msg = unsafe_string(ccall((:pte_last_error, libpte), Cstring, (Ptr{Cvoid},), r.handle))
    error(msg)    # same wording class as the reference's exceptions (SliceSampler.jl:52-60,179-185)
end

# create_replicas(inputs, shared, source)  (src/replicas/replicas.jl:65-98) -- the method PT(inputs) calls
function Pigeons.create_replicas(inputs::Inputs{<:OnDevice}, shared::Shared, source = nothing)
    t = inputs.target
    code, dim, params = device_family(t.target, inputs)
    N = inputs.n_chains
    cfg = PteConfig(device = t.device, target = code, n_chains = N, dim = dim, seed = inputs.seed,
                    max_scans_per_round = 2^inputs.n_rounds, target_params = params,
                    n_chains_variational = inputs.n_chains_variational, rank = t.rank, world_size = t.world_size)
    cfg.struct_size = sizeof(PteConfig)
    ex = shared.explorer
    if t.target isa DeviceIsing || t.target isa DeviceSpinGlass
        cfg.explorer = EXPLORER_ISING; cfg.slice_n_passes = t.target.n_sweeps
    elseif t.target isa DeviceSpinGlass3D
        cfg.explorer = EXPLORER_CHECKERBOARD_METROPOLIS; cfg.slice_n_passes = t.target.n_sweeps
    elseif ex isa Compose
        cfg.explorer = set_explorer!(cfg, ex.first, 1); cfg.explorer2 = set_explorer!(cfg, ex.second, 2)
    else
        cfg.explorer = set_explorer!(cfg, ex, 1)
    end
    cfg.record_flags = record_flags(inputs, shared)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    rc = ccall((:pte_create, libpte), Cint, (Ref{PteConfig}, Ref{Ptr{Cvoid}}), cfg, h)
    rc == 0 || error(unsafe_string(ccall((:pte_last_error, libpte), Cstring, (Ptr{Cvoid},), C_NULL)))
    info = zeros(Int64, 3)
    ccall((:pte_shard_info, libpte), Cint, (Ptr{Cvoid}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}), h[], pointer(info, 1), pointer(info, 2), pointer(info, 3))
    r = DeviceReplicas(h[], N + inputs.n_chains_variational, dim, info[1], info[2], t.world_size, cfg.record_flags,
                       Pigeons.create_recorders(inputs, shared))
    finalizer(x -> ccall((:pte_destroy, libpte), Cint, (Ptr{Cvoid},), x.handle), r)
    if t.target isa DeviceGaussianMixture           # the components, row-major [K][dim] as pte_set_target_mixture reads them
        m = t.target
        check(r, ccall((:pte_set_target_mixture, libpte), Cint, (Ptr{Cvoid}, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                       r.handle, length(m.weights), m.weights, collect(vec(permutedims(m.means))), collect(vec(permutedims(m.std_devs)))))
    end
    if t.target isa DeviceBayesianGLM               # the data, X row-major [n][dim] as pte_set_target_glm reads it
        g = t.target
        lik = g.likelihood === :normal_identity ? GLM_NORMAL_IDENTITY : GLM_BERNOULLI_LOGIT
        check(r, ccall((:pte_set_target_glm, libpte), Cint, (Ptr{Cvoid}, Int32, Int64, Ptr{Float64}, Ptr{Float64}, Float64),
                       r.handle, lik, length(g.y), collect(vec(permutedims(g.X))), g.y, g.noise_sd))
    end
    if t.target isa DeviceMixtureModelPosterior     # the observations as pte_set_target_mixture_model reads them
        check(r, ccall((:pte_set_target_mixture_model, libpte), Cint, (Ptr{Cvoid}, Int64, Ptr{Float64}), r.handle, length(t.target.y), t.target.y))
    end
    if t.target isa DeviceSpikeSlabRegression       # the data, X row-major [n][d] as pte_set_target_varsel reads it
        g = t.target
        lik = g.likelihood === :normal_identity ? GLM_NORMAL_IDENTITY : GLM_BERNOULLI_LOGIT
        check(r, ccall((:pte_set_target_varsel, libpte), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Int64, Int64, Int32, Float64, Float64),
                       r.handle, collect(vec(permutedims(g.X))), g.y, length(g.y), size(g.X, 2), lik, g.noise_sd, g.inclusion_prob))
    end
    if t.target isa DeviceHierarchicalNormalMeans   # the groups' estimates and standard errors as pte_set_target_hier reads them
        g = t.target
        par = g.parameterization === :noncentered ? HIER_NONCENTERED : HIER_CENTERED
        check(r, ccall((:pte_set_target_hier, libpte), Cint, (Ptr{Cvoid}, Int32, Int64, Ptr{Float64}, Ptr{Float64}, Float64, Float64),
                       r.handle, par, length(g.y), g.y, g.sigma, g.mu_sd, g.tau_scale))
    end
    if t.target isa DeviceLatentAR1                 # the observations and the priors as pte_set_target_ar1 reads them
        g = t.target
        lik = g.likelihood === :normal_identity ? AR1_NORMAL_IDENTITY : AR1_STOCHASTIC_VOLATILITY
        check(r, ccall((:pte_set_target_ar1, libpte), Cint, (Ptr{Cvoid}, Int32, Int64, Ptr{Float64}, Float64, Float64, Float64, Float64, Float64),
                       r.handle, lik, length(g.y), g.y, g.obs_sd, g.mu_sd, g.phi_loc, g.phi_scale, g.sigma_scale))
    end
    if t.target isa DeviceDenseNormal               # the mean and the precision matrix as pte_set_target_dense reads them
        g = t.target
        Q = Matrix{Float64}(permutedims(g.precision))     # row-major for the C ABI (the matrix is symmetric: the same bits)
        check(r, ccall((:pte_set_target_dense, libpte), Cint, (Ptr{Cvoid}, Int64, Ptr{Float64}, Ptr{Float64}), r.handle, length(g.mean), g.mean, Q))
    end
    if t.target isa DeviceSpinGlass                 # the bond planes as pte_set_target_spin_glass reads them
        g = t.target
        R = Matrix{Int8}(permutedims(g.bonds_right)); D = Matrix{Int8}(permutedims(g.bonds_down))     # row-major for the C ABI
        check(r, ccall((:pte_set_target_spin_glass, libpte), Cint, (Ptr{Cvoid}, Int64, Ptr{Int8}, Ptr{Int8}), r.handle, size(R, 1), R, D))
    end
    if t.target isa DeviceSpinGlass3D               # the bond planes as pte_set_target_spin_glass_3d reads them
        g = t.target
        c_order(A) = Array{Int8, 3}(permutedims(A, (3, 2, 1)))     # [z, y, x] column-major -> [z][y][x] row-major for the C ABI
        X = c_order(g.bonds_x); Y = c_order(g.bonds_y); Z = c_order(g.bonds_z)
        check(r, ccall((:pte_set_target_spin_glass_3d, libpte), Cint, (Ptr{Cvoid}, Int64, Ptr{Int8}, Ptr{Int8}, Ptr{Int8}), r.handle, size(X, 1), X, Y, Z))
    end
    if t.target isa DevicePoissonChangePoint        # the counts as pte_set_target_changepoint reads them
        check(r, ccall((:pte_set_target_changepoint, libpte), Cint, (Ptr{Cvoid}, Ptr{Float64}, Int64), r.handle, t.target.y, length(t.target.y)))
    end
    source === nothing || restore!(r, source)          # FromCheckpoint: pte_set_state from the deserialised Replica structs
    return r
end

# checkpoint fields of Replica (src/pt/checkpoint.jl:110-145): state, chain (1-based on this side), rng words
function replica_states(r::DeviceReplicas)
    x = zeros(r.dim, r.n_local); chain = zeros(Int64, r.n_local); rng = zeros(UInt64, 2, r.n_local)
    check(r, ccall((:pte_get_state, libpte), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Int64}, Ptr{UInt64}), r.handle, x, chain, rng))
    return x, chain .+ 1, rng
end
replica_state(r::DeviceReplicas, i::Int) = replica_states(r)[1][:, i]
function restore!(r::DeviceReplicas, source::Pigeons.FromCheckpoint)
    reps = [Pigeons.deserialize("$(source.checkpoint_folder)/replica=$i.jls") for i in (r.first_chain + 1):(r.first_chain + r.n_local)]
    x = reduce(hcat, [Float64.(rep.state) for rep in reps]); chain = Int64[rep.chain - 1 for rep in reps]
    rng = reduce(hcat, [UInt64[rep.rng.seed, rep.rng.gamma] for rep in reps])
    check(r, ccall((:pte_set_state, libpte), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Int64}, Ptr{UInt64}), r.handle, x, chain, rng))
end

# ---- the hot path ----------------------------------------------------------------------------------------------------------
# explore!(pt, replica, explorer)  (src/pt/pigeons.jl:101-143): one ccall for ALL local replicas; the bookkeeping around the
# explorer (energy_ac1, online, traces) is fused into the kernels (record_flags)
function Pigeons.explore!(pt, b::DeviceBatch, explorer)
    pt.shared.iterators.scan == 1 && after_adapt!(pt)   # first scan of a round: what adapt() decided reaches the device here
    check(b.replicas, ccall((:pte_explore, libpte), Cint, (Ptr{Cvoid}, Int64), b.replicas.handle, pt.shared.iterators.scan))
end

# swap!(pair_swapper, replicas, swap_graph)  (src/swap/swap.jl:6-39): the DEO parity is iseven(scan) (src/swap/DEO.jl:12);
# OddEven and VariationalOddEven (src/swap/OddEven.jl) both carry it in `.even`
Pigeons.swap!(pair_swapper, r::DeviceReplicas, swap_graph) =
    check(r, ccall((:pte_swap, libpte), Cint, (Ptr{Cvoid}, Int64), r.handle, swap_graph.even ? 2 : 1))

# run_one_round!: the fused `while next_scan!` loop (src/pt/pigeons.jl:46-55), one ccall per round.  Optional: without this method
# the reference's own loop runs with the two hooks above.  PT's first type parameter is its `inputs` field (src/pt/PT.jl:6-12).
@assert fieldnames(PT)[1] === :inputs "PT's field order changed: re-derive the dispatch of the fused run_one_round!"
function Pigeons.run_one_round!(pt::PT{<:Inputs{<:OnDevice}})
    r = pt.replicas::DeviceReplicas
    n = Pigeons.n_scans_in_round(pt.shared.iterators)
    after_adapt!(pt)                                    # the schedule / explorer parameters of this round
    timed = @timed check(r, ccall((:pte_run_scans, libpte), Cint, (Ptr{Cvoid}, Int64, Int64), r.handle, 1, n))
    pt.shared.iterators.scan = 0
    Pigeons.record_timed_if_requested!(r.host_recorders, :round, timed)
    return Pigeons.reduce_recorders!(pt, r)
end

# Which form pte_run_scans takes on this engine (round 5): "" = an explore and a swap launch per scan; otherwise the ONE kernel that runs all the
# scans of the call ("k_scans_slice8", "k_scans_automala": workgroup c keeps chain c, the DEO swap of a pair is a hand-shake between its two
# waves; "k_scans_automala_wg": four consecutive chains per workgroup, inner pairs shake hands through LDS).  Results are bit-identical
# either way; `debug_kernel = PTE_KERNEL_TWO_LAUNCHES` (0x1000) in the config forces the per-scan loop, `PTE_KERNEL_SCAN_LOOP_ONE_CHAIN`
# (0x2000) the one-chain-per-workgroup form of the one-kernel loop.
scan_loop_name(r::DeviceReplicas) = unsafe_string(ccall((:pte_scan_loop_name, libpte), Cstring, (Ptr{Cvoid},), r.handle))
# Round 6: the one kernel cannot hang (residency gate inside the launch, fallback to the launch-per-scan loop: include/pte.h, pte_scan_loop_stats).
# (fused_calls, gate_aborts, poisoned): calls that ran as one launch; launches that found a workgroup missing and fell back (same results); whether
# a failure inside the kernel has poisoned the handle -- then only `pte_set_state` (a checkpoint's state, chain, rng) or `pte_destroy` are accepted.
function scan_loop_stats(r::DeviceReplicas)
    f = Ref{Int64}(0); a = Ref{Int64}(0); p = Ref{Int32}(0)
    check(r, ccall((:pte_scan_loop_stats, libpte), Cint, (Ptr{Cvoid}, Ref{Int64}, Ref{Int64}, Ref{Int32}), r.handle, f, a, p))
    return (fused_calls = f[], gate_aborts = a[], poisoned = p[] != 0)
end

# adapt(pt, reduced_recorders) ran on the host (adapt_tempering: src/tempering/NonReversiblePT.jl:46-66, StabilizedPT.jl:53-65;
# adapt_explorer: AutoMALA.jl:70-79, MALA.jl:63-69, Compose.jl:10-14; update_reference!: GaussianReference.jl:24-31): push the results
function after_adapt!(pt)
    r = pt.replicas::DeviceReplicas
    tempering = pt.shared.tempering
    betas = tempering isa Pigeons.StabilizedPT ?
        vcat(tempering.variational_leg.schedule.grids, reverse(tempering.fixed_leg.schedule.grids)) :   # concatenate_log_potentials order
        tempering.schedule.grids
    check(r, ccall((:pte_set_schedule, libpte), Cint, (Ptr{Cvoid}, Ptr{Float64}, Int64), r.handle, betas, length(betas)))
    for ex in explorers(pt.shared.explorer)
        ex isa Union{AutoMALA, MALA, Pigeons.AAPS} || continue
        std = ex.estimated_target_std_deviations
        check(r, ccall((:pte_set_explorer_adaptation, libpte), Cint, (Ptr{Cvoid}, Float64, Ptr{Float64}, Int64), r.handle, ex.step_size,
                       std === nothing ? C_NULL : pointer(std), std === nothing ? 0 : length(std)))
    end
    v = pt.inputs.variational
    if v isa Pigeons.GaussianReference && !isempty(v.mean)
        m = v.mean[:singleton_variable]; s = v.standard_deviation[:singleton_variable]
        uses = Int32[c <= pt.inputs.n_chains_variational || pt.inputs.n_chains_variational == 0 ? 1 : 0 for c in 1:r.n_chains]
        check(r, ccall((:pte_set_variational_reference, libpte), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Int64, Ptr{Int32}),
                       r.handle, m, s, length(m), uses))
    end
end
explorers(e::Compose) = (e.first, e.second)
explorers(e) = (e,)

# ---- reduce_recorders!(pt, replicas)  (src/recorders/recorders.jl:88-130): rebuild every recorder from the flat arrays ----------
# Keys are 1-based chains / replica indices on this side.  The device keeps per-pair / per-chain sums where the reference merges
# per-replica OnlineStats in a tree (src/mpi_utils/Entangler.jl:188-251): integers are identical, floats agree to 1e-9.
function Pigeons.reduce_recorders!(pt, r::DeviceReplicas)
    check(r, ccall((:pte_reduce, libpte), Cint, (Ptr{Cvoid},), r.handle))
    rec = Pigeons.create_recorders(pt.inputs, pt.shared)
    N, K, c0 = r.n_chains, r.n_local, r.first_chain
    has(name) = haskey(rec, name)
    # swap_acceptance_pr: GroupBy(Tuple{Int,Int}, Mean()); log_sum_ratio: GroupBy(Tuple{Int,Int}, LogSum()) (recorder.jl:54,84)
    np = r.world_size == 1 ? N - 1 : K
    mean = zeros(np); n = zeros(Int64, np)
    check(r, ccall((:pte_get_swap_acceptance, libpte), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Int64}), r.handle, mean, n))
    up = zeros(np); dn = zeros(np); un = zeros(Int64, np); dnn = zeros(Int64, np)
    check(r, ccall((:pte_get_log_sum_ratio, libpte), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Int64}, Ptr{Float64}, Ptr{Int64}), r.handle, up, un, dn, dnn))
    for i in 1:np
        c = c0 + i                                       # lower chain of the pair, 1-based
        if has(:swap_acceptance_pr) && n[i] > 0
            put!(rec.swap_acceptance_pr, (c, c + 1), Mean(mean[i], EqualWeight(), n[i]), n[i])
        end
        if has(:log_sum_ratio) && un[i] > 0
            put!(rec.log_sum_ratio, (c, c + 1), LogSum(up[i], un[i]), un[i])
            put!(rec.log_sum_ratio, (c + 1, c), LogSum(dn[i], dnn[i]), dnn[i])
        end
    end
    # round_trip (RoundTripRecorder.jl:4-19): the per-replica state machines live on the device, the counts are already summed
    if has(:round_trip)
        a = Ref{Int64}(0); b = Ref{Int64}(0)
        check(r, ccall((:pte_get_round_trip, libpte), Cint, (Ptr{Cvoid}, Ref{Int64}, Ref{Int64}), r.handle, a, b))
        rec.round_trip.n_tempered_restarts = a[]; rec.round_trip.n_round_trips = b[]
    end
    # index_process: Dict{Int, Vector{Int}}, replica index => chain at every scan (recorder.jl:81; swap.jl:115)
    if has(:index_process)
        S = Pigeons.n_scans_in_round(pt.shared.iterators)
        ip = zeros(Int64, S, N); ns = Ref{Int64}(0)      # C layout [replica][scan] == column-major (scan, replica)
        check(r, ccall((:pte_get_index_process, libpte), Cint, (Ptr{Cvoid}, Ptr{Int64}, Ref{Int64}), r.handle, ip, ns))
        for i in 1:N
            rec.index_process[i] = ip[1:ns[], i] .+ 1
        end
    end
    # explorer_acceptance_pr: GroupBy(Int, Mean()); explorer_n_steps: GroupBy(Int, Sum()) (recorder.jl:61,68)
    am = zeros(K); an = zeros(Int64, K); ss = zeros(K); sn = zeros(Int64, K)
    check(r, ccall((:pte_get_explorer_stats, libpte), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Int64}, Ptr{Float64}, Ptr{Int64}), r.handle, am, an, ss, sn))
    for i in 1:K
        has(:explorer_acceptance_pr) && an[i] > 0 && put!(rec.explorer_acceptance_pr, c0 + i, Mean(am[i], EqualWeight(), an[i]), an[i])
        has(:explorer_n_steps) && sn[i] > 0 && put!(rec.explorer_n_steps, c0 + i, Sum(ss[i], sn[i]), sn[i])
    end
    # am_factors, reversibility_rate: GroupBy(Int, Mean()) (AutoMALA.jl:277,294)
    if has(:am_factors) || has(:reversibility_rate)
        fm = zeros(K); fn = zeros(Int64, K); rm = zeros(K); rn = zeros(Int64, K)
        check(r, ccall((:pte_get_automala_stats, libpte), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Int64}, Ptr{Float64}, Ptr{Int64}), r.handle, fm, fn, rm, rn))
        for i in 1:K
            has(:am_factors) && fn[i] > 0 && put!(rec.am_factors, c0 + i, Mean(fm[i], EqualWeight(), fn[i]), fn[i])
            has(:reversibility_rate) && rn[i] > 0 && put!(rec.reversibility_rate, c0 + i, Mean(rm[i], EqualWeight(), rn[i]), rn[i])
        end
    end
    # online / _transformed_online: OnlineStateRecorder, stats[(:singleton_variable => Mean / Variance)] = Group of d + 1 stats of
    # extract_sample(state, lp) = [state; lp]  (OnlineStateRecorder.jl:95-110, src/pt/state.jl:79)
    for name in (:online, :_transformed_online)
        has(name) || continue
        m = zeros(r.dim); v = zeros(r.dim); cnt = Ref{Int64}(0); lm = Ref{Float64}(0.0); lv = Ref{Float64}(0.0)
        check(r, ccall((:pte_get_online, libpte), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ref{Int64}), r.handle, m, v, cnt))
        cnt[] > 0 || continue
        check(r, ccall((:pte_get_online_log_density, libpte), Cint, (Ptr{Cvoid}, Ref{Float64}, Ref{Float64}), r.handle, lm, lv))
        ms = name === :online ? vcat(m, lm[]) : m; vs = name === :online ? vcat(v, lv[]) : v
        stats = getproperty(rec, name).stats
        stats[Pair(:singleton_variable, Mean)] = Group([Mean(ms[i], EqualWeight(), cnt[]) for i in eachindex(ms)])
        stats[Pair(:singleton_variable, Variance)] = Group([Variance(vs[i], ms[i], EqualWeight(), cnt[]) for i in eachindex(ms)])
    end
    # energy_ac1: GroupBy(Int, CovMatrix(2)) of (lp before, lp after) per chain (recorder.jl:113; pigeons.jl:134-143)
    if has(:energy_ac1)
        cor = zeros(K); en = zeros(Int64, K); mom = zeros(5, K)
        check(r, ccall((:pte_get_energy_ac1, libpte), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Int64}, Ptr{Float64}), r.handle, cor, en, mom))
        for i in 1:K
            en[i] > 0 || continue
            mb, ma, cbb, cba, caa = mom[:, i]            # running means and co-moment sums (Welford)
            o = CovMatrix(2)
            o.b .= (mb, ma); o.n = en[i]                 # OnlineStatsBase 1.x: A = running mean of x x', b = running mean
            o.A .= [cbb / en[i] + mb^2  cba / en[i] + mb * ma; cba / en[i] + mb * ma  caa / en[i] + ma^2]
            put!(rec.energy_ac1, c0 + i, o, en[i])
        end
    end
    # traces: Dict{Pair{Int,Int}, Any}, (chain => scan) => [state; lp] (recorder.jl:27,39-43)
    if has(:traces)
        rows = (r.record_flags & RECORD_TRACES_EXTENDED) != 0 ? K : (pt.inputs.n_chains_variational > 0 ? 2 : 1)
        S = Pigeons.n_scans_in_round(pt.shared.iterators)
        buf = zeros(r.dim + 1, rows, S); ns = Ref{Int64}(0)
        check(r, ccall((:pte_get_traces, libpte), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ref{Int64}), r.handle, buf, ns))
        chains = rows == K ? collect((c0 + 1):(c0 + K)) : target_chains(pt)
        for s in 1:ns[], (j, c) in enumerate(chains)
            rec.traces[c => s] = buf[:, j, s]
        end
    end
    # what the host itself recorded this round (timing_extrema, allocation_extrema): merge, then reset (recorders.jl:121-125)
    for name in (:timing_extrema, :allocation_extrema)
        has(name) && haskey(r.host_recorders, name) || continue
        rec = merge(rec, NamedTuple{(name,)}((merge(getproperty(rec, name), getproperty(r.host_recorders, name)),)))
        empty!(getproperty(r.host_recorders, name))
    end
    return rec
end
# a GroupBy{T,S} keeps `value::OrderedDict{T,S}` and the total count `n`
function put!(g::GroupBy, key, stat, n)
    g.value[key] = stat
    g.n += n
end
target_chains(pt) = [c for c in 1:Pigeons.n_chains(pt.inputs) if Pigeons.is_target(pt.shared.tempering.swap_graphs, c)]

# ---- distributed runs: one Julia process per GPU (the reference's MPI layout, docs/src/distributed.md), chains sharded ----------
# The reference's transport (src/mpi_utils/Entangler.jl:118-180 `transmit!`, swap! over EntangledReplicas src/swap/swap.jl:79-102)
# is replaced by RCCL send/recv that libpte enqueues itself; Julia only hands the 128-byte communicator id around once:
#
#     id = zeros(UInt8, 128)
#     MPI.Comm_rank(comm) == 0 && ccall((:pte_comm_unique_id, libpte), Cint, (Ptr{UInt8},), id)
#     MPI.Bcast!(id, 0, comm)
#     pt = PT(Inputs(target = on_mi355x(toy_mvn_target(4096); device = local_rank, rank = MPI.Comm_rank(comm), world_size = MPI.Comm_size(comm)), ...))
#     comm_init!(pt.replicas, id)                        # collective: ncclCommInitRank inside libpte
#
# and from then on run_one_round! above is unchanged: pte_run_scans on a sharded engine performs explore, the two swap phases and
# the boundary exchange (one {SwapStat, payload} message per active side and scan) on the engine's HIP stream.  The per-rank
# recorder slices (keyed by chain / pair) are concatenated in rank order -- that IS the deterministic reduction of
# all_reduce_deterministically -- with `allgather` below or MPI.Allgatherv.
comm_init!(r::DeviceReplicas, id::Vector{UInt8}) =
    check(r, ccall((:pte_comm_init, libpte), Cint, (Ptr{Cvoid}, Ptr{UInt8}), r.handle, id))
function allgather(r::DeviceReplicas, mine::Vector{UInt8})
    out = zeros(UInt8, length(mine) * r.world_size)
    check(r, ccall((:pte_comm_allgather, libpte), Cint, (Ptr{Cvoid}, Ptr{UInt8}, Int64, Ptr{UInt8}), r.handle, mine, length(mine), out))
    return out
end
barrier(r::DeviceReplicas) = check(r, ccall((:pte_comm_barrier, libpte), Cint, (Ptr{Cvoid},), r.handle))

# One Julia process driving G GPUs (no MPI at all): G engines with rank = g - 1, world_size = G, device = g - 1
function run_scans_group!(rs::Vector{DeviceReplicas}, first_scan, n_scans)
    hs = [r.handle for r in rs]
    check(rs[1], ccall((:pte_group_run_scans, libpte), Cint, (Ptr{Ptr{Cvoid}}, Int32, Int64, Int64), hs, length(hs), first_scan, n_scans))
end

# ---- the replica overlap between two runs of a lattice family (include/pte.h pte_overlap_*; DESIGN 4.20) -----------------------
"""The overlap recorder over two `DeviceReplicas` of the same lattice model (same bonds, N and schedule; different seeds).  It holds no
state of either; `close!` leaves both usable.  `n_links == 0`: no link overlap is recorded on this lattice."""
mutable struct DeviceOverlap
    handle::Ptr{Cvoid}
    a::DeviceReplicas
    b::DeviceReplicas
    n_chains::Int
    dim::Int
    n_links::Int
end
function DeviceOverlap(a::DeviceReplicas, b::DeviceReplicas)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    rc = ccall((:pte_overlap_create, libpte), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Ptr{Cvoid}}), a.handle, b.handle, h)
    rc == 0 || error(unsafe_string(ccall((:pte_last_error, libpte), Cstring, (Ptr{Cvoid},), C_NULL)))
    n, d, nl = Ref{Int64}(0), Ref{Int64}(0), Ref{Int64}(0)
    check(a, ccall((:pte_overlap_info, libpte), Cint, (Ptr{Cvoid}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}), h[], n, d, nl))
    return DeviceOverlap(h[], a, b, n[], d[], nl[])
end
close!(o::DeviceOverlap) = (ccall((:pte_overlap_destroy, libpte), Cint, (Ptr{Cvoid},), o.handle); o.handle = C_NULL; nothing)
record!(o::DeviceOverlap) = check(o.a, ccall((:pte_overlap_record, libpte), Cint, (Ptr{Cvoid},), o.handle))
run_scans!(o::DeviceOverlap, first_scan, n_scans) =
    check(o.a, ccall((:pte_overlap_run_scans, libpte), Cint, (Ptr{Cvoid}, Int64, Int64), o.handle, first_scan, n_scans))
"""-> (n, hist [d + 1, N] (column c = chain c), link_n, link_sum, link_sum2), all Int64; the device's accumulators start again from zero"""
function reduce!(o::DeviceOverlap)
    check(o.a, ccall((:pte_overlap_reduce, libpte), Cint, (Ptr{Cvoid},), o.handle))
    n, ln, ls, ls2 = (zeros(Int64, o.n_chains) for _ in 1:4)
    hist = zeros(Int64, o.dim + 1, o.n_chains)          # the ABI's row-major [N][d + 1]
    check(o.a, ccall((:pte_overlap_get, libpte), Cint, (Ptr{Cvoid}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}), o.handle, n, hist, ln, ls, ls2))
    return (n = n, hist = hist, link_n = ln, link_sum = ls, link_sum2 = ls2)
end

# Houdayer's cluster move between the two copies (include/pte.h pte_overlap_*cluster*; DESIGN 4.21)
"""`every = 0` turns the move off; otherwise `run_scans!` makes it at every scan `s` with `s % every == 0`, on the chains with
`betas[c] >= min_beta`.  The move draws from a stream of its own, keyed by `seed`."""
set_cluster_move!(o::DeviceOverlap; every = 1, min_beta = 0.0, seed = 1) =
    check(o.a, ccall((:pte_overlap_set_cluster_move, libpte), Cint, (Ptr{Cvoid}, Int64, Cdouble, UInt64), o.handle, every, min_beta, seed))
cluster_move!(o::DeviceOverlap) = check(o.a, ccall((:pte_overlap_cluster_move, libpte), Cint, (Ptr{Cvoid},), o.handle))
"""-> the cluster accumulators of the last `reduce!`, all Int64 and keyed by chain, and the number of launches they cover"""
function cluster_record(o::DeviceOverlap)
    n, empty, size_sum, k_sum, abs_ds_sum, passes_sum = (zeros(Int64, o.n_chains) for _ in 1:6)
    launched = Ref{Int64}(0)
    check(o.a, ccall((:pte_overlap_cluster_get, libpte), Cint,
                     (Ptr{Cvoid}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}),
                     o.handle, n, empty, size_sum, k_sum, abs_ds_sum, passes_sum, launched))
    return (n = n, empty = empty, size_sum = size_sum, k_sum = k_sum, abs_ds_sum = abs_ds_sum, passes_sum = passes_sum, moves_launched = launched[])
end

# the plane autocorrelation of the overlap field (include/pte.h pte_overlap_*planes*; DESIGN 4.22): chi_SG(k) along the axes and xi_L
"""`on = true`: every record from now on also adds the plane autocorrelation; refused on a 2-D lattice whose base length is not a
multiple of 32."""
set_planes!(o::DeviceOverlap, on::Bool = true) = check(o.a, ccall((:pte_overlap_set_planes, libpte), Cint, (Ptr{Cvoid}, Cint), o.handle, on ? 1 : 0))
"""-> (n_axes, base_length, on); `n_axes == 0`: the plane sums are not recorded on this lattice"""
function planes_info(o::DeviceOverlap)
    na, bl, on = Ref{Int64}(0), Ref{Int64}(0), Ref{Int64}(0)
    check(o.a, ccall((:pte_overlap_planes_info, libpte), Cint, (Ptr{Cvoid}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}), o.handle, na, bl, on))
    return (n_axes = Int(na[]), base_length = Int(bl[]), on = on[] != 0)
end
"""-> the plane accumulators of the last `reduce!`, Int64: `plane_n [N]` and `plane_corr [L, n_axes, N]` (the ABI's row-major
`[N][n_axes][L]`: `plane_corr[r + 1, axis + 1, c + 1]` is the sum of C_axis(r) of chain c)"""
function planes_record(o::DeviceOverlap)
    info = planes_info(o)
    plane_n = zeros(Int64, o.n_chains)
    plane_corr = zeros(Int64, info.base_length, info.n_axes, o.n_chains)
    check(o.a, ccall((:pte_overlap_planes_get, libpte), Cint, (Ptr{Cvoid}, Ptr{Int64}, Ptr{Int64}), o.handle, plane_n, plane_corr))
    return (plane_n = plane_n, plane_corr = plane_corr)
end

end # module
