// pte_automala.hpp -- k_explore_automala: AutoMALA (reference src/explorers/AutoMALA.jl:84-275,
// src/explorers/hamiltonian_dynamics.jl:48-102, src/explorers/Preconditioner.jl:57-77) on the
// device log-potential families, one wavefront per replica.
//
// Every vector of the algorithm (state, momentum, preconditioner, start state, the two "before"
// copies, gradient) lives in registers: lane l holds elements 64j + l, j < E.  A log-density / norm
// evaluation is E DPP wave reductions (the fixed tree of pte_device.hpp) -- no LDS, no HBM traffic
// between the initial load and the final store of the state.  Log potentials:
//   TGT_MVN    ScaledPrecisionNormalLogPotential, analytic gradient (src/paths/ScaledPrecisionNormalPath.jl:19-34)
//   TGT_FUNNEL InterpolatedAD of {ScaledPrecisionNormal(p0) reference, Neal's funnel}
//              (src/explorers/BufferedAD.jl:89-112; funnel test/supporting/dimensional-analysis.jl:36-48)
//   TGT_MIXTURE the same path with a normalised mixture of KB (or fewer) diagonal Gaussians as the target (pte_mixture.hpp)
//   TGT_GLM    the same path with prior x likelihood of a Bayesian GLM as the target, LIK = GLM_* (pte_glm.hpp): the one family
//              that reads data -- through LDS, outside the register-only scheme above
//   TGT_MIXMODEL the same path with prior x likelihood of a finite mixture model given data y as the target (DESIGN 4.11;
//              pte_mixture_model.hpp): theta = [mu, s, alpha] in one block, lanes over observations, K <= KB components
//   TGT_HIER   the same path with a hierarchical normal-means posterior as the target, LIK = HIER_* the parameterisation (DESIGN 4.14;
//              pte_hier.hpp): x = [mu, log tau, one coordinate per group], elementwise but for the two hyper-parameters' gradient sums
//   TGT_AR1    the same path with a latent-AR(1) state-space posterior as the target, LIK = AR1_* the observation model (DESIGN 4.15;
//              pte_ar1.hpp): x = [mu, a, ls, h_0 .. h_{T-1}], every h coupled to its two neighbours through a one-lane wave shift
//   TGT_DENSE  the same path with N(m, Q^-1), Q a dense precision matrix, as the target (pte_dense.hpp): O(d^2) per evaluation,
//              the matrix read row by row from L2, every z_k broadcast by a read-lane
#pragma once
#include "pte_automala_params.hpp"
#include "pte_glm_params.hpp"
#include "pte_mixture_model_params.hpp"
#include "pte_hier_params.hpp"
#include "pte_ar1_params.hpp"
#include "pte_dense_params.hpp"
#include "pte_slice_coord.hpp"

namespace pte {

// tree over the E block sums (uniform values), E a power of two
template <int E>
__device__ __forceinline__ double block_tree(double (&s)[E]) {
#pragma unroll
    for (int w = E; w > 1; w >>= 1)
#pragma unroll
        for (int i = 0; i < w / 2; ++i) s[i] = s[2 * i] + s[2 * i + 1];
    return s[0];
}
template <int E>
__device__ __forceinline__ double tree_sum_regs(const double (&t)[E]) {
    if constexpr (E >= 4) {                            // block sums four at a time, blocks 2i and 2i+1 added in the same pass
        double s[E / 2];
#pragma unroll
        for (int j0 = 0; j0 < E; j0 += 4) {
            double v[4], o[2];
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = t[j0 + j];
            wave_sum_pairs<4>(v, o);
            s[j0 / 2] = o[0]; s[j0 / 2 + 1] = o[1];
        }
        return block_tree<E / 2>(s);
    } else {
#ifndef PTE_WSP_ROWS_ONLY
        if constexpr (E == 2) return wave_sum_pair(t[0], t[1]);
#endif
        double s[E];
#pragma unroll
        for (int j = 0; j < E; ++j) s[j] = t[j];
        wave_sum_dpp_multi<E>(s);                      // their tree levels interleaved
        return block_tree<E>(s);
    }
}
// K reductions at once (K = 2 or 4, E >= 2): the block sums of all of them in lockstep, blocks 2i and 2i+1 of each at a time
template <int E, int K>
__device__ __forceinline__ void tree_sum_regs_multi(const double (&t)[K][E], double (&out)[K]) {
    if constexpr (E >= 2 && (K == 2 || K == 4)) {
        double s[K][E / 2];
#pragma unroll
        for (int j0 = 0; j0 < E; j0 += 2) {
            double v[2 * K], o[K];
#pragma unroll
            for (int k = 0; k < K; ++k) { v[2 * k] = t[k][j0]; v[2 * k + 1] = t[k][j0 + 1]; }
            wave_sum_pairs<2 * K>(v, o);
#pragma unroll
            for (int k = 0; k < K; ++k) s[k][j0 / 2] = o[k];
        }
#pragma unroll
        for (int k = 0; k < K; ++k) out[k] = block_tree<E / 2>(s[k]);
    } else {
        double s[K][E];
        constexpr int G = E < 2 ? E : 2;
#pragma unroll
        for (int j0 = 0; j0 < E; j0 += G) {
            double v[K * G];
#pragma unroll
            for (int k = 0; k < K; ++k)
#pragma unroll
                for (int j = 0; j < G; ++j) v[k * G + j] = t[k][j0 + j];
            wave_sum_dpp_multi<K * G>(v);
#pragma unroll
            for (int k = 0; k < K; ++k)
#pragma unroll
                for (int j = 0; j < G; ++j) s[k][j0 + j] = v[k * G + j];
        }
#pragma unroll
        for (int k = 0; k < K; ++k) out[k] = block_tree<E>(s[k]);
    }
}
template <int E>
__device__ __forceinline__ double sqr_norm_regs(const double (&v)[E]) {
    double t[E];
#pragma unroll
    for (int j = 0; j < E; ++j) t[j] = v[j] * v[j];
    return tree_sum_regs<E>(t);
}

// FULL: d == 64 E, every lane of every block holds an element -- the masks, selects and EXEC-guarded divisions of a ragged last
// block vanish (25 instructions of ~600 per leapfrog at E = 2)
// TGT_GLM's data and this wave's LDS (theta [64 E], then r [n_pad]): an empty base everywhere else, so that the other families' AmTarget
// keeps its layout -- and their instantiations their generated code (a larger AmTarget moved k_explore_aaps<4, TGT_FUNNEL>'s)
template <bool ON> struct AmGlmData {};
template <> struct AmGlmData<true> { GlmParams gl; double *glds; };
// TGT_MIXMODEL's data and its number of components (d / 3): the same arrangement
template <bool ON> struct AmMixModelData {};
template <> struct AmMixModelData<true> { MixModelParams mm; int mk; };
// TGT_HIER's data: the same arrangement.  y, 1 / sigma and log sigma of this lane's coordinates stay in registers for the replica's
// lifetime at E <= 2 (3 E doubles); from E = 4 on they are read again from L2 in every evaluation
template <bool ON, int E> struct AmHierData {};
template <int E> struct AmHierData<true, E> {
    static constexpr bool H_IN_REGS = (E <= 2);
    HierParams hp;
    double hy[H_IN_REGS ? E : 1], his[H_IN_REGS ? E : 1], hls[H_IN_REGS ? E : 1];
};
// TGT_AR1's data: the same arrangement.  The datum of this lane's coordinates that the observation model reads (y^2 under stochastic
// volatility, y under the normal model) stays in registers at E <= 2 (E doubles); from E = 4 on it is read again from L2
template <bool ON, int E> struct AmAr1Data {};
template <int E> struct AmAr1Data<true, E> {
    static constexpr bool A_IN_REGS = (E <= 2);
    Ar1Params ar;
    double ad[A_IN_REGS ? E : 1];
};
// TGT_DENSE's data: the same arrangement.  Nothing of it stays in registers: the mean is read once per evaluation, the matrix row by row
template <bool ON, int E> struct AmDenseData {};
template <int E> struct AmDenseData<true, E> { DenseParams dn; };
// The whole wave shifted by one lane (DPP wave_shr:1 / wave_shl:1, two v_mov_b32_dpp per double): lane l takes v of lane l - 1 (l + 1); the
// lane at the end that has no source keeps `edge` -- the neighbouring 64-block's value (uniform), so a chain over coordinates 64 j + lane
// reaches its predecessor and its successor without LDS or memory (TGT_AR1)
__device__ __forceinline__ double wave_from_below_f64(double v, double edge) {
    const int lo = __builtin_amdgcn_update_dpp(__double2loint(edge), __double2loint(v), 0x138, 0xF, 0xF, false);
    const int hi = __builtin_amdgcn_update_dpp(__double2hiint(edge), __double2hiint(v), 0x138, 0xF, 0xF, false);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double wave_from_above_f64(double v, double edge) {
    const int lo = __builtin_amdgcn_update_dpp(__double2loint(edge), __double2loint(v), 0x130, 0xF, 0xF, false);
    const int hi = __builtin_amdgcn_update_dpp(__double2hiint(edge), __double2hiint(v), 0x130, 0xF, 0xF, false);
    return __hiloint2double(hi, lo);
}

// what a path without data (TGT_MVN, TGT_FUNNEL) hands automala_body in the place of a family's parameter struct
struct AmNoData {};

template <int E, int TGT, bool FULL = false, int KB = 1, int LIK = 0>
struct AmTarget : AmGlmData<TGT == TGT_GLM>, AmMixModelData<TGT == TGT_MIXMODEL>, AmHierData<TGT == TGT_HIER, E>, AmAr1Data<TGT == TGT_AR1, E>, AmDenseData<TGT == TGT_DENSE, E> {
    int64_t d; int lane;
    double nhp, nprec;          // MVN: -0.5*prec, -prec of this chain
    double beta, omb, ref_nhp, ref_nprec, log3;   // funnel path
    // GaussianReference end of the path (variational leg): per-coordinate constants in registers when `vr`
    bool vr = false;
    static constexpr bool V_IN_REGS = (E < 16);      // d > 512: the replica's own vectors already fill the register file
    double vm[V_IN_REGS ? E : 1], vc0[V_IN_REGS ? E : 1], vi2[V_IN_REGS ? E : 1], vgf[V_IN_REGS ? E : 1];
    const double *pm = nullptr, *pc0 = nullptr, *pi2 = nullptr, *pgf = nullptr;
    __device__ __forceinline__ void load_variational(const EngineDev &e) {
        pm = e.v_mean; pc0 = e.v_c0; pi2 = e.v_i2; pgf = e.v_gf;
        if (V_IN_REGS) {
#pragma unroll
            for (int j = 0; j < E; ++j) {
                const bool ok = valid(j);
                const int64_t i = 64 * (int64_t)j + lane;
                vm[j % (V_IN_REGS ? E : 1)] = ok ? e.v_mean[i] : 0.0; vc0[j % (V_IN_REGS ? E : 1)] = ok ? e.v_c0[i] : 0.0;
                vi2[j % (V_IN_REGS ? E : 1)] = ok ? e.v_i2[i] : 0.0; vgf[j % (V_IN_REGS ? E : 1)] = ok ? e.v_gf[i] : 0.0;
            }
        }
    }
    __device__ __forceinline__ double VM(int j) const { return V_IN_REGS ? vm[j % (V_IN_REGS ? E : 1)] : (valid(j) ? pm[64 * j + lane] : 0.0); }
    __device__ __forceinline__ double VC0(int j) const { return V_IN_REGS ? vc0[j % (V_IN_REGS ? E : 1)] : (valid(j) ? pc0[64 * j + lane] : 0.0); }
    __device__ __forceinline__ double VI2(int j) const { return V_IN_REGS ? vi2[j % (V_IN_REGS ? E : 1)] : (valid(j) ? pi2[64 * j + lane] : 0.0); }
    __device__ __forceinline__ double VGF(int j) const { return V_IN_REGS ? vgf[j % (V_IN_REGS ? E : 1)] : (valid(j) ? pgf[64 * j + lane] : 0.0); }
    // gaussian_logdensity (GaussianReference.jl:43-49) with the fixed tree in place of the sequential sum
    __device__ __forceinline__ double variational_lp(const double (&x)[E]) const {
        double t[E];
#pragma unroll
        for (int j = 0; j < E; ++j) { const double dx = x[j] - VM(j); t[j] = valid(j) ? (VC0(j) - VI2(j) * (dx * dx)) : 0.0; }
        return tree_sum_regs<E>(t);
    }
    __device__ __forceinline__ double ref_lp(const double (&x)[E], double S) const { if (__builtin_expect(vr, 0)) return variational_lp(x); return ref_nhp * S; }
    __device__ __forceinline__ bool valid(int j) const { return FULL || 64 * (int64_t)j + lane < d; }

    // funnel: log density and (optionally) gradient; S = sum x^2 supplied by the caller
    __device__ __forceinline__ double funnel(const double (&x)[E], double (*g)[E]) const {
        const double y = readlane_f64(x[0], 0);
        const double sigma = exp(y / 2.0);
        const double logsigma = log(sigma);
        const double LOG2PI = 1.8378770664093453;
        double t[E], zi[E];
#pragma unroll
        for (int j = 0; j < E; ++j) {
            zi[j] = x[j] / sigma;
            t[j] = valid(j) ? (-(zi[j] * zi[j] + LOG2PI) / 2.0 - logsigma) : 0.0;
        }
        const double zv = y / 3.0;
        if (lane == 0) t[0] = -(zv * zv + LOG2PI) / 2.0 - log3;
        const double lp = tree_sum_regs<E>(t);
        if (g) {
#pragma unroll
            for (int j = 0; j < E; ++j) {
                (*g)[j] = valid(j) ? -(zi[j] / sigma) : 0.0;
                t[j] = valid(j) ? (zi[j] * zi[j] - 1.0) / 2.0 : 0.0;
            }
            if (lane == 0) t[0] = -(y / 9.0);
            const double gy = tree_sum_regs<E>(t);
            if (lane == 0) (*g)[0] = gy;
        }
        return lp;
    }
    // the same, with S = sum x^2 (and, when q is given, Q = sum q^2: the kinetic energy the caller needs next) taken alongside:
    // the block sums of the two to four reductions are independent and run in lockstep (wave_sum_dpp_multi) instead of one
    // dependent DPP chain after the other
    template <bool GRAD, bool WITH_Q>
    __device__ __forceinline__ double funnel_and_sqr_norm(const double (&x)[E], double (&g)[E], double &S, const double (&q)[E], double &Q) const {
        const double y = readlane_f64(x[0], 0);
        const double sigma = exp(y / 2.0);
        const double logsigma = log(sigma);
        const double LOG2PI = 1.8378770664093453;
        constexpr int K = 2 + (GRAD ? 1 : 0) + (WITH_Q ? 1 : 0), KG = 2, KQ = GRAD ? 3 : 2;
        double t[K][E], out[K];
#pragma unroll
        for (int j = 0; j < E; ++j) {
            const double zi = x[j] / sigma;
            t[0][j] = x[j] * x[j];
            t[1][j] = valid(j) ? (-(zi * zi + LOG2PI) / 2.0 - logsigma) : 0.0;
            if (GRAD) {
                g[j] = valid(j) ? -(zi / sigma) : 0.0;
                t[KG % K][j] = valid(j) ? (zi * zi - 1.0) / 2.0 : 0.0;
            }
            if (WITH_Q) t[KQ % K][j] = q[j] * q[j];
        }
        const double zv = y / 3.0;
        if (lane == 0) { t[1][0] = -(zv * zv + LOG2PI) / 2.0 - log3; if (GRAD) t[KG % K][0] = -(y / 9.0); }
        tree_sum_regs_multi<E, K>(t, out);
        S = out[0];
        if (GRAD) { if (lane == 0) g[0] = out[KG % K]; }
        if (WITH_Q) Q = out[KQ % K];
        return out[1];
    }
    __device__ __forceinline__ void load(const MixParams &m) {
        mx = m;
#pragma unroll
        for (int k = 0; k < KB; ++k) mxc[k] = k < m.K ? m.c[k] : 0.0;
    }
    // (x_i - mu_ki) inv_ki of component k, block j (0 outside the state / the components)
    __device__ __forceinline__ double mix_z(const double (&x)[E], int k, int j) const {
        if (k >= mx.K || !valid(j)) return 0.0;
        const int64_t i = k * mx.ld + 64 * (int64_t)j + lane;
        return (x[j] - mx.mu[i]) * mx.inv[i];
    }
    // the mixture's log density: q_k = sum_i ((x_i - mu_ki) inv_ki)^2 for every component, S = sum x^2 (and, WITH_Q, Q = sum q^2)
    // reduced in lockstep over the fixed tree; a_k = c_k - q_k / 2, lp = m + log(sum_k exp(a_k - m)) in component order.  GRAD: g = its gradient,
    // sum_k r_k (-(x - mu_k) inv_k^2) with r_k = exp(a_k - lp), in component order
    template <bool GRAD, bool WITH_Q>
    __device__ __forceinline__ double mixture_and_sqr_norm(const double (&x)[E], double (&g)[E], double &S, const double (&q)[E], double &Q) const {
        constexpr int NS = KB + 1 + (WITH_Q ? 1 : 0);
        double t[NS][E], out[NS];
#pragma unroll
        for (int j = 0; j < E; ++j) {
            t[0][j] = x[j] * x[j];
#pragma unroll
            for (int k = 0; k < KB; ++k) { const double z = mix_z(x, k, j); t[1 + k][j] = z * z; }
            if (WITH_Q) t[(NS - 1) % NS][j] = q[j] * q[j];
        }
        tree_sum_regs_multi<E, NS>(t, out);
        S = out[0];
        if (WITH_Q) Q = out[(NS - 1) % NS];
        double a[KB];
        double m = -INFINITY;
#pragma unroll
        for (int k = 0; k < KB; ++k) { a[k] = mxc[k] - out[1 + k] / 2.0; if (k < mx.K) m = (k == 0 || a[k] > m) ? a[k] : m; }
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < KB; ++k) if (k < mx.K) s += exp(a[k] - m);
        const double lp = m + log(s);
        if (GRAD) {
#pragma unroll
            for (int k = 0; k < KB; ++k) {
                if (k >= mx.K) break;
                const double r = exp(a[k] - lp);
#pragma unroll
                for (int j = 0; j < E; ++j) {
                    double gk = 0.0;
                    if (valid(j)) {
                        const int64_t i = k * mx.ld + 64 * (int64_t)j + lane;
                        const double iv = mx.inv[i];
                        gk = -((x[j] - mx.mu[i]) * (iv * iv));
                    }
                    g[j] = k == 0 ? r * gk : g[j] + r * gk;
                }
            }
        }
        return lp;
    }
    // the GLM's target log density: target = -(p/2) S + c_prior + sum_i l_i(eta_i) + c_obs, eta = X theta.  Two passes through
    // this wave's LDS: theta is broadcast from it to lanes that run over observations (eta_i sequential in j, one fused multiply-add per
    // block of 64 observations; lane l sums its own l_i in increasing i), then, GRAD, r_i = dl_i / deta_i goes back through it to lanes that
    // run over coordinates (sum_i X_ij r_i sequential in i).  The 64 lane sums are reduced over the fixed tree in lockstep with S (and Q).
    template <bool GRAD, bool WITH_Q>
    __device__ __forceinline__ double glm_and_sqr_norm(const double (&x)[E], double (&g)[E], double &S, const double (&q)[E], double &Q) const {
        constexpr int CH = 4;                           // blocks of observations per pass over theta (the last chunk re-reads its last block)
        const GlmParams &gl = this->gl;
        double *th = this->glds, *rr = this->glds + 64 * E;
        const int n = gl.n, nb = gl.n_pad >> 6;
        __syncthreads();                                // the last evaluation's reads of theta and r are done
#pragma unroll
        for (int j = 0; j < E; ++j) th[64 * j + lane] = x[j];
        __syncthreads();
        double lsum = 0.0;
        for (int m0 = 0; m0 < nb; m0 += CH) {
            int off[CH];
            double eta[CH];
#pragma unroll
            for (int c = 0; c < CH; ++c) { off[c] = 64 * min(m0 + c, nb - 1) + lane; eta[c] = 0.0; }
            const double *col = gl.xc;
            for (int64_t j = 0; j < d; ++j, col += gl.n_pad) {
                const double t = th[j];                 // one address: a broadcast
#pragma unroll
                for (int c = 0; c < CH; ++c) eta[c] = __builtin_fma(col[off[c]], t, eta[c]);
            }
#pragma unroll
            for (int c = 0; c < CH; ++c) {
                if (m0 + c >= nb) break;
                const int i = 64 * (m0 + c) + lane;
                const bool ok = i < n;                  // padded observations contribute exactly 0 (a zero row would give -log 2 under the logit)
                const double yi = gl.y[i], e = eta[c];
                double l, r;
                if constexpr (LIK == GLM_BERNOULLI_LOGIT) {
                    const double t = exp(-fabs(e));     // softplus(e) = max(e, 0) + log1p(exp(-|e|)); sigmoid in the sign-split form
                    l = yi * e - (fmax(e, 0.0) + log1p(t));
                    r = yi - (e >= 0.0 ? 1.0 : t) / (1.0 + t);
                } else {
                    const double res = yi - e;
                    l = -(res * res) * gl.w2;
                    r = res * gl.w1;
                }
                if (ok) lsum = lsum + l;
                if (GRAD) rr[i] = ok ? r : 0.0;
            }
        }
        constexpr int NS = 2 + (WITH_Q ? 1 : 0);
        double t[NS][E], out[NS];
#pragma unroll
        for (int j = 0; j < E; ++j) {
            t[0][j] = x[j] * x[j];
            t[1][j] = j == 0 ? lsum : 0.0;
            if (WITH_Q) t[(NS - 1) % NS][j] = q[j] * q[j];
        }
        tree_sum_regs_multi<E, NS>(t, out);
        S = out[0];
        if (WITH_Q) Q = out[(NS - 1) % NS];
        const double lp = (((ref_nhp * S) + gl.c_prior) + out[1]) + gl.c_obs;
        if (GRAD) {
            __syncthreads();                            // every r_i is in LDS
            double acc[E];
#pragma unroll
            for (int j = 0; j < E; ++j) acc[j] = 0.0;
            const double *row = gl.xr + lane;           // (lanes past d read the zero padding or the next row: discarded below)
            for (int i = 0; i < n; ++i, row += gl.ld) {
                const double ri = rr[i];
#pragma unroll
                for (int j = 0; j < E; ++j) acc[j] = __builtin_fma(row[64 * j], ri, acc[j]);
            }
#pragma unroll
            for (int j = 0; j < E; ++j) g[j] = valid(j) ? (ref_nprec * x[j]) + acc[j] : 0.0;
        }
        return lp;
    }
    // the mixture model's target log density: target = -(p/2) S + c_prior + sum_i l_i + c_obs, l_i = log sum_k exp(a_ik),
    // a_ik = b_k - z_ik^2 / 2, z_ik = (y_i - mu_k) e_k.  The parameters of component k sit in lanes k, K + k, 2 K + k of the one block: they
    // are read from there into scalar registers, and e_k = exp(-s_k), b_k = log w_k - s_k, w_k = softmax(alpha)_k are the same in every lane.
    // One pass over y with lanes over observations: lane l sums l_i and, GRAD, r_ik, r_ik z_ik, r_ik (z_ik^2 - 1) (r_ik = the responsibilities)
    // of its own observations in increasing i; the 64 lane sums go over the fixed tree in lockstep with S (and Q), and the totals go back to
    // lane j for coordinate j.  Components k >= K of the bucket carry alpha = -inf: a_ik = -inf, u_ik = 0.
    template <bool GRAD, bool WITH_Q>
    __device__ __forceinline__ double mixmodel_and_sqr_norm(const double (&x)[E], double (&g)[E], double &S, const double (&q)[E], double &Q) const {
        static_assert(E == 1 || TGT != TGT_MIXMODEL, "d = 3 K <= 24: one block per lane");
        const MixModelParams &mm = this->mm;
        const int K = this->mk;
        double mu[KB], ek[KB], bk[KB], wk[KB], s[KB], al[KB];
        double am = -INFINITY;
#pragma unroll
        for (int k = 0; k < KB; ++k) {
            const bool on = k < K;
            const double m_ = readlane_f64(x[0], k), s_ = readlane_f64(x[0], K + k), a_ = readlane_f64(x[0], 2 * K + k);
            mu[k] = on ? m_ : 0.0; s[k] = on ? s_ : 0.0; al[k] = on ? a_ : -INFINITY;
            am = (k == 0 || al[k] > am) ? al[k] : am;
        }
        double se = 0.0;
#pragma unroll
        for (int k = 0; k < KB; ++k) se += exp(al[k] - am);
        const double A = am + log(se);
#pragma unroll
        for (int k = 0; k < KB; ++k) {              // (uniform values: held in scalar registers through the loop over observations)
            ek[k] = readlane_f64(exp(-s[k]), 0);
            bk[k] = readlane_f64((al[k] - A) - s[k], 0);
            wk[k] = exp(al[k] - A);
        }
        double ls = 0.0, R[KB], Z1[KB], Z2[KB];
#pragma unroll
        for (int k = 0; k < KB; ++k) { R[k] = 0.0; Z1[k] = 0.0; Z2[k] = 0.0; }
        const double *yp = mm.y + lane;
#pragma unroll(KB >= 8 ? 1 : 8 / KB)
        for (int i0 = 0; i0 < mm.n_pad; i0 += 64) {
            const double yi = yp[i0];
            const bool ok = i0 + lane < mm.n;       // padded observations contribute exactly 0
            double z[KB], a[KB], u[KB];
            double mi = -INFINITY;
#pragma unroll
            for (int k = 0; k < KB; ++k) {
                z[k] = (yi - mu[k]) * ek[k];
                const double t = bk[k] - (z[k] * z[k]) / 2.0;
                a[k] = (t != t) ? -INFINITY : t;    // 0 x inf at y_i == mu_k with an overflowed e_k
                mi = (k == 0 || a[k] > mi) ? a[k] : mi;
            }
            const bool dead = mi == -INFINITY;
            double su = 0.0;
#pragma unroll
            for (int k = 0; k < KB; ++k) { u[k] = exp(a[k] - mi); su += u[k]; }
            const double li = dead ? -INFINITY : mi + log(su);
            ls = ok ? ls + li : ls;
            if (GRAD) {
#pragma unroll
                for (int k = 0; k < KB; ++k) {
                    const double r = dead ? 0.0 : u[k] / su;
                    R[k] = ok ? R[k] + r : R[k];
                    Z1[k] = ok ? Z1[k] + r * z[k] : Z1[k];
                    Z2[k] = ok ? Z2[k] + r * (z[k] * z[k] - 1.0) : Z2[k];
                }
            }
        }
        constexpr int NQ = 2, NG = NQ + (WITH_Q ? 1 : 0), NS = NG + (GRAD ? 3 * KB : 0);
        double v[NS];
        v[0] = x[0] * x[0]; v[1] = ls;
        if (WITH_Q) v[NQ % NS] = q[0] * q[0];
        if (GRAD) {
#pragma unroll
            for (int k = 0; k < KB; ++k) { v[(NG + 3 * k) % NS] = R[k]; v[(NG + 3 * k + 1) % NS] = Z1[k]; v[(NG + 3 * k + 2) % NS] = Z2[k]; }
        }
        wave_sum_dpp_multi<NS>(v);
        S = v[0];
        if (WITH_Q) Q = v[NQ % NS];
        const double lp = (((ref_nhp * S) + mm.c_prior) + v[1]) + mm.c_obs;
        if (GRAD) {
            double gl = 0.0;
#pragma unroll
            for (int k = 0; k < KB; ++k) {
                if (k >= K) break;
                gl = lane == k ? ek[k] * v[(NG + 3 * k + 1) % NS] : gl;
                gl = lane == K + k ? v[(NG + 3 * k + 2) % NS] : gl;
                gl = lane == 2 * K + k ? v[(NG + 3 * k) % NS] - mm.nd * wk[k] : gl;
            }
            g[0] = valid(0) ? (ref_nprec * x[0]) + gl : 0.0;
        }
        return lp;
    }
    // the hierarchical normal-means posterior: x = [mu, lt = log tau, x_2 .. x_{J+1}], LIK = HIER_CENTERED (x_{2+j} = theta_j) or
    // HIER_NONCENTERED (x_{2+j} = eta_j, theta_j = mu + tau eta_j).  The density is one sum over the fixed tree with the leaves in state order:
    // leaf 0 the prior of mu, leaf 1 the half-Cauchy of tau with the Jacobian of lt, leaf 2 + j = log N(y_j; theta_j, sigma_j^2) + the group
    // coordinate's prior.  tau = exp(lt), 1 / tau = exp(-lt) and log1p((tau / tau_scale)^2) are computed once, on the value lanes 0 and 1 of
    // block 0 hold.  GRAD: the group coordinates' derivatives are elementwise; those of mu and lt are two more sums over the same tree, in
    // lockstep with the density, S = sum x^2 and (WITH_Q) Q = sum q^2.  Lanes past d are masked by index and contribute exactly 0.
    __device__ __forceinline__ void load(const HierParams &h) {
        this->hp = h;
        if constexpr (AmHierData<true, E>::H_IN_REGS) {
#pragma unroll
            for (int j = 0; j < E; ++j) { this->hy[j] = h.y[64 * j + lane]; this->his[j] = h.isig[64 * j + lane]; this->hls[j] = h.lsig[64 * j + lane]; }
        }
    }
    template <bool GRAD, bool WITH_Q>
    __device__ __forceinline__ double hier_and_sqr_norm(const double (&x)[E], double (&g)[E], double &S, const double (&q)[E], double &Q) const {
        constexpr bool NC = (LIK == HIER_NONCENTERED);
        constexpr bool IN_REGS = AmHierData<true, E>::H_IN_REGS;
        const HierParams &hp = this->hp;
        const double LOG2PI = 1.8378770664093453;
        const double mu = readlane_f64(x[0], 0), lt = readlane_f64(x[0], 1);
        const double tau = exp(lt);
        const double itau = NC ? 0.0 : exp(-lt);
        const double ts = tau * hp.its, r = ts * ts;
        constexpr int K = 2 + (GRAD ? 2 : 0) + (WITH_Q ? 1 : 0), KM = 2, KT = 3, KQ = GRAD ? 4 : 2;
        double t[K][E], out[K];
#pragma unroll
        for (int j = 0; j < E; ++j) {
            const bool grp = (j > 0 || lane >= 2) && valid(j);          // this lane's coordinate of block j is a group's
            double yj, is, ls;
            if constexpr (IN_REGS) { yj = this->hy[j]; is = this->his[j]; ls = this->hls[j]; }
            else { yj = hp.y[64 * j + lane]; is = hp.isig[64 * j + lane]; ls = hp.lsig[64 * j + lane]; }      // ([512]: in bounds whatever d)
            const double xj = x[j];
            t[0][j] = xj * xj;
            double lf, gj, gm, gt;
            if constexpr (NC) {
                const double th = mu + tau * xj;
                const double z = (yj - th) * is, zi = z * is, zt = zi * tau;
                lf = (-(z * z + LOG2PI) / 2.0 - ls) + (-(xj * xj + LOG2PI) / 2.0);
                gj = zt - xj; gm = zi; gt = zt * xj;
            } else {
                const double z = (yj - xj) * is, u = (xj - mu) * itau, ui = u * itau;
                lf = (-(z * z + LOG2PI) / 2.0 - ls) + (-(u * u + LOG2PI) / 2.0 - lt);
                gj = z * is - ui; gm = ui; gt = u * u - 1.0;
            }
            t[1][j] = grp ? lf : 0.0;
            if (GRAD) { g[j] = grp ? gj : 0.0; t[KM % K][j] = grp ? gm : 0.0; t[KT % K][j] = grp ? gt : 0.0; }
            if (WITH_Q) t[KQ % K][j] = q[j] * q[j];
        }
        const double m = mu * hp.imu;
        if (lane == 0) { t[1][0] = -(m * m + LOG2PI) / 2.0 - hp.lmu; if (GRAD) t[KM % K][0] = -m * hp.imu; }
        if (lane == 1) { t[1][0] = (hp.c_tau - log1p(r)) + lt; if (GRAD) t[KT % K][0] = 1.0 - (2.0 * r) / (1.0 + r); }
        tree_sum_regs_multi<E, K>(t, out);
        S = out[0];
        if (GRAD) g[0] = lane == 0 ? out[KM % K] : lane == 1 ? out[KT % K] : g[0];
        if (WITH_Q) Q = out[KQ % K];
        return out[1];
    }
    // the latent-AR(1) posterior: x = [mu, a, ls, h_0 .. h_{T-1}], phi = tanh(a), sigma = exp(ls), LIK = AR1_STOCHASTIC_VOLATILITY
    // (y_t ~ N(0, exp(h_t))) or AR1_NORMAL_IDENTITY (y_t ~ N(h_t, obs_sd^2)).  The density is one sum over the fixed tree with the leaves in
    // state order: leaves 0..2 the priors of mu, a and sigma (with the Jacobian of ls), leaf 3 + t = the transition term of h_t + its
    // observation term.  phi, om = 1 - phi^2 = sech^2(a), sqrt(om), log(om), 1 - phi, isg = exp(-ls) and r = (sigma / sigma_scale)^2 are computed once, on the values
    // lanes 0..2 of block 0 hold.  The predecessor's h - mu comes from the lane below (lane 0: lane 63 of the block before); coordinate 3 = h_0
    // has the stationary law and reads no neighbour.  GRAD: the h components are elementwise given the successor's residual, which comes from
    // the lane above (lane 63: lane 0 of the block after); those of mu, a and ls are three more sums over the same tree, in lockstep with the
    // density, S = sum x^2 and (WITH_Q) Q = sum q^2.  Lanes past d are masked by index and contribute exactly 0.
    __device__ __forceinline__ void load(const Ar1Params &a) {
        this->ar = a;
        if constexpr (AmAr1Data<true, E>::A_IN_REGS) {
            const double *src = LIK == AR1_NORMAL_IDENTITY ? a.y : a.y2;
#pragma unroll
            for (int j = 0; j < E; ++j) this->ad[j] = src[64 * j + lane];
        }
    }
    template <bool GRAD, bool WITH_Q>
    __device__ __forceinline__ double ar1_and_sqr_norm(const double (&x)[E], double (&g)[E], double &S, const double (&q)[E], double &Q) const {
        constexpr bool NORMAL = (LIK == AR1_NORMAL_IDENTITY);
        constexpr bool IN_REGS = AmAr1Data<true, E>::A_IN_REGS;
        const Ar1Params &ar = this->ar;
        const double LOG2PI = 1.8378770664093453;
        const double mu = readlane_f64(x[0], 0), a = readlane_f64(x[0], 1), ls = readlane_f64(x[0], 2);
        // om = sech^2(a), its root and its log, and 1 - phi, from e = exp(-2 |a|): 1 - tanh^2 cancels (1e-8 relative at |a| = 10, 0 from 19.07)
        const double LOG2 = 0.6931471805599453;
        const double phi = tanh(a);
        const double ta = fabs(a), e2 = exp(-2.0 * ta), q2 = 1.0 + e2;
        const double sqom = (2.0 * exp(-ta)) / q2, om = sqom * sqom, lom = 2.0 * ((LOG2 - ta) - log1p(e2));
        const double omp = a > 0.0 ? (2.0 * e2) / q2 : 2.0 / q2;        // 1 - phi
        const double isg = exp(-ls), sg = exp(ls);
        const double ts = sg * ar.iss, r = ts * ts;
        const double c0 = isg * sqom, pis = phi * isg, cm = omp * isg, ca = isg * om;
        constexpr int K = 2 + (GRAD ? 3 : 0) + (WITH_Q ? 1 : 0), KM = 2, KA = 3, KL = 4, KQ = GRAD ? 5 : 2;
        double t[K][E], out[K];
        double hm[E], u[E], ut[E], obd[E];
#pragma unroll
        for (int j = 0; j < E; ++j) hm[j] = x[j] - mu;
#pragma unroll
        for (int j = 0; j < E; ++j) {
            const bool lat = (j > 0 || lane >= 3) && valid(j);           // this lane's coordinate of block j is a latent state h_t
            const bool first = (j == 0 && lane == 3);                   // ... and it is h_0
            const double pv = wave_from_below_f64(hm[j], j > 0 ? readlane_f64(hm[j > 0 ? j - 1 : 0], 63) : 0.0);      // h_{t-1} - mu
            double dj;
            if constexpr (IN_REGS) dj = this->ad[j];
            else dj = (NORMAL ? ar.y : ar.y2)[64 * j + lane];            // ([512]: in bounds whatever d)
            const double xj = x[j];
            t[0][j] = xj * xj;
            const double u1 = (hm[j] - phi * pv) * isg, u0 = (hm[j] * isg) * sqom;
            const double uj = first ? u0 : u1;
            double tr = -(uj * uj + LOG2PI) / 2.0 - ls;
            if (j == 0) tr = first ? tr + lom / 2.0 : tr;
            double ob;
            if constexpr (NORMAL) {
                const double z = (dj - xj) * ar.iobs;
                ob = -(z * z + LOG2PI) / 2.0 - ar.lobs;
                obd[j] = z * ar.iobs;
            } else {
                const double ye = dj * exp(-xj);
                ob = -((ye + xj) + LOG2PI) / 2.0;
                obd[j] = (ye - 1.0) / 2.0;
            }
            t[1][j] = lat ? tr + ob : 0.0;
            u[j] = lat ? uj : 0.0;
            ut[j] = (lat && !first) ? uj : 0.0;                          // the residuals that read a predecessor
            if constexpr (GRAD) {
                t[KM][j] = lat ? (first ? uj * c0 : uj * cm) : 0.0;
                t[KA][j] = lat ? (first ? (uj * uj - 1.0) * phi : (uj * pv) * ca) : 0.0;
                t[KL][j] = lat ? uj * uj - 1.0 : 0.0;
            }
            if constexpr (WITH_Q) t[KQ][j] = q[j] * q[j];
        }
        if constexpr (GRAD) {
#pragma unroll
            for (int j = 0; j < E; ++j) {
                const bool lat = (j > 0 || lane >= 3) && valid(j);
                const bool first = (j == 0 && lane == 3);
                const double us = wave_from_above_f64(ut[j], j + 1 < E ? readlane_f64(ut[j + 1 < E ? j + 1 : j], 0) : 0.0);      // u_{t+1}
                const double ow = first ? u[j] * c0 : u[j] * isg;
                g[j] = lat ? (us * pis - ow) + obd[j] : 0.0;
            }
        }
        const double m = mu * ar.imu, za = (a - ar.phi_loc) * ar.ips;
        if (lane == 0) { t[1][0] = -(m * m + LOG2PI) / 2.0 - ar.lmu; if constexpr (GRAD) t[KM][0] = -m * ar.imu; }
        if (lane == 1) { t[1][0] = -(za * za + LOG2PI) / 2.0 - ar.lps; if constexpr (GRAD) t[KA][0] = -za * ar.ips; }
        if (lane == 2) { t[1][0] = (ar.c_sigma - log1p(r)) + ls; if constexpr (GRAD) t[KL][0] = 1.0 - (2.0 * r) / (1.0 + r); }
        tree_sum_regs_multi<E, K>(t, out);
        S = out[0];
        if constexpr (GRAD) g[0] = lane == 0 ? out[KM] : lane == 1 ? out[KA] : lane == 2 ? out[KL] : g[0];
        if constexpr (WITH_Q) Q = out[KQ];
        return out[1];
    }
    // the dense-precision Gaussian N(m, Q^-1): z = x - m, u = Q z, A = z' u, l2 = c - A / 2, gradient -u.  u_i = sum_k Q[k][i] z_k
    // is accumulated for k = 0 .. d-1 in that order, one fused multiply-add per term from 0.0: row k of the symmetric matrix is E coalesced
    // loads (lane l takes Q[k][64 j + l]), z_k reaches every lane through a read-lane with a uniform index -- no LDS, no memory round trip.
    // DENSE_ROWS rows are requested before the first of their multiply-adds, so that a row costs an issue slot, not an L2 latency.  The rows
    // are zero from d on, and so are x and m: lanes past d hold u = z = 0 without a mask.  A = the fixed-tree sum of z_i u_i, in lockstep with
    // S = sum x^2 and (WITH_Q) Q = sum q^2.
    static constexpr int DENSE_ROWS = 8;
    __device__ __forceinline__ void dense_core(const double (&x)[E], double (&z)[E], double (&u)[E]) const {
        const DenseParams &dn = this->dn;
        const int dd = FULL ? 64 * E : (int)d;
#pragma unroll
        for (int j = 0; j < E; ++j) { z[j] = x[j] - dn.mean[64 * j + lane]; u[j] = 0.0; }      // ([ld]: in bounds whatever d)
        const double *row = dn.q + lane;
        const int64_t ld = dn.ld;
#pragma unroll
        for (int jb = 0; jb < E; ++jb) {
            const int nl = FULL ? 64 : max(0, min(64, dd - 64 * jb));
            int l = 0;
#pragma nounroll                                           // (whole blocks have a constant trip count: unrolled further, the rows in flight spill)
            for (; l + DENSE_ROWS <= nl; l += DENSE_ROWS, row += DENSE_ROWS * ld) {
                double r[DENSE_ROWS][E];
#pragma unroll
                for (int t = 0; t < DENSE_ROWS; ++t)
#pragma unroll
                    for (int j = 0; j < E; ++j) r[t][j] = row[t * ld + 64 * j];
#pragma unroll
                for (int t = 0; t < DENSE_ROWS; ++t) {
                    const double zk = readlane_f64(z[jb], l + t);
#pragma unroll
                    for (int j = 0; j < E; ++j) u[j] = __builtin_fma(r[t][j], zk, u[j]);
                }
            }
#pragma nounroll
            for (; l < nl; ++l, row += ld) {
                const double zk = readlane_f64(z[jb], l);
#pragma unroll
                for (int j = 0; j < E; ++j) u[j] = __builtin_fma(row[64 * j], zk, u[j]);
            }
        }
    }
    // A and S (and Q) of a state whose z and u are at hand
    template <bool WITH_Q>
    __device__ __forceinline__ void dense_sums(const double (&x)[E], const double (&z)[E], const double (&u)[E], double &A, double &S,
                                               const double (&q)[E], double &Q) const {
        constexpr int K = 2 + (WITH_Q ? 1 : 0);
        double t[K][E], out[K];
#pragma unroll
        for (int j = 0; j < E; ++j) {
            t[0][j] = x[j] * x[j];
            t[1][j] = z[j] * u[j];
            if constexpr (WITH_Q) t[2][j] = q[j] * q[j];
        }
        tree_sum_regs_multi<E, K>(t, out);
        S = out[0]; A = out[1];
        if constexpr (WITH_Q) Q = out[2];
    }
    template <bool GRAD, bool WITH_Q>
    __device__ __forceinline__ double dense_and_sqr_norm(const double (&x)[E], double (&g)[E], double &S, const double (&q)[E], double &Q) const {
        double z[E], u[E], A;
        dense_core(x, z, u);
        dense_sums<WITH_Q>(x, z, u, A, S, q, Q);
        if constexpr (GRAD) {
#pragma unroll
            for (int j = 0; j < E; ++j) g[j] = -u[j];
        }
        return this->dn.c - 0.5 * A;
    }
    // The six data families -- paths (1 - beta) reference + beta target whose target is a <family>_and_sqr_norm member -- are dispatched HERE and
    // nowhere else: a new family adds its TGT to DATA_FAMILY, a line to the chain below and a load() overload.
    // (The chain is a macro, not a forwarding member: one more level of inlining reorders the loads of the families' kernels -- DESIGN 4.10)
    static constexpr bool DATA_FAMILY = TGT == TGT_DENSE || TGT == TGT_AR1 || TGT == TGT_HIER || TGT == TGT_MIXMODEL || TGT == TGT_GLM || TGT == TGT_MIXTURE;
#define PTE_AM_TARGET_AND_SQR_NORM(l2, GRAD, WITH_Q, ...)                                                    \
    if constexpr (TGT == TGT_DENSE) l2 = dense_and_sqr_norm<GRAD, WITH_Q>(__VA_ARGS__);                      \
    else if constexpr (TGT == TGT_AR1) l2 = ar1_and_sqr_norm<GRAD, WITH_Q>(__VA_ARGS__);                     \
    else if constexpr (TGT == TGT_HIER) l2 = hier_and_sqr_norm<GRAD, WITH_Q>(__VA_ARGS__);                   \
    else if constexpr (TGT == TGT_MIXMODEL) l2 = mixmodel_and_sqr_norm<GRAD, WITH_Q>(__VA_ARGS__);           \
    else if constexpr (TGT == TGT_GLM) l2 = glm_and_sqr_norm<GRAD, WITH_Q>(__VA_ARGS__);                     \
    else l2 = mixture_and_sqr_norm<GRAD, WITH_Q>(__VA_ARGS__)
    // the target's log density alone: what the swap statistic suff2 holds
    __device__ __forceinline__ double target(const double (&x)[E]) const {
        double l2, S, Q, dummy[E];
        PTE_AM_TARGET_AND_SQR_NORM(l2, false, false, x, dummy, S, x, Q);
        return l2;
    }
    // the family's data, as its kernel takes it (d and lane are set): one overload per parameter struct (MixParams, HierParams and Ar1Params: above,
    // beside their members), an empty one for the paths without data
    __device__ __forceinline__ void load(const AmNoData &) {}
    __device__ __forceinline__ void load(const GlmParams &gp) {
        extern __shared__ __attribute__((aligned(16))) double glm_lds[];      // after automala_body's s_wi / s_ki / s_fi (6 KiB: the base stays 16-B aligned)
        this->gl = gp; this->glds = glm_lds;
    }
    __device__ __forceinline__ void load(const MixModelParams &m) { this->mm = m; this->mk = (int)(d / 3); }
    __device__ __forceinline__ void load(const DenseParams &n) { this->dn = n; }
    // log_potentials[chain](x) as a plain callable: InterpolatedLogPotential(x) (src/paths/InterpolatedLogPotential.jl:9-16)
    // WITH its beta == 0 / beta == 1 short-circuits -- what SliceSampler evaluates (the AD form below has none)
    __device__ __forceinline__ double path_lp(const double (&x)[E]) const {
        if constexpr (DATA_FAMILY) {
            if (beta == 0.0) return ref_nhp * sqr_norm_regs<E>(x);
            double S, Q, dummy[E], l2;
            PTE_AM_TARGET_AND_SQR_NORM(l2, false, false, x, dummy, S, x, Q);
            if (beta == 1.0) return l2;
            return omb * (ref_nhp * S) + beta * l2;
        }
        const double S = sqr_norm_regs<E>(x);
        if (TGT == TGT_MVN) return nhp * S;
        if (beta == 0.0) return ref_lp(x, S);
        if (beta == 1.0) return funnel(x, nullptr);
        const double l1 = ref_lp(x, S);
        const double l2 = funnel(x, nullptr);
        return omb * l1 + beta * l2;
    }
    // LogDensityProblems.logdensity
    __device__ __forceinline__ double logdensity(const double (&x)[E]) const {
        if (TGT == TGT_MVN) return nhp * sqr_norm_regs<E>(x);
        double S, l2, dummy[E], dq;
        if constexpr (DATA_FAMILY) {
            PTE_AM_TARGET_AND_SQR_NORM(l2, false, false, x, dummy, S, x, dq);
            return omb * (ref_nhp * S) + beta * l2;
        }
        if (E <= 4) l2 = funnel_and_sqr_norm<false, false>(x, dummy, S, x, dq);
        else { S = sqr_norm_regs<E>(x); l2 = funnel(x, nullptr); }
        const double l1 = ref_lp(x, S);
        return omb * l1 + beta * l2;
    }
    // LogDensityProblems.logdensity_and_gradient; WITH_Q: also Q = sum q^2 (fixed tree), reduced in lockstep with the sums of the density
    template <bool WITH_Q>
    __device__ __forceinline__ double logdensity_and_gradient_q(const double (&x)[E], double (&g)[E], const double (&q)[E], double &Q) const {
        double S = 0.0;
        if (TGT == TGT_MVN) {
            if (WITH_Q) {
                double t[2][E], out[2];
#pragma unroll
                for (int j = 0; j < E; ++j) { t[0][j] = x[j] * x[j]; t[1][j] = q[j] * q[j]; }
                tree_sum_regs_multi<E, 2>(t, out);
                S = out[0]; Q = out[1];
            } else S = sqr_norm_regs<E>(x);
#pragma unroll
            for (int j = 0; j < E; ++j) g[j] = nprec * x[j];
            return nhp * S;
        }
        double logdens = 0.0;
        double g2[E];
        double l2;
        if constexpr (DATA_FAMILY) {
            PTE_AM_TARGET_AND_SQR_NORM(l2, true, WITH_Q, x, g2, S, q, Q);
            logdens += (ref_nhp * S) * omb;
            logdens += l2 * beta;
#pragma unroll
            for (int j = 0; j < E; ++j) g[j] = (ref_nprec * x[j]) * omb + g2[j] * beta;
            return logdens;
        }
        if (E <= 4) l2 = funnel_and_sqr_norm<true, WITH_Q>(x, g2, S, q, Q);
        else { S = sqr_norm_regs<E>(x); l2 = funnel(x, &g2); if (WITH_Q) Q = sqr_norm_regs<E>(q); }
        const double l1 = ref_lp(x, S);
        logdens += l1 * omb;
        logdens += l2 * beta;
        if (__builtin_expect(vr, 0)) {               // BufferedAD{GaussianReference}: -1/s^2 (x - m)   (the fixed reference falls through)
#pragma unroll
            for (int j = 0; j < E; ++j) g[j] = (VGF(j) * (x[j] - VM(j))) * omb + g2[j] * beta;
        } else {
#pragma unroll
            for (int j = 0; j < E; ++j) g[j] = (ref_nprec * x[j]) * omb + g2[j] * beta;
        }
        return logdens;
    }
    __device__ __forceinline__ double logdensity_and_gradient(const double (&x)[E], double (&g)[E]) const {
        double dq;
        return logdensity_and_gradient_q<false>(x, g, x, dq);
    }
    // (last: the members above keep their order -- and the MVN / funnel instantiations their generated code)
    MixParams mx;               // TGT_MIXTURE: the components (K <= KB), their constants c_k in registers
    double mxc[KB];
};
#undef PTE_AM_TARGET_AND_SQR_NORM

// SLICE = true instantiates the same prologue (reference-chain refresh, state load) and epilogue (swap statistics, recorders)
// around the SliceSampler sweep instead of the Langevin refreshes: a separate kernel, so that neither pays for the other's registers.
#ifndef PTE_AM_PERMUTE
#define PTE_AM_PERMUTE 97                  // (a prime: coprime to every chain count it does not divide)
#endif
// Neighbouring chains do similar work (the slow ones -- most step-size trials -- sit next to the reference) and neighbouring
// workgroups share a CU, whose FP64 pipe the four SIMDs contend for: a stride permutation of workgroup -> chain spreads the slow
// chains over the chip.  Measured at C3, interleaved on one box: 0.231 -> 0.227 ms / scan (the same permutation makes the slice
// kernel 2.5 % SLOWER -- it is not applied there).
__device__ __forceinline__ int64_t am_chain_of_workgroup(int64_t K, int64_t wg) { return (K % PTE_AM_PERMUTE) ? (wg * PTE_AM_PERMUTE) % K : wg; }

// DIRECT (the scan loop with several chains per workgroup, k_scans_automala_wg): `wg` IS the local chain, and the table staging ends in a
// wave-level wait instead of a workgroup barrier -- every wave writes all the (identical) entries itself, so it only has to see its own stores
// fp: the family's data as its kernel takes it (MixParams, GlmParams, ... -- FP is deduced; nothing on the MVN and funnel paths), handed to
// AmTarget::load; KB (the components' bucket, K <= KB) and LIK (the likelihood / parameterisation / observation model) are the family's
// compile-time choices.  Which target it is is asked in AmTarget alone (DATA_FAMILY, its chain over the families, target, load): the body below
// names no family but the funnel, whose path has a reference of its own (the variational leg, suff3).  TGT_GLM's dynamic LDS (theta and r:
// pte_glm.hpp) lies behind the tables staged here.
template <int E, int TGT, bool SLICE = false, bool FULL = false, bool DIRECT = false, int KB = 1, int LIK = 0, class FP = AmNoData>
__device__ __forceinline__ void automala_body(EngineDev e, AmParams ap, const int64_t wg, const FP &fp = FP{}) {      // wg: blockIdx.x
    constexpr int NLU = (E == 1 ? 0 : E == 2 ? 1 : E == 4 ? 2 : E == 8 ? 3 : 4);
    const int lane = lane_id();
    // the ziggurat tables of the momentum draws, staged once: a global gather per block of draws costs a memory round trip each time
    __shared__ double s_wi[256];
    __shared__ unsigned long long s_ki[256];
    __shared__ double s_fi[256];
    if (!SLICE) {
        for (int i = lane; i < 256; i += 64) { s_wi[i] = ZIG_WI[i]; s_ki[i] = ZIG_KI[i]; s_fi[i] = ZIG_FI[i]; }
        if constexpr (DIRECT) { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); __builtin_amdgcn_wave_barrier(); }
        else __syncthreads();
    }
    const int64_t cl = DIRECT ? wg : am_chain_of_workgroup(e.K, wg);
    if (cl >= e.K) return;
    const int64_t c = e.c0 + cl;
    const int slot = e.slot_of_chain[cl];
    const int64_t d = e.d;
    double *xrow = e.x + (int64_t)slot * e.ld;
    using Target = AmTarget<E, TGT, FULL, KB, LIK>;
    Target T;
    T.d = d; T.lane = lane;
    T.load(fp);
    T.nhp = e.nhp[c]; T.nprec = e.nprec[c];
    T.beta = e.beta[c]; T.omb = 1.0 - T.beta;
    T.ref_nhp = -0.5 * ap.ref_prec; T.ref_nprec = -ap.ref_prec; T.log3 = ap.log3;
    const bool v_on = (TGT == TGT_FUNNEL) && e.v_use != nullptr;      // a GaussianReference is active on this engine
    if (v_on) { T.load_variational(e); T.vr = e.v_use[c] != 0; }

    double x[E];
    if (is_ref_chain(e, c)) {
        if (e.compose_phase == 2) return;
        const double lp0 = lp_before_explore(e, c, slot);
        double S0;
        if (v_on && T.vr) {
            // sample_iid!(::GaussianReference) (GaussianReference.jl:33-40): x_i = randn * sd_i + mean_i, in draw order
            SeqRng r0{e.rng[2 * slot], e.rng[2 * slot + 1]};
#pragma unroll
            for (int j = 0; j < E; ++j) {
                const int nl = (int)max((int64_t)0, min((int64_t)64, d - 64 * (int64_t)j));
                x[j] = 0.0;
                if (nl > 0) {
                    const double z = wave_randn_block(r0, lane, nl);
                    x[j] = lane < nl ? z * e.v_std[64 * j + lane] + T.VM(j) : 0.0;
                    if (lane < nl) xrow[64 * j + lane] = x[j];
                }
            }
            S0 = sqr_norm_regs<E>(x);
            if (lane == 0) { e.suff[slot] = S0; e.rng[2 * slot] = r0.seed; }
        } else {
            S0 = iid_refresh<NLU>(e, slot, e.sd[c], lane);            // sample_iid! at the reference (pigeons.jl:104-105)
            __threadfence_block();
#pragma unroll
            for (int j = 0; j < E; ++j) x[j] = T.valid(j) ? xrow[64 * j + lane] : 0.0;
        }
        double l20 = 0.0, l30 = 0.0;
        if (TGT == TGT_FUNNEL) {
            l20 = T.funnel(x, nullptr);
            if (lane == 0) e.suff2[slot] = l20;
            if (v_on) { l30 = T.variational_lp(x); if (lane == 0) e.suff3[slot] = l30; }
        }
        if constexpr (Target::DATA_FAMILY) {
            l20 = T.target(x);
            if (lane == 0) e.suff2[slot] = l20;
        }
        record_after_explore_impl(e, cl, c, slot, lane, lp0, S0, l20, l30);
        return;
    }
    const double lp_before = lp_before_explore(e, c, slot);
#pragma unroll
    for (int j = 0; j < E; ++j) x[j] = T.valid(j) ? xrow[64 * j + lane] : 0.0;

    SeqRng r{e.rng[2 * slot], e.rng[2 * slot + 1]};
    // build_preconditioner! (Preconditioner.jl:57-77)
    double M[E];
#pragma unroll
    for (int j = 0; j < E; ++j) M[j] = 1.0;
    if (ap.target_std != nullptr && ap.precond != 0) {
        double sdv[E];
#pragma unroll
        for (int j = 0; j < E; ++j) sdv[j] = T.valid(j) ? ap.target_std[64 * j + lane] : 1.0;
        if (ap.precond == 1) {
#pragma unroll
            for (int j = 0; j < E; ++j) M[j] = sdv[j] == 0.0 ? 1.0 : 1.0 / sdv[j];
        } else {
            const double u = r.rand();
            if (u <= ap.p0) {
#pragma unroll
                for (int j = 0; j < E; ++j) M[j] = sdv[j] == 0.0 ? 1.0 : 1.0 / sdv[j];
            } else if (u <= ap.p0 + ap.p1) {
                // ones
            } else {
                const double mix = r.rand(), rmix = 1.0 - mix;
#pragma unroll
                for (int j = 0; j < E; ++j) M[j] = sdv[j] == 0.0 ? 1.0 : mix + rmix / sdv[j];
            }
        }
    }

#ifdef PTE_PROFILE_AM                      // debug builds only (tools/prof_automala.py): shader-clock time per section of the refresh loop
    uint64_t am_prof[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    uint64_t am_tlast = __builtin_amdgcn_s_memtime();
    const uint64_t am_rt0 = __builtin_amdgcn_s_memrealtime();
#define AM_STAMP(k) do { asm volatile("" ::: "memory"); const uint64_t t_ = __builtin_amdgcn_s_memtime(); am_prof[k] += t_ - am_tlast; am_tlast = t_; asm volatile("" ::: "memory"); } while (0)
#else
#define AM_STAMP(k) do { } while (0)
#endif
    double p[E], g[E], xs[E], xb[E], pb[E];
    long long steps_sum = 0; int steps_n = 0;
    double fac_sum = 0.0; int fac_n = 0;
    int rev_sum = 0, rev_n = 0;
    double acc_sum = 0.0; int acc_n = 0;
    int err = 0;

    // The reference re-evaluates the log density / gradient at points where it already has them (the start point of
    // every trial leapfrog of a step-size search; log_joint right after a leapfrog).  They are pure functions of
    // the state, so the kernel evaluates each point once and reuses the bits: identical results, ~2.5x fewer funnel
    // evaluations per auto_step_size call.
    double g0[E];            // conditioned gradient at the current x (valid after grad_at_start, until x moves for good)
    double lp0 = 0.0;        // log density at the current x
    double pp0 = 0.0;        // |p|^2 of the fresh momentum, reduced alongside the sums of the density
    auto grad_at_start = [&]() {
        lp0 = T.template logdensity_and_gradient_q<true>(x, g0, p, pp0);
#pragma unroll
        for (int j = 0; j < E; ++j) g0[j] = g0[j] / M[j];
    };
    auto kinetic = [&]() -> double { return 0.5 * sqr_norm_regs<E>(p); };
    // hamiltonian_dynamics! with n_steps = 1 from a point whose conditioned gradient is g0; logp_out = log density
    // at the new position (== what log_joint would recompute there)
    // ke_out = 0.5 |p|^2 of the momentum it leaves behind (what log_joint would recompute next)
    auto leap_frog = [&](double eps, double &logp_out, double &ke_out) -> bool {
        const double half = eps / 2;
#pragma unroll
        for (int j = 0; j < E; ++j) p[j] = p[j] + half * g0[j];
#pragma unroll
        for (int j = 0; j < E; ++j) x[j] = x[j] + eps * (p[j] / M[j]);
        double pp_mid;                                    // |p|^2 after the first half step: independent of the gradient, reduced with it
        const double logp = T.template logdensity_and_gradient_q<true>(x, g, p, pp_mid);
        logp_out = logp;
#pragma unroll
        for (int j = 0; j < E; ++j) g[j] = g[j] / M[j];
        const double ke_mid = 0.5 * pp_mid;
        ke_out = ke_mid;
        const double cur = logp - ke_mid;
        if (__builtin_expect(!isfinite(cur), 0)) return false;          // (rare: laid out behind the loop -- a lone wave refetches after every taken branch)
#pragma unroll
        for (int j = 0; j < E; ++j) p[j] = p[j] + half * g[j];
        const double sq = sqr_norm_regs<E>(p);
        ke_out = 0.5 * sq;
        if (__builtin_expect(!isfinite(sq), 0)) return false;
        return true;
    };
    // auto_step_size (:184-214): returns the exponent; h_before = log_joint at the start point (g0 / lp0 valid there).
    // keep: the forward search.  The reference follows it with leap_frog!(start point, step_size * 2^exponent) -- a leapfrog the search
    // has ALREADY made from the same point with the same step: its last trial when it shrank (exponent = -n) or did not move
    // (exponent = 0), its last but one when it grew (exponent = n - 1).  That trial's outcome (state, momentum, conditioned gradient,
    // log density, kinetic energy, return value) is kept instead of being thrown away and recomputed: the same bits, one gradient
    // evaluation per refresh less.
    double xk[E], pk[E], gk[E], lpk = 0.0, kek = 0.0; bool okk = true;
    auto auto_step_size = [&](double lower, double upper, double h_before, bool keep) -> int {
#pragma unroll
        for (int j = 0; j < E; ++j) { xb[j] = x[j]; pb[j] = p[j]; }
        double eps = ap.step_size;
        // one trial; save = this trial is (so far) the one the proposal would repeat
        double t_lp = 0.0, t_ke = 0.0; bool t_ok = true;
        auto trial = [&](double ee) -> double {
            t_ok = leap_frog(ee, t_lp, t_ke);
            return (t_lp - t_ke) - h_before;
        };
        auto save_trial = [&]() {
#pragma unroll
            for (int j = 0; j < E; ++j) { xk[j] = x[j]; pk[j] = p[j]; gk[j] = g[j]; }
            lpk = t_lp; kek = t_ke; okk = t_ok;
        };
        auto restore = [&]() {
#pragma unroll
            for (int j = 0; j < E; ++j) { x[j] = xb[j]; p[j] = pb[j]; }
        };
        double diff = trial(eps);
        if (keep) save_trial();
        restore();
        int n_steps = 0, exponent = 0;
        if (!isfinite(diff) || diff < lower) {
            for (int n = 1;; ++n) {
                eps /= 2.0;
                diff = trial(eps);
                if (keep) save_trial();                       // shrinking: the last trial is the one
                restore();
                if (eps == 0.0) { err = ERR_AM_STEP; break; }
                if (diff > lower) { n_steps = n; exponent = -n; break; }
            }
        } else if (diff > upper) {
            for (int n = 1;; ++n) {
                eps *= 2.0;
                diff = trial(eps);
                const bool stop = !isfinite(diff) || diff < upper;
                if (keep && !stop) save_trial();              // growing: the last trial BEFORE the one that went too far
                restore();
                if (stop) { n_steps = n; exponent = n - 1; break; }
            }
        }
        steps_sum += 1 + n_steps; steps_n += 1;
        if (e.am_log != nullptr && lane == 0 && fac_n < e.am_log_cap) e.am_log[(e.trace_idx * e.K + cl) * e.am_log_cap + fac_n] = (int16_t)exponent;
        fac_sum += ldexp(1.0, exponent); fac_n += 1;
        return exponent;
    };

    if constexpr (SLICE) {
        // ---- step!(::SliceSampler) on a path without a closed-form single-coordinate update: slice_coord (pte_slice_coord.hpp) over the
        // coordinates in state order, n_passes times (slice_sample! :43-62), every log potential evaluated in full (E wave reductions of
        // the fixed tree + the funnel's exp / log).  The state stays in registers, so there is nothing to hold.
        WaveDraws dr;
        dr.init(r.seed, r.gamma, lane);
        double lp = T.path_lp(x);                               // cached_log_potential (:32-41)
        if (lp == -INFINITY) { if (lane == 0) set_error(e, ERR_SLICE_SUPPORT, (int)c, -1); return; }
        const SliceKnobs kn{ap.slice_w, 1.1 * ap.slice_w, ap.slice_p, ap.slice_max_iter};
        SliceTally tally;
        for (int pass = 0; pass < ap.slice_n_passes && !err; ++pass) {
#pragma unroll
            for (int j = 0; j < E; ++j) {
                const int nl = (int)max((int64_t)0, min((int64_t)64, d - 64 * (int64_t)j));
                for (int l = 0; l < nl && !err; ++l) {
                    struct {
                        const decltype(T) &T; double (&x)[E]; double &xj; bool mine;      // mine: this lane holds the coordinate
                        __device__ __forceinline__ double eval(double v) { xj = mine ? v : xj; return T.path_lp(x); }   // pointer[] = v; lp(state)
                        __device__ __forceinline__ void hold() {}
                        __device__ __forceinline__ void commit(double v) { xj = mine ? v : xj; }
                    } coord{T, x, x[j], lane == l};
                    const int serr = slice_coord<double>(coord, dr, lane, kn, tally, readlane_f64(x[j], l), kn.w, lp);
                    if (serr) { if (lane == 0) set_error(e, serr, (int)c, 64 * j + l); return; }
                }
            }
        }
        steps_sum += tally.steps_sum; steps_n += tally.steps_n;
        acc_sum += tally.acc_sum;     acc_n += tally.acc_n;
        r.seed = dr.final_seed();
    } else
    for (int it = 0; it < ap.n_refresh && !err; ++it) {
        AM_STAMP(7);
#pragma unroll
        for (int j = 0; j < E; ++j) {
            xs[j] = x[j];
            const int nl = FULL ? 64 : (int)max((int64_t)0, min((int64_t)64, d - 64 * (int64_t)j));
            p[j] = 0.0;
            if (nl > 0) { const double v = wave_randn_block(r, lane, nl, s_wi, s_ki, s_fi); p[j] = lane < nl ? v : 0.0; }
        }
        AM_STAMP(0);
        // Log density and conditioned gradient at the start point.  The reference evaluates them afresh in every refresh; they are
        // pure functions of x (the preconditioner is fixed for the scan), and from the second refresh on x is either the point the
        // last proposal leapfrog ended at -- evaluated there -- or the last start point -- evaluated then: the bits are carried
        // instead of recomputed (one of ~7 gradient evaluations per refresh), and only |p|^2 of the new momentum is reduced.
        if (it == 0) grad_at_start();
        else pp0 = sqr_norm_regs<E>(p);
        const double lp_s = lp0;
        double g_s[E];
#pragma unroll
        for (int j = 0; j < E; ++j) g_s[j] = g0[j];
        const double init_joint = lp0 - 0.5 * pp0;
        AM_STAMP(1);
        if (!isfinite(init_joint)) { err = ERR_AM_DENSITY; break; }
        if (ap.mala) {                                   // mala! (MALA.jl:79-96)
            double lpn, ken;
            leap_frog(ap.step_size, lpn, ken);
#pragma unroll
            for (int j = 0; j < E; ++j) p[j] = p[j] * -1.0;
            const double ex = exp((lpn - ken) - init_joint);          // |-p|^2 == |p|^2 bit for bit
            const double probability = ex < 1.0 ? ex : (isnan(ex) ? ex : 1.0);
            acc_sum += probability; acc_n += 1;
            if (!(r.rand() < probability)) {
#pragma unroll
                for (int j = 0; j < E; ++j) x[j] = xs[j];             // (lp0, g0 stay those of the start point)
            } else {
                lp0 = lpn;
#pragma unroll
                for (int j = 0; j < E; ++j) g0[j] = g[j];
            }
            steps_sum += 1; steps_n += 1;
            continue;
        }
        const double ua = r.rand(), ub = r.rand();
        const double lower = log(ua < ub ? ua : ub), upper = log(ua < ub ? ub : ua);
        AM_STAMP(2);
        const int proposed = auto_step_size(lower, upper, init_joint, true);
        if (err) break;
        AM_STAMP(3);
        // leap_frog!(..., step_size * 2^proposed) from the start point == the trial the search kept
#pragma unroll
        for (int j = 0; j < E; ++j) { x[j] = xk[j]; p[j] = pk[j]; g[j] = gk[j]; }
        const double lp_moved = lpk, ke_moved = kek;
        const bool moved_ok = okk;
        AM_STAMP(4);
        if (ap.use_mh) {
#pragma unroll
            for (int j = 0; j < E; ++j) p[j] = p[j] * -1.0;
            // log density and conditioned gradient at the proposed point: the leapfrog just computed them
            lp0 = lp_moved;
#pragma unroll
            for (int j = 0; j < E; ++j) g0[j] = g[j];
            const double h_rev = lp0 - (moved_ok ? ke_moved : kinetic());
            const int reversed = auto_step_size(lower, upper, h_rev, false);
            if (err) break;
            AM_STAMP(5);
            const bool passed = reversed == proposed;
            rev_sum += passed ? 1 : 0; rev_n += 1;
            double probability = 0.0;
            if (passed) {
                const double ex = exp(h_rev - init_joint);      // final_joint_log == log_joint at the proposed point
                probability = ex < 1.0 ? ex : (isnan(ex) ? ex : 1.0);
            }
            acc_sum += probability; acc_n += 1;
            if (!(r.rand() < probability)) {
                lp0 = lp_s;
#pragma unroll
                for (int j = 0; j < E; ++j) { x[j] = xs[j]; g0[j] = g_s[j]; }
            }
            AM_STAMP(6);
        } else {                                         // no MH step: the chain stays where the proposal leapfrog ended
            lp0 = lp_moved;
#pragma unroll
            for (int j = 0; j < E; ++j) g0[j] = g[j];
        }
    }
#ifdef PTE_PROFILE_AM
    if (lane == 0) {
        double *o = e.on_m2 + 2 * (d + 1) + 12 * cl;
        for (int k = 0; k < 8; ++k) o[k] = (double)am_prof[k];
        o[8] = (double)(__builtin_amdgcn_s_memrealtime() - am_rt0); o[9] = (double)steps_sum; o[10] = (double)steps_n; o[11] = (double)ap.n_refresh;
    }
#endif
    if (err) { if (lane == 0) set_error(e, err, (int)c, -1); return; }
#pragma unroll
    for (int j = 0; j < E; ++j) if (T.valid(j)) xrow[64 * j + lane] = x[j];
    const double S = sqr_norm_regs<E>(x);
    double l2 = 0.0, l3 = 0.0;
    if (TGT == TGT_FUNNEL) l2 = T.funnel(x, nullptr);
    if constexpr (Target::DATA_FAMILY) l2 = T.target(x);
    if (v_on) l3 = T.variational_lp(x);
    if (lane == 0) {
        e.suff[slot] = S;
        if (TGT == TGT_FUNNEL || Target::DATA_FAMILY) e.suff2[slot] = l2;
        if (v_on) e.suff3[slot] = l3;
        e.rng[2 * slot] = r.seed;
        e.expl_steps_sum[cl] += (double)steps_sum; e.expl_steps_n[cl] += steps_n;
        e.expl_acc_sum[cl] += acc_sum;             e.expl_acc_n[cl] += acc_n;
        e.am_fac_sum[cl] += fac_sum;               e.am_fac_n[cl] += fac_n;
        e.am_rev_sum[cl] += (double)rev_sum;       e.am_rev_n[cl] += rev_n;
    }
    record_after_explore(e, cl, c, slot, lane, lp_before, S, l2, l3);
}

#ifndef PTE_AM_E16_ONE_WAVE
#define PTE_AM_E16_ONE_WAVE 1
#endif
template <int E, int TGT, bool SLICE = false, bool FULL = false>
__global__ __launch_bounds__(64)
#if PTE_AM_E16_ONE_WAVE
__attribute__((amdgpu_waves_per_eu(1, (E >= 16 && !SLICE) ? 1 : 8)))      // E = 16 (d > 512): one wave per SIMD may use the whole unified register file -- spills go to AGPRs, not to scratch
#endif
void k_explore_automala(EngineDev e, AmParams ap) {
    automala_body<E, TGT, SLICE, FULL>(e, ap, blockIdx.x);
}

// (the body as a CALLED function in the scan loop: inlined, the loop's long-lived values -- the engine's ~70 pointers, the hand-shake words --
// push 32 spill reloads into every step-size search loop; called, the body keeps the register allocation of the per-scan kernel)
template <int E, int TGT, bool FULL>
__device__ __attribute__((noinline)) void automala_body_called(const EngineDev &e, const AmParams &ap, const int64_t wg) {
    automala_body<E, TGT, false, FULL>(e, ap, wg);
}

// One launch per pte_run_scans (pte_kernels.hpp "ScanLoop"; round 5): AutoMALA / MALA refreshes, then the pairwise swap hand-shake, for all
// the scans of the call.  `scan != 1` (AutoMALA.jl:87,96-102: no MH step in the first scan of a round) is decided per scan inside.
template <int E, int TGT, bool FULL>
__global__ __launch_bounds__(64) void k_scans_automala(EngineDev e, AmParams ap, ScanLoop sl) {
    const int lane = lane_id();
    const int64_t cl = am_chain_of_workgroup(e.K, blockIdx.x);
    int go = 1;
    if (lane == 0) go = scan_loop_gate(sl) ? 1 : 0;        // every workgroup of the launch is resident, or nobody starts (pte_kernels.hpp)
    if (!__builtin_amdgcn_readfirstlane(go)) return;
    for (int64_t i = 0; i < sl.n_scans; ++i) {
#ifndef PTE_TEST_NO_E_COPY
        e.trace_idx = sl.scan_idx0 + i;
#endif
        if (!ap.mala) ap.use_mh = (sl.first_scan + i != 1) ? 1 : 0;
#ifdef PTE_AM_SCANS_INLINE
        automala_body<E, TGT, false, FULL>(e, ap, blockIdx.x);
#else
        automala_body_called<E, TGT, FULL>(e, ap, blockIdx.x);
#endif
        __syncthreads();                                   // every lane's stores of the explore step happen before lane 0's release
        int slot = 0;
        if (lane == 0) slot = swap_handshake(e, sl, i, cl, e.slot_of_chain[cl]);
        slot = __builtin_amdgcn_readfirstlane(slot);
        __syncthreads();                                   // ... and lane 0's acquire before every lane's loads of the next one
        if (slot < 0) return;
    }
}

// The same loop with PTE_SCAN_WG consecutive chains per workgroup, one per wave (pte_kernels.hpp, ScanWg): three of four pairs shake hands
// through LDS.  Workgroup b holds the chain GROUP the XCD-aware dealing gives it (scan_loop_group); the stride permutation of the per-scan
// kernel does not apply (it would tear the pairs apart).
#ifndef PTE_SCAN_WG
#define PTE_SCAN_WG 4
#endif
#ifndef PTE_AM_WG_PERMUTE
#define PTE_AM_WG_PERMUTE 0          // measured at C3: 0.2000 against 0.1979-0.1986 ms per scan -- the XCD-aware dealing of consecutive groups wins
#endif
template <int E, int TGT, bool FULL>
__device__ __attribute__((noinline)) void automala_body_called_direct(const EngineDev &e, const AmParams &ap, const int64_t cl) {
    automala_body<E, TGT, false, FULL, true>(e, ap, cl);
}
template <int E, int TGT, bool FULL>
__global__ __launch_bounds__(64 * PTE_SCAN_WG) void k_scans_automala_wg(EngineDev e, AmParams ap, ScanLoop sl) {
    constexpr int NW = PTE_SCAN_WG;
    __shared__ ScanWg<NW> wg;
    __shared__ int wg_go;
    const int lane = lane_id();
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (threadIdx.x < NW) wg.flag[threadIdx.x] = sl.epoch0;          // "has published every epoch up to the last call's"
    if (threadIdx.x == 0) wg_go = scan_loop_gate(sl) ? 1 : 0;        // every workgroup of the launch is resident, or nobody starts (pte_kernels.hpp)
    __syncthreads();
    if (!wg_go) return;
#if PTE_AM_WG_PERMUTE       // the per-scan kernel's stride permutation, over the GROUPS: neighbouring groups do similar work (the slow chains sit next to the reference)
    const int64_t G = (e.K + NW - 1) / NW;
    const int64_t cl = am_chain_of_workgroup(G, blockIdx.x) * NW + w;
#else
    const int64_t cl = scan_loop_group((e.K + NW - 1) / NW) * NW + w;
#endif
    if (cl >= e.K) return;
    for (int64_t i = 0; i < sl.n_scans; ++i) {
        e.trace_idx = sl.scan_idx0 + i;
        if (!ap.mala) ap.use_mh = (sl.first_scan + i != 1) ? 1 : 0;
        automala_body_called_direct<E, TGT, FULL>(e, ap, cl);
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");      // every lane's stores of the explore step are out before lane 0 publishes
        __builtin_amdgcn_wave_barrier();
        int slot = 0;
        if (lane == 0) slot = swap_handshake<NW>(e, sl, i, cl, e.slot_of_chain[cl], &wg);
        slot = __builtin_amdgcn_readfirstlane(slot);
        asm volatile("" ::: "memory");                                      // (lane 0's acquire precedes the other lanes' loads in program order: one wave)
        __builtin_amdgcn_wave_barrier();
        if (slot < 0) return;
    }
}

// Swap statistics of every slot recomputed from the stored states (pte_set_state, pte_set_target_<family>) on a data family's path:
// suff = sum x^2 with the fixed tree, suff2 = the target's log density.  The body of k_refresh_<family>_stats(EngineDev e, <Family>Params fp),
// one workgroup of one wave per slot.  (A macro: as a called body, however inlined, it moved the schedule of every kernel made of it --
// DESIGN 4.10.  The GLM's and the mixture model's kernels, which set their data in the kernel itself, keep their own for the same reason.)
#define PTE_REFRESH_STATS_BODY(E, TGT, KB, LIK, fp)                                                 \
    const int lane = lane_id();                                                                    \
    const int64_t slot = blockIdx.x;                                                               \
    if (slot >= e.K) return;                                                                       \
    AmTarget<E, TGT, false, KB, LIK> T;                                                            \
    T.d = e.d; T.lane = lane;                                                                      \
    T.load(fp);                                                                                    \
    const double *xrow = e.x + slot * e.ld;                                                        \
    double x[E];                                                                                   \
    _Pragma("unroll")                                                                              \
    for (int j = 0; j < E; ++j) x[j] = T.valid(j) ? xrow[64 * j + lane] : 0.0;                     \
    const double S = sqr_norm_regs<E>(x);                                                          \
    const double l2 = T.target(x);                                                                 \
    if (lane == 0) { e.suff[slot] = S; e.suff2[slot] = l2; }

// The same on the funnel path (a body of its own: suff3, the variational reference's log density, beside the two):
// suff = sum x^2 with the fixed tree, suff2 = the funnel's log density.
template <int E>
__global__ __launch_bounds__(64) void k_refresh_funnel_stats(EngineDev e, double log3) {
    const int lane = lane_id();
    const int64_t slot = blockIdx.x;
    if (slot >= e.K) return;
    AmTarget<E, TGT_FUNNEL> T;
    T.d = e.d; T.lane = lane; T.log3 = log3;
    const double *xrow = e.x + slot * e.ld;
    double x[E];
#pragma unroll
    for (int j = 0; j < E; ++j) x[j] = T.valid(j) ? xrow[64 * j + lane] : 0.0;
    const double S = sqr_norm_regs<E>(x);
    const double l2 = T.funnel(x, nullptr);
    if (lane == 0) { e.suff[slot] = S; e.suff2[slot] = l2; }
    if (e.v_use != nullptr) {
        T.load_variational(e);
        const double l3 = T.variational_lp(x);
        if (lane == 0) e.suff3[slot] = l3;
    }
}

}  // namespace pte
