// pte_slice_coord.hpp -- one SliceSampler coordinate update for the targets without a closed-form predicate: every log potential
// is evaluated in full by the family.  The reference's procedure as it stands (slice_sample_coord! :89-95, slice_double :97-126,
// slice_shrink! :144-186, slice_accept :192-237; the Integer method's initialize_slice_endpoints :136-142 and draw_new_position :189; the Bool
// method :65-86), statement for statement the oracle's mixed_coord_float / mixed_coord_integer / mixed_coord_bool, the replica's stream
// consumed through 64 buffered draws.  All control flow is uniform: every value it branches on comes out of a wave reduction or a uniform draw.
//
// The family hands in a coordinate object with three operations:
//   double eval(double v)   the path's log potential with this coordinate at v
//   void hold()             called right after the proposal (or the flipped value) is evaluated: keep what that evaluation left, because
//                           slice_accept evaluates more points before the commit
//   void commit(double v)   the coordinate ends at v, with what hold kept
// and keeps set_error and its own return: slice_coord returns 0, ERR_SLICE_MAX_ITER or ERR_SLICE_INVALID_LP.
#pragma once
#include "pte_kernels.hpp"

namespace pte {

struct SliceTally { long long steps_sum = 0; int steps_n = 0; double acc_sum = 0.0; int acc_n = 0; };      // the explorer's recorders
struct SliceKnobs { double w, w11; int p, max_iter; };                                                      // w, 1.1 w, the doubling cap, slice_shrink!'s cap

// randexp(rng) on the buffered draws: the ziggurat's fast path on one raw draw, the sequential procedure otherwise
__device__ __forceinline__ double wave_randexp(WaveDraws &dr, int lane) {
    const uint64_t raw = dr.next_raw(lane);
    const uint64_t ri = raw & MASK52;
    const int zi = (int)(ri & 0xFF);
    double Ex = (double)ri * ZIG_WE[zi];
    if (!(ri < ZIG_KE[zi])) { SeqRng sq = dr.to_seq(); Ex = randexp_from_raw(sq, raw); dr.from_seq(sq, lane); }
    return Ex;
}

// rand(rng, 0:n-1) on Int64 (Random.SamplerRangeNDL, the oracle's po_rand_range): Lemire's nearly division-less sampler over any source of
// rand(rng, UInt64)
template <class Next>
__device__ __forceinline__ int64_t rand_range0_from(Next next, uint64_t n) {
    uint64_t x = next();
    uint64_t low = x * n, hi = __umul64hi(x, n);
    if (low < n) {
        const uint64_t t = (0ULL - n) % n;
        while (low < t) { x = next(); low = x * n; hi = __umul64hi(x, n); }
    }
    return (int64_t)hi;
}

// slice_accept, one body for both methods: on an Integer coordinate every midpoint is integral (R - L = w 2^k, w integral)
template <class Coord>
__device__ __forceinline__ bool slice_accept(Coord &coord, const SliceKnobs &kn, SliceTally &tally, double xold, double newpos, double z,
                                             double L, double R, double aL, double aR) {
    double Lhat = L, Rhat = R;
    bool Rstale = false, Lstale = false, D = false, take = true;
    while (Rhat - Lhat > kn.w11) {
        const double Mid = (Lhat + Rhat) / 2.0;
        if ((xold < Mid && newpos >= Mid) || (xold >= Mid && newpos < Mid)) D = true;
        if (newpos < Mid) { Rhat = Mid; Rstale = true; } else { Lhat = Mid; Lstale = true; }
        if (D) {
            if (Lstale) { aL = coord.eval(Lhat); Lstale = false; }
            if (Rstale) { aR = coord.eval(Rhat); Rstale = false; }
            if (z >= aL && z >= aR) { take = false; break; }
        }
    }
    tally.acc_sum += take ? 1.0 : 0.0; tally.acc_n += 1;
    return take;
}

// where the Float64 and the Integer method differ: the first left end, the new position, the collapse test
__device__ __forceinline__ double slice_first_left(WaveDraws &dr, int lane, double xold, double w) { return xold - w * dr.rand(lane); }
__device__ __forceinline__ int64_t slice_first_left(WaveDraws &dr, int lane, int64_t xold, int64_t width) {
    return xold - rand_range0_from([&]() { return dr.next_raw(lane); }, (uint64_t)width + 1ull);
}
__device__ __forceinline__ double slice_new_position(WaveDraws &dr, int lane, double Lbar, double Rbar) { return Lbar + dr.rand(lane) * (Rbar - Lbar); }
__device__ __forceinline__ int64_t slice_new_position(WaveDraws &dr, int lane, int64_t Lbar, int64_t Rbar) {
    return Lbar + rand_range0_from([&]() { return dr.next_raw(lane); }, (uint64_t)(Rbar - Lbar) + 1ull);
}
__device__ __forceinline__ bool slice_collapsed(double Lbar, double Rbar) { return jl_isapprox(Lbar, Rbar); }
__device__ __forceinline__ bool slice_collapsed(int64_t Lbar, int64_t Rbar) { return Lbar == Rbar; }

// One coordinate at xold with the path at lp: P = double is the Float64 method (width = w), P = int64_t the Integer method (width = ceil(w)).
// lp ends as the path's log potential where the coordinate ends.
template <class P, class Coord>
__device__ __forceinline__ int slice_coord(Coord &coord, WaveDraws &dr, int lane, const SliceKnobs &kn, SliceTally &tally, P xold, P width, double &lp) {
    const double z = lp - wave_randexp(dr, lane);
    P L = slice_first_left(dr, lane, xold, width);
    P R = L + width;
    int K = kn.p;
    double lp_L = coord.eval((double)L), lp_R = coord.eval((double)R);
    while (K > 0 && (z < lp_L || z < lp_R)) {                    // slice_double
        const double V = dr.rand(lane);
        if (V <= 0.5) { L = L - (R - L); lp_L = coord.eval((double)L); }
        else { R = R + (R - L); lp_R = coord.eval((double)R); }
        K -= 1;
    }
    tally.steps_sum += kn.p - K; tally.steps_n += 1;
    P Lbar = L, Rbar = R;
    for (int it = 1; it <= kn.max_iter; ++it) {                  // slice_shrink!
        const P newpos = slice_new_position(dr, lane, Lbar, Rbar);
        const double newlp = coord.eval((double)newpos);
        coord.hold();
        if (z < newlp && slice_accept(coord, kn, tally, (double)xold, (double)newpos, z, (double)L, (double)R, lp_L, lp_R)) {
            coord.commit((double)newpos); lp = newlp;
            tally.steps_sum += it; tally.steps_n += 1;
            return isfinite(lp) ? 0 : ERR_SLICE_INVALID_LP;
        }
        if (newpos < xold) Lbar = newpos; else Rbar = newpos;
        if (slice_collapsed(Lbar, Rbar)) {
            lp = coord.eval((double)xold);
            tally.steps_sum += it; tally.steps_n += 1;
            return isfinite(lp) ? 0 : ERR_SLICE_INVALID_LP;
        }
    }
    return ERR_SLICE_MAX_ITER;
}

// The Bool method: the full conditional from one evaluation at the flipped value and one rand(rng).  It records nothing.
template <class Coord>
__device__ __forceinline__ int slice_coord_bool(Coord &coord, WaveDraws &dr, int lane, double xold, double &lp) {
    const bool on = xold != 0.0;
    const double lpf = coord.eval(on ? 0.0 : 1.0);
    coord.hold();
    const double lp0 = on ? lpf : lp, lp1 = on ? lp : lpf;
    const double prob_ratio = exp(lp1 - lp0);
    const double prob_zero = 1.0 / (1.0 + prob_ratio);
    const bool zero = dr.rand(lane) < prob_zero;
    if (zero == on) { coord.commit(zero ? 0.0 : 1.0); lp = lpf; }
    return isfinite(lp) ? 0 : ERR_SLICE_INVALID_LP;
}

}  // namespace pte
