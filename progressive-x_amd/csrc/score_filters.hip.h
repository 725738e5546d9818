// score_filters.hip.h — the conservative rejection filters of the score path: Filter<MT> (FP64, division-free), Filter32<MT>
// (FP32 pre-filter per pair + the group bound of the cull kernel).  A filter may only say "certainly an outlier"; every pair it
// does not reject goes through the exact FP64 residual in the reference's operation order, so counts, masks and scores are
// those of evaluating every pair.  The error budgets are derived in docs/lab-notebook.md (5.2) and machine-checked by
// scripts/verify_filters.py (exact rational arithmetic) and by the PGX_VERIFY=1 mode of the group-major kernel.
//
// Replaces nothing in the reference (its getScore evaluates every pair: scoring_function_with_compound_model.h:78-121).
#pragma once
#include <cmath>
#include <cstddef>
#include <type_traits>

#include "pgx_internal.h"

namespace pgx {

// ---- conservative rejection filter ------------------------------------------------------------
// Most (point, hypothesis) pairs are far from the threshold.  For those the two IEEE divisions of the reprojection /
// transfer residual (~110 of ~230 VALU cycles per wave-iteration) are wasted: the pair only has to be PROVEN an outlier.
// reject() evaluates the division-free form  (u pz - px)^2 + (v pz - py)^2 > T2 (1 + 2^-20) pz^2  with FMA arithmetic
// and returns true only when, additionally, pz is large enough against the rounding error E <= 4.5 eps L_h P_i of the
// projection (L_h = largest row 1-norm of the hypothesis, P_i = max(|coords of point i|, 1), both precomputed) that the
// inequality cannot be flipped by rounding in either arithmetic:  E (1 + Umax + T) 2^24 / T <= |pz|, with the host
// guaranteeing Umax / T <= 2^28 (otherwise the unfiltered instance is launched).  Every pair that is not rejected —
// including everything involving NaN/Inf, for which all comparisons are false — goes through the exact, oracle-order,
// no-FMA path below, so counts, masks and scores are bit-identical to the unfiltered kernel; the proof that no true
// inlier (exact r^2 < T2) can be rejected is in DESIGN.md §5.2.
constexpr double kFilterDelta = 1.0 / 1048576.0;  // 2^-20 > 12 * 2^-24

template <int MT> struct Filter {
    static constexpr bool enabled = false;
    struct Lane {};
    template <class MD> static __device__ __forceinline__ Lane prep(const MD&, double) { return {}; }
    template <class PT, class MD>
    static __device__ __forceinline__ bool reject(const PT&, const MD&, const Lane&, double, double) { return false; }
};

template <> struct Filter<kPnP> {
    static constexpr bool enabled = true;
    struct Lane { double c; };
    template <class MD> static __device__ __forceinline__ Lane prep(const MD& m, double guard) {
        const double l0 = fabs(m[0]) + fabs(m[1]) + fabs(m[2]) + fabs(m[3]);
        const double l1 = fabs(m[4]) + fabs(m[5]) + fabs(m[6]) + fabs(m[7]);
        const double l2 = fabs(m[8]) + fabs(m[9]) + fabs(m[10]) + fabs(m[11]);
        const double l = fmax(l0, fmax(l1, l2));
        // the test squares pz: outside this range of scales it is not trusted at all (trust = c * pmax <= |pz| fails for c = inf)
        return {(l > 1e-100 && l < 1e100) ? guard * l : 1.0 / 0.0};
    }
    template <class PT, class MD>
    static __device__ __forceinline__ bool reject(const PT& p, const MD& m, const Lane& ln, double pmax, double T2d) {
        const double px = __builtin_fma(m[0], p[2], __builtin_fma(m[1], p[3], __builtin_fma(m[2], p[4], m[3])));
        const double py = __builtin_fma(m[4], p[2], __builtin_fma(m[5], p[3], __builtin_fma(m[6], p[4], m[7])));
        const double pz = __builtin_fma(m[8], p[2], __builtin_fma(m[9], p[3], __builtin_fma(m[10], p[4], m[11])));
        const double a = __builtin_fma(p[0], pz, -px);
        const double b = __builtin_fma(p[1], pz, -py);
        const double lhs = __builtin_fma(b, b, a * a);
        const double rhs = (pz * pz) * T2d;
        const bool trust = ln.c * pmax <= fabs(pz);  // false on NaN
        return trust && (lhs > rhs);                 // false on NaN
    }
};

template <> struct Filter<kHomography> {
    static constexpr bool enabled = true;
    struct Lane { double c; };
    template <class MD> static __device__ __forceinline__ Lane prep(const MD& h, double guard) {
        const double l0 = fabs(h[0]) + fabs(h[1]) + fabs(h[2]);
        const double l1 = fabs(h[3]) + fabs(h[4]) + fabs(h[5]);
        const double l2 = fabs(h[6]) + fabs(h[7]) + fabs(h[8]);
        const double l = fmax(l0, fmax(l1, l2));
        return {(l > 1e-100 && l < 1e100) ? guard * l : 1.0 / 0.0};   // (see Filter<kPnP>)
    }
    template <class PT, class MD>
    static __device__ __forceinline__ bool reject(const PT& p, const MD& h, const Lane& ln, double pmax, double T2d) {
        const double t1 = __builtin_fma(h[0], p[0], __builtin_fma(h[1], p[1], h[2]));
        const double t2 = __builtin_fma(h[3], p[0], __builtin_fma(h[4], p[1], h[5]));
        const double t3 = __builtin_fma(h[6], p[0], __builtin_fma(h[7], p[1], h[8]));
        const double a = __builtin_fma(p[2], t3, -t1);
        const double b = __builtin_fma(p[3], t3, -t2);
        const double lhs = __builtin_fma(b, b, a * a);
        const double rhs = (t3 * t3) * T2d;
        const bool trust = ln.c * pmax <= fabs(t3);
        return trust && (lhs > rhs);
    }
};

// Symmetric transfer error, model [H | H^-1]: r^2 = fl(forward + backward) >= the forward term, which is computed in exactly
// the operation order of Residual<kHomography> (residuals.hip.h) - rounding is monotone and the backward term is >= 0 or NaN -
// so every pair the forward filters prove "not an inlier" is not an inlier of the symmetric residual either: the
// homography filters are reused on the first nine entries.  (The backward term is not filtered.)
template <> struct Filter<kHomographySym> : Filter<kHomography> {};

// ---- FP32 pre-filter -------------------------------------------------------------------------------
// Same inequality evaluated in single precision on f32 copies of the point (one 32-byte row: coords, scale) and of the
// hypothesis: 18 VALU ops at the f32 rate instead of 17 at the f64 rate.  Error budget: inputs rounded to f32 and three
// chained FMAs give |p~ - p*| <= E32 = 5.5 * 2^-24 * (L3_h P_i + t_h) (L3_h = largest 1-norm of the multiplying part of a
// row, t_h = largest |constant term|); with tau = 2^-10 the trust test E32 (1 + U + T) / (tau T) <= |p~z| (one FMA +
// compare per pair; constants rounded up) and the host guard U / T <= tau * 2^24 bound every error term by tau T |p~z|,
// and the chain of inequalities of §5.2 gives a~^2 + b~^2 <= p~z^2 T^2 (1 + 7.7 tau + O(tau^2) + 6 * 2^-24)
// < p~z^2 T^2 (1 + 2^-7) for every pair the exact path accepts.  Candidates go straight to the exact FP64 path.
constexpr double kFilter32Delta = 1.0 / 128.0;  // 2^-7
constexpr double kInflate = 1.000001;           // (float)(x * kInflate) >= x for every finite double x > 0

__device__ __forceinline__ float f32_up(double x) { return (float)(x * kInflate); }

// The f32 tests below are homogeneous in the hypothesis (a residual does not change when its model is multiplied by a constant -
// for lines the threshold scales along), but their intermediate SQUARES are not representable for every scale: a hypothesis
// 1e-24 times a perfectly good one (tests/soak_scoring.py found it) made pz^2 underflow to 0 before the multiplication by T2,
// and "lhs > 0" rejected true inliers.  Every f32 copy is therefore made from the hypothesis scaled by a power of two (exact)
// that brings its largest entry into [0.5, 1): returns that factor (1 when the largest entry is 0, Inf or NaN).
// *off: the hypothesis is outside the band of scales (largest entry in [1e-75, 1e75]) in which the EXACT path's own f64
// arithmetic neither overflows nor underflows for coordinates up to 1e30 (the dispatch checks that): outside it the oracle's
// residual is whatever IEEE makes of it (a vanishing point 1e158 away divides by inf and every segment becomes an "inlier"
// with residual 0), and only the exact path reproduces that - such a hypothesis is never rejected or culled.
template <int P, class MD> __device__ __forceinline__ double pow2_normaliser(const MD& m, bool* off)
{
    double mx = 0.0;
#pragma unroll
    for (int k = 0; k < P; ++k) { const double a = fabs(m[k]); if (a > mx) mx = a; }   // NaN entries are skipped by the comparison
    *off = !(mx >= 1e-75) || !(mx <= 1e75);
    if (!(mx > 0.0) || !(mx < 1.7976931348623157e308)) return 1.0;
    int e;
    (void)frexp(mx, &e);
    return ldexp(1.0, -e);
}

template <int MT> struct Filter32 {
    static constexpr bool enabled = false;
    static constexpr int kRowVals = 6;    // floats of a point's f32 row the filter reads
    static constexpr int kGroupVals = 9;  // floats of a group row the bound test reads
    struct Lane {};
    template <class MD> static __device__ __forceinline__ Lane prep(const MD&, double, double) { return {}; }
    static __device__ __forceinline__ bool reject(const float*, const Lane&, float) { return false; }
    static __device__ __forceinline__ bool group_reject(const float*, const Lane&, float) { return false; }
};

// The staged form of a hypothesis: the leading floats of Filter32<MT>::Lane that reject() reads.  The cull kernel stores them per
// hypothesis, the group-major kernel stages them in LDS and rebuilds a Lane from them for reject() (the rest of the lane is not
// touched there).  A type says so with `kStagedVals`; without it the whole lane is staged.
template <class F, class = void> struct StagedVals { static constexpr int value = (int)(sizeof(typename F::Lane) / sizeof(float)); };
template <class F> struct StagedVals<F, std::void_t<decltype(F::kStagedVals)>> { static constexpr int value = F::kStagedVals; };

// The wave's survivors of one hypothesis: bit i = lane i's pair is NOT rejected.  A filter whose reject() is the conjunction of two
// comparisons can hand them out one by one (reject_terms): each comparison's lane mask is a ballot as it stands, and the masks are
// combined on the scalar unit - the ballot of the combined bool goes through a 0 / 1 register and a second comparison in every lane.
template <class F, class = void> struct RejectTerms {
    static __device__ __forceinline__ unsigned long long passed(const float* p, const typename F::Lane& ln, float T2d) {
        return __builtin_amdgcn_ballot_w64(!F::reject(p, ln, T2d));
    }
};
template <class F> struct RejectTerms<F, std::void_t<decltype(&F::reject_terms)>> {
    static __device__ __forceinline__ unsigned long long passed(const float* p, const typename F::Lane& ln, float T2d) {
        bool a, b;
        F::reject_terms(p, ln, T2d, &a, &b);
        return ~(__builtin_amdgcn_ballot_w64(a) & __builtin_amdgcn_ballot_w64(b));   // (every lane of the wave is active in the step loop)
    }
};

// ---- group-level rejection ---------------------------------------------------------------------------
// The points are kept in Morton order of all their coordinates, so 64 consecutive points form a compact group: centre c
// and radius rho of the part the projective map multiplies, centre (ub, vb) and half extents (ru, rv) of the observed
// part.  For every point of the group |z_i - z_c| <= ||p_z|| rho =: dz (likewise dx, dy), hence
//   |u_i z_i - x_i| >= |ub z_c - x_c| - (ru (|z_c| + dz) + |ub| dz + dx)      and      T |z_i| <= T (|z_c| + dz),
// and an inlier needs |u_i z_i - x_i| < T |z_i| in both coordinates: if either lower bound exceeds the upper bound no
// point of the group is an inlier of this hypothesis.  Evaluated in f32 at the centre under the point filter's trust
// test (centre errors <= a few tau T |z_c|), radii and norms stored rounded up by 1e-5, T inflated by 2^-6.  A wave
// skips the 64 points when all of its 64 hypotheses reject the group (the batch is in locality order, so a wave's
// hypotheses look at the same image region): 74 % of the (wave, group) pairs of the metric batch.
// kGroupInflate, kGroupRow, kSuper: pgx_internal.h (shared with setpoints.hip, which builds the rows on the device)

template <> struct Filter32<kPnP> {
    static constexpr bool enabled = true;
    static constexpr int kRowVals = 6, kGroupVals = 9;
    struct Lane { float m[12]; float c1, c0; float n0, n1, n2; float nanh; };
    // reject() reads m, c1, c0 and nothing behind them (n0, n1, n2, nanh belong to group_reject, which the cull kernel runs from
    // registers): the staged form of a hypothesis - what the cull kernel stores and the group kernel stages - is this prefix
    static constexpr int kStagedVals = 14;
    static_assert(offsetof(Lane, c0) == (kStagedVals - 1) * sizeof(float) && offsetof(Lane, n0) == kStagedVals * sizeof(float), "m, c1, c0 lead the lane");
    template <class MD> static __device__ __forceinline__ Lane prep(const MD& m0, double guard32, double) {
        Lane ln;
        bool nan = false;
        bool off;
        const double sc = pow2_normaliser<12>(m0, &off);
        double m[12];
#pragma unroll
        for (int k = 0; k < 12; ++k) { m[k] = m0[k] * sc; ln.m[k] = (float)m[k]; nan |= !(m0[k] == m0[k]); }
        ln.nanh = nan ? 1.0f : 0.0f;  // a NaN entry makes every residual NaN (all 12 enter it): never an inlier
        ln.n0 = (float)(sqrt(m[0] * m[0] + m[1] * m[1] + m[2] * m[2]) * kGroupInflate);
        ln.n1 = (float)(sqrt(m[4] * m[4] + m[5] * m[5] + m[6] * m[6]) * kGroupInflate);
        ln.n2 = (float)(sqrt(m[8] * m[8] + m[9] * m[9] + m[10] * m[10]) * kGroupInflate);
        const double l3 = fmax(fabs(m[0]) + fabs(m[1]) + fabs(m[2]),
                               fmax(fabs(m[4]) + fabs(m[5]) + fabs(m[6]), fabs(m[8]) + fabs(m[9]) + fabs(m[10])));
        const double t = fmax(fabs(m[3]), fmax(fabs(m[7]), fabs(m[11])));
        ln.c1 = f32_up(guard32 * l3);
        ln.c0 = off ? __builtin_inff() : fmaxf(f32_up(guard32 * t), 1e-30f);   // inf: the trust test never holds
        return ln;
    }
    // p = (u, v, X, Y, Z, scale, -, -) in f32
    static __device__ __forceinline__ bool reject(const float* p, const Lane& ln, float T2d) {
        bool trust, over;
        reject_terms(p, ln, T2d, &trust, &over);
        return trust && over;
    }
    // the two comparisons reject() is the conjunction of, for a caller that wants their lane masks (RejectTerms below)
    static __device__ __forceinline__ void reject_terms(const float* p, const Lane& ln, float T2d, bool* trust, bool* over) {
        const float* m = ln.m;
        const float px = __builtin_fmaf(m[0], p[2], __builtin_fmaf(m[1], p[3], __builtin_fmaf(m[2], p[4], m[3])));
        const float py = __builtin_fmaf(m[4], p[2], __builtin_fmaf(m[5], p[3], __builtin_fmaf(m[6], p[4], m[7])));
        const float pz = __builtin_fmaf(m[8], p[2], __builtin_fmaf(m[9], p[3], __builtin_fmaf(m[10], p[4], m[11])));
        const float a = __builtin_fmaf(p[0], pz, -px);
        const float b = __builtin_fmaf(p[1], pz, -py);
        const float lhs = __builtin_fmaf(b, b, a * a);
        const float rhs = (pz * pz) * T2d;
        *trust = __builtin_fmaf(ln.c1, p[5], ln.c0) <= fabsf(pz);  // false on NaN
        *over = lhs > rhs;                                         // false on NaN
    }
    // g = (cX, cY, cZ, rho, ub, vb, ru, rv, scale, -, -, -)
    static __device__ __forceinline__ bool group_reject(const float* g, const Lane& ln, float Tup) {
        const float* m = ln.m;
        const float cx = __builtin_fmaf(m[0], g[0], __builtin_fmaf(m[1], g[1], __builtin_fmaf(m[2], g[2], m[3])));
        const float cy = __builtin_fmaf(m[4], g[0], __builtin_fmaf(m[5], g[1], __builtin_fmaf(m[6], g[2], m[7])));
        const float cz = __builtin_fmaf(m[8], g[0], __builtin_fmaf(m[9], g[1], __builtin_fmaf(m[10], g[2], m[11])));
        // NaN hypothesis: its residuals are NaN, never an inlier.  (Tested on the hypothesis itself: an entry that merely
        // overflows f32 gives inf - inf = NaN HERE although its f64 residuals may be perfectly good - such a group is kept,
        // every comparison below being false on NaN.)
        if (ln.nanh != 0.0f) return true;
        const bool trust = __builtin_fmaf(ln.c1, g[8], ln.c0) <= fabsf(cz);
        const float dz = ln.n2 * g[3], dx = ln.n0 * g[3], dy = ln.n1 * g[3];
        const float zs = fabsf(cz) + dz;
        const float ex = fabsf(__builtin_fmaf(g[4], cz, -cx)), ey = fabsf(__builtin_fmaf(g[5], cz, -cy));
        const float mx = __builtin_fmaf(g[6], zs, __builtin_fmaf(fabsf(g[4]), dz, dx));
        const float my = __builtin_fmaf(g[7], zs, __builtin_fmaf(fabsf(g[5]), dz, dy));
        const float tol = Tup * zs;
        return trust && ((ex - mx > tol) || (ey - my > tol));  // false on NaN/inf arithmetic
    }
};

// Homographies are scored in PIXEL coordinates (|coordinates| ~ 1e3): there the trust test of the PnP filter above (errors
// <= tau T |t3| with tau = 2^-10) fails for almost every pair - E32 (1 + U) ~ 0.5 px against tau T ~ 0.004 px - and the
// filter would pass everything on.  So this filter carries its error terms explicitly instead (like the vanishing-point and
// Sampson filters below): with E_t = 5.5 u (L2 P + t) + 4 eta bounding the f32 error of t1, t2, t3 AND the exact path's own
// f64 rounding (L2 = largest |h_a| + |h_b| of a row, t = largest |h_c|, P = max(|coordinates|, 1) rounded up),
//   |a~ - a*| <= E_a = E_t (1 + P) + 1.01 u (P |t3~| + |a~|)        (a = x2 t3 - t1: the product, the rounded x2, the FMA)
//   reject  <=>  max(|a~| - E_a, 0)^2 + max(|b~| - E_b, 0)^2  >  T2 (1 + 2^-6) (|t3~| + E_t)^2
// which implies (a*^2 + b*^2) / t3*^2 > T2 (1 + 2^-6)(1 - 8 u) and the computed r_c^2 >= that (1 - 10 eps) > T2.  Overflow of
// an f32 product makes E_a infinite (it contains P |t3~| and |a~|): inf - inf = NaN, not rejected.  No global guard.
// Group test: as for PnP with the same explicit terms at the group's scales - |u_i z_i - x_i| >= ex - mx - E_g and
// |z_i| <= |cz| + dz + E_t, E_g = E_t (1 + |ub|) + 1.01 u (|ub| |cz| + ex).
template <> struct Filter32<kHomography> {
    static constexpr bool enabled = true;
    static constexpr int kRowVals = 6, kGroupVals = 9;
    struct Lane { float m[9]; float e1, e0; float n0, n1, n2; float nanh; };
    template <class MD> static __device__ __forceinline__ Lane prep(const MD& h0, double, double) {
        Lane ln;
        bool nan = false;
        bool off;
        const double sc = pow2_normaliser<9>(h0, &off);
        double h[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) { h[k] = h0[k] * sc; ln.m[k] = (float)h[k]; nan |= !(h0[k] == h0[k]); }
        ln.nanh = nan ? 1.0f : 0.0f;
        ln.n0 = (float)(sqrt(h[0] * h[0] + h[1] * h[1]) * kGroupInflate);
        ln.n1 = (float)(sqrt(h[3] * h[3] + h[4] * h[4]) * kGroupInflate);
        ln.n2 = (float)(sqrt(h[6] * h[6] + h[7] * h[7]) * kGroupInflate);
        const double l2 = fmax(fabs(h[0]) + fabs(h[1]), fmax(fabs(h[3]) + fabs(h[4]), fabs(h[6]) + fabs(h[7])));
        const double t = fmax(fabs(h[2]), fmax(fabs(h[5]), fabs(h[8])));
        const double u = 5.9604644775390625e-8, eta = 1.1754943508222875e-38;
        ln.e1 = f32_up(5.5 * u * l2 + 4.0 * eta);
        ln.e0 = off ? __builtin_inff() : f32_up(5.5 * u * t + eta);   // inf: every error term is infinite, nothing is rejected
        return ln;
    }
    // p = (x1, y1, x2, y2, -, P, -, -) in f32, P = max(|all four coordinates|, 1) rounded up
    static __device__ __forceinline__ bool reject(const float* p, const Lane& ln, float T2d) {
        const float* h = ln.m;
        const float t1 = __builtin_fmaf(h[0], p[0], __builtin_fmaf(h[1], p[1], h[2]));
        const float t2 = __builtin_fmaf(h[3], p[0], __builtin_fmaf(h[4], p[1], h[5]));
        const float t3 = __builtin_fmaf(h[6], p[0], __builtin_fmaf(h[7], p[1], h[8]));
        const float a = fabsf(__builtin_fmaf(p[2], t3, -t1));
        const float b = fabsf(__builtin_fmaf(p[3], t3, -t2));
        const float Et = __builtin_fmaf(ln.e1, p[5], ln.e0);
        const float at3 = fabsf(t3);
        const float base = __builtin_fmaf(6.0202e-8f /* 1.01 u */ * p[5], at3, __builtin_fmaf(Et, p[5], Et));
        const float ma = fmaxf(a - __builtin_fmaf(6.0202e-8f, a, base), 0.0f);   // fmaxf(NaN, 0) = 0: never rejects on its own
        const float mb = fmaxf(b - __builtin_fmaf(6.0202e-8f, b, base), 0.0f);
        const float den = at3 + Et;
        return __builtin_fmaf(mb, mb, ma * ma) > (den * den) * T2d && (base == base);   // NaN / inf error terms: not rejected
    }
    // g = (c1x, c1y, 0, rho, x2b, y2b, r2x, r2y, scale, -, -, -)
    static __device__ __forceinline__ bool group_reject(const float* g, const Lane& ln, float Tup) {
        const float* h = ln.m;
        const float cx = __builtin_fmaf(h[0], g[0], __builtin_fmaf(h[1], g[1], h[2]));
        const float cy = __builtin_fmaf(h[3], g[0], __builtin_fmaf(h[4], g[1], h[5]));
        const float cz = __builtin_fmaf(h[6], g[0], __builtin_fmaf(h[7], g[1], h[8]));
        if (ln.nanh != 0.0f) return true;  // NaN entry: every residual is NaN
        const float Et = __builtin_fmaf(ln.e1, g[8], ln.e0);
        const float dz = ln.n2 * g[3], dx = ln.n0 * g[3], dy = ln.n1 * g[3];
        const float acz = fabsf(cz);
        const float zs = acz + dz + Et;
        const float ex = fabsf(__builtin_fmaf(g[4], cz, -cx)), ey = fabsf(__builtin_fmaf(g[5], cz, -cy));
        const float aub = fabsf(g[4]), avb = fabsf(g[5]);
        const float Egx = __builtin_fmaf(Et, aub, Et) + 6.0202e-8f * __builtin_fmaf(aub, acz, ex);
        const float Egy = __builtin_fmaf(Et, avb, Et) + 6.0202e-8f * __builtin_fmaf(avb, acz, ey);
        const float mx = __builtin_fmaf(g[6], zs, __builtin_fmaf(aub, dz, dx)) + Egx;
        const float my = __builtin_fmaf(g[7], zs, __builtin_fmaf(avb, dz, dy)) + Egy;
        const float tol = Tup * zs;
        return (ex - mx * 1.0001f > tol) || (ey - my * 1.0001f > tol);  // false on NaN / inf arithmetic
    }
};

// ---- vanishing points (vanishing_point_estimator.h:166-189) ---------------------------------------------------------------
// r = |N| / D with N = lx xs + ly ys + lz and D = ||(lx, ly)||, l = m x v (m = the segment's midpoint).  Expanding l gives
//   N = v0 a + v1 b + v2 c,   a = (ys - ye) / 2,  b = (xe - xs) / 2,  c = (xs ye - xe ys) / 2      (exact identity)
//   lx = my v2 - v1,  ly = v0 - mx v2
// so a segment's f32 row holds (a, b, c, mx, my, P, P^2), P = max(|coordinates|, 1) rounded up, and the filter is 17 f32
// operations without a division or a root.  Error budget (u = 2^-24, eps = 2^-53, tau = 2^-10):
//   |N~ - N*| <= E_N = 8 u (|v0||a| + |v1||b| + |v2||c|) + 2^-50 |v2| P^2      (inputs rounded to f32, three FMAs; c itself is
//                                                                              a difference of two f64 products)
//   ||(lx~, ly~) - (lx*, ly*)|| <= 6 u (P |v2| + |v0| + |v1|) =: E_D
//   the exact path's own f64 evaluation: |N_c - N*| <= 8 eps (2 P^2 |v2| + 3 P (|v0| + |v1|)) =: E64
// trust test  D~ >= t(P) = e2 P^2 + e1 P + e0  (constants below) makes E_D <= tau D and E64 <= tau T D; then
//   reject  <=>  trust  and  m := |N~| - E_N > 0  and  m^2 > T2 (1 + 2^-6) D~^2
// implies r* = |N*| / D* > T (1 + tau)^3 and the computed r_c >= r* (1 - tau) / (1 + tau) > T: the exact path would not
// have accepted.  NaN / Inf anywhere make a comparison false: not rejected.
// Group test: the same quantities on the group's box of ORIENTED, LENGTH-NORMALISED features (a, b, c) / h, h = half the
// segment length (the residual is h |sin angle(segment, direction to the vanishing point)|): with centre (A, B, C, MX, MY),
// radii (rA, rB, rC), rM = radius of the midpoints, hmin = the shortest half length,
//   |N^_i| >= |N^(centre)| - (|v0| rA + |v1| rB + |v2| rC),   D_i <= D(centre) + |v2| rM,
// and no member is an inlier when hmin (|N^c| - R_N) > T'' (Dc + R_D), under the trust test at Dc - R_D with the group's
// largest P.  Groups are 64 consecutive segments of the Hough order of their lines (theta, rho, length) - setpoints.hip sp_vp_rows_kernel.
template <> struct Filter32<kVanishingPoint> {
    static constexpr bool enabled = true;
    static constexpr int kRowVals = 7, kGroupVals = 12;
    struct Lane { float v[3]; float e2, e1, e0, e50, t2pp, invT, nanh; };
    template <class MD> static __device__ __forceinline__ Lane prep(const MD& v0, double, double T2) {
        Lane ln;
        bool off;
        const double sc = pow2_normaliser<3>(v0, &off);
        const double v[3] = {v0[0] * sc, v0[1] * sc, v0[2] * sc};
        ln.v[0] = (float)v[0]; ln.v[1] = (float)v[1]; ln.v[2] = (float)v[2];
        ln.nanh = (v0[0] == v0[0] && v0[1] == v0[1] && v0[2] == v0[2]) ? 0.0f : 1.0f;
        const double V1 = fabs(v[0]) + fabs(v[1]), V2 = fabs(v[2]), T = sqrt(T2);
        const double k38 = 3.637978807091713e-12 /* 2^-38 */, k11 = 4.8828125e-4 /* 2^-11 */;
        ln.e2 = f32_up(k38 * V2 / T * 1.001);
        ln.e1 = f32_up((k11 * V2 + k38 * V1 / T) * 1.001);
        ln.e0 = off ? __builtin_inff() : fmaxf(f32_up(k11 * V1 * 1.001), 1e-37f);   // inf: the trust test never holds
        ln.e50 = f32_up(8.881784197001252e-16 /* 2^-50 */ * V2 * 1.001);
        ln.t2pp = f32_up(T2 * (1.0 + 1.0 / 64.0));
        ln.invT = (float)(1.0 / (T * (1.0 + 1.0 / 64.0)) * 0.99999);  // rounded DOWN: 1 / T''
        return ln;
    }
    // p = (a, b, c, mx, my, P, P^2, -) in f32
    static __device__ __forceinline__ bool reject(const float* p, const Lane& ln, float) {
        const float* v = ln.v;
        const float N = __builtin_fmaf(v[0], p[0], __builtin_fmaf(v[1], p[1], v[2] * p[2]));
        const float S = __builtin_fmaf(fabsf(v[0]), fabsf(p[0]), __builtin_fmaf(fabsf(v[1]), fabsf(p[1]), fabsf(v[2]) * fabsf(p[2])));
        const float lx = __builtin_fmaf(p[4], v[2], -v[1]);
        const float ly = __builtin_fmaf(-p[3], v[2], v[0]);
        const float D2 = __builtin_fmaf(lx, lx, ly * ly);
        const float tt = __builtin_fmaf(ln.e2, p[6], __builtin_fmaf(ln.e1, p[5], ln.e0));
        const float m = fabsf(N) - __builtin_fmaf(4.76837158203125e-7f /* 8 u */, S, ln.e50 * p[6]);
        return (D2 >= tt * tt) && (m > 0.0f) && (m * m > ln.t2pp * D2);  // every comparison is false on NaN
    }
    // g = (A, B, C, MX, MY, rA, rB, rC, rM, hmin, Pmax, P2max)
    static __device__ __forceinline__ bool group_reject(const float* g, const Lane& ln, float) {
        const float* v = ln.v;
        if (ln.nanh != 0.0f) return true;  // NaN entry in the hypothesis: every residual is NaN, never an inlier
        const float N = __builtin_fmaf(v[0], g[0], __builtin_fmaf(v[1], g[1], v[2] * g[2]));
        const float S = __builtin_fmaf(fabsf(v[0]), fabsf(g[0]), __builtin_fmaf(fabsf(v[1]), fabsf(g[1]), fabsf(v[2]) * fabsf(g[2])));
        const float RN = __builtin_fmaf(fabsf(v[0]), g[5], __builtin_fmaf(fabsf(v[1]), g[6], fabsf(v[2]) * g[7]));
        const float lx = __builtin_fmaf(g[4], v[2], -v[1]);
        const float ly = __builtin_fmaf(-g[3], v[2], v[0]);
        const float D2 = __builtin_fmaf(lx, lx, ly * ly);
        const float RD = fabsf(v[2]) * g[8] * 1.001f;
        const float tt0 = __builtin_fmaf(ln.e2, g[11], __builtin_fmaf(ln.e1, g[10], ln.e0));
        const float tt = tt0 + RD;  // trust at Dc - R_D
        const float L = fabsf(N) - RN * 1.001f - 1.9073486328125e-6f /* 32 u */ * S;
        const float G = L * g[9] * ln.invT - RD;
        // Trust: every member's D must stay above t(Pmax).  Two lower bounds on D_i: Dc - R_D (midpoints within rM of the centre), and
        // the member's own |N^_i| >= L - the distance of the vanishing point from the segment's LINE never exceeds its distance from the
        // midpoint ON that line (D_i = |v2| |m_i - vp| >= |v2| dist(vp, line_i) = |N^_i|).  The second one is what lets groups of
        // collinear segments spread over the whole image (Hough order, setpoints.hip) be culled: their rM is hundreds of pixels.
        const bool trust = (D2 >= tt * tt * 1.001f) || (L >= tt0 * 1.01f);
        return trust && (G > 0.0f) && (G * G > D2 * 1.004f);
    }
};

// ---- fundamental matrices: Sampson distance [U-2] (residuals.hip.h Residual<kFundamental>) -----------------------------------
// n(p) = x_b^T F x_a (x_a = (p0, p1, 1), x_b = (p2, p3, 1)) is BILINEAR in the four image coordinates and the Sampson
// denominator is the squared norm of its gradient: (rxc, ryc, rx, ry) = (dn/dp0, dn/dp1, dn/dp2, dn/dp3).  So the squared
// residual is n^2 / |grad n|^2 and the filter needs neither the division nor a root: 21 f32 operations per pair.
// With A4 = |f0| + |f1| + |f3| + |f4|, B4 = |f2| + |f5| + |f6| + |f7|, P = max(|coordinates|, 1) rounded up, u = 2^-24,
// eta = 2^-126 (an operation that underflows may be flushed), tau = 2^-10:
//   |n~ - n*| and |n_c - n*| (the exact path's own f64 evaluation) together  <= E_n = 8.5 u (A4 P^2 + B4 P + |f8|) + 16 eta P^2
//                                   (inputs rounded to f32, at most seven roundings on any of the nine terms)
//   ||grad~ - grad*|| + ||grad_c - grad*||  <= E_D = 4.1 u (2 A4 P + B4) + 8 eta P      (four components, two FMAs each)
// trust test  D~ >= t(P) = E_D / tau  gives D_c <= D~ (1 + 1.01 tau)^2 (D~ = ||grad~||), and then
//   reject  <=>  trust  and  m := |n~| - E_n > 0  and  m^2 > T2 (1 + 2^-6) D~^2
// implies the computed r_c^2 = fl(fl(n_c^2) / D_c) >= m^2 / (D~^2 (1 + 1.01 tau)^2) (1 - 3 eps) > T2: the exact path would not have
// accepted.  NaN / Inf make a comparison false: not rejected; a hypothesis with |f_k| Pmax^2 > 1e36 for some entry (a term of
// n~ could overflow f32 and not the one that cancels it) gets t(P) = inf and is never rejected; one with a NaN entry has NaN
// residuals everywhere (all nine entries enter n) and is culled outright.
// Group test: for a member c + d of the group (d1, d2 = the offsets in the two images, |d1| <= r1, |d2| <= r2, |d| <= R),
//   n(c + d) = n(c) + grad n(c) . d + d2^T A d1,   A = (f0 f1; f3 f4),        grad n(c + d) = grad n(c) + (A^T d2, A d1),
// so |n| >= |n(c)| - ||grad n(c)|| R - ||A|| r1 r2 and ||grad n|| <= ||grad n(c)|| + ||A|| R: no member is an inlier when
//   |n~(c)| - E_n - (G + E_D) R - ||A||_F r1 r2  >  T'' (G + E_D + ||A||_F R),   G = ||grad~(c)||,
// the error terms taken at the group's largest P (the centre lies inside the box), every subtracted term inflated.
// Groups are 64 consecutive points of the Morton order of all four coordinates (setpoints.hip): 51 % of the (hypothesis,
// group) pairs of the C3 set are culled (scripts/analysis_sampson_bound.py; per-coordinate extents would give 53 %).
template <> struct Filter32<kFundamental> {
    static constexpr bool enabled = true;
    static constexpr int kRowVals = 7, kGroupVals = 9;
    struct Lane { float f[9]; float e1, e0, n2, n1, n0, t2pp, nA, nanh; };
    template <class MD> static __device__ __forceinline__ Lane prep(const MD& f0, double pscale2 /* max(|coordinate|, 1)^2 over the point set */, double T2) {
        Lane ln;
        bool nan = false, big = false;
        bool off;
        const double sc = pow2_normaliser<9>(f0, &off);
        big = off;
        double f[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) { f[k] = f0[k] * sc; ln.f[k] = (float)f[k]; nan |= !(f0[k] == f0[k]); big |= !(fabs(f[k]) * pscale2 <= 1e36); }
        ln.nanh = nan ? 1.0f : 0.0f;
        const double A4 = fabs(f[0]) + fabs(f[1]) + fabs(f[3]) + fabs(f[4]), B4 = fabs(f[2]) + fabs(f[5]) + fabs(f[6]) + fabs(f[7]);
        const double u = 5.9604644775390625e-8, eta = 1.1754943508222875e-38, itau = 1024.0;
        ln.e1 = f32_up((4.1 * u * 2.0 * A4 + 8.0 * eta) * itau);
        ln.e0 = big ? __builtin_inff() : fmaxf(f32_up(4.1 * u * B4 * itau), 1e-12f);
        ln.n2 = f32_up(8.5 * u * A4 + 16.0 * eta);
        ln.n1 = f32_up(8.5 * u * B4);
        ln.n0 = f32_up(8.5 * u * fabs(f[8]));
        ln.t2pp = f32_up(T2 * (1.0 + 1.0 / 64.0));
        ln.nA = f32_up(sqrt(f[0] * f[0] + f[1] * f[1] + f[3] * f[3] + f[4] * f[4]) * 1.001);
        return ln;
    }
    // p = (x_a, y_a, x_b, y_b, -, P, P^2, -) in f32
    static __device__ __forceinline__ bool reject(const float* p, const Lane& ln, float) {
        const float* f = ln.f;
        const float rxc = __builtin_fmaf(f[0], p[2], __builtin_fmaf(f[3], p[3], f[6]));
        const float ryc = __builtin_fmaf(f[1], p[2], __builtin_fmaf(f[4], p[3], f[7]));
        const float rwc = __builtin_fmaf(f[2], p[2], __builtin_fmaf(f[5], p[3], f[8]));
        const float n = __builtin_fmaf(p[0], rxc, __builtin_fmaf(p[1], ryc, rwc));
        const float rx = __builtin_fmaf(f[0], p[0], __builtin_fmaf(f[1], p[1], f[2]));
        const float ry = __builtin_fmaf(f[3], p[0], __builtin_fmaf(f[4], p[1], f[5]));
        const float D2 = __builtin_fmaf(rxc, rxc, __builtin_fmaf(ryc, ryc, __builtin_fmaf(rx, rx, ry * ry)));
        const float tt = __builtin_fmaf(ln.e1, p[5], ln.e0);
        const float m = fabsf(n) - __builtin_fmaf(ln.n2, p[6], __builtin_fmaf(ln.n1, p[5], ln.n0));
        return (D2 >= tt * tt) && (m > 0.0f) && (m * m > ln.t2pp * D2);  // every comparison is false on NaN
    }
    // g = (ca_x, ca_y, cb_x, cb_y, r1, r2, R, Pmax, P2max, -, -, -)
    static __device__ __forceinline__ bool group_reject(const float* g, const Lane& ln, float Tup) {
        const float* f = ln.f;
        if (ln.nanh != 0.0f) return true;  // NaN entry in the hypothesis: every residual is NaN, never an inlier
        const float rxc = __builtin_fmaf(f[0], g[2], __builtin_fmaf(f[3], g[3], f[6]));
        const float ryc = __builtin_fmaf(f[1], g[2], __builtin_fmaf(f[4], g[3], f[7]));
        const float rwc = __builtin_fmaf(f[2], g[2], __builtin_fmaf(f[5], g[3], f[8]));
        const float n = __builtin_fmaf(g[0], rxc, __builtin_fmaf(g[1], ryc, rwc));
        const float rx = __builtin_fmaf(f[0], g[0], __builtin_fmaf(f[1], g[1], f[2]));
        const float ry = __builtin_fmaf(f[3], g[0], __builtin_fmaf(f[4], g[1], f[5]));
        const float D2 = __builtin_fmaf(rxc, rxc, __builtin_fmaf(ryc, ryc, __builtin_fmaf(rx, rx, ry * ry)));
        const float ED = __builtin_fmaf(ln.e1, g[7], ln.e0) * 9.765625e-4f /* tau */;   // inf for a hypothesis beyond f32: never culled
        const float G = __builtin_sqrtf(D2) * 1.001f + ED;
        const float En = __builtin_fmaf(ln.n2, g[8], __builtin_fmaf(ln.n1, g[7], ln.n0));
        const float L = fabsf(n) - En - (G * g[6] + ln.nA * g[4] * g[5]) * 1.001f;
        const float U = __builtin_fmaf(ln.nA, g[6], G) * 1.001f;
        return L > Tup * U;  // false on NaN / Inf arithmetic
    }
};

// ---- symmetric transfer error: the homography filter and group bound on the forward part (see Filter<kHomographySym>) --------
template <> struct Filter32<kHomographySym> : Filter32<kHomography> {
    template <class MD> static __device__ __forceinline__ Lane prep(const MD& h, double guard32, double T2) {
        Lane ln = Filter32<kHomography>::prep(h, guard32, T2);
        bool nan = false;
#pragma unroll
        for (int k = 0; k < 18; ++k) nan |= !(h[k] == h[k]);   // a NaN anywhere (also in the inverse) makes every residual NaN
        ln.nanh = nan ? 1.0f : 0.0f;
        return ln;
    }
};

// ---- the flat family: 2-D lines [U-4] and 3-D planes, r = |n . p + d| (FlatResidual<DIM>), inlier iff r^2 < T2 ------------------
// The model is homogeneous: the f32 copies are made from the model after the exact power-of-two scaling and tested against the
// threshold scaled along (Ts = T sc must be an ordinary f32 as well).  Per point, DIM + 1 inputs and DIM f32 FMAs, right-nested with
// the constant innermost - this operation order is the contract of the f32 test (tests restate it in numpy):
//   DIM = 2   n~ = fma(a~, x~, fma(b~, y~, c~))                         P = max(|x|, |y|, 1) rounded up
//   DIM = 3   n~ = fma(a~, x~, fma(b~, y~, fma(c~, z~, d~)))            P = max(|x|, |y|, |z|, 1) rounded up
// every input rounded to f32; u = 2^-24, eta = 2^-126.  Relative roundings each term of n* = n . p + d carries in the f32 chain (its
// two inputs, and every fma from its own outwards):
//                       DIM = 2                        DIM = 3
//   a x                 a~, x~, the outer fma     3    a~, x~, the outer fma          3
//   b y                 b~, y~, both fmas         4    b~, y~, the two outer fmas     4
//   c z                 -                              c~, z~, all three fmas         5
//   constant term       c~, both fmas             3    d~, all three fmas             4
// so |n~ - n*| <= k u (sum |n_j p_j| + |d|) + O(u^2) with k = 4 (DIM = 2), 5 (DIM = 3); the exact path's own f64 chain (product and
// DIM sums: <= (DIM + 1) * 2^-53 per term) and the O(u^2) terms fit in the extra 0.1 u.  Absolute (subnormal) errors, each < eta: the
// DIM coefficients times a coordinate (DIM eta P), the DIM coordinates times a coefficient of magnitude < 1 (the normaliser: DIM eta),
// the DIM fma results and the constant's copy (DIM + 1 eta): 3 eta P + 7 eta <= 6 eta P + 4 eta for P >= 1 (DIM = 3); 2 eta P + 5 eta
// <= 4 eta P + eta for P >= 2 (DIM = 2), and below that the missing 4 eta vanish in the 0.1 u slack, which is at least 0.05 u: the
// normaliser leaves the largest entry in [0.5, 1), so S P + |d| >= 0.5 (sc = 1 for an all-zero model, which is switched off below).
// Hence, with S = sum |n_j|,
//   |n~ - n*| + |n_c - n*| (the exact path's own rounding)  <=  E = e1 P + e0
//                 e1                       e0
//   DIM = 2       4.1 u S + 4 eta          4.1 u |d| + eta
//   DIM = 3       5.1 u S + 6 eta          5.1 u |d| + 4 eta             (kept as the literals of FlatBudget<DIM>, not computed)
//   reject  <=>  m := |n~| - E > T'' = T (1 + 2^-6):  then |n_c| > T (1 + 2^-7) (m itself is rounded once) and the computed
//   r_c^2 = fl(n_c^2) > T2.
// Group test on the DIM-ball (centre, radius R, Pmax) of 64 Morton-consecutive points (sp_line_bounds_kernel<SPAN, DIM>): for p in
// the ball |n(p)| >= |n(centre)| - ||n|| R, the error term taken at the group's largest P (which bounds the stored centre too):
//   reject the group  <=>  |n~(centre)| - ||n|| R - E(Pmax) > T''  (each factor inflated by 1.001).
// Switch-off: a coefficient times the set's largest P beyond 1e36, a constant term beyond 1e36, a threshold outside the ordinary f32
// range or a model outside pow2_normaliser's band gives E = inf (never rejected); a NaN entry culls the hypothesis outright (all
// DIM + 1 entries enter every residual).  The dense kernel costs ~10 instructions per pair, so the filter itself buys nothing - the
// cull does: a line's inliers are a strip, a plane's a slab of width 2T, and the cull removes most (hypothesis, group) pairs.
template <int DIM> struct FlatBudget;
template <> struct FlatBudget<2> { static constexpr double k = 4.1, eta1 = 4.0, eta0 = 1.0; };
template <> struct FlatBudget<3> { static constexpr double k = 5.1, eta1 = 6.0, eta0 = 4.0; };

template <int DIM> struct FlatFilter32 {
    static constexpr bool enabled = true;
    static constexpr int kRowVals = 6, kGroupVals = DIM + 2;
    struct Lane { float n[DIM + 1]; float e1, e0, nrm, tpp, nanh; };   // a row of floats in this order (score.hip HypRow)
    static_assert(offsetof(Lane, e1) == (DIM + 1) * sizeof(float) && offsetof(Lane, nanh) == (DIM + 5) * sizeof(float) &&
                  sizeof(Lane) == (DIM + 6) * sizeof(float), "coefficients, e1, e0, nrm, tpp, nanh");
    template <class MD> static __device__ __forceinline__ Lane prep(const MD& m0, double pscale /* max(|coordinate|, 1) over the set */, double T2) {
        Lane ln;
        // r = |n . p + d| scales with the model: the scaled copy is tested against the scaled threshold (sc is a power of two)
        bool off;
        const double sc = pow2_normaliser<DIM + 1>(m0, &off);
        double m[DIM + 1];
        bool nan = false;
#pragma unroll
        for (int k = 0; k <= DIM; ++k) { m[k] = m0[k] * sc; ln.n[k] = (float)m[k]; nan |= !(m0[k] == m0[k]); }
        ln.nanh = nan ? 1.0f : 0.0f;
        const double Ts = sqrt(T2) * sc;   // the threshold in the scaled model's units: must be an ordinary f32 as well
        bool big = !(fabs(m[DIM]) <= 1e36) || !(Ts > 1e-30) || !(Ts < 1e30) || off;
        double l1 = fabs(m[0]), n2 = m[0] * m[0];
#pragma unroll
        for (int k = 1; k < DIM; ++k) { l1 = l1 + fabs(m[k]); n2 = n2 + m[k] * m[k]; }
#pragma unroll
        for (int k = 0; k < DIM; ++k) big |= !(fabs(m[k]) * pscale <= 1e36);
        using B = FlatBudget<DIM>;
        const double u = 5.9604644775390625e-8, eta = 1.1754943508222875e-38;
        ln.e1 = f32_up(B::k * u * l1 + B::eta1 * eta);
        ln.e0 = big ? __builtin_inff() : f32_up(B::k * u * fabs(m[DIM]) + B::eta0 * eta);
        ln.nrm = f32_up(sqrt(n2) * 1.001);
        ln.tpp = f32_up(Ts * (1.0 + 1.0 / 64.0));
        return ln;
    }
    static __device__ __forceinline__ float dot(const float* p, const Lane& ln) {
        float n = ln.n[DIM];
#pragma unroll
        for (int k = DIM - 1; k >= 0; --k) n = __builtin_fmaf(ln.n[k], p[k], n);
        return n;
    }
    // p = (coordinates[DIM], -, .., P, -, -) in f32, P at p[5]
    static __device__ __forceinline__ bool reject(const float* p, const Lane& ln, float) {
        const float m = fabsf(dot(p, ln)) - __builtin_fmaf(ln.e1, p[5], ln.e0);
        return m > ln.tpp;  // false on NaN / inf - inf
    }
    // g = (centre[DIM], R, Pmax)
    static __device__ __forceinline__ bool group_reject(const float* g, const Lane& ln, float) {
        if (ln.nanh != 0.0f) return true;  // NaN entry in the hypothesis: every residual is NaN, never an inlier
        const float m = fabsf(dot(g, ln)) - __builtin_fmaf(ln.e1, g[DIM + 1], ln.e0) - ln.nrm * g[DIM] * 1.001f;
        return m > ln.tpp * 1.001f;
    }
};
template <> struct Filter32<kLine2D> : FlatFilter32<2> {};
template <> struct Filter32<kPlane3D> : FlatFilter32<3> {};

// ---- the round family: 2-D circles and 3-D spheres, r = |sqrt(d . d) - cr| (RoundResidual<DIM>), inlier iff r^2 < T2 ----------------
// Not homogeneous in the model (the centre is a point, the radius a length): no power-of-two scaling, the f32 copies are the model's
// entries rounded once.  Per point, in f32, right-nested with the innermost term a plain product - this operation order is the
// contract of the f32 test (tests restate it in numpy):
//   d~ = p~ - c~ (componentwise),  s~ = sqrtf(q~),  n~ = s~ - r~,
//   DIM = 2   q~ = fma(dx, dx, dy dy)                     P = max(|x|, |y|, 1) rounded up
//   DIM = 3   q~ = fma(dx, dx, fma(dy, dy, dz dz))        P = max(|x|, |y|, |z|, 1) rounded up
// With u = 2^-24, eta = 2^-126, s* = |p - c| (exact), |.| the Euclidean norm; every coefficient derived for both term counts:
//   inputs     |p~ - p| <= u |p| <= sqrt(DIM) u P  (sqrt(2) u P | sqrt(3) u P),  |c~ - c| <= u |c|,  |r~ - cr| <= u |cr|;  s is
//              1-Lipschitz in p and in c, so these move s by at most sqrt(DIM) u P + u |c|, and n by u |cr| more
//   d~         one rounding per component: |d~ - (p~ - c~)| <= u |p~ - c~| <= u s* + O(u^2)                       (both dimensions)
//   q~         DIM non-negative terms; the innermost is rounded as a product and again by every fma outside it, the outermost by its
//              fma alone: at most DIM roundings on a term, q~ = |d~|^2 (1 + t), |t| <= DIM u + O(u^2) -> after the root DIM / 2 u
//              (DIM = 2: dy dy 2 roundings, dx dx 1, 2 u -> 1 u  |  DIM = 3: at most three each, 3 u -> 1.5 u)
//   sqrtf      gfx950 lowers sqrtf (no fast-math) to v_sqrt_f32 plus a correction step and a denormal scaling; the budget takes
//              only v_sqrt_f32's documented 1 ulp = 2 u, whatever correction the lowering adds (correct rounding would be u)
//   exact path d (1 rounding), the sum of squares (DIM = 2: 2 on the larger term -> 1 after the root), sqrt (1), in f64:
//              <= 3 * 2^-53 s* < 0.01 u s* (DIM = 2), <= 3.5 * 2^-53 s* (~0.25 u s* is charged, DIM = 3); and 2^-53 |s_c - cr| for the
//              final subtraction, which is part of the T'' margin below
//   n~         the subtraction s~ - r~ is rounded once, relatively: n~ = (s~ - r~)(1 + t), |t| <= u (<= u s~ + u |cr|).  It is charged
//              to the T'' margin and not to E: m > T'' gives |s~ - r~| >= (T'' + E) (1 - u), and T (1 + 2^-6)(1 - u) > T (1 + 2^-7),
//              E (1 - u) >= the sum of the terms above as soon as E carries a relative margin of u over them (it carries > 10 %)
// so |(s~ - r~) - (s_c - cr)| <= sqrt(DIM) u P + u (|c| + |cr|) + k_s u s* + O(u^2),
//              k_s = 1 + 1 + 2 + 0.01 = 4.01 (DIM = 2),   1 + 1.5 + 2 + 0.25 = 4.75 (DIM = 3).
// Underflow: the products and fmas below 2^-126 carry absolute errors <= eta each (even with denormals flushed), and a subnormal
// difference d~ is exact (flushed: off by < eta, which moves s by < 2 eta); DIM = 2: 2 eta under the root move it by <= sqrt(2 eta) <
// 1.6e-19, DIM = 3: 4 eta, sqrt(4 eta) < 2.2e-19.
// One set of coefficients serves both dimensions; each bounds its term with room (more than 10 % for DIM = 3, more for DIM = 2) for
// evaluating E itself in f32 (three roundings, < 4 u relative) and for writing s~ for s* (the difference is O(u) s*):
//   E = e1 P + e0 + e2 s~     e1 = 2 u                          >= 1.41 * sqrt(2) u,  1.15 * sqrt(3) u
//                             e0 = 2 u (|c| + |cr|) + 1e-18     >= 2 * u (|c| + |cr|) + 6 * 1.6e-19, + 4 * 2.2e-19   (|c| inflated by 1.001 on top)
//                             e2 = 8 u                          >= 1.99 * 4.01 u,  1.68 * 4.75 u
//   reject  <=>  m := |n~| - E > T'' = T (1 + 2^-6):  m is rounded once and monotonically, so |s_c - cr| > T (1 + 2^-7), and the
//   computed r_c^2 = fl(fl(|s_c - cr|)^2) > T2.
// Group test on the DIM-ball (stored centre g, radius rho, Pmax) of 64 Morton-consecutive points (sp_line_bounds_kernel<SPAN, DIM>,
// the rows of the flat family): every member's distance to the model's centre lies in [s_g - rho, s_g + rho], s_g = |g - c| (g is an
// f32 value: no input rounding, the e1 Pmax term is kept all the same), so its residual is at least the distance from cr to that
// interval, |s_g - cr| - rho, less the errors above with P = Pmax and s* <= s_g + rho:
//   reject the group  <=>  |s~_g - r~| - E(Pmax, s~_g + rho) - 1.001 rho > 1.001 T''.
// One rule for points outside the shell, inside it, for r = 0 (the residual is s) and for r < 0 (every residual is s + |r|).  A NaN
// entry culls the hypothesis (all DIM + 1 enter every residual).  A set with coordinates beyond 1e17, a centre or radius beyond 1e17
// (q~ must stay below the f32 overflow) or a threshold outside the ordinary f32 range gives E = inf: never rejected, the exact path
// decides (r = inf included: inf - inf is NaN, and a NaN comparison is false).  Scenes far from the origin lose the filter's
// precision (e1 P grows with the offset, not with the scene): correct, only slower.
template <int DIM> struct RoundFilter32 {
    static constexpr bool enabled = true;
    static constexpr int kRowVals = 6, kGroupVals = DIM + 2;
    struct Lane { float c[DIM]; float r, e1, e0, e2, tpp, nanh; };   // a row of floats in this order (score.hip HypRow)
    static_assert(offsetof(Lane, r) == DIM * sizeof(float) && offsetof(Lane, nanh) == (DIM + 5) * sizeof(float) &&
                  sizeof(Lane) == (DIM + 6) * sizeof(float), "centre, r, e1, e0, e2, tpp, nanh");
    template <class MD> static __device__ __forceinline__ Lane prep(const MD& m, double pscale /* max(|coordinate|, 1) over the set */, double T2) {
        Lane ln;
        bool nan = !(m[DIM] == m[DIM]);
        double c2 = m[0] * m[0];
#pragma unroll
        for (int k = 1; k < DIM; ++k) c2 = c2 + m[k] * m[k];
#pragma unroll
        for (int k = 0; k < DIM; ++k) { ln.c[k] = (float)m[k]; nan |= !(m[k] == m[k]); }
        ln.r = (float)m[DIM];
        ln.nanh = nan ? 1.0f : 0.0f;
        const double Ts = sqrt(T2);
        const double cn = sqrt(c2) * 1.001;
        const bool big = !(pscale <= 1e17) || !(cn <= 1e17) || !(fabs(m[DIM]) <= 1e17) || !(Ts > 1e-30) || !(Ts < 1e30);
        const double u = 5.9604644775390625e-8;
        ln.e1 = f32_up(2.0 * u);
        ln.e0 = big ? __builtin_inff() : f32_up(2.0 * u * (cn + fabs(m[DIM])) + 1e-18);
        ln.e2 = f32_up(8.0 * u);
        ln.tpp = f32_up(Ts * (1.0 + 1.0 / 64.0));
        return ln;
    }
    static __device__ __forceinline__ float dist(const float* p, const Lane& ln) {
        float d[DIM];
#pragma unroll
        for (int k = 0; k < DIM; ++k) d[k] = p[k] - ln.c[k];
        float q = d[DIM - 1] * d[DIM - 1];
#pragma unroll
        for (int k = DIM - 2; k >= 0; --k) q = __builtin_fmaf(d[k], d[k], q);
        return sqrtf(q);
    }
    // p = (coordinates[DIM], -, .., P, -, -) in f32, P at p[5]
    static __device__ __forceinline__ bool reject(const float* p, const Lane& ln, float) {
        const float s = dist(p, ln);
        const float m = fabsf(s - ln.r) - (__builtin_fmaf(ln.e1, p[5], ln.e0) + ln.e2 * s);
        return m > ln.tpp;  // false on NaN / inf - inf
    }
    // g = (centre[DIM], rho, Pmax)
    static __device__ __forceinline__ bool group_reject(const float* g, const Lane& ln, float) {
        if (ln.nanh != 0.0f) return true;
        const float s = dist(g, ln);
        const float m = fabsf(s - ln.r) - (__builtin_fmaf(ln.e1, g[DIM + 1], ln.e0) + ln.e2 * (s + g[DIM])) - g[DIM] * 1.001f;
        return m > ln.tpp * 1.001f;
    }
};
template <> struct Filter32<kCircle2D> : RoundFilter32<2> {};
template <> struct Filter32<kSphere3D> : RoundFilter32<3> {};

// ---- the axial family: 3-D lines, cylinders, cones and tori - a residual made of the distance to an axis (p, d) ------------------------
// What the four filters share is stated here once; what each one derives - its operation order, its error budget E = e1 P + e0 + e2 l~,
// its switch-off cases - is stated with its shape below (LineShape32, CylinderShape32, ConeShape32, TorusShape32), and every shape's
// derivation builds on the 3-D line's.  An axial type supplies: its Lane (p[3], d[3], its own fields, then e1, e0, e2, tpp, nrm, nanh)
// with kStagedVals, kModelVals (the model entries, every one of which enters every residual), budget() - its own lane fields in the
// filter's units, its own switch-off cases, and e1, e0, e2, nrm - and magnitude(), the non-negative quantity that is compared.
//
// s~ and l~ of a point or a centre, for any lane with p[3] and d[3] (the 3-D line's derivation states the operation order)
template <class L> __device__ __forceinline__ float axial_dist(const float* p, const L& ln, float* l1) {
    const float e0 = p[0] - ln.p[0], e1 = p[1] - ln.p[1], e2 = p[2] - ln.p[2];
    const float* d = ln.d;
    const float c0 = __builtin_fmaf(e1, d[2], -(e2 * d[1]));
    const float c1 = __builtin_fmaf(e2, d[0], -(e0 * d[2]));
    const float c2 = __builtin_fmaf(e0, d[1], -(e1 * d[0]));
    *l1 = (fabsf(e0) + fabsf(e1)) + fabsf(e2);
    return sqrtf(__builtin_fmaf(c0, c0, __builtin_fmaf(c1, c1, c2 * c2)));
}
// h~ of the same point: axial_dist's own e~ (the same subtractions), then the dot product with d~ (the cone's derivation)
template <class L> __device__ __forceinline__ float axial_height(const float* p, const L& ln) {
    const float e0 = p[0] - ln.p[0], e1 = p[1] - ln.p[1], e2 = p[2] - ln.p[2];
    return __builtin_fmaf(e2, ln.d[2], __builtin_fmaf(e1, ln.d[1], e0 * ln.d[0]));
}

template <class Shape> struct AxialFilter32 : Shape {
    using Lane = typename Shape::Lane;
    static constexpr bool enabled = true;
    static constexpr int kRowVals = 6, kGroupVals = 5;
    template <class MD> static __device__ __forceinline__ Lane prep(const MD& m, double pscale /* max(|coordinate|, 1) over the set */, double T2) {
        Lane ln;
        const double d0[3] = {m[3], m[4], m[5]};
        bool off;
        const double sc = pow2_normaliser<3>(d0, &off);
        bool nan = false;
#pragma unroll
        for (int k = 6; k < Shape::kModelVals; ++k) nan |= !(m[k] == m[k]);
        double d[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            d[k] = d0[k] * sc;
            ln.p[k] = (float)m[k];
            ln.d[k] = (float)d[k];
            nan |= !(m[k] == m[k]) || !(d0[k] == d0[k]);
        }
        ln.nanh = nan ? 1.0f : 0.0f;
        const double Ts = sqrt(T2) * sc;   // the threshold in the scaled direction's units: must be an ordinary f32 as well
        const double dn = sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]) * 1.001;
        const double pn = sqrt((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2]) * 1.001;
        const bool out = !(pscale <= 1e17) || !(pn <= 1e17) || !(Ts > 1e-30) || !(Ts < 1e30) || off;   // the 3-D line's switch-off cases
        const double u = 5.9604644775390625e-8;
        Shape::budget(ln, m, sc, dn, pn, u, out);
        ln.tpp = f32_up(Ts * (1.0 + 1.0 / 64.0));
        return ln;
    }
    // p = (x, y, z, -, -, P, -, -) in f32
    static __device__ __forceinline__ bool reject(const float* p, const Lane& ln, float) {
        float l1;
        const float a = Shape::magnitude(p, ln, &l1);
        const float m = a - __builtin_fmaf(ln.e2, l1, __builtin_fmaf(ln.e1, p[5], ln.e0));
        return m > ln.tpp;  // false on NaN / inf - inf
    }
    // g = (centre[3], rho, Pmax)
    static __device__ __forceinline__ bool group_reject(const float* g, const Lane& ln, float) {
        if (ln.nanh != 0.0f) return true;  // NaN entry in the hypothesis: every residual is NaN, never an inlier
        float l1;
        const float a = Shape::magnitude(g, ln, &l1);
        const float m = a - __builtin_fmaf(ln.e2, __builtin_fmaf(1.74f, g[3], l1), __builtin_fmaf(ln.e1, g[4], ln.e0)) - ln.nrm * g[3] * 1.001f;
        return m > ln.tpp * 1.001f;
    }
};

// ---- 3-D lines: r = |(x - p) x d| (Residual<kLine3D>), inlier iff r^2 < T2 ------------------------------------------------------------
// Homogeneous in the direction d only (p is a point): the f32 copy of d is made from d after the exact power-of-two scaling
// sc = pow2_normaliser<3>(d), which leaves its largest entry in [0.5, 1) and |d| in [0.5, sqrt(3)), and is tested against the threshold
// scaled along, Ts = T sc (must be an ordinary f32 as well).  p is rounded once and not scaled.  Below d is the scaled direction and
// r* = |(x - p) x d| in exact arithmetic on the f64 inputs.  Per point, in f32 - this operation order is the contract of the f32 test
// (tests restate it with fma as one rounding):
//   e~_k = x~_k - p~_k                                                            P = max(|x|, |y|, |z|, 1) rounded up
//   c~_0 = fma(e~_1, d~_2, -(e~_2 d~_1)),  c~_1 = fma(e~_2, d~_0, -(e~_0 d~_2)),  c~_2 = fma(e~_0, d~_1, -(e~_1 d~_0))
//   q~ = fma(c~_0, c~_0, fma(c~_1, c~_1, c~_2 c~_2)),  s~ = sqrtf(q~),  l~ = (|e~_0| + |e~_1|) + |e~_2|
// (c~_1 has the sign of the exact path's c1 reversed: only its square is used.)  With u = 2^-24, eta = 2^-126, |.| the Euclidean norm
// unless marked |.|_1, and e^ = x~ - p~ exactly:
//   inputs     e -> e x d is |d|-Lipschitz in e and |e|-Lipschitz in d: |x~ - x| <= u |x| <= sqrt(3) u P and |p~ - p| <= u |p| move c by
//              at most |d| (sqrt(3) u P + u |p|); |d~ - d| <= u |d| moves it by u |d| |e^|
//   e~         one rounding per component, |e~ - e^| <= u |e^|: moves c by at most u |d~| |e^|
//   c~_k       the inner product is rounded once and the fma once: |c~_k - c_k(e~, d~)| <= u |e~_j d~_i| + u |c_k| + O(u^2); the three
//              inner products are three different entries of the outer product e~ d~^T, so their vector is at most |e~| |d~| long:
//              u |e~| |d~| + u |c~|
//   q~         three non-negative terms; the innermost is rounded as a product and by both fmas outside it, the outermost by its fma
//              alone: at most 3 roundings on a term, q~ = |c~|^2 (1 + t), |t| <= 3 u + O(u^2) -> 1.5 u |c~| after the root
//   sqrtf      v_sqrt_f32's documented 1 ulp = 2 u |c~|, whatever correction the lowering adds (as the round family charges it)
//   exact path three differences, six products, three differences of products, then three squares and two sums, in f64 without
//              contraction: |c_c - c*| <= 4 * 2^-53 |e| |d| + O(2^-106), absolute and not relative to r; the sum of squares adds a
//              relative 2 * 2^-53 after the root.  Together < 2^-50 |e| |d| = u 2^-26 |e| |d|
// and |c~| <= |e~| |d~| (1 + O(u)), so
//   |s~ - r*| + |r_c - r*| <= sqrt(3) u |d| P + u |d| |p| + (1 + 1 + 1 + 1 + 1.5 + 2) u |d~| |e~| + 2^-50 |e| |d| + O(u^2)
//                          =  sqrt(3) u |d| P + u |d| |p| + 7.5 u |d~| |e~| + ...
// |e~|_1 >= |e~| bounds the length without a second root.  Underflow: an inner product or fma result below 2^-126 carries an absolute
// error <= eta (even with denormals flushed), which moves c by < 4 eta; a subnormal difference e~_k is exact (flushed: off by < eta,
// c moves by < 2 eta); the three squares and two fmas of q~ put at most 4 eta under the root and move it by <= sqrt(4 eta) < 2.2e-19.
// The exact path's own underflow: the band of pow2_normaliser keeps |c| sc^-1 above 2^-511 or its square's error below 3 * 2^-1074,
// which moves r sc by < 1e-80.  The coefficients, each with room for evaluating E itself in f32 (four roundings, < 5 u relative), for
// writing |d~|, |e~| for |d|, |e^| (factors 1 + O(u)) and for the O(u^2) terms:
//   E = e1 P + e0 + e2 l~      e1 = 2 u D                   >= 1.15 * sqrt(3) u |d|              D = 1.001 |d| (f64, rounded up)
//                              e0 = 2 u D |p| 1.001 + 1e-18 >= 2 * u |d| |p|, + 4 * 2.2e-19
//                              e2 = 8 u D                   >= 1.06 * (7.5 + 2^-26) u |d~|
//   reject  <=>  m := s~ - E > T'' = Ts (1 + 2^-6).  m is rounded once and monotonically, which is paid from the margin of the threshold
//   as in the round family: r_c > Ts (1 + 2^-7), and the computed r_c^2, which the exact path compares, exceeds Ts^2 = T2 sc^2 - the
//   exact path's arithmetic on d / sc is that on d scaled by a power of two.  The root form is kept: the squared form (q~ against
//   (T'' + E)^2) would be correct only because the 1e-18 floor keeps the square a normal f32, a coupling this budget should not hide.
// Group test on the 3-D ball (stored centre g, radius rho, Pmax) of 64 Morton-consecutive points (sp_line_bounds_kernel<SPAN, 3>, the
// rows planes and spheres get): r* is |d|-Lipschitz in x, so every member has r* >= r*(g) - |d| rho, and its |e|_1 is at most
// |e_g|_1 + sqrt(3) rho, which bounds the error terms of the member's own exact evaluation (g is an f32 value: no input rounding, the
// e1 Pmax term is kept all the same):
//   reject the group  <=>  s~_g - E(Pmax, l~_g + 1.74 rho) - 1.001 D rho > 1.001 T''.
// Switch-off, E = inf and the exact path decides: a set with coordinates beyond 1e17 or |p| beyond 1e17 (q~ must stay below the f32
// overflow: |c~| <= sqrt(3) * 3.5e17), a threshold Ts outside the ordinary f32 range, a direction outside pow2_normaliser's band -
// d = 0, whose residuals are all 0 on the exact path, and Inf entries among them: inf - inf is NaN, and a NaN comparison is false.
// A NaN entry culls the hypothesis outright (all six enter every residual).  The exact path is 17 FP64 operations without a division or
// a root, so as for planes the per-pair filter buys little and the cull buys almost everything: a line's inliers are a tube of
// radius T, which few 64-point balls touch (DESIGN.md 4.8 has the measurement).
struct LineShape32 {
    struct Lane { float p[3]; float d[3]; float e1, e0, e2, tpp, nrm, nanh; };   // a row of floats in this order (score.hip HypRow)
    // reject() reads p, d, e1, e0, e2, tpp and nothing behind them (nrm and nanh belong to group_reject)
    static constexpr int kStagedVals = 10;
    static constexpr int kModelVals = 6;
    static_assert(offsetof(Lane, d) == 3 * sizeof(float) && offsetof(Lane, e1) == 6 * sizeof(float) &&
                  offsetof(Lane, tpp) == (kStagedVals - 1) * sizeof(float) && offsetof(Lane, nrm) == kStagedVals * sizeof(float) &&
                  sizeof(Lane) == 12 * sizeof(float), "p, d, e1, e0, e2, tpp lead the lane; nrm, nanh follow");
    template <class MD> static __device__ __forceinline__ void budget(Lane& ln, const MD&, double, double dn, double pn, double u, bool big) {
        ln.e1 = f32_up(2.0 * u * dn);
        ln.e0 = big ? __builtin_inff() : f32_up(2.0 * u * dn * pn + 1e-18);   // inf: nothing is rejected
        ln.e2 = f32_up(8.0 * u * dn);
        ln.nrm = f32_up(dn);
    }
    // s~ itself is compared: a root is never negative, and an absolute value here would be an operation the budget does not have
    static __device__ __forceinline__ float magnitude(const float* p, const Lane& ln, float* l1) { return axial_dist(p, ln, l1); }
};
template <> struct Filter32<kLine3D> : AxialFilter32<LineShape32> {};

// ---- cylinders: r = | |(x - p) x d| - cr | (Residual<kCylinder3D>), inlier iff r^2 < T2 ----------------------------------------------
// The 3-D line's distance followed by the round family's last step, and so is the test.  Homogeneous in the direction only: with the
// 3-D line's sc = pow2_normaliser<3>(d), s* = |(x - p) x (d sc)| and the radius in the same units, R = cr sc (exact in f64: a power of
// two), the residual times sc is |s* - R|, tested against Ts = T sc.  Scaling by sc commutes with the exact path, root included: the
// exact path's c on d sc is its c on d times sc, its sum of squares is q sc^2, and sc^2 is an EVEN power of two, so the correctly
// rounded sqrt(q sc^2) is sc sqrt(q) bit for bit; the subtraction of cr sc and the square scale along.  The exact path's decision on
// (d, cr, T2) is the one its arithmetic would take on (d sc, R, T2 sc^2).  Per point, in f32 - this operation order is the contract
// of the f32 test (tests restate it with fma as one rounding):
//   s~, l~ = axial_dist(x~, p~, d~)  (the shared code),   r~ = (float)(cr sc),   n~ = s~ - r~
// With u = 2^-24 and the 3-D line's terms as derived above (inputs, e~, c~_k, q~, sqrtf: sqrt(3) u |d| P + u |d| |p| + 7.5 u |d~| |e~|
// and the underflow floor) the cylinder adds:
//   input r~   |r~ - R| <= u |R|, and n is 1-Lipschitz in R: u |R|
//   exact path its extra root is one more relative 2^-53 on s_c <= |e| |d|: the 3-D line's 4 + 2 become 4 + 2 + 1 = 7 units of 2^-53
//              |e| |d|, still < 2^-50 |e| |d| = u 2^-26 |e| |d|, which the 3-D line's e2 already carries; the subtraction s_c - cr is
//              rounded once, relatively, 2^-53 |s_c - cr|, which is part of the T'' margin below (as in the round family)
//   n~         the subtraction s~ - r~ is rounded once, relatively: n~ = (s~ - r~)(1 + t), |t| <= u.  Charged to the T'' margin and not
//              to E, as the round family charges it: m > T'' gives |s~ - r~| >= (T'' + E)(1 - u), Ts (1 + 2^-6)(1 - u) > Ts (1 + 2^-7),
//              and E (1 - u) covers the terms as soon as E carries a relative margin of u over them (it carries > 6 %)
// so |(s~ - r~) - (s_c sc - R)| <= sqrt(3) u |d| P + u (|d| |p| + |R|) + (7.5 + 2^-26) u |d~| |e~| + O(u^2), and with the 3-D line's D:
//   E = e1 P + e0 + e2 l~      e1 = 2 u D                              >= 1.15 * sqrt(3) u |d|          D = 1.001 |d| (f64, rounded up)
//                              e0 = 2 u (D |p| 1.001 + |R|) + 1e-18    >= 2 * u (|d| |p| + |R|), + 4 * 2.2e-19
//                              e2 = 8 u D                              >= 1.06 * (7.5 + 2^-26) u |d~|
//   reject  <=>  m := |n~| - E > T'' = Ts (1 + 2^-6):  m is rounded once and monotonically, so |s_c sc - R| > Ts (1 + 2^-7), and the
//   computed residual's square, which the exact path compares, exceeds Ts^2 = T2 sc^2.
// Group test on the 3-D ball rows (stored centre g, radius rho, Pmax) that planes, spheres and lines get: s* is |d|-Lipschitz in x, so
// every member's s* lies in [s*_g - |d| rho, s*_g + |d| rho] and its residual is at least |s*_g - R| - |d| rho, less the errors above
// with P = Pmax and |e|_1 <= |e_g|_1 + sqrt(3) rho:
//   reject the group  <=>  |s~_g - r~| - E(Pmax, l~_g + 1.74 rho) - 1.001 D rho > 1.001 T''.
// One rule for points outside the cylinder, inside it, for cr = 0 (the 3-D line) and cr < 0 (every residual is s + |cr|).
// Switch-off, E = inf and the exact path decides: the 3-D line's cases - coordinates beyond 1e17 or |p| beyond 1e17, Ts outside the
// ordinary f32 range, a direction outside pow2_normaliser's band (d = 0, whose residuals are all |cr| on the exact path, and Inf
// entries among them) - and a radius beyond 1e17 in the filter's units (|R| > 1e17; Inf included: r~ must stay an ordinary f32, or
// s~ - inf would reject everything.  inf - inf is NaN, and a NaN comparison is false).  A NaN entry culls the hypothesis outright (all
// seven enter every residual).  The exact path is the 3-D line's 17 FP64 operations plus a root, a subtraction and a square.
struct CylinderShape32 {
    struct Lane { float p[3]; float d[3]; float r, e1, e0, e2, tpp, nrm, nanh; };   // a row of floats in this order (score.hip HypRow)
    // reject() reads p, d, r, e1, e0, e2, tpp and nothing behind them (nrm and nanh belong to group_reject)
    static constexpr int kStagedVals = 11;
    static constexpr int kModelVals = 7;
    static_assert(offsetof(Lane, d) == 3 * sizeof(float) && offsetof(Lane, r) == 6 * sizeof(float) && offsetof(Lane, e1) == 7 * sizeof(float) &&
                  offsetof(Lane, tpp) == (kStagedVals - 1) * sizeof(float) && offsetof(Lane, nrm) == kStagedVals * sizeof(float) &&
                  sizeof(Lane) == 13 * sizeof(float), "p, d, r, e1, e0, e2, tpp lead the lane; nrm, nanh follow");
    template <class MD> static __device__ __forceinline__ void budget(Lane& ln, const MD& m, double sc, double dn, double pn, double u, bool out) {
        const double R = m[6] * sc;        // the radius in the scaled direction's units
        ln.r = (float)R;
        const bool big = out || !(fabs(R) <= 1e17);
        ln.e1 = f32_up(2.0 * u * dn);
        ln.e0 = big ? __builtin_inff() : f32_up(2.0 * u * (dn * pn + fabs(R)) + 1e-18);   // inf: nothing is rejected
        ln.e2 = f32_up(8.0 * u * dn);
        ln.nrm = f32_up(dn);
    }
    static __device__ __forceinline__ float magnitude(const float* p, const Lane& ln, float* l1) {
        const float s = axial_dist(p, ln, l1);
        return fabsf(s - ln.r);
    }
};
template <> struct Filter32<kCylinder3D> : AxialFilter32<CylinderShape32> {};

// ---- cones: r = |c rho - s h|, rho = |(x - a) x d|, h = (x - a) . d (Residual<kCone3D>), inlier iff r^2 < T2 -------------------------
// The 3-D line's distance and a dot product with the same direction, combined by the half-angle's (c, s).  Homogeneous in d and in
// (c, s).  d gets the 3-D line's sc = pow2_normaliser<3>(d): rho and h on d sc are rho sc and h sc (sc^2 is an even power of two, so
// the root scales bit for bit, as for cylinders; the three products and two sums of h scale exactly), the two products with c and s and
// their difference scale along, and the exact path's decision on (d, T2) is the one its arithmetic would take on (d sc, T2 sc^2):
// the test is against Ts = T sc.  (c, s) is NOT rescaled: it is rounded to f32 as it is, every term below is relative to
// K1 = |c| + |s|, and outside the band 2^-10 <= K1 <= 2^10 the filter is off.  Below d is the scaled direction, rho* = |(x - a) x d|,
// h* = (x - a) . d and n* = c rho* - s h* in exact arithmetic on the f64 inputs.  Per point, in f32 - this operation order is the
// contract of the f32 test (tests restate it with fma as one rounding):
//   s~, l~ = axial_dist(x~, a~, d~)  (the shared code; e~_k = x~_k - a~_k),   h~ = axial_height: fma(e~_2, d~_2, fma(e~_1, d~_1, e~_0 d~_0)),
//   c~ = (float)c,  s_~ = (float)s,   n~ = fma(s~, c~, -(h~ s_~))
// With u = 2^-24 and the 3-D line's terms as derived above, B = sqrt(3) u |d| P + u |d| |a| for the inputs x~ and a~ and t = u |d~| |e~|:
//   rho        |s~ - rho*| + |rho_c - rho*| <= B + (7.5 + 2^-26) t and the underflow floor: the 3-D line's budget, its exact path included
//   h~         h is |d|-Lipschitz in e and |e|-Lipschitz in d, so the inputs x~, a~ move it by at most B and d~ by t; e~ is rounded once
//              per component, t; the innermost product is rounded three times (as a product and by both fmas), the middle one twice, the
//              outer fma once: at most 3 u (|e~_0 d~_0| + |e~_1 d~_1| + |e~_2 d~_2|) <= 3 t by Cauchy-Schwarz.  |h~ - h*| <= B + 5 t
//   exact h    three differences, three products, two sums in f64: < 2^-50 |e| |d| = 2^-26 t, inside the slack of e2 below
//   c~, s_~    |c~ - c| <= u |c|, |s_~ - s| <= u |s|: n moves by u (|c| rho + |s| |h|) <= u K1 |e| |d| = K1 t  (rho, |h| <= |e| |d|)
//   carried    the errors of s~ and h~ enter n~ times |c~| and |s_~|: (|c| + |s|)(B + 7.5 t) = K1 (B + 7.5 t), the larger of the two for both
//   n~         the product h~ s_~ is rounded once, u |h~| |s_~| <= K1 t; the fma's own rounding is relative to n~ and is charged to
//              the T'' margin and not to E, as the cylinder's subtraction is
//   exact n    two products and a difference in f64: the products' 2^-53 (|c| rho + |s| |h|) is inside the same slack, the
//              difference's rounding is relative and part of the T'' margin
// so |n~ / (1 + t') - n*| + |n_c - n*| <= K1 (sqrt(3) u |d| P + u |d| |a| + (9.5 + 2^-25) u |d~| |e~|) + O(u^2), |t'| <= u, and with the
// 3-D line's D = 1.001 |d| and K = 1.001 (|c| + |s|) (f64, rounded up):
//   E = e1 P + e0 + e2 l~      e1 = 2 u D K                            >= 1.15 * sqrt(3) u |d| K1
//                              e0 = 2 u D K |a| 1.001 + 1e-18 (K + 1)  >= 2 * u |d| |a| K1; the floor: the 3-D line's 4 * 2.2e-19 on s~
//                                                                      times |c~| <= K, and 4 eta for h~ and the product h~ s_~
//                              e2 = 10.5 u D K                         >= 1.1 * (9.5 + 2^-25) u |d~| K1
//   reject  <=>  m := |n~| - E > T'' = Ts (1 + 2^-6):  m is rounded once and monotonically, so |n_c| > Ts (1 + 2^-7), and the computed
//   residual's square, which the exact path compares, exceeds Ts^2 = T2 sc^2.
// Group test on the 3-D ball rows (stored centre g, radius rho_g, Pmax) that planes, spheres, lines and cylinders get, nothing new in
// setpoints.hip: x -> (h, rho) drops the angle about the axis and is |d|-Lipschitz, so the signed residual c rho - s h is L-Lipschitz in
// x with L = |d| sqrt(c^2 + s^2) (its gradient is c rhohat - s d, of unit length for a unit d and a unit (c, s)).  Every member's
// |n*| is at least |n*_g| - L rho_g, less the errors above with P = Pmax and |e|_1 <= |e_g|_1 + sqrt(3) rho_g:
//   reject the group  <=>  |n~_g| - E(Pmax, l~_g + 1.74 rho_g) - 1.001 L rho_g > 1.001 T'',   L stored as nrm (times 1.001, rounded up).
// Switch-off, E = inf and the exact path decides: the 3-D line's cases - coordinates beyond 1e17 or |a| beyond 1e17, Ts outside the
// ordinary f32 range, a direction outside pow2_normaliser's band (d = 0, whose residuals are all 0 on the exact path, and Inf entries
// among them) - and |c| + |s| outside [2^-10, 2^10], which a non-finite c or s is too (n~ stays below 2^10 * 6.1e17 * 2, an ordinary
// f32, and an Inf entry would make inf - inf = NaN at best).  A NaN entry culls the hypothesis outright (all eight enter every
// residual).  The exact path is the 3-D line's 17 FP64 operations plus a root, five for h, two products, a difference and a square.
struct ConeShape32 {
    struct Lane { float p[3]; float d[3]; float c, s, e1, e0, e2, tpp, nrm, nanh; };   // a row of floats in this order (score.hip HypRow)
    // reject() reads p, d, c, s, e1, e0, e2, tpp and nothing behind them (nrm and nanh belong to group_reject): three float4 chunks
    static constexpr int kStagedVals = 12;
    static constexpr int kModelVals = 8;
    static_assert(offsetof(Lane, d) == 3 * sizeof(float) && offsetof(Lane, c) == 6 * sizeof(float) && offsetof(Lane, e1) == 8 * sizeof(float) &&
                  offsetof(Lane, tpp) == (kStagedVals - 1) * sizeof(float) && offsetof(Lane, nrm) == kStagedVals * sizeof(float) &&
                  sizeof(Lane) == 14 * sizeof(float), "p, d, c, s, e1, e0, e2, tpp lead the lane; nrm, nanh follow");
    template <class MD> static __device__ __forceinline__ void budget(Lane& ln, const MD& m, double, double dn, double pn, double u, bool out) {
        ln.c = (float)m[6];
        ln.s = (float)m[7];
        const double k1 = fabs(m[6]) + fabs(m[7]);
        const double K = k1 * 1.001;
        const bool big = out || !(k1 >= 0.0009765625) || !(k1 <= 1024.0);
        ln.e1 = f32_up(2.0 * u * dn * K);
        ln.e0 = big ? __builtin_inff() : f32_up(2.0 * u * dn * K * pn + 1e-18 * (K + 1.0));   // inf: nothing is rejected
        ln.e2 = f32_up(10.5 * u * dn * K);
        ln.nrm = f32_up(dn * sqrt(m[6] * m[6] + m[7] * m[7]));
    }
    // |n~|: s~ and l~ on this lane's p and d, then h~ and the final fma
    static __device__ __forceinline__ float magnitude(const float* p, const Lane& ln, float* l1) {
        const float s = axial_dist(p, ln, l1);
        const float h = axial_height(p, ln);
        const float n = __builtin_fmaf(s, ln.c, -(h * ln.s));
        return fabsf(n);
    }
};
template <> struct Filter32<kCone3D> : AxialFilter32<ConeShape32> {};

// ---- tori: r = | sqrt((rho - R)^2 + h^2) - cr |, rho = |(x - c) x d|, h = (x - c) . d (Residual<kTorus3D>), inlier iff r^2 < T2 ------
// The 3-D line's distance and the cone's dot product, then the 2-D circle's last step in the half-plane (h, rho).  Homogeneous in the
// direction only, as the cylinder is: with the 3-D line's sc = pow2_normaliser<3>(d), rho and h on d sc are rho sc and h sc (the root
// scales bit for bit, sc^2 being an even power of two; the products and sums of h scale exactly), and with both radii in the same
// units, R = (major radius) sc and r = cr sc (exact in f64), t = rho - R, t t + h h, its root and the last difference scale along: the
// exact path's decision on (d, R, cr, T2) is the one its arithmetic would take on (d sc, R sc, cr sc, T2 sc^2), and the test is against
// Ts = T sc.  Below d, R and r are the scaled ones, and rho*, h*, w* = sqrt((rho* - R)^2 + h*^2), n* = w* - r are exact on the f64
// inputs.  Per point, in f32 - this operation order is the contract of the f32 test (tests restate it with fma as one rounding):
//   s~, l~ = axial_dist(x~, c~, d~)  (the shared code; e~_k = x~_k - c~_k),   h~ = axial_height: fma(e~_2, d~_2, fma(e~_1, d~_1, e~_0 d~_0)),
//   R~ = (float)R,  r~ = (float)r,   t~ = s~ - R~,   w~ = sqrtf(fma(t~, t~, h~ h~)),   n~ = w~ - r~
// With u = 2^-24, B = sqrt(3) u |d| P + u |d| |c| for the inputs x~ and c~ and t = u |d~| |e~| as in the cone's derivation:
//   rho        |s~ - rho*| + |rho_c - rho*| <= B + (7.5 + 2^-26) t and the underflow floor: the 3-D line's budget, its exact path included
//   h~         |h~ - h*| <= B + 5 t: the cone's budget for the same expression; the exact h is inside the slack of e2
//   R~, t~     |R~ - R| <= u |R|; the subtraction is rounded once, u |t~|
//   w~         (t, h) -> sqrt(t^2 + h^2) is 1-Lipschitz, so the errors of t~ and h~ move w by at most their sum,
//              2 B + 12.5 t + u |R|; h~ h~ is rounded as a product and by the fma, t~ t~ by the fma alone: at most 2 u relative under the
//              root, u w~ after it; v_sqrt_f32's documented 1 ulp = 2 u w~; with t~'s own rounding 4 u w~, and
//              w~ <= sqrt(rho^2 + h^2) + |R| = |e| |d| + |R|: 4 t + 4 u |R|
//   r~, n~     |r~ - r| <= u |r|; the last subtraction is rounded once, relatively, and is charged to the T'' margin as the cylinder's is
//   exact path rho - R, two squares, a sum and a root in f64: < 4 * 2^-53 (|e| |d| + |R|), inside the slack of e2 and of e0's |R| term;
//              the last difference is relative and part of the T'' margin
// so |n~ / (1 + t') - n*| + |n_c - n*| <= 2 sqrt(3) u |d| P + 2 u |d| |c| + 5 u |R| + u |r| + (16.5 + 2^-25) u |d~| |e~| + O(u^2), |t'| <= u,
// and with the 3-D line's D = 1.001 |d| (f64, rounded up):
//   E = e1 P + e0 + e2 l~      e1 = 4 u D                                         >= 1.15 * 2 sqrt(3) u |d|
//                              e0 = 2 u (2 D |c| 1.001 + 3 |R| + |r|) + 2e-18     >= 2 u |d| |c| + 5 u |R| + u |r| with a fifth to spare; the
//                                                                                 floor: the 3-D line's 4 * 2.2e-19 on s~, 4 eta for h~, and
//                                                                                 two squares below 2^-126 put <= 2 eta under w~'s root,
//                                                                                 sqrt(2 eta) < 1.6e-19
//                              e2 = 18 u D                                        >= 1.09 * (16.5 + 2^-25) u |d~|
//   reject  <=>  m := |n~| - E > T'' = Ts (1 + 2^-6):  m is rounded once and monotonically, so |n_c| > Ts (1 + 2^-7), and the computed
//   residual's square, which the exact path compares, exceeds Ts^2 = T2 sc^2.
// Group test on the 3-D ball rows (stored centre g, radius rho_g, Pmax), nothing new in setpoints.hip: x -> (h, rho) drops the angle
// about the axis and is |d|-Lipschitz, the distance to the spine's point (0, R) of the half-plane and the difference with r are
// 1-Lipschitz, so the signed residual w - r is |d|-Lipschitz in x.  Every member's |n*| is at least |n*_g| - |d| rho_g, less the errors
// above with P = Pmax and |e|_1 <= |e_g|_1 + sqrt(3) rho_g:
//   reject the group  <=>  |n~_g| - E(Pmax, l~_g + 1.74 rho_g) - 1.001 D rho_g > 1.001 T''.
// One rule for points outside the tube, inside it, in the hole and on the axis (rho = 0 is no special case of w).
// Switch-off, E = inf and the exact path decides: the 3-D line's cases - coordinates beyond 1e17 or |c| beyond 1e17, Ts outside the
// ordinary f32 range, a direction outside pow2_normaliser's band (d = 0, whose residuals are all ||R| - cr| on the exact path, and Inf
// entries among them) - and |R| or |r| beyond 1e17 in the filter's units, which a non-finite radius is too (t~^2 + h~^2 stays below
// 2 (7e17)^2, an ordinary f32).  A NaN entry culls the hypothesis outright (all eight enter every residual).  The exact path is the
// 3-D line's 17 FP64 operations plus two roots, five operations for h, four for w, a difference and a square.
struct TorusShape32 {
    struct Lane { float p[3]; float d[3]; float R, r, e1, e0, e2, tpp, nrm, nanh; };   // a row of floats in this order (score.hip HypRow)
    // reject() reads p, d, R, r, e1, e0, e2, tpp and nothing behind them (nrm and nanh belong to group_reject): three float4 chunks,
    // the cone's count
    static constexpr int kStagedVals = 12;
    static constexpr int kModelVals = 8;
    static_assert(offsetof(Lane, d) == 3 * sizeof(float) && offsetof(Lane, R) == 6 * sizeof(float) && offsetof(Lane, e1) == 8 * sizeof(float) &&
                  offsetof(Lane, tpp) == (kStagedVals - 1) * sizeof(float) && offsetof(Lane, nrm) == kStagedVals * sizeof(float) &&
                  sizeof(Lane) == 14 * sizeof(float), "p, d, R, r, e1, e0, e2, tpp lead the lane; nrm, nanh follow");
    template <class MD> static __device__ __forceinline__ void budget(Lane& ln, const MD& m, double sc, double dn, double pn, double u, bool out) {
        const double R = m[6] * sc, r = m[7] * sc;   // both radii in the scaled direction's units
        ln.R = (float)R;
        ln.r = (float)r;
        const bool big = out || !(fabs(R) <= 1e17) || !(fabs(r) <= 1e17);
        ln.e1 = f32_up(4.0 * u * dn);
        ln.e0 = big ? __builtin_inff() : f32_up(2.0 * u * ((2.0 * dn * pn + 3.0 * fabs(R)) + fabs(r)) + 2e-18);   // inf: nothing is rejected
        ln.e2 = f32_up(18.0 * u * dn);
        ln.nrm = f32_up(dn);
    }
    // |n~|: s~ and l~ on this lane's p and d, then h~, t~, w~ and the last difference
    static __device__ __forceinline__ float magnitude(const float* p, const Lane& ln, float* l1) {
        const float s = axial_dist(p, ln, l1);
        const float h = axial_height(p, ln);
        const float t = s - ln.R;
        const float w = sqrtf(__builtin_fmaf(t, t, h * h));
        return fabsf(w - ln.r);
    }
};
template <> struct Filter32<kTorus3D> : AxialFilter32<TorusShape32> {};

// ---- mixed primitives: the constituent's filter behind the class (Residual<kPrimitive3D>) -------------------------------------------
// Nothing is derived here.  A lane is the class followed by the constituent's own lane, float for float as its prep() made it from the
// constituent's model row q = m + 1; reject() and group_reject() hand that lane to the constituent's functions, so every f32 operation,
// every constant and every decision is the constituent's, and so are its budget and its switch-off cases (tests hold the union's
// surviving (hypothesis, group) pairs and masks to the constituents').  The point rows and the group rows are the four types' common
// ones: kRowVals = 6, kGroupVals = 5.  The widest staged form is the cone's 12 floats, so 13 are staged: the plane's and the sphere's
// nine (their whole lanes), the cylinder's 11 and the cone's 12 all lie inside them, and what lies behind (nrm, nanh of the cylinder and
// the cone) only group_reject() reads, in the cull kernel, from registers.
// An unknown class never rejects a pair or a group: its lane holds class 0 and zeros, and the exact path produces the NaN residual.  The
// one exception is a NaN class in group_reject(): it culls, as a NaN entry does in every constituent (the class enters every residual,
// and the solver's empty slots are all-NaN rows: without the cull each of them would be evaluated against every point).
// The class is compared, never used as an index: a lane copy is a fixed sequence of register moves, and a divergent word of the cull
// kernel or of the hypothesis-per-lane kernel runs the paths of the classes it holds one after the other under their lane masks.  In
// the group-major and the pointwise kernels a hypothesis is uniform over the wave and exactly one path runs.
template <> struct Filter32<kPrimitive3D> {
    using Plane = Filter32<kPlane3D>;
    using Sphere = Filter32<kSphere3D>;
    using Cylinder = Filter32<kCylinder3D>;
    using Cone = Filter32<kCone3D>;
    static constexpr bool enabled = true;
    static constexpr int kRowVals = 6, kGroupVals = 5;
    static constexpr int kSubVals = 14;   // the widest constituent lane (the cone's)
    struct Lane { float cls; float v[kSubVals]; };   // a row of floats in this order (score.hip HypRow)
    static constexpr int kStagedVals = 1 + StagedVals<Cone>::value;
    static_assert(Plane::kRowVals == 6 && Sphere::kRowVals == 6 && Cylinder::kRowVals == 6 && Cone::kRowVals == 6 && Plane::kGroupVals == 5 &&
                  Sphere::kGroupVals == 5 && Cylinder::kGroupVals == 5 && Cone::kGroupVals == 5, "the four constituents read the same rows");
    static_assert(sizeof(Plane::Lane) <= kSubVals * sizeof(float) && sizeof(Sphere::Lane) <= kSubVals * sizeof(float) &&
                  sizeof(Cylinder::Lane) <= kSubVals * sizeof(float) && sizeof(Cone::Lane) == kSubVals * sizeof(float) &&
                  StagedVals<Plane>::value < kStagedVals && StagedVals<Sphere>::value < kStagedVals && StagedVals<Cylinder>::value < kStagedVals &&
                  offsetof(Lane, v) == sizeof(float) && sizeof(Lane) == (1 + kSubVals) * sizeof(float), "class, then the constituent's lane");
    // the constituent's lane into v, zeros behind it / out of v again: constant indices only
    template <class L> static __device__ __forceinline__ void put(Lane& ln, const L& sub) {
        const float* src = reinterpret_cast<const float*>(&sub);
#pragma unroll
        for (int k = 0; k < kSubVals; ++k) ln.v[k] = k < (int)(sizeof(L) / sizeof(float)) ? src[k] : 0.0f;
    }
    template <class L> static __device__ __forceinline__ L sub(const Lane& ln) {
        L out;
        float* dst = reinterpret_cast<float*>(&out);
#pragma unroll
        for (int k = 0; k < (int)(sizeof(L) / sizeof(float)); ++k) dst[k] = ln.v[k];
        return out;
    }
    template <class MD> static __device__ __forceinline__ Lane prep(const MD& m, double pscale /* max(|coordinate|, 1) over the set */, double T2) {
        Lane ln;
        const double cls = m[0];
        const double q[8] = {m[1], m[2], m[3], m[4], m[5], m[6], m[7], m[8]};
        ln.cls = cls == cls ? 0.0f : __builtin_nanf("");
#pragma unroll
        for (int k = 0; k < kSubVals; ++k) ln.v[k] = 0.0f;
        if (cls == (double)kPlane3D) { ln.cls = (float)kPlane3D; put(ln, Plane::prep(q, pscale, T2)); }
        else if (cls == (double)kSphere3D) { ln.cls = (float)kSphere3D; put(ln, Sphere::prep(q, pscale, T2)); }
        else if (cls == (double)kCylinder3D) { ln.cls = (float)kCylinder3D; put(ln, Cylinder::prep(q, pscale, T2)); }
        else if (cls == (double)kCone3D) { ln.cls = (float)kCone3D; put(ln, Cone::prep(q, pscale, T2)); }
        return ln;
    }
    // p = (x, y, z, -, -, P, -, -) in f32
    static __device__ __forceinline__ bool reject(const float* p, const Lane& ln, float T2d) {
        if (ln.cls == (float)kPlane3D) return Plane::reject(p, sub<Plane::Lane>(ln), T2d);
        if (ln.cls == (float)kSphere3D) return Sphere::reject(p, sub<Sphere::Lane>(ln), T2d);
        if (ln.cls == (float)kCylinder3D) return Cylinder::reject(p, sub<Cylinder::Lane>(ln), T2d);
        if (ln.cls == (float)kCone3D) return Cone::reject(p, sub<Cone::Lane>(ln), T2d);
        return false;
    }
    // g = (centre[3], rho, Pmax)
    static __device__ __forceinline__ bool group_reject(const float* g, const Lane& ln, float Tup) {
        if (ln.cls == (float)kPlane3D) return Plane::group_reject(g, sub<Plane::Lane>(ln), Tup);
        if (ln.cls == (float)kSphere3D) return Sphere::group_reject(g, sub<Sphere::Lane>(ln), Tup);
        if (ln.cls == (float)kCylinder3D) return Cylinder::group_reject(g, sub<Cylinder::Lane>(ln), Tup);
        if (ln.cls == (float)kCone3D) return Cone::group_reject(g, sub<Cone::Lane>(ln), Tup);
        return ln.cls != ln.cls;   // a NaN class: every residual is NaN, never an inlier; any other unknown class is kept
    }
};

// ---- oriented mixed primitives (Residual<kOrientedPrimitive3D>): type 18's filter and group test as they stand --------------------------
// Both reject by the distance alone.  An oriented inlier is a type-18 inlier whose normal also agrees: the test of the normal only takes
// pairs away, so a pair or a group that type 18 may drop holds no oriented inlier either - every rejection stays conservative, with the
// constituents' budgets unchanged.  A NaN class is culled as under type 18 (the solver's empty and incompatible slots are all-NaN rows).
template <> struct Filter32<kOrientedPrimitive3D> : Filter32<kPrimitive3D> {};

}  // namespace pgx
