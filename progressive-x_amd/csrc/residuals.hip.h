// residuals.hip.h — per-(point, model) residuals for the five Progressive-X problem types and the geometric primitives: the two
// families flat (2-D lines, 3-D planes) and round (2-D circles, 3-D spheres), each written once per dimension, and the 3-D line
// (distance to an axis), the cylinder (that distance less a radius), the cone (the distance to a generatrix), the torus (the distance
// to the tube's centre circle less the tube radius), the union of plane, sphere, cylinder and cone whose model row carries its class,
// and that union with a test of the point's normal.  gfx950 device code.
//
// FP64 throughout, compiled with -ffp-contract=off: the reference is built for baseline x86-64 (no FMA,
// /root/reference/CMakeLists.txt:23) and parity of inlier masks is bit-exact, so every product and sum is
// rounded separately; `/` and sqrt() lower to the correctly-rounded AMDGPU expansions.
//
// Each functor documents the reference interface it replaces (paths relative to
// /root/reference/src/pyprogressivex/).  U-n = upstream source absent from the snapshot (graph-cut-ransac
// submodule is empty), restated from the published definition; see DESIGN.md §3.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "score_plan.h"   // GroupBound: the planner of a scoring launch reads it too, without HIP

namespace pgx {

enum ModelType : int {
    kLine2D = 0, kHomography = 1, kFundamental = 2, kPnP = 3, kVanishingPoint = 4, kHomographySym = 5, kPlane3D = 6,
    kSphere3D = 8, kCircle2D = 10, kLine3D = 12, kCylinder3D = 14, kCone3D = 16, kPrimitive3D = 18,
    kOrientedPrimitive3D = 20, kTorus3D = 22,
    kNumModelTypes = 23   // 7, 9, 11, 13, 15, 17, 19 and 21 are not assigned (pgx_model_dims on each of them is an error)
};

// OpenCV's MIN/MAX macros (the reference sees them via progx_model.h:36): MAX(a,b) ((a) < (b) ? (b) : (a)).
__device__ __forceinline__ double cv_max(double a, double b) { return a < b ? b : a; }
__device__ __forceinline__ double cv_min(double a, double b) { return a > b ? b : a; }

// Residual<MT> is the one description of a model type: every per-type fact the library needs is a member here, and
// with_model_type() below is the one list of types.  Besides the two residual functions:
//   D, P            doubles per point row / per model
//   sample, slots   minimal sample size and hypothesis slots per sample of the device solver (solve.hip); 0 = no solver
//   bound           the kind of group bound
//   obs0            first of the two observed image coordinates (-1: none; then no scales either)
//   in0 .. in1      coordinates whose magnitude, at least 1, scales the point filter (in1 < in0: none)
//   in0 .. box1     coordinates the projective map multiplies (the box / ball part of a kBoundBox row)
//   normals_solver  only where the minimal solver reads the resident normals (pgx_set_normals): its name in the refusal without them
//   oriented        only where squared() reads the point's resident normal as well (squared_at() below is how the kernels call it)
template <int MT> struct Residual;

template <class R, class = void> struct NormalsSolver { static constexpr const char* name = nullptr; };
template <class R> struct NormalsSolver<R, std::void_t<decltype(R::normals_solver)>> { static constexpr const char* name = R::normals_solver; };

struct NoProjectiveMap { static constexpr int obs0 = -1, in0 = 0, in1 = -1, box1 = -1; };

// The flat family: a hyperplane of DIM-space, model (n[DIM], d), r = |n . p + d| with the sum a left fold -
//   DIM = 2   |(a x + b y) + c|             2-D lines: Default2DLineEstimator (progressivex_python.cpp:489) [U-4]
//   DIM = 3   |((a x + b y) + c z) + d|     3-D planes (findPlanes; no reference counterpart), (a, b, c) a unit normal
// This operation order is the contract of every line and plane check (tests restate it in numpy).
template <int DIM> struct FlatResidual : NoProjectiveMap {
    static constexpr int D = DIM, P = DIM + 1, slots = 1, bound = kBoundBall;
    template <class PT, class MD>
    static __device__ __forceinline__ double plain(const PT& p, const MD& m) {
        double s = m[0] * p[0];
#pragma unroll
        for (int k = 1; k < DIM; ++k) s = s + m[k] * p[k];
        return fabs(s + m[DIM]);
    }
    template <class PT, class MD>
    static __device__ __forceinline__ double squared(const PT& p, const MD& m) {
        const double r = plain(p, m);
        return r * r;
    }
};
template <> struct Residual<kLine2D> : FlatResidual<2> { static constexpr int sample = 2; };
template <> struct Residual<kPlane3D> : FlatResidual<3> { static constexpr int sample = 3; };

// The round family (no reference counterpart): a sphere of DIM-space, model (c[DIM], cr), d = p - c componentwise,
// r = |sqrt(d . d) - cr| with the sum a left fold, plain IEEE sqrt (no intrinsic, no contraction) -
//   DIM = 2   |sqrt(dx dx + dy dy) - cr|               2-D circles (findCircles)
//   DIM = 3   |sqrt((dx dx + dy dy) + dz dz) - cr|     3-D spheres (findSpheres)
// This operation order is the contract of every circle and sphere check (tests restate it in numpy).
template <int DIM> struct RoundResidual : NoProjectiveMap {
    static constexpr int D = DIM, P = DIM + 1, slots = 1, bound = kBoundBall;
    template <class PT, class MD>
    static __device__ __forceinline__ double plain(const PT& p, const MD& m) {
        double d[DIM];
#pragma unroll
        for (int k = 0; k < DIM; ++k) d[k] = p[k] - m[k];
        double q = d[0] * d[0];
#pragma unroll
        for (int k = 1; k < DIM; ++k) q = q + d[k] * d[k];
        return fabs(sqrt(q) - m[DIM]);
    }
    template <class PT, class MD>
    static __device__ __forceinline__ double squared(const PT& p, const MD& m) {
        const double r = plain(p, m);
        return r * r;
    }
};
template <> struct Residual<kCircle2D> : RoundResidual<2> { static constexpr int sample = 3; };
template <> struct Residual<kSphere3D> : RoundResidual<3> { static constexpr int sample = 4; };

// 3-D line (findLines3D; no reference counterpart): model (p[3], d[3]), a point on the line and a direction.  e = x - p componentwise,
// c = e x d in solve.hip cross3's component order,
//   c0 = e1 d2 - e2 d1,   c1 = -(e0 d2 - e2 d0),   c2 = e0 d1 - e1 d0,   r^2 = (c0 c0 + c1 c1) + c2 c2,   r = sqrt(r^2).
// squared() is primary and has no root in it.  The direction is taken as given: r is the distance to the axis times |d| (the solver
// and the refit return unit directions), there is no division by |d|.  The cross-product form, not |e|^2 - (e . d)^2, which cancels
// for points far along the line.  Every entry of the model enters at least two components of c: one NaN entry makes every residual
// NaN; d = 0 makes every residual 0.  This operation order is the contract of every 3-D line check (tests restate it in numpy).
template <> struct Residual<kLine3D> : NoProjectiveMap {
    static constexpr int D = 3, P = 6, sample = 2, slots = 1, bound = kBoundBall;
    template <class PT, class MD>
    static __device__ __forceinline__ double squared(const PT& p, const MD& m) {
        const double e0 = p[0] - m[0], e1 = p[1] - m[1], e2 = p[2] - m[2];
        const double c0 = e1 * m[5] - e2 * m[4];
        const double c1 = -(e0 * m[5] - e2 * m[3]);
        const double c2 = e0 * m[4] - e1 * m[3];
        return (c0 * c0 + c1 * c1) + c2 * c2;
    }
    template <class PT, class MD>
    static __device__ __forceinline__ double plain(const PT& p, const MD& m) { return sqrt(squared(p, m)); }
};

// Cylinder (findCylinders; no reference counterpart): model (p[3], d[3], r), a point on the axis, a direction and a radius.  The 3-D
// line's distance followed by the round family's last step:
//   q = Residual<kLine3D>::squared(x, m)  (the same expressions: the code is shared),  plain = |sqrt(q) - r|,  squared = plain * plain.
// The direction is taken as given, as for kLine3D (unit from the solver and the refit; otherwise the axis distance comes times |d|).
// Every entry of (p, d) enters q and r enters the subtraction: a NaN in any of the seven entries makes every residual NaN.  d = 0 makes
// q = 0 and every residual |r|.  r = 0 gives the 3-D line's residual, r < 0 the axis distance plus |r|.  This operation order is the
// contract of every cylinder check (tests restate it in numpy).
template <> struct Residual<kCylinder3D> : NoProjectiveMap {
    static constexpr int D = 3, P = 7, sample = 2, slots = 1, bound = kBoundBall;
    static constexpr const char* normals_solver = "cylinder";
    template <class PT, class MD>
    static __device__ __forceinline__ double plain(const PT& p, const MD& m) {
        return fabs(sqrt(Residual<kLine3D>::squared(p, m)) - m[6]);
    }
    template <class PT, class MD>
    static __device__ __forceinline__ double squared(const PT& p, const MD& m) {
        const double r = plain(p, m);
        return r * r;
    }
};

// Cone (findCones; no reference counterpart): model (a[3], d[3], c, s), the apex, an axis direction pointing into the nappe and the
// cosine and sine of the half-angle.  The angle is stored as (c, s) so that the exact path has only + - x and sqrt in it: no sin or cos
// runs on the device.  With e = x - a componentwise:
//   q = Residual<kLine3D>::squared(x, (a, d))  (the same expressions: the code is shared),  rho = sqrt(q),  h = (e0 d0 + e1 d1) + e2 d2,
//   plain = |c rho - s h|,  squared = plain * plain.
// What plain measures: in the half-plane (h, rho) of a point - height along the axis, distance from it - the nappe is the ray from the
// origin along (c, s), and plain is the distance to the LINE that carries this ray (the generatrix).  For h c + rho s >= 0 the foot
// lies on the ray and plain is the distance to the surface; near the apex on the far side (h c + rho s < 0) the nearest surface point
// is the apex itself and plain is smaller than the true distance sqrt(h^2 + rho^2).  The other nappe (the line continued) is not part
// of the model: a double-cone residual is a different one.
// Scaling: d, c and s are taken as given (unit d and c^2 + s^2 = 1 from the solver and the refit).  rho and h are homogeneous of degree
// 1 in d, and plain is homogeneous of degree 1 in d and in (c, s): d or (c, s) times k gives |k| times the residual, there is no division.
// Every entry of (a, d) enters q, and c and s each enter a product: a NaN in any of the eight entries makes every residual NaN.  d = 0
// makes every residual 0.  This operation order is the contract of every cone check (tests restate it in numpy).
template <> struct Residual<kCone3D> : NoProjectiveMap {
    static constexpr int D = 3, P = 8, sample = 3, slots = 1, bound = kBoundBall;
    static constexpr const char* normals_solver = "cone";
    template <class PT, class MD>
    static __device__ __forceinline__ double plain(const PT& p, const MD& m) {
        const double e0 = p[0] - m[0], e1 = p[1] - m[1], e2 = p[2] - m[2];
        const double rho = sqrt(Residual<kLine3D>::squared(p, m));
        const double h = (e0 * m[3] + e1 * m[4]) + e2 * m[5];
        return fabs(m[6] * rho - m[7] * h);
    }
    template <class PT, class MD>
    static __device__ __forceinline__ double squared(const PT& p, const MD& m) {
        const double r = plain(p, m);
        return r * r;
    }
};

// Torus (findTori; no reference counterpart): model (c[3], d[3], R, r), the centre, the axis direction, the major radius (from the axis
// to the tube's centre circle, the spine) and the minor (tube) radius.  With e = x - c componentwise:
//   q = Residual<kLine3D>::squared(x, (c, d))  (the same expressions: the code is shared),  rho = sqrt(q),  h = (e0 d0 + e1 d1) + e2 d2,
//   t = rho - R,  w = sqrt(t t + h h),  plain = |w - r|,  squared = plain * plain.
// Only + - x and sqrt: no division, no contraction.  What plain measures: in the half-plane (h, rho) of a point - height along the axis,
// distance from it - the tube is the circle of radius r about (0, R), w is the distance to the spine and plain the distance to that
// circle.  For a ring torus (R > r > 0, what the solver and the refit return) this is the distance to the surface: the mirror circle
// about (0, -R) of the same meridian plane is farther from every point with rho >= 0.  For R <= r (spindle and horn tori) the inner
// part of the self-crossing surface still counts as surface; for r < 0 plain is w + |r|.
// Scaling: d is taken as given, as for lines, cylinders and cones (unit from the solver and the refit).  rho and h are homogeneous of
// degree 1 in d, R and r are not rescaled with them: with d times k the residual is that of the torus (c, d / |d|, R / |k|, r / |k|)
// times |k|.  Every entry of (c, d) enters q, R enters t and r the last difference: a NaN in any of the eight entries makes every
// residual NaN.  d = 0 makes rho = h = 0 and every residual ||R| - r|.  This operation order is the contract of every torus check
// (tests restate it in numpy).
template <> struct Residual<kTorus3D> : NoProjectiveMap {
    static constexpr int D = 3, P = 8, sample = 4, slots = 2, bound = kBoundBall;
    static constexpr const char* normals_solver = "torus";
    template <class PT, class MD>
    static __device__ __forceinline__ double plain(const PT& p, const MD& m) {
        const double e0 = p[0] - m[0], e1 = p[1] - m[1], e2 = p[2] - m[2];
        const double rho = sqrt(Residual<kLine3D>::squared(p, m));
        const double h = (e0 * m[3] + e1 * m[4]) + e2 * m[5];
        const double t = rho - m[6];
        const double w = sqrt(t * t + h * h);
        return fabs(w - m[7]);
    }
    template <class PT, class MD>
    static __device__ __forceinline__ double squared(const PT& p, const MD& m) {
        const double r = plain(p, m);
        return r * r;
    }
};

// Mixed primitives (findPrimitives; no reference counterpart): a tagged union of the four surface types.  Model (class, q[8]): class is
// the constituent's type number as a double - 6 plane, 8 sphere, 14 cylinder, 16 cone - and q is that type's model row, padded with
// zeros.  The residual is the constituent's on q: the same functions, so the same bits as the model scored under its own type.  Any
// other class value (NaN and values that are no whole number included: the comparisons are on the double itself) gives a NaN residual,
// which is never an inlier.  The padding is never read.  The four types share D = 3 and the ball bound, so the resident point rows,
// their Morton order and the group rows are the same whichever of the five types is resident.  Instances never change class.
template <> struct Residual<kPrimitive3D> : NoProjectiveMap {
    static constexpr int D = 3, P = 9, sample = 4, slots = 4, bound = kBoundBall;
    static constexpr const char* normals_solver = "primitive";
    template <class PT, class MD>
    static __device__ __forceinline__ double plain(const PT& p, const MD& m) {
        const double cls = m[0];
        const double q[8] = {m[1], m[2], m[3], m[4], m[5], m[6], m[7], m[8]};
        if (cls == (double)kPlane3D) return Residual<kPlane3D>::plain(p, q);
        if (cls == (double)kSphere3D) return Residual<kSphere3D>::plain(p, q);
        if (cls == (double)kCylinder3D) return Residual<kCylinder3D>::plain(p, q);
        if (cls == (double)kCone3D) return Residual<kCone3D>::plain(p, q);
        return __builtin_nan("");
    }
    template <class PT, class MD>
    static __device__ __forceinline__ double squared(const PT& p, const MD& m) {
        const double cls = m[0];
        const double q[8] = {m[1], m[2], m[3], m[4], m[5], m[6], m[7], m[8]};
        if (cls == (double)kPlane3D) return Residual<kPlane3D>::squared(p, q);
        if (cls == (double)kSphere3D) return Residual<kSphere3D>::squared(p, q);
        if (cls == (double)kCylinder3D) return Residual<kCylinder3D>::squared(p, q);
        if (cls == (double)kCone3D) return Residual<kCone3D>::squared(p, q);
        return __builtin_nan("");
    }
};

// Oriented mixed primitives (findOrientedPrimitives; no reference counterpart): type 18's model row (class, q[8]) and type 18's distance,
// but a point supports a model only if its resident normal n (pgx_set_normals) also agrees with the surface normal of the model at the
// point - the compatibility test of Schnabel, Wahl and Klein, "Efficient RANSAC for Point-Cloud Shape Detection", section 4.3.  With g the
// UNNORMALISED direction of the model's normal at the point x,
//   plane    (a, b, c, d)     g = (a, b, c)
//   sphere   (c, r)           g = x - c                            componentwise
//   cylinder (p, d, r)        e = x - p,  t = (e0 d0 + e1 d1) + e2 d2,  g_k = e_k - t d_k
//   cone     (a, d, c, s)     e = x - a,  h = (e0 d0 + e1 d1) + e2 d2,  w_k = e_k - h d_k,  rho = sqrt(Residual<kLine3D>::squared(x, (a, d)))
//                             (the root the cone's residual computes),  g_k = c w_k - (s rho) d_k
// (d and (c, s) taken as given, as in the residuals: unit from the solver and the refit), every dot product a left fold,
//   nn = (n0 n0 + n1 n1) + n2 n2,   gg = (g0 g0 + g1 g1) + g2 g2,   ng = (n0 g0 + n1 g1) + n2 g2,   w = nn gg,
// the point is COMPATIBLE iff  ng ng >= kappa w  and  w > 0,  kappa = cos^2(tolerance) (pgx_set_normal_tolerance).  FP64, no contraction, no
// division, no root besides the cone's own.  The squares make the test blind to the sign and the length of n: normals may stay unsigned
// and unnormalised.  Every comparison is false on NaN, so a NaN anywhere, a zero normal and a point on the axis, at the apex or at the
// centre (g = 0) are incompatible.  This operation order is the contract of every oriented check (tests restate it in numpy).
//   squared  type 18's squared where the point is compatible, +inf where it is not; a class that is no class still gives NaN
//   plain    type 18's plain, WITHOUT the test: it is the quantity the refits minimise and pgx_residual_sum(s) adds up over a label's
//            points, and PEARL's coherence term may hand a model a point whose normal disagrees - the sum must not become infinite
//            because of it (a refit's own inlier lists come from squared and hold compatible points only)
// squared_within(.., T2, ..) is what the kernels evaluate: the distance first, the test only where the value is at most T2 (or NaN) - it
// equals squared wherever squared <= T2 and lies above T2 wherever squared does, which is all that any caller decides by (sq < T2,
// sq <= T2, sq > T2, max(0, 1 - sq / T2)).  Filter32 and the group bound are type 18's: they reject by distance alone and the normal test
// only removes inliers, so every rejection stays conservative.
template <> struct Residual<kOrientedPrimitive3D> : NoProjectiveMap {
    using Base = Residual<kPrimitive3D>;
    static constexpr int D = 3, P = 9, sample = 4, slots = 4, bound = kBoundBall;
    static constexpr const char* normals_solver = "oriented-primitive";
    static constexpr bool oriented = true;
    template <class PT, class MD>
    static __device__ __forceinline__ double plain(const PT& p, const MD& m) { return Base::plain(p, m); }
    // g of the table above; false for a class that is no class
    template <class PT, class MD>
    static __device__ __forceinline__ bool surface_normal(const PT& p, const MD& m, double (&g)[3]) {
        const double cls = m[0];
        if (cls == (double)kPlane3D) {
            g[0] = m[1]; g[1] = m[2]; g[2] = m[3];
            return true;
        }
        if (cls == (double)kSphere3D) {
            g[0] = p[0] - m[1]; g[1] = p[1] - m[2]; g[2] = p[2] - m[3];
            return true;
        }
        if (cls == (double)kCylinder3D) {
            const double e0 = p[0] - m[1], e1 = p[1] - m[2], e2 = p[2] - m[3];
            const double t = (e0 * m[4] + e1 * m[5]) + e2 * m[6];
            g[0] = e0 - t * m[4]; g[1] = e1 - t * m[5]; g[2] = e2 - t * m[6];
            return true;
        }
        if (cls == (double)kCone3D) {
            const double q[6] = {m[1], m[2], m[3], m[4], m[5], m[6]};
            const double e0 = p[0] - m[1], e1 = p[1] - m[2], e2 = p[2] - m[3];
            const double h = (e0 * m[4] + e1 * m[5]) + e2 * m[6];
            const double rho = sqrt(Residual<kLine3D>::squared(p, q));
            const double sr = m[8] * rho;
            g[0] = m[7] * (e0 - h * m[4]) - sr * m[4];
            g[1] = m[7] * (e1 - h * m[5]) - sr * m[5];
            g[2] = m[7] * (e2 - h * m[6]) - sr * m[6];
            return true;
        }
        return false;
    }
    template <class NT>
    static __device__ __forceinline__ bool agrees(const NT& n, const double (&g)[3], double kappa) {
        const double nn = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2];
        const double gg = (g[0] * g[0] + g[1] * g[1]) + g[2] * g[2];
        const double ng = (n[0] * g[0] + n[1] * g[1]) + n[2] * g[2];
        const double w = nn * gg;
        return ng * ng >= kappa * w && w > 0.0;
    }
    template <class PT, class NT, class MD>
    static __device__ __forceinline__ double squared(const PT& p, const NT& n, const MD& m, double kappa) {
        const double sq = Base::squared(p, m);
        double g[3];
        if (!surface_normal(p, m, g)) return sq;   // no class: NaN
        return agrees(n, g, kappa) ? sq : __builtin_inf();
    }
    template <class PT, class NT, class MD>
    static __device__ __forceinline__ double squared_within(const PT& p, const NT& n, const MD& m, double T2, double kappa) {
        const double sq = Base::squared(p, m);
        if (!(sq <= T2)) return sq;   // beyond T2 either way, or NaN: never an inlier, priced as beyond the threshold
        double g[3];
        return surface_normal(p, m, g) && agrees(n, g, kappa) ? sq : __builtin_inf();
    }
};

// DefaultHomographyEstimator (progressivex_python.cpp:252) [U-1]: one-way forward transfer error,
// H row-major 3x3 (progressivex_python.cpp:292-300).
template <> struct Residual<kHomography> {
    static constexpr int D = 4, P = 9, sample = 4, slots = 1, bound = kBoundBox;
    static constexpr int obs0 = 2, in0 = 0, in1 = 3, box1 = 1;   // the scale runs over all four coordinates (Filter32<kHomography>)
    template <class PT, class MD>
    static __device__ __forceinline__ double squared(const PT& p, const MD& h) {
        const double t1 = h[0] * p[0] + h[1] * p[1] + h[2];
        const double t2 = h[3] * p[0] + h[4] * p[1] + h[5];
        const double t3 = h[6] * p[0] + h[7] * p[1] + h[8];
        const double d1 = p[2] - (t1 / t3);
        const double d2 = p[3] - (t2 / t3);
        return d1 * d1 + d2 * d2;
    }
    template <class PT, class MD>
    static __device__ __forceinline__ double plain(const PT& p, const MD& m) { return sqrt(squared(p, m)); }
};

// Symmetric transfer error (north-star wording): model = [H | H^-1].
template <> struct Residual<kHomographySym> {
    static constexpr int D = 4, P = 18, sample = 0, slots = 0, bound = kBoundBox;
    static constexpr int obs0 = 2, in0 = 0, in1 = 3, box1 = 1;   // the forward part
    template <class PT, class MD>
    static __device__ __forceinline__ double squared(const PT& p, const MD& h) {
        const double t1 = h[0] * p[0] + h[1] * p[1] + h[2];
        const double t2 = h[3] * p[0] + h[4] * p[1] + h[5];
        const double t3 = h[6] * p[0] + h[7] * p[1] + h[8];
        const double d1 = p[2] - (t1 / t3);
        const double d2 = p[3] - (t2 / t3);
        const double s1 = h[9] * p[2] + h[10] * p[3] + h[11];
        const double s2 = h[12] * p[2] + h[13] * p[3] + h[14];
        const double s3 = h[15] * p[2] + h[16] * p[3] + h[17];
        const double e1 = p[0] - (s1 / s3);
        const double e2 = p[1] - (s2 / s3);
        return (d1 * d1 + d2 * d2) + (e1 * e1 + e2 * e2);
    }
    template <class PT, class MD>
    static __device__ __forceinline__ double plain(const PT& p, const MD& m) { return sqrt(squared(p, m)); }
};

// DefaultFundamentalMatrixEstimator (progressivex_python.cpp:616) [U-2]: squared Sampson distance,
// F row-major (progressivex_python.cpp:654-662).
template <> struct Residual<kFundamental> : NoProjectiveMap {
    static constexpr int D = 4, P = 9, sample = 7, slots = 3, bound = kBoundBoxAll;
    template <class PT, class MD>
    static __device__ __forceinline__ double squared(const PT& p, const MD& f) {
        const double rxc = f[0] * p[2] + f[3] * p[3] + f[6];
        const double ryc = f[1] * p[2] + f[4] * p[3] + f[7];
        const double rwc = f[2] * p[2] + f[5] * p[3] + f[8];
        const double r = p[0] * rxc + p[1] * ryc + rwc;
        const double rx = f[0] * p[0] + f[1] * p[1] + f[2];
        const double ry = f[3] * p[0] + f[4] * p[1] + f[5];
        return r * r / (rxc * rxc + ryc * ryc + rx * rx + ry * ry);
    }
    template <class PT, class MD>
    static __device__ __forceinline__ double plain(const PT& p, const MD& m) { return sqrt(squared(p, m)); }
};

// DefaultPnPEstimator (progressivex_python.cpp:119) [U-3]: squared reprojection error in normalised image
// coordinates; P=[R|t] row-major 3x4 (progressivex_python.cpp:156-167); row (u,v,X,Y,Z) (:88-92).
template <> struct Residual<kPnP> {
    static constexpr int D = 5, P = 12, sample = 3, slots = 4, bound = kBoundBox;
    static constexpr int obs0 = 0, in0 = 2, in1 = 4, box1 = 4;
    template <class PT, class MD>
    static __device__ __forceinline__ double squared(const PT& p, const MD& m) {
        const double px = m[0] * p[2] + m[1] * p[3] + m[2] * p[4] + m[3];
        const double py = m[4] * p[2] + m[5] * p[3] + m[6] * p[4] + m[7];
        const double pz = m[8] * p[2] + m[9] * p[3] + m[10] * p[4] + m[11];
        const double du = p[0] - (px / pz);
        const double dv = p[1] - (py / pz);
        return du * du + dv * dv;
    }
    template <class PT, class MD>
    static __device__ __forceinline__ double plain(const PT& p, const MD& m) { return sqrt(squared(p, m)); }
};

// VanishingPointEstimator::residual, vanishing_point_estimator.h:166-189 (squared at :134-140), in-tree.
template <> struct Residual<kVanishingPoint> : NoProjectiveMap {
    static constexpr int D = 4, P = 3, sample = 2, slots = 1, bound = kBoundVanishing;
    template <class PT, class MD>
    static __device__ __forceinline__ double plain(const PT& p, const MD& v) {
        const double mx = (p[0] + p[2]) / 2.0, my = (p[1] + p[3]) / 2.0;
        const double lx = my * v[2] - v[1];
        const double ly = -(mx * v[2] - v[0]);
        const double lz = mx * v[1] - my * v[0];
        return fabs(lx * p[0] + ly * p[1] + lz) / sqrt(lx * lx + ly * ly);
    }
    template <class PT, class MD>
    static __device__ __forceinline__ double squared(const PT& p, const MD& m) {
        const double r = plain(p, m);
        return r * r;
    }
};

// The one list of model types: calls f(std::integral_constant<int, MT>{}) for the runtime type mt; false if mt is not a type.
template <class F> inline bool with_model_type(int mt, F&& f) {
    switch (mt) {
    case kLine2D: f(std::integral_constant<int, kLine2D>{}); return true;
    case kHomography: f(std::integral_constant<int, kHomography>{}); return true;
    case kFundamental: f(std::integral_constant<int, kFundamental>{}); return true;
    case kPnP: f(std::integral_constant<int, kPnP>{}); return true;
    case kVanishingPoint: f(std::integral_constant<int, kVanishingPoint>{}); return true;
    case kHomographySym: f(std::integral_constant<int, kHomographySym>{}); return true;
    case kPlane3D: f(std::integral_constant<int, kPlane3D>{}); return true;
    case kSphere3D: f(std::integral_constant<int, kSphere3D>{}); return true;
    case kCircle2D: f(std::integral_constant<int, kCircle2D>{}); return true;
    case kLine3D: f(std::integral_constant<int, kLine3D>{}); return true;
    case kCylinder3D: f(std::integral_constant<int, kCylinder3D>{}); return true;
    case kCone3D: f(std::integral_constant<int, kCone3D>{}); return true;
    case kPrimitive3D: f(std::integral_constant<int, kPrimitive3D>{}); return true;
    case kOrientedPrimitive3D: f(std::integral_constant<int, kOrientedPrimitive3D>{}); return true;
    case kTorus3D: f(std::integral_constant<int, kTorus3D>{}); return true;
    default: return false;
    }
}

// ---- oriented types: how the kernels reach a point's normal --------------------------------------------------------------------------
// An oriented type's row buffers carry the normals and kappa BEHIND the rows, in the rows' own order, so that no kernel takes another
// argument and the instances of the other types stay what they were:
//   rows [count][D]  |  normals [count][3]  |  kappa                     the caller's order (pts) and the Morton order (pts_s), count = n
//   rows [groups][D][64]  |  normals [groups][3][64]  |  kappa           the group-blocked copy (pts_g), the tail group padded with its
//                                                                        last point's normal, as its rows are
// pgx_set_points reserves the room, pgx_set_normals and pgx_set_normal_tolerance fill it (capi.hip).  Normal<MT> is what a kernel
// carries per point: three doubles for an oriented type, nothing for the others - whose code is then R::squared(pt, mdl) as before.
template <class R, class = void> struct IsOriented : std::false_type {};
template <class R> struct IsOriented<R, std::enable_if_t<R::oriented>> : std::true_type {};
template <int MT> constexpr bool kOriented = IsOriented<Residual<MT>>::value;

template <int MT, bool = kOriented<MT>> struct Normal {};
template <int MT> struct Normal<MT, true> { double v[3]; };

template <int MT> __device__ __forceinline__ double oriented_kappa(const double* __restrict__ rows, int64_t count /* n, or groups * 64 */)
{
    if constexpr (kOriented<MT>) return rows[count * (Residual<MT>::D + 3)];
    else return 0.0;
}
// normal of row i of an array-of-rows buffer of n rows
template <int MT> __device__ __forceinline__ Normal<MT> load_normal(const double* __restrict__ rows, int64_t n, int64_t i)
{
    Normal<MT> nr;
    if constexpr (kOriented<MT>) {
        const double* __restrict__ q = rows + n * Residual<MT>::D + i * 3;
#pragma unroll
        for (int k = 0; k < 3; ++k) nr.v[k] = q[k];
    }
    return nr;
}
// normal of lane `lane` of group g of the group-blocked copy
template <int MT> __device__ __forceinline__ Normal<MT> load_normal_blocked(const double* __restrict__ rows_g, int groups, int g, int lane)
{
    Normal<MT> nr;
    if constexpr (kOriented<MT>) {
        const double* __restrict__ q = rows_g + ((int64_t)groups * Residual<MT>::D + (int64_t)g * 3) * 64 + lane;
#pragma unroll
        for (int k = 0; k < 3; ++k) nr.v[k] = q[k * 64];
    }
    return nr;
}
// The one way the scoring and the pointwise kernels evaluate a squared residual: R::squared(pt, mdl) for every type but the oriented
// ones, whose value also depends on the point's normal and is only needed up to T2 (Residual<kOrientedPrimitive3D>::squared_within).
template <int MT, class PT, class MD>
__device__ __forceinline__ double squared_at(const PT& p, const Normal<MT>& nr, const MD& m, double T2, double kappa)
{
    if constexpr (kOriented<MT>) return Residual<MT>::squared_within(p, nr.v, m, T2, kappa);
    else return Residual<MT>::squared(p, m);
}

// The constants of Residual<mt> for host code that holds the type as a number.
struct ModelInfo { int D, P, sample, slots, bound, obs0, in0, in1, box1; const char* normals_solver; bool oriented; };

inline bool model_info(int mt, ModelInfo* out) {
    return with_model_type(mt, [&](auto t) {
        using R = Residual<decltype(t)::value>;
        *out = {R::D, R::P, R::sample, R::slots, R::bound, R::obs0, R::in0, R::in1, R::box1, NormalsSolver<R>::name, IsOriented<R>::value};
    });
}

inline int model_dims(int mt, int* d, int* p) {
    ModelInfo mi;
    if (!model_info(mt, &mi)) return -1;
    if (d) *d = mi.D;
    if (p) *p = mi.P;
    return 0;
}

}  // namespace pgx
