// solve.hip — batched minimal solvers on the resident points (first slice): the two solvers with
// an exact in-tree or closed-form specification.  The hypotheses are generated straight into the resident hypothesis
// buffer, so scoring them needs no host -> device model upload.
//
// Replaces, per sample of the proposal engine's main loop (gcransac::GCRANSAC::run, graph-cut-ransac submodule, absent):
//   vanishing point from two segments   /root/reference/src/pyprogressivex/include/solver_vanishing_point_two_lines.h:147-185
//                                       (l_i = e_i0 x e_i1 :174-179, v = l_0 x l_1 :180-182, vec_norm :123-131)
//   2D line through two points          Default2DLineEstimator's minimal solver (progressivex_python.cpp:489), absent
//                                       upstream [U-4]: unit normal (-dy, dx) / |d|, offset c = -(n . a)
//   fundamental matrix from 7 points    DefaultFundamentalMatrixEstimator's minimal solver (progressivex_python.cpp:616), absent
//                                       upstream: null space of the 7x9 epipolar system by Gauss-Jordan elimination with
//                                       full pivoting, det(l F1 + (1-l) F2) = 0 as a cubic, real roots by bisection of
//                                       one root + the quadratic factor (only + - * / sqrt: identical on CPU and GPU),
//                                       where det(F1 - F2) vanishes F1 - F2 itself follows the finite roots (the chart's root at
//                                       infinity); up to three models per sample (three slots, NaN = no root)
//   homography from 4 correspondences   DefaultHomographyEstimator's minimal solver (progressivex_python.cpp:252), absent
//                                       upstream: h33 = 1, the 8x8 DLT system of the isotropically scaled points by
//                                       Gaussian elimination with partial pivoting (rank test 1e-12), scaling undone
//   absolute pose from 3 points (P3P)   DefaultPnPEstimator's minimal solver (progressivex_python.cpp:119), absent upstream:
//                                       Grunert's quartic, positive real roots by bisection between the critical points (a
//                                       critical point itself where the quartic touches zero), u = s2/s1 from the linear formula
//                                       or, where that fails its gates (two poses sharing v), from the first side constraint;
//                                       pose from the orthonormal frames of the two congruent triangles; four slots
//   3-D plane through three points      findPlanes' minimal solver (no reference counterpart; the flat family with the line): n =
//                                       (p1 - p0) x (p2 - p0) in cross3's component order, ln = sqrt(n . n), (a, b, c) = n / ln,
//                                       d = -((a x0 + b y0) + c z0); collinear or coincident points (ln == 0) give NaN
//   the round family (no reference counterpart): the centre offset e from p0 solves a_i . e = |a_i|^2 / 2 (a_i = p_i - p0);
//   singular systems (det == 0), non-finite values and radii outside the context's pgx_set_radius_range give NaN
//     3-D sphere through four points    findSpheres' minimal solver: Cramer's rule on cross products (det == 0: coplanar points)
//     2-D circle through three points   findCircles' minimal solver: Cramer's rule on the 2x2 system (det == 0: collinear points)
//   3-D line through two points         findLines3D's minimal solver (no reference counterpart): d = (b - a) / |b - a|, p = a;
//                                       coincident points and a length that is not finite give NaN
//   cylinder through two oriented points findCylinders' minimal solver (no reference counterpart): the axis along na x nb through the
//                                       point where a + s na and b + t nb cross seen along it, r = |s| |na|; the normals are the
//                                       resident side array of pgx_set_normals; parallel normals, non-finite values and radii
//                                       outside pgx_set_radius_range give NaN
//   cone through three oriented points  findCones' minimal solver (no reference counterpart): the apex is the common point of the
//                                       three tangent planes, the axis is orthogonal to the differences of the three unit vectors
//                                       from the apex to the samples; tangent planes without a common point, a sample at the apex,
//                                       non-finite values, cos <= 0 and a sine outside pgx_set_radius_range give NaN
//   torus through four oriented points  findTori's minimal solver (no reference counterpart), two slots per sample: the axis is a common
//                                       transversal of the four normal LINES (at most two), the tube's circle goes through three
//                                       samples in the half-plane about it; no transversal, a singular circle, non-finite values,
//                                       R <= r and radii outside pgx_set_radius_range / pgx_set_major_radius_range give NaN
// The eight solvers with one model per sample (line, vanishing point, plane, sphere, circle, 3-D line, cylinder, cone) and the torus'
// with two share one kernel shell, solve_kernel<MT>, one lane per model row;
// the 7-point, 4-point and P3P solvers and the mixed-primitive solver (four slots of four classes per sample) run one lane per sample in
// kernels of their own.
// Operation order is the contract (bit-exact against the oracle's C restatement, no contraction, IEEE sqrt and divide).
// A degenerate sample (coincident points / parallel or identical lines) yields a NaN model, which can never have an
// inlier; the caller drops it (the reference's solvers return "no model").
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <type_traits>

#include "pgx_internal.h"
#include "rng.hip.h"

namespace pgx {

namespace {

constexpr int kSolveBlock = 256;

__device__ __forceinline__ void cross3(double a1, double b1, double c1, double a2, double b2, double c2, double* o)
{
    o[0] = b1 * c2 - c1 * b2;      // solver_vanishing_point_two_lines.h:106-121
    o[1] = -(a1 * c2 - c1 * a2);
    o[2] = a1 * b2 - b1 * a2;
}

// ---- the lane-per-model solvers: one __device__ function per type, one kernel shell ---------------------------------------------
// solve_minimal(type, p, nq, rmin, rmax, m): p = the sample's Residual<MT>::sample point rows (all inside the point set), nq = the same
// points' rows of the resident normals (pgx_set_normals; only the types with Residual<MT>::normals_solver read them, and the launch
// refuses those without them), m = the model, preset to NaN - a degenerate sample leaves it so.  rmin, rmax: the context's
// pgx_set_radius_range (the round family and the cylinder read them as radii, the cone as the range of its sine, the torus as the
// range of its tube radius).  A type with more than one slot takes (type, p, nq, rmin, rmax, Rmin, Rmax, slot, m): the torus, with
// Rmin, Rmax the context's pgx_set_major_radius_range and slot the solution asked for.
template <int MT> using Type = std::integral_constant<int, MT>;

// 2-point line [U-4]: unit normal (-dy, dx) / |d|, offset c = -(n . a); coincident points (ln == 0; also false on NaN) give NaN, and so
// does a length that is not finite (an overflowing square): (-dy, dx) / inf would be a zero normal, and every point is an inlier of that.
__device__ __forceinline__ void solve_minimal(Type<kLine2D>, const double* const* p, const double* const*, double, double, double* m)
{
    const double ax = p[0][0], ay = p[0][1];
    const double dx = p[1][0] - ax, dy = p[1][1] - ay;
    const double ln = sqrt(dx * dx + dy * dy);
    if (ln > 0.0 && isfinite(ln)) {
        m[0] = -dy / ln;
        m[1] = dx / ln;
        m[2] = -(m[0] * ax + m[1] * ay);
    }
}

// vanishing point of two segments (solver_vanishing_point_two_lines.h:174-182); parallel or identical lines give NaN, and so does a
// norm that is not finite (the 2-point line's guard: v / inf would be the zero vector).
__device__ __forceinline__ void solve_minimal(Type<kVanishingPoint>, const double* const* p, const double* const*, double, double, double* m)
{
    const double *a = p[0], *b = p[1];
    double l0[3], l1[3], v[3];
    cross3(a[0], a[1], 1.0, a[2], a[3], 1.0, l0);
    cross3(b[0], b[1], 1.0, b[2], b[3], 1.0, l1);
    cross3(l0[0], l0[1], l0[2], l1[0], l1[1], l1[2], v);
    const double ln = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    if (ln > 0.0 && isfinite(ln)) { m[0] = v[0] / ln; m[1] = v[1] / ln; m[2] = v[2] / ln; }
}

// 3-point plane -> (a, b, c, d).  Operation order (the contract; PlaneEstimator.minimal restates it):
//   u = p1 - p0, v = p2 - p0 (componentwise), n = cross3(u, v), ln = sqrt((n0 n0 + n1 n1) + n2 n2),
//   a = n0 / ln, b = n1 / ln, c = n2 / ln, d = -((a x0 + b y0) + c z0).
// ln == 0 (coincident or collinear points; also false on NaN) gives a NaN model, and so does a non-finite ln (an overflowing product):
// n / inf would be a zero normal with a NaN offset, a row that is neither a model nor all NaN.
__device__ __forceinline__ void solve_minimal(Type<kPlane3D>, const double* const* p, const double* const*, double, double, double* m)
{
    const double *p0 = p[0], *p1 = p[1], *p2 = p[2];
    double nv[3];
    cross3(p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2], p2[0] - p0[0], p2[1] - p0[1], p2[2] - p0[2], nv);
    const double ln = sqrt((nv[0] * nv[0] + nv[1] * nv[1]) + nv[2] * nv[2]);
    if (ln > 0.0 && isfinite(ln)) {
        m[0] = nv[0] / ln;
        m[1] = nv[1] / ln;
        m[2] = nv[2] / ln;
        m[3] = -((m[0] * p0[0] + m[1] * p0[1]) + m[2] * p0[2]);
    }
}

// The tail both round solvers share: the model (c, r) counts only if the system was regular (det != 0: no coplanar / collinear or
// coincident points), centre and radius are finite and rmin <= r <= rmax; otherwise it stays NaN.
template <int DIM>
__device__ __forceinline__ void accept_round(double det, const double* c, double r, double rmin, double rmax, double* m)
{
    bool ok = det != 0.0 && isfinite(r) && r >= rmin && r <= rmax;
    for (int k = 0; k < DIM; ++k) ok = ok && isfinite(c[k]);
    if (!ok) return;
    for (int k = 0; k < DIM; ++k) m[k] = c[k];
    m[DIM] = r;
}

// 4-point sphere -> (cx, cy, cz, r).  Operation order (the contract; SphereEstimator.minimal restates it):
//   a_i = p_i - p0 (componentwise, i = 1..3), h_i = 0.5 ((a_i0 a_i0 + a_i1 a_i1) + a_i2 a_i2),
//   n1 = cross3(a2, a3), n2 = cross3(a3, a1), n3 = cross3(a1, a2), det = (a1_0 n1_0 + a1_1 n1_1) + a1_2 n1_2,
//   e_k = ((h1 n1_k + h2 n2_k) + h3 n3_k) / det, r = sqrt((e_0 e_0 + e_1 e_1) + e_2 e_2), c = p0 + e.
__device__ __forceinline__ void solve_minimal(Type<kSphere3D>, const double* const* p, const double* const*, double rmin, double rmax, double* m)
{
    const double* p0 = p[0];
    double a[3][3], h[3];
    for (int i = 0; i < 3; ++i) {
        for (int k = 0; k < 3; ++k) a[i][k] = p[i + 1][k] - p0[k];
        h[i] = 0.5 * ((a[i][0] * a[i][0] + a[i][1] * a[i][1]) + a[i][2] * a[i][2]);
    }
    double n1[3], n2[3], n3[3];
    cross3(a[1][0], a[1][1], a[1][2], a[2][0], a[2][1], a[2][2], n1);
    cross3(a[2][0], a[2][1], a[2][2], a[0][0], a[0][1], a[0][2], n2);
    cross3(a[0][0], a[0][1], a[0][2], a[1][0], a[1][1], a[1][2], n3);
    const double det = (a[0][0] * n1[0] + a[0][1] * n1[1]) + a[0][2] * n1[2];
    double e[3];
    for (int k = 0; k < 3; ++k) e[k] = ((h[0] * n1[k] + h[1] * n2[k]) + h[2] * n3[k]) / det;
    const double r = sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]);
    const double c[3] = {p0[0] + e[0], p0[1] + e[1], p0[2] + e[2]};
    accept_round<3>(det, c, r, rmin, rmax, m);
}

// 3-point circle -> (cx, cy, r).  Operation order (the contract; CircleEstimator.minimal restates it):
//   a_i = p_i - p0 (componentwise, i = 1, 2), h_i = 0.5 (a_i0 a_i0 + a_i1 a_i1), det = a_10 a_21 - a_11 a_20,
//   e_0 = (h_1 a_21 - h_2 a_11) / det, e_1 = (a_10 h_2 - a_20 h_1) / det, r = sqrt(e_0 e_0 + e_1 e_1), c = p0 + e.
__device__ __forceinline__ void solve_minimal(Type<kCircle2D>, const double* const* p, const double* const*, double rmin, double rmax, double* m)
{
    const double *p0 = p[0], *p1 = p[1], *p2 = p[2];
    const double a10 = p1[0] - p0[0], a11 = p1[1] - p0[1], a20 = p2[0] - p0[0], a21 = p2[1] - p0[1];
    const double h1 = 0.5 * (a10 * a10 + a11 * a11), h2 = 0.5 * (a20 * a20 + a21 * a21);
    const double det = a10 * a21 - a11 * a20;
    const double e0 = (h1 * a21 - h2 * a11) / det, e1 = (a10 * h2 - a20 * h1) / det;
    const double r = sqrt(e0 * e0 + e1 * e1);
    const double c[2] = {p0[0] + e0, p0[1] + e1};
    accept_round<2>(det, c, r, rmin, rmax, m);
}

// 2-point 3-D line -> (p, d), a point on the line and a unit direction.  Operation order (the contract; Line3DEstimator.minimal
// restates it):
//   v = b - a (componentwise), ln = sqrt((v0 v0 + v1 v1) + v2 v2), d = v / ln, p = a.
// ln == 0 (coincident points; also false on NaN) gives a NaN model, and so does a non-finite ln, as in the 2-D line, vanishing point
// and plane solvers: v / inf would be a zero direction, and every point is an inlier of that.
__device__ __forceinline__ void solve_minimal(Type<kLine3D>, const double* const* p, const double* const*, double, double, double* m)
{
    const double *a = p[0], *b = p[1];
    const double v0 = b[0] - a[0], v1 = b[1] - a[1], v2 = b[2] - a[2];
    const double ln = sqrt((v0 * v0 + v1 * v1) + v2 * v2);
    if (ln > 0.0 && isfinite(ln)) {
        m[0] = a[0];
        m[1] = a[1];
        m[2] = a[2];
        m[3] = v0 / ln;
        m[4] = v1 / ln;
        m[5] = v2 / ln;
    }
}

// 2-point cylinder from oriented points -> (c, d, r), a point on the axis, a unit direction and a radius (findCylinders; no reference
// counterpart).  Both normals are orthogonal to the axis and both points lie r from it, so with samples (a, b) and their normals
// (na, nb), which need be neither unit nor consistently signed: the axis runs along na x nb, and it meets the line a + s na where
// that line, seen along the axis, crosses the line b + t nb.  Operation order (the contract; CylinderEstimator.minimal restates it):
//   D = cross3(na, nb), dd = (D0 D0 + D1 D1) + D2 D2, ln = sqrt(dd), d = D / ln,
//   v = b - a (componentwise), k = (v0 d0 + v1 d1) + v2 d2, w = v - k d (componentwise: w_j = v_j - k d_j),
//   x = cross3(w, nb), s = ((x0 D0 + x1 D1) + x2 D2) / dd,
//   c = a + s na (c_j = a_j + s na_j), r = |s| sqrt((na0 na0 + na1 na1) + na2 na2).
// (w + t nb = s na crossed with nb and dotted with D gives s |D|^2 = (w x nb) . D.)  Flipping or rescaling a normal changes D and s
// together and leaves c, r and the axis - d up to its sign - the same up to rounding.  The model stays NaN unless ln > 0 and ln is
// finite (parallel normals, a zero normal, coincident samples with one normal, the same index twice, non-finite input or an
// overflowing square), every entry of c and r are finite, and rmin <= r <= rmax.  Coincident points with different normals give r = 0.
__device__ __forceinline__ void solve_minimal(Type<kCylinder3D>, const double* const* p, const double* const* nq, double rmin, double rmax, double* m)
{
    const double *a = p[0], *b = p[1], *na = nq[0], *nb = nq[1];
    double D[3], x[3];
    cross3(na[0], na[1], na[2], nb[0], nb[1], nb[2], D);
    const double dd = (D[0] * D[0] + D[1] * D[1]) + D[2] * D[2];
    const double ln = sqrt(dd);
    if (!(ln > 0.0) || !isfinite(ln)) return;
    const double d0 = D[0] / ln, d1 = D[1] / ln, d2 = D[2] / ln;
    const double v0 = b[0] - a[0], v1 = b[1] - a[1], v2 = b[2] - a[2];
    const double k = (v0 * d0 + v1 * d1) + v2 * d2;
    cross3(v0 - k * d0, v1 - k * d1, v2 - k * d2, nb[0], nb[1], nb[2], x);
    const double s = ((x[0] * D[0] + x[1] * D[1]) + x[2] * D[2]) / dd;
    const double c0 = a[0] + s * na[0], c1 = a[1] + s * na[1], c2 = a[2] + s * na[2];
    const double r = fabs(s) * sqrt((na[0] * na[0] + na[1] * na[1]) + na[2] * na[2]);
    if (!(isfinite(c0) && isfinite(c1) && isfinite(c2) && isfinite(r) && r >= rmin && r <= rmax)) return;
    m[0] = c0; m[1] = c1; m[2] = c2;
    m[3] = d0; m[4] = d1; m[5] = d2;
    m[6] = r;
}

// 3-point cone from oriented points -> (a, d, c, s), the apex, a unit axis direction pointing into the nappe and the cosine and sine of
// the half-angle (findCones; no reference counterpart).  Every tangent plane of a cone passes through its apex, and the unit vectors
// from the apex to points of one nappe all make the half-angle with the axis.  With samples p_i and their normals n_i (i = 0, 1, 2),
// which need be neither unit nor consistently signed.  Operation order (the contract; ConeEstimator.minimal restates it):
//   X0 = cross3(n1, n2), X1 = cross3(n2, n0), X2 = cross3(n0, n1), det = (n0_0 X0_0 + n0_1 X0_1) + n0_2 X0_2,
//   b_i = (n_i0 p_i0 + n_i1 p_i1) + n_i2 p_i2,  a_k = ((b0 X0_k + b1 X1_k) + b2 X2_k) / det       (Cramer's rule on n_i . a = b_i),
//   w_i = p_i - a (componentwise), l_i = sqrt((w_i0 w_i0 + w_i1 w_i1) + w_i2 w_i2), g_i = w_i / l_i,
//   D = cross3(g1 - g0, g2 - g0), ln = sqrt((D0 D0 + D1 D1) + D2 D2), d = D / ln,
//   t_i = (d0 g_i0 + d1 g_i1) + d2 g_i2; if (t0 + t1) + t2 < 0 then d = -d (each component);
//   c = (d0 g_00 + d1 g_01) + d2 g_02 (with the final d),  s = sqrt(Residual<kLine3D>::squared(g0, (0, 0, 0, d))).
// Flipping or rescaling a normal scales its b_i, two of the X_j and det together and leaves a, and everything after it, the same up to
// rounding.  The model stays NaN unless det != 0, every l_i > 0, ln > 0, all eight entries are finite, c > 0 (a half-angle below 90
// degrees: the three samples then lie on the nappe d points into) and rmin <= s <= rmax: the context's radius range bounds the sine
// of the half-angle here.  A zero normal makes det 0 exactly, the same point twice makes g1 - g0 or g2 - g0 (and so D) 0 exactly, a sample
// at the apex has l_i = 0.  Coplanar normals make det 0 only up to rounding: where it comes out as a tiny number the apex lies far
// away and the model, if finite, collects no inliers.
__device__ __forceinline__ void solve_minimal(Type<kCone3D>, const double* const* p, const double* const* nq, double rmin, double rmax, double* m)
{
    const double *n0 = nq[0], *n1 = nq[1], *n2 = nq[2];
    double X[3][3], b[3], a[3], g[3][3], D[3];
    cross3(n1[0], n1[1], n1[2], n2[0], n2[1], n2[2], X[0]);
    cross3(n2[0], n2[1], n2[2], n0[0], n0[1], n0[2], X[1]);
    cross3(n0[0], n0[1], n0[2], n1[0], n1[1], n1[2], X[2]);
    const double det = (n0[0] * X[0][0] + n0[1] * X[0][1]) + n0[2] * X[0][2];
    if (det == 0.0) return;
    for (int i = 0; i < 3; ++i) b[i] = (nq[i][0] * p[i][0] + nq[i][1] * p[i][1]) + nq[i][2] * p[i][2];
    for (int k = 0; k < 3; ++k) a[k] = ((b[0] * X[0][k] + b[1] * X[1][k]) + b[2] * X[2][k]) / det;
    for (int i = 0; i < 3; ++i) {
        const double w0 = p[i][0] - a[0], w1 = p[i][1] - a[1], w2 = p[i][2] - a[2];
        const double l = sqrt((w0 * w0 + w1 * w1) + w2 * w2);
        if (!(l > 0.0)) return;
        g[i][0] = w0 / l; g[i][1] = w1 / l; g[i][2] = w2 / l;
    }
    cross3(g[1][0] - g[0][0], g[1][1] - g[0][1], g[1][2] - g[0][2], g[2][0] - g[0][0], g[2][1] - g[0][1], g[2][2] - g[0][2], D);
    const double ln = sqrt((D[0] * D[0] + D[1] * D[1]) + D[2] * D[2]);
    if (!(ln > 0.0)) return;
    double d[3] = {D[0] / ln, D[1] / ln, D[2] / ln};
    double t[3];
    for (int i = 0; i < 3; ++i) t[i] = (d[0] * g[i][0] + d[1] * g[i][1]) + d[2] * g[i][2];
    if ((t[0] + t[1]) + t[2] < 0.0) { d[0] = -d[0]; d[1] = -d[1]; d[2] = -d[2]; }
    const double c = (d[0] * g[0][0] + d[1] * g[0][1]) + d[2] * g[0][2];
    const double axis[6] = {0.0, 0.0, 0.0, d[0], d[1], d[2]};
    const double s = sqrt(Residual<kLine3D>::squared(g[0], axis));
    if (!(isfinite(a[0]) && isfinite(a[1]) && isfinite(a[2]) && isfinite(d[0]) && isfinite(d[1]) && isfinite(d[2]) && isfinite(c) &&
          isfinite(s) && c > 0.0 && s >= rmin && s <= rmax))
        return;
    m[0] = a[0]; m[1] = a[1]; m[2] = a[2];
    m[3] = d[0]; m[4] = d[1]; m[5] = d[2];
    m[6] = c; m[7] = s;
}

// 4-point torus from oriented points -> (c, d, R, r), the centre, a unit axis direction and the major and minor radius (findTori; no
// reference counterpart), TWO slots per sample.  Every normal of a surface of revolution meets its axis, so the axis is a common
// transversal of the four normal lines (p_i, n_i), of which there are at most two: slot j takes the j-th.  The normals are read as
// LINES here, not as tangent planes; they need be neither unit nor consistently signed.  A transversal through a = p0 + s n0 and
// b = p1 + t n1 meets line i (i = 2, 3) iff det[b - a, n_i, p_i - a] = 0, which is bilinear in (s, t): A_i s t + B_i s + C_i t + D_i = 0
// (the s^2 term is n0 . (n_i x n0) = 0).  Operation order (the contract; TorusEstimator.minimal restates it), dot(x, y) = (x0 y0 + x1 y1)
// + x2 y2 throughout:
//   q = p1 - p0, and for i = 2, 3 (written 1, 2 below):  g = p_i - p0,  X = cross3(n_i, g),  Y = cross3(n_i, n0),
//   A_i = -dot(n1, Y),  B_i = -(dot(q, Y) + dot(n0, X)),  C_i = dot(n1, X),  D_i = dot(q, X);
//   t = -(B1 s + D1) / (A1 s + C1) in the second condition leaves qa s^2 + qb s + qc = 0 with
//   qa = B2 A1 - A2 B1,  qb = ((B2 C1 - A2 D1) - C2 B1) + D2 A1,  qc = D2 C1 - C2 D1,  disc = qb qb - (4 qa) qc,  sq = sqrt(disc),
//   s = (-qb + sq) / (2 qa) in slot 0 and (-qb - sq) / (2 qa) in slot 1,  den = A1 s + C1,  t = -(B1 s + D1) / den,
//   a = p0 + s n0,  b = p1 + t n1,  Dv = b - a (componentwise),  ln = sqrt(dot(Dv, Dv)),  d = Dv / ln,
//   for k = 0, 1, 2:  e = p_k - a,  h_k = dot(e, d),  rho_k = sqrt(Residual<kLine3D>::squared(p_k, (a, d))),
//   the circle through (h_k, rho_k) by the 3-point circle solver's own arithmetic: a1 = (h_1 - h_0, rho_1 - rho_0), a2 likewise,
//   g_i = 0.5 (a_i0 a_i0 + a_i1 a_i1), det = a_10 a_21 - a_11 a_20, z_0 = (g_1 a_21 - g_2 a_11) / det, z_1 = (a_10 g_2 - a_20 g_1) / det,
//   r = sqrt(z_0 z_0 + z_1 z_1),  hc = h_0 + z_0,  R = rho_0 + z_1,  c = a + hc d.
// The model stays NaN unless disc >= 0, qa != 0, den != 0, ln > 0, det != 0, all eight entries are finite, R > r (a ring torus),
// rmin <= r <= rmax (pgx_set_radius_range bounds the tube radius here) and Rmin <= R <= Rmax (pgx_set_major_radius_range).  Normal
// lines that are coplanar or parallel make every coefficient, and so qa, 0 up to rounding: where it comes out as a tiny number the
// model, if finite, collects no inliers.  The fourth sample enters through the transversal alone.
__device__ __forceinline__ double dot3(const double* x, const double* y) { return (x[0] * y[0] + x[1] * y[1]) + x[2] * y[2]; }
__device__ __forceinline__ void solve_minimal(Type<kTorus3D>, const double* const* p, const double* const* nq, double rmin, double rmax, double Rmin,
                                              double Rmax, int slot, double* m)
{
    const double *p0 = p[0], *p1 = p[1], *n0 = nq[0], *n1 = nq[1];
    const double q[3] = {p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2]};
    double A[2], B[2], C[2], D[2];
    for (int i = 0; i < 2; ++i) {
        const double *pi = p[i + 2], *ni = nq[i + 2];
        const double g[3] = {pi[0] - p0[0], pi[1] - p0[1], pi[2] - p0[2]};
        double X[3], Y[3];
        cross3(ni[0], ni[1], ni[2], g[0], g[1], g[2], X);
        cross3(ni[0], ni[1], ni[2], n0[0], n0[1], n0[2], Y);
        A[i] = -dot3(n1, Y);
        B[i] = -(dot3(q, Y) + dot3(n0, X));
        C[i] = dot3(n1, X);
        D[i] = dot3(q, X);
    }
    const double qa = B[1] * A[0] - A[1] * B[0];
    const double qb = ((B[1] * C[0] - A[1] * D[0]) - C[1] * B[0]) + D[1] * A[0];
    const double qc = D[1] * C[0] - C[1] * D[0];
    const double disc = qb * qb - (4.0 * qa) * qc;
    if (!(disc >= 0.0) || qa == 0.0) return;
    const double sq = sqrt(disc);
    const double s = slot == 0 ? (-qb + sq) / (2.0 * qa) : (-qb - sq) / (2.0 * qa);
    const double den = A[0] * s + C[0];
    if (den == 0.0) return;
    const double t = -(B[0] * s + D[0]) / den;
    const double a[3] = {p0[0] + s * n0[0], p0[1] + s * n0[1], p0[2] + s * n0[2]};
    const double b[3] = {p1[0] + t * n1[0], p1[1] + t * n1[1], p1[2] + t * n1[2]};
    const double Dv[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]};
    const double ln = sqrt(dot3(Dv, Dv));
    if (!(ln > 0.0)) return;
    const double axis[6] = {a[0], a[1], a[2], Dv[0] / ln, Dv[1] / ln, Dv[2] / ln};
    const double* d = axis + 3;
    double h[3], rho[3];
    for (int k = 0; k < 3; ++k) {
        const double e[3] = {p[k][0] - a[0], p[k][1] - a[1], p[k][2] - a[2]};
        h[k] = dot3(e, d);
        rho[k] = sqrt(Residual<kLine3D>::squared(p[k], axis));
    }
    const double a10 = h[1] - h[0], a11 = rho[1] - rho[0], a20 = h[2] - h[0], a21 = rho[2] - rho[0];
    const double g1 = 0.5 * (a10 * a10 + a11 * a11), g2 = 0.5 * (a20 * a20 + a21 * a21);
    const double det = a10 * a21 - a11 * a20;
    if (det == 0.0) return;
    const double z0 = (g1 * a21 - g2 * a11) / det, z1 = (a10 * g2 - a20 * g1) / det;
    const double r = sqrt(z0 * z0 + z1 * z1);
    const double hc = h[0] + z0, R = rho[0] + z1;
    const double c[3] = {a[0] + hc * d[0], a[1] + hc * d[1], a[2] + hc * d[2]};
    if (!(isfinite(c[0]) && isfinite(c[1]) && isfinite(c[2]) && isfinite(d[0]) && isfinite(d[1]) && isfinite(d[2]) && isfinite(R) && isfinite(r) &&
          R > r && r >= rmin && r <= rmax && R >= Rmin && R <= Rmax))
        return;
    m[0] = c[0]; m[1] = c[1]; m[2] = c[2];
    m[3] = d[0]; m[4] = d[1]; m[5] = d[2];
    m[6] = R; m[7] = r;
}

// The shell: samples[S][sample] -> (slots S) x P models, rows slots * s + j, one lane per padded model.  An index outside 0 .. n-1 gives
// a NaN model.  normals may be null for every type whose solver does not read them.  A solver with more than one slot takes the slot
// and the major radius range as well (the torus).
template <int MT>
__global__ __launch_bounds__(kSolveBlock) void solve_kernel(const double* __restrict__ pts, const double* __restrict__ normals, int64_t n,
                                                            const int* __restrict__ samples, int S, double rmin, double rmax, double Rmin, double Rmax,
                                                            double* __restrict__ models, int* __restrict__ perm, int Mpad)
{
    using R = Residual<MT>;
    const int row = (int)(blockIdx.x * kSolveBlock + threadIdx.x);
    if (row < Mpad) perm[row] = row < R::slots * S ? row : 0;  // generated in the caller's order: no locality permutation
    if (row >= R::slots * S) return;
    const int s = row / R::slots;
    int ix[R::sample];
    bool inb = true;
    for (int k = 0; k < R::sample; ++k) {
        ix[k] = samples[R::sample * s + k];
        inb = inb && ix[k] >= 0 && ix[k] < n;
    }
    double m[R::P];
    for (int k = 0; k < R::P; ++k) m[k] = __builtin_nan("");
    if (inb) {
        const double *p[R::sample], *nq[R::sample];
        for (int k = 0; k < R::sample; ++k) {
            p[k] = pts + (int64_t)ix[k] * R::D;
            nq[k] = normals ? normals + (int64_t)ix[k] * 3 : nullptr;
        }
        if constexpr (R::slots == 1) solve_minimal(Type<MT>{}, p, nq, rmin, rmax, m);
        else solve_minimal(Type<MT>{}, p, nq, rmin, rmax, Rmin, Rmax, row % R::slots, m);
    }
    for (int k = 0; k < R::P; ++k) models[(int64_t)row * R::P + k] = m[k];
}

// ---- mixed primitives: four hypotheses of four classes per sample ---------------------------------------------------------------------
// One lane per sample of four oriented points (i0, i1, i2, i3); its four slots are rows 4 s + j of the batch, each (class, q[8]):
//   slot 0  class 6   the plane of points 0, 1, 2                          solve_minimal(Type<kPlane3D>)
//   slot 1  class 8   the sphere of points 0 .. 3                          solve_minimal(Type<kSphere3D>), radii in [rmin, rmax]
//   slot 2  class 14  the cylinder of points 0, 1 and their normals        solve_minimal(Type<kCylinder3D>), radii in [rmin, rmax]
//   slot 3  class 16  the cone of points 0, 1, 2 and their normals         solve_minimal(Type<kCone3D>), sines in [smin, smax]
// Each slot is the constituent's own device function on the sample's prefix - the same code, so the same bits as that type's solver on
// the same indices - written behind its class number, the rest of the row zeros.  A slot whose solver leaves its model all NaN, whose
// class is switched off (bit j of `mask`, pgx_set_primitive_classes) or whose PREFIX - the indices its solver reads - has an index
// outside 0 .. n-1 is an all-NaN row, class included: an index behind a slot's prefix does not concern that slot, as under its own type.
__global__ __launch_bounds__(64) void solve_primitive_kernel(const double* __restrict__ pts, const double* __restrict__ normals, int64_t n,
                                                             const int* __restrict__ samples, int S, int mask, double rmin, double rmax,
                                                             double smin, double smax, double* __restrict__ models, int* __restrict__ perm,
                                                             int Mpad)
{
    using R = Residual<kPrimitive3D>;
    const int s = (int)(blockIdx.x * 64 + threadIdx.x);
    for (int t = s; t < Mpad; t += (int)(gridDim.x * 64)) perm[t] = t < 4 * S ? t : 0;
    if (s >= S) return;
    const double nan = __builtin_nan("");
    const double *p[4], *nq[4];
    int inb = 0;   // the leading indices that are inside the point set
    for (int k = 0; k < 4; ++k) {
        const int i = samples[4 * s + k];
        const bool in = i >= 0 && i < n;
        if (in && inb == k) inb = k + 1;
        p[k] = pts + (int64_t)(in ? i : 0) * 3;
        nq[k] = normals + (int64_t)(in ? i : 0) * 3;
    }
    double* out = models + (int64_t)s * 4 * R::P;
    auto slot = [&](int j, auto type) {
        constexpr int MT = decltype(type)::value;
        double q[Residual<MT>::P];
        for (int k = 0; k < Residual<MT>::P; ++k) q[k] = nan;
        if (inb >= Residual<MT>::sample && ((mask >> j) & 1)) solve_minimal(type, p, nq, MT == kCone3D ? smin : rmin, MT == kCone3D ? smax : rmax, q);
        bool have = false;   // any entry set: the row is the constituent's as it stands (a plane of overflowing points may hold a NaN)
        for (int k = 0; k < Residual<MT>::P; ++k) have = have || q[k] == q[k];
        double* row = out + j * R::P;
        row[0] = have ? (double)MT : nan;
        for (int k = 0; k < R::P - 1; ++k) row[1 + k] = !have ? nan : k < Residual<MT>::P ? q[k] : 0.0;
    };
    slot(0, Type<kPlane3D>{});
    slot(1, Type<kSphere3D>{});
    slot(2, Type<kCylinder3D>{});
    slot(3, Type<kCone3D>{});
}

// ---- oriented mixed primitives: Schnabel's candidate test behind the mixed-primitive solver -------------------------------------------
// Type 20's slots are solve_primitive_kernel's, on the same indices with the same bits.  This pass then takes out every slot whose model
// does not agree with the normals of its OWN sample: a slot is kept iff each point of its prefix (3 plane, 4 sphere, 2 cylinder, 3 cone)
// is compatible with it at kappa - Residual<kOrientedPrimitive3D>'s test, the distance left out (the sample lies on its model up to
// rounding).  Any other slot becomes an all-NaN row, class included: such a hypothesis could never count its own sample, and as a NaN
// row it dies in the cull.  The plane of three points whose normals lie in it is the typical case.  One lane per slot; a slot that is
// an all-NaN row already (no model, class off, index outside the points) is left alone, so every index read here is inside the points.
__global__ __launch_bounds__(64) void oriented_slots_kernel(const double* __restrict__ pts, const double* __restrict__ normals, const int* __restrict__ samples,
                                                            int S, double kappa, double* __restrict__ models)
{
    using R = Residual<kOrientedPrimitive3D>;
    const int t = (int)(blockIdx.x * 64 + threadIdx.x);
    if (t >= 4 * S) return;
    double* row = models + (int64_t)t * R::P;
    double m[R::P];
    for (int k = 0; k < R::P; ++k) m[k] = row[k];
    if (m[0] != m[0]) return;
    const int j = t & 3;
    const int prefix = j == 0 ? Residual<kPlane3D>::sample : j == 1 ? Residual<kSphere3D>::sample : j == 2 ? Residual<kCylinder3D>::sample : Residual<kCone3D>::sample;
    bool ok = true;
    for (int k = 0; k < prefix; ++k) {
        const int64_t i = samples[4 * (t >> 2) + k];
        const double p[3] = {pts[i * 3], pts[i * 3 + 1], pts[i * 3 + 2]};
        const double nq[3] = {normals[i * 3], normals[i * 3 + 1], normals[i * 3 + 2]};
        double g[3];
        ok = ok && R::surface_normal(p, m, g) && R::agrees(nq, g, kappa);
    }
    if (!ok)
        for (int k = 0; k < R::P; ++k) row[k] = __builtin_nan("");
}

// ---- P3P -------------------------------------------------------------------------------------------------------------
/* monic cubic x^3 + a x^2 + b x + c: one real root by 200 bisection steps inside the Cauchy bound, the other two from the
 * quadratic factor (NaN when complex).  Only + - * / sqrt. */
__device__ void cubic_roots(double a, double b, double c, double *r)
{
    r[0] = r[1] = r[2] = __builtin_nan("");
    double lo = -(1.0 + fmax(fabs(a), fmax(fabs(b), fabs(c)))), hi = -lo;
    for (int it = 0; it < 200; ++it) {
        const double mid = 0.5 * (lo + hi);
        // once the midpoint rounds onto an end point this update either changes nothing or collapses the interval onto it; either
        // way every later step reproduces the state: stopping after it gives the bits of all 200 steps (~60 are needed)
        const bool last = mid == lo || mid == hi;
        const double pv = ((mid + a) * mid + b) * mid + c;
        if (pv < 0.0) lo = mid; else hi = mid;
        if (last) break;
    }
    const double l0 = 0.5 * (lo + hi);
    r[0] = l0;
    const double qb = a + l0, qc = b + qb * l0;
    const double disc = qb * qb - 4.0 * qc;
    if (disc >= 0.0) {
        const double sq = sqrt(disc);
        r[1] = (-qb - sq) / 2.0;
        r[2] = (-qb + sq) / 2.0;
    }
}

__device__ double quartic_eval(const double *m, double x) { return (((x + m[3]) * x + m[2]) * x + m[1]) * x + m[0]; }

__device__ __forceinline__ bool p3p_change(double a, double b) { return (a < 0.0 && b >= 0.0) || (a >= 0.0 && b < 0.0); }

/* the gates of one (u, v) at s1: positive finite depths and the two unused side constraints to 1e-6.  Returns 1 and writes the
 * depths and |e2|, or 0. */
__device__ int p3p_gate(double u, double v, double s1, double cg, double ca, double c2, double a2, double *dep, double *e2abs)
{
    const double s2 = u * s1, s3 = v * s1;
    if (!(s1 > 0.0) || !(s2 > 0.0) || !(s3 > 0.0) || !(s1 < 1e300) || !(s2 < 1e300) || !(s3 < 1e300)) return 0;
    const double e1 = s1 * s1 + s2 * s2 - 2.0 * s1 * s2 * cg - c2;
    const double e2 = s2 * s2 + s3 * s3 - 2.0 * s2 * s3 * ca - a2;
    if (!(fabs(e1) < 1e-6 * c2) || !(fabs(e2) < 1e-6 * a2)) return 0;
    dep[0] = s1; dep[1] = s2; dep[2] = s3;
    *e2abs = fabs(e2);
    return 1;
}

/* the pose of one depth triple: camera-frame points and the two orthonormal frames, R = EY^T EX, t = Y0 - R X0.  Returns 1 and
 * writes P (12, [R|t] row-major); 0 and P = NaN on a degenerate frame or a non-finite entry. */
__device__ int p3p_pose(double f[3][3], double X[3][3], const double *dep, double *P)
{
    double Y[3][3];
    for (int r = 0; r < 3; ++r) for (int k = 0; k < 3; ++k) Y[r][k] = f[r][k] * dep[r];
    double EX[3][3], EY[3][3];
    for (int w = 0; w < 2; ++w) {
        double (*Q)[3] = w == 0 ? X : Y;
        double (*E)[3] = w == 0 ? EX : EY;
        double p1[3], p2[3];
        for (int k = 0; k < 3; ++k) { p1[k] = Q[1][k] - Q[0][k]; p2[k] = Q[2][k] - Q[0][k]; }
        const double n1 = sqrt(p1[0] * p1[0] + p1[1] * p1[1] + p1[2] * p1[2]);
        if (!(n1 > 0.0)) return 0;
        for (int k = 0; k < 3; ++k) E[0][k] = p1[k] / n1;
        double cr[3] = {E[0][1] * p2[2] - E[0][2] * p2[1], E[0][2] * p2[0] - E[0][0] * p2[2], E[0][0] * p2[1] - E[0][1] * p2[0]};
        const double n3 = sqrt(cr[0] * cr[0] + cr[1] * cr[1] + cr[2] * cr[2]);
        if (!(n3 > 0.0)) return 0;
        for (int k = 0; k < 3; ++k) E[2][k] = cr[k] / n3;
        E[1][0] = E[2][1] * E[0][2] - E[2][2] * E[0][1];
        E[1][1] = E[2][2] * E[0][0] - E[2][0] * E[0][2];
        E[1][2] = E[2][0] * E[0][1] - E[2][1] * E[0][0];
    }
    double R[3][3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) R[i][j] = EY[0][i] * EX[0][j] + EY[1][i] * EX[1][j] + EY[2][i] * EX[2][j];
    int fin = 1;
    for (int i = 0; i < 3; ++i) {
        const double t = Y[0][i] - (R[i][0] * X[0][0] + R[i][1] * X[0][1] + R[i][2] * X[0][2]);
        if (!(fabs(t) < 1e300)) fin = 0;
        for (int j = 0; j < 3; ++j) { if (!(fabs(R[i][j]) < 1e300)) fin = 0; P[4 * i + j] = R[i][j]; }
        P[4 * i + 3] = t;
    }
    if (!fin) for (int k = 0; k < 12; ++k) P[k] = __builtin_nan("");
    return fin;
}

/* P3P (Grunert's quartic in v = s3/s1 as in Fischler-Bolles; DefaultPnPEstimator's minimal solver is absent upstream):
 * rows (u, v, X, Y, Z) in normalised image coordinates; positive real roots of the quartic by bisection between the
 * critical points (roots of the derivative cubic) inside (0, Cauchy bound), and a critical point itself where the quartic
 * vanishes to its evaluation error without a sign change on either side (a double root); u = s2/s1 from the linear combination
 * of the constraints, or - where that fails its gates, as it does when two poses share v (0 / 0) - from the quadratic
 * u^2 - 2 cg u + 1 - c2 / s1^2 = 0: at a simple root the u with the smaller |e2|, at a double root both; gates: positive depths,
 * the two unused side constraints to 1e-6; pose from the orthonormal frames of the two congruent triangles.
 * out = 4 slots x 12 ([R|t] row-major) in ascending v, NaN = no solution. */
__device__ void solve_p3p(const double *pts, int64_t n, const int32_t *smp, double *out)
{
    for (int k = 0; k < 48; ++k) out[k] = __builtin_nan("");
    double f[3][3], X[3][3];
    for (int r = 0; r < 3; ++r) {
        const int32_t i = smp[r];
        if (i < 0 || i >= n) return;
        const double u = pts[(int64_t)i * 5], v = pts[(int64_t)i * 5 + 1];
        const double ln = sqrt(u * u + v * v + 1.0);
        f[r][0] = u / ln; f[r][1] = v / ln; f[r][2] = 1.0 / ln;
        X[r][0] = pts[(int64_t)i * 5 + 2]; X[r][1] = pts[(int64_t)i * 5 + 3]; X[r][2] = pts[(int64_t)i * 5 + 4];
    }
    double d12[3], d02[3], d01[3];
    for (int k = 0; k < 3; ++k) { d12[k] = X[1][k] - X[2][k]; d02[k] = X[0][k] - X[2][k]; d01[k] = X[0][k] - X[1][k]; }
    const double a2 = d12[0] * d12[0] + d12[1] * d12[1] + d12[2] * d12[2];
    const double b2 = d02[0] * d02[0] + d02[1] * d02[1] + d02[2] * d02[2];
    const double c2 = d01[0] * d01[0] + d01[1] * d01[1] + d01[2] * d01[2];
    if (!(a2 > 0.0) || !(b2 > 0.0) || !(c2 > 0.0)) return;
    const double ca = f[1][0] * f[2][0] + f[1][1] * f[2][1] + f[1][2] * f[2][2];
    const double cb = f[0][0] * f[2][0] + f[0][1] * f[2][1] + f[0][2] * f[2][2];
    const double cg = f[0][0] * f[1][0] + f[0][1] * f[1][1] + f[0][2] * f[1][2];
    const double q = (a2 - c2) / b2, rr = (a2 + c2) / b2;
    const double A4 = (q - 1.0) * (q - 1.0) - 4.0 * c2 / b2 * ca * ca;
    const double A3 = 4.0 * (q * (1.0 - q) * cb - (1.0 - rr) * ca * cg + 2.0 * c2 / b2 * ca * ca * cb);
    const double A2 = 2.0 * (q * q - 1.0 + 2.0 * q * q * cb * cb + 2.0 * (b2 - c2) / b2 * ca * ca - 4.0 * rr * ca * cb * cg +
                             2.0 * (b2 - a2) / b2 * cg * cg);
    const double A1 = 4.0 * (-q * (1.0 + q) * cb + 2.0 * a2 / b2 * cg * cg * cb - (1.0 - rr) * ca * cg);
    const double A0 = (1.0 + q) * (1.0 + q) - 4.0 * a2 / b2 * cg * cg;
    if (!(fabs(A4) > 1e-14) || !(fabs(A4) < 1e300)) return;
    double m[4] = {A0 / A4, A1 / A4, A2 / A4, A3 / A4};  /* monic: x^4 + m3 x^3 + m2 x^2 + m1 x + m0 */
    for (int k = 0; k < 4; ++k) if (!(fabs(m[k]) < 1e300)) return;
    const double B = 1.0 + fmax(fmax(fabs(m[0]), fabs(m[1])), fmax(fabs(m[2]), fabs(m[3])));
    double crit[3];
    cubic_roots(0.75 * m[3], 0.5 * m[2], 0.25 * m[1], crit);
    /* break points of (0, B): the positive critical points in ascending order */
    double bp[5];
    int nb = 0;
    bp[nb++] = 0.0;
    for (int pass = 0; pass < 3; ++pass) {          /* selection in ascending order (at most three values) */
        double best = B;
        for (int k = 0; k < 3; ++k)
            if (crit[k] == crit[k] && crit[k] > bp[nb - 1] && crit[k] < best) best = crit[k];
        if (best < B) bp[nb++] = best; else break;
    }
    bp[nb++] = B;
    int slot = 0;
    /* candidates in ascending order: even c = the interval (bp[c/2], bp[c/2 + 1]), odd c = the critical point between two intervals */
    for (int c = 0; c <= 2 * (nb - 2) && slot < 4; ++c) {
        const int s = c >> 1, dbl = c & 1;
        double v;
        if (!dbl) {
            double lo = bp[s], hi = bp[s + 1];
            const double plo = quartic_eval(m, lo), phi = quartic_eval(m, hi);
            if (!p3p_change(plo, phi)) continue;
            const int rising = plo < 0.0;
            for (int it = 0; it < 200; ++it) {
                const double mid = 0.5 * (lo + hi);
                const bool last = mid == lo || mid == hi;   // (see cubic_roots: the state is a fixed point after this update)
                const double pv = quartic_eval(m, mid);
                if ((pv < 0.0) == rising) lo = mid; else hi = mid;
                if (last) break;
            }
            v = 0.5 * (lo + hi);
        } else {
            /* a double root has no sign change on either side: the critical point counts as a root where |p| is within the
             * evaluation error of Horner's rule there, 16 eps (((v + |m3|) v + |m2|) v + |m1|) v + |m0|) */
            v = bp[s + 1];
            const double pl = quartic_eval(m, bp[s]), pv = quartic_eval(m, v), pr = quartic_eval(m, bp[s + 2]);
            if (p3p_change(pl, pv) || p3p_change(pv, pr)) continue;
            const double bound = 0x1p-48 * ((((v + fabs(m[3])) * v + fabs(m[2])) * v + fabs(m[1])) * v + fabs(m[0]));
            if (!(fabs(pv) <= bound)) continue;
        }
        if (!(v > 0.0)) continue;
        const double s1 = sqrt(b2 / (1.0 + v * v - 2.0 * v * cb));
        double da[3], db[3], ea = 0.0, eb = 0.0;
        int oka = 0, okb = 0;
        if (!dbl) {     /* u from the linear combination of the constraints (0 / 0 where two poses share v) */
            const double den = 2.0 * (cg - v * ca);
            const double u = ((-1.0 + q) * v * v - 2.0 * q * cb * v + 1.0 + q) / den;
            oka = p3p_gate(u, v, s1, cg, ca, c2, a2, da, &ea);
        }
        if (!oka) {     /* the second way: u^2 - 2 cg u + 1 - c2 / s1^2 = 0 (the first side constraint over s1^2), both roots through the gates */
            const double disc = cg * cg - 1.0 + c2 / (s1 * s1);
            if (disc >= 0.0) {
                const double sq = sqrt(disc);
                oka = p3p_gate(cg - sq, v, s1, cg, ca, c2, a2, da, &ea);
                okb = sq > 0.0 && p3p_gate(cg + sq, v, s1, cg, ca, c2, a2, db, &eb);
                if (!dbl && oka && okb) {   /* a simple root carries one pose: the u with the smaller |e2| */
                    if (eb < ea) oka = 0; else okb = 0;
                }
            }
        }
        if (oka && slot < 4) slot += p3p_pose(f, X, da, out + 12 * slot);
        if (okb && slot < 4) slot += p3p_pose(f, X, db, out + 12 * slot);
    }
}

__global__ __launch_bounds__(64) void solve_p3p_kernel(const double* __restrict__ pts, int64_t n, const int* __restrict__ samples,
                                                       int S, double* __restrict__ models, int* __restrict__ perm, int Mpad)
{
    const int s = (int)(blockIdx.x * 64 + threadIdx.x);
    for (int t = s; t < Mpad; t += (int)(gridDim.x * 64)) perm[t] = t < 4 * S ? t : 0;
    if (s >= S) return;
    solve_p3p(pts, n, samples + (int64_t)s * 3, models + (int64_t)s * 48);
}

// ---- 4-point homography -----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void solve_h4_kernel(const double* __restrict__ pts, int64_t n, const int* __restrict__ samples,
                                                      int S, double scale, double* __restrict__ models, int* __restrict__ perm,
                                                      int Mpad)
{
    const int s = (int)(blockIdx.x * 64 + threadIdx.x);
    for (int t = s; t < Mpad; t += (int)(gridDim.x * 64)) perm[t] = t < S ? t : 0;
    if (s >= S) return;
    const double nan = __builtin_nan("");
    double* out = models + (int64_t)s * 9;
    for (int k = 0; k < 9; ++k) out[k] = nan;
    double M[8][9];  // rows 0..3: x-equations of the four points, rows 4..7: y-equations; column 8 = right-hand side
    for (int r = 0; r < 4; ++r) {
        const int i = samples[4 * s + r];
        if (i < 0 || i >= n) return;
        const double x1 = pts[(int64_t)i * 4] / scale, y1 = pts[(int64_t)i * 4 + 1] / scale;
        const double x2 = pts[(int64_t)i * 4 + 2] / scale, y2 = pts[(int64_t)i * 4 + 3] / scale;
        double* a = M[r];
        double* b = M[r + 4];
        a[0] = -x1; a[1] = -y1; a[2] = -1.0; a[3] = 0.0; a[4] = 0.0; a[5] = 0.0; a[6] = x2 * x1; a[7] = x2 * y1; a[8] = -x2;
        b[0] = 0.0; b[1] = 0.0; b[2] = 0.0; b[3] = -x1; b[4] = -y1; b[5] = -1.0; b[6] = y2 * x1; b[7] = y2 * y1; b[8] = -y2;
    }
    for (int c = 0; c < 8; ++c) {
        int pr = c;
        double best = fabs(M[c][c]);
        for (int i = c + 1; i < 8; ++i) { const double a = fabs(M[i][c]); if (a > best) { best = a; pr = i; } }
        if (!(best >= 1e-12)) return;  // degenerate sample (three collinear points, repeated point) or NaN
        if (pr != c) for (int j = c; j < 9; ++j) { const double t = M[c][j]; M[c][j] = M[pr][j]; M[pr][j] = t; }
        for (int i = c + 1; i < 8; ++i) {
            const double f = M[i][c] / M[c][c];
            for (int j = c; j < 9; ++j) M[i][j] = M[i][j] - f * M[c][j];
        }
    }
    double h[9];
    for (int c = 7; c >= 0; --c) {
        double acc = M[c][8];
        for (int j = c + 1; j < 8; ++j) acc = acc - M[c][j] * h[j];
        h[c] = acc / M[c][c];
    }
    h[8] = 1.0;
    h[2] = h[2] * scale; h[5] = h[5] * scale; h[6] = h[6] / scale; h[7] = h[7] / scale;  // H = S^-1 Hn S, S = diag(1/s, 1/s, 1)
    for (int k = 0; k < 9; ++k) if (!(fabs(h[k]) < 1e300)) return;
    for (int k = 0; k < 9; ++k) out[k] = h[k];
}

// ---- 7-point fundamental matrix -------------------------------------------------------------------------------------
__device__ __forceinline__ double det3(const double* a)
{
    return a[0] * (a[4] * a[8] - a[5] * a[7]) - a[1] * (a[3] * a[8] - a[5] * a[6]) + a[2] * (a[3] * a[7] - a[4] * a[6]);
}

__global__ __launch_bounds__(64) void solve_f7_kernel(const double* __restrict__ pts, int64_t n, const int* __restrict__ samples,
                                                      int S, double scale, double* __restrict__ models, int* __restrict__ perm,
                                                      int Mpad)
{
    const int s = (int)(blockIdx.x * 64 + threadIdx.x);
    for (int t = s; t < Mpad; t += (int)(gridDim.x * 64)) perm[t] = t < 3 * S ? t : 0;
    if (s >= S) return;
    const double nan = __builtin_nan("");
    double* out = models + (int64_t)s * 27;
    for (int k = 0; k < 27; ++k) out[k] = nan;
    double M[7][9];
    for (int r = 0; r < 7; ++r) {
        const int i = samples[7 * s + r];
        if (i < 0 || i >= n) return;
        const double x1 = pts[(int64_t)i * 4] / scale, y1 = pts[(int64_t)i * 4 + 1] / scale;
        const double x2 = pts[(int64_t)i * 4 + 2] / scale, y2 = pts[(int64_t)i * 4 + 3] / scale;
        M[r][0] = x2 * x1; M[r][1] = x2 * y1; M[r][2] = x2;
        M[r][3] = y2 * x1; M[r][4] = y2 * y1; M[r][5] = y2;
        M[r][6] = x1; M[r][7] = y1; M[r][8] = 1.0;
    }
    int col[9];
    for (int j = 0; j < 9; ++j) col[j] = j;
    for (int r = 0; r < 7; ++r) {  // Gauss-Jordan with full pivoting (first maximum in row-major order)
        int pr = r, pc = r;
        double best = -1.0;
        for (int i = r; i < 7; ++i)
            for (int j = r; j < 9; ++j) {
                const double a = fabs(M[i][j]);
                if (a > best) { best = a; pr = i; pc = j; }
            }
        if (!(best >= 1e-12)) return;  // rank deficient sample (or NaN)
        if (pr != r) for (int j = 0; j < 9; ++j) { const double t = M[r][j]; M[r][j] = M[pr][j]; M[pr][j] = t; }
        if (pc != r) {
            for (int i = 0; i < 7; ++i) { const double t = M[i][r]; M[i][r] = M[i][pc]; M[i][pc] = t; }
            const int t = col[r]; col[r] = col[pc]; col[pc] = t;
        }
        const double piv = M[r][r];
        for (int j = r; j < 9; ++j) M[r][j] = M[r][j] / piv;
        for (int i = 0; i < 7; ++i) {
            if (i == r) continue;
            const double f = M[i][r];
            for (int j = r; j < 9; ++j) M[i][j] = M[i][j] - f * M[r][j];
        }
    }
    double F1[9], F2[9];  // null vectors: free variable col[7] (resp. col[8]) = 1
    for (int k = 0; k < 7; ++k) { F1[col[k]] = -M[k][7]; F2[col[k]] = -M[k][8]; }
    F1[col[7]] = 1.0; F1[col[8]] = 0.0;
    F2[col[7]] = 0.0; F2[col[8]] = 1.0;
    // det(F2 + l D), D = F1 - F2:  c3 l^3 + c2 l^2 + c1 l + c0
    double D[9], T[9];
    for (int k = 0; k < 9; ++k) D[k] = F1[k] - F2[k];
    const double c0 = det3(F2), c3 = det3(D);
    double c1 = 0.0, c2 = 0.0;
    for (int r = 0; r < 3; ++r) {
        for (int k = 0; k < 9; ++k) T[k] = F2[k];
        for (int k = 0; k < 3; ++k) T[3 * r + k] = D[3 * r + k];
        c1 = c1 + det3(T);
        for (int k = 0; k < 9; ++k) T[k] = D[k];
        for (int k = 0; k < 3; ++k) T[3 * r + k] = F2[3 * r + k];
        c2 = c2 + det3(T);
    }
    double roots[3] = {nan, nan, nan};
    const double cm = fmax(fmax(fabs(c0), fabs(c1)), fmax(fabs(c2), fabs(c3)));
    // c3 = det(F1 - F2) vanishes: F1 - F2 itself is singular, the root at infinity of this chart (slot qinf, after the finite ones)
    int qinf = -1;
    if (!(cm > 0.0) || !(cm < 1e300)) return;
    if (fabs(c3) > 1e-14 * cm) {
        const double a = c2 / c3, b = c1 / c3, c = c0 / c3;
        double lo = -(1.0 + fmax(fabs(a), fmax(fabs(b), fabs(c)))), hi = -lo;  // Cauchy bound: p(lo) < 0 < p(hi)
        for (int it = 0; it < 200; ++it) {
            const double mid = 0.5 * (lo + hi);
            const bool last = mid == lo || mid == hi;   // (see cubic_roots: the state is a fixed point after this update)
            const double pv = ((mid + a) * mid + b) * mid + c;
            if (pv < 0.0) lo = mid; else hi = mid;
            if (last) break;
        }
        const double l0 = 0.5 * (lo + hi);
        roots[0] = l0;
        const double qb = a + l0, qc = b + qb * l0;  // p(l) = (l - l0)(l^2 + qb l + qc)
        const double disc = qb * qb - 4.0 * qc;
        if (disc >= 0.0) {
            const double sq = sqrt(disc);
            roots[1] = (-qb - sq) / 2.0;
            roots[2] = (-qb + sq) / 2.0;
        }
    } else if (fabs(c2) > 1e-14 * cm) {
        qinf = 2;
        const double disc = c1 * c1 - 4.0 * c2 * c0;
        if (disc >= 0.0) {
            const double sq = sqrt(disc);
            roots[0] = (-c1 - sq) / (2.0 * c2);
            roots[1] = (-c1 + sq) / (2.0 * c2);
        }
    } else if (fabs(c1) > 1e-14 * cm) {
        qinf = 1;
        roots[0] = -c0 / c1;
    } else {
        qinf = 0;
    }
    const double s1 = scale, s2 = scale * scale;
    for (int q = 0; q < 3; ++q) {
        const double l = roots[q];
        if (q != qinf && !(l == l)) continue;
        double F[9];
        for (int k = 0; k < 9; ++k) F[k] = q == qinf ? D[k] : l * F1[k] + (1.0 - l) * F2[k];
        // undo the isotropic scaling: F <- diag(1/s, 1/s, 1) F diag(1/s, 1/s, 1)
        F[0] = F[0] / s2; F[1] = F[1] / s2; F[2] = F[2] / s1;
        F[3] = F[3] / s2; F[4] = F[4] / s2; F[5] = F[5] / s1;
        F[6] = F[6] / s1; F[7] = F[7] / s1;
        double nn = 0.0;
        for (int k = 0; k < 9; ++k) nn = nn + F[k] * F[k];
        const double nrm = sqrt(nn);
        if (!(nrm > 0.0) || !(nrm < 1e300)) continue;
        for (int k = 0; k < 9; ++k) out[9 * q + k] = F[k] / nrm;
    }
}

}  // namespace

// The sample indices go through a pinned staging buffer owned by the context: the caller's array is consumed before the
// call returns, so a launch that hands nothing back (models_out == NULL: the batch stays resident for pgx_score_launch) needs
// no synchronisation at all - the host goes straight on to enqueue the scoring kernels behind the solver.  An event guards
// the staging buffer against the next call.
static int upload_samples(pgx_ctx* ctx, const int32_t* samples, size_t bytes)
{
    PGX_TRY(ctx->h_samples.acquire(ctx, bytes));
    std::memcpy(ctx->h_samples.buf.p, samples, bytes);
    PGX_TRY(ensure(ctx, ctx->scratch, bytes));
    PGX_HIP(ctx, hipMemcpyAsync(ctx->scratch.p, ctx->h_samples.buf.p, bytes, hipMemcpyHostToDevice, ctx->stream));
    return ctx->h_samples.submitted(ctx, ctx->stream);
}

// ---- samples drawn on the device (rng.hip.h): one lane per sample, straight into the buffer the solvers read -----------------
__global__ __launch_bounds__(256) void sample_uniform_kernel(unsigned long long key, unsigned batch, int S, int64_t n, int m, int* __restrict__ samples)
{
    const int s = (int)(blockIdx.x * 256 + threadIdx.x);
    if (s >= S) return;
    int32_t row[kMaxSampleSize];
    sample_distinct(key, batch, (uint64_t)s, n, m, row);
    for (int j = 0; j < m; ++j) samples[(int64_t)s * m + j] = row[j];
}

__global__ __launch_bounds__(256) void sample_napsac_kernel(unsigned long long key, unsigned batch, int S, int64_t n, const int* __restrict__ off,
                                                            const int* __restrict__ idx, int m, int* __restrict__ samples)
{
    const int s = (int)(blockIdx.x * 256 + threadIdx.x);
    if (s >= S) return;
    int32_t row[kMaxSampleSize];
    sample_napsac(key, batch, (uint64_t)s, n, off, idx, m, row);
    for (int j = 0; j < m; ++j) samples[(int64_t)s * m + j] = row[j];
}

__global__ __launch_bounds__(256) void sample_prosac_kernel(unsigned long long key, unsigned batch, int S, int64_t n, const int* __restrict__ tops, int m,
                                                            int* __restrict__ samples)
{
    const int s = (int)(blockIdx.x * 256 + threadIdx.x);
    if (s >= S) return;
    int32_t row[kMaxSampleSize];
    sample_prosac(key, batch, (uint64_t)s, n, tops[s], m, row);
    for (int j = 0; j < m; ++j) samples[(int64_t)s * m + j] = row[j];
}

// pgx_sampler_prosac_set: the subset size n_k of PROSAC's sample number k = 1 .. count (0 = uniform over all points)
int sampler_prosac_set(pgx_ctx* ctx, const int32_t* tops, int count)
{
    if (ctx->n <= 0) return fail(ctx, PGX_ERR_INVALID, "pgx_sampler_prosac_set: points not set");
    if (!tops || count <= 0) return fail(ctx, PGX_ERR_INVALID, "pgx_sampler_prosac_set: empty table");
    for (int k = 0; k < count; ++k)
        if (tops[k] < 0 || tops[k] > ctx->n)
            return fail(ctx, PGX_ERR_INVALID, "pgx_sampler_prosac_set: subset size %d of sample %d is outside 0 .. %lld", tops[k], k + 1, (long long)ctx->n);
    PGX_TRY(ensure(ctx, ctx->prosac_tops, (size_t)count * sizeof(int32_t)));
    PGX_HIP(ctx, hipMemcpyAsync(ctx->prosac_tops.p, tops, (size_t)count * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    PGX_HIP(ctx, hipStreamSynchronize(ctx->stream));   // (the caller's buffer is free on return)
    ctx->prosac_count = count;
    ctx->prosac_points_version = ctx->expansion.points_version;
    return PGX_OK;
}

int solve_minimal_launch(pgx_ctx* ctx, const int32_t* samples, int S, double* models_out, bool resident)
{
    if (ctx->n <= 0 || ctx->model_type < 0) return fail(ctx, PGX_ERR_INVALID, "pgx_solve_minimal: points not set");
    if ((!samples && !resident) || S <= 0) return fail(ctx, PGX_ERR_INVALID, "pgx_solve_minimal: empty sample batch");
    const int mt = ctx->model_type;
    ModelInfo mi;
    if (!model_info(mt, &mi) || mi.slots == 0)
        return fail(ctx, PGX_ERR_INVALID, "pgx_solve_minimal: no device solver for model type %d yet (built: 2-point line, 2-segment vanishing point, 3-point plane, 4-point sphere, 3-point circle, 2-point 3-D line, 2-point cylinder, 3-point cone, 4-point mixed primitives, 4-point torus, 4-point homography, 7-point fundamental matrix, P3P)", mt);
    if (mi.normals_solver && ctx->normals_n != ctx->n)
        return fail(ctx, PGX_ERR_INVALID, "pgx_solve_minimal: the %s solver needs the resident points' normals (pgx_set_normals after pgx_set_points)", mi.normals_solver);
    // isotropic pre-scaling by the largest coordinate magnitude (pmax of set_points is 1 for these model types, so the solvers take
    // fscale, which pgx_set_points computes from the caller-visible data: umax is not kept either)
    const bool scaled = mt == kFundamental || mt == kHomography;
    if (scaled && !(ctx->fscale >= 1.0)) return fail(ctx, PGX_ERR_INVALID, "pgx_solve_minimal: coordinate scale not available");
    const int Mtot = mi.slots * S;
    const int Mpad = ((Mtot + 255) / 256) * 256;   // (255 .. 257 and the other edges of the rounding: test_score_batch_sizes_across_the_reorder_and_the_padding)
    PGX_TRY(ensure(ctx, ctx->models, (size_t)Mtot * mi.P * sizeof(double)));
    PGX_TRY(ensure(ctx, ctx->perm, (size_t)Mpad * sizeof(int)));
    if (!resident) PGX_TRY(upload_samples(ctx, samples, (size_t)S * mi.sample * sizeof(int32_t)));
    const double* pts = ctx->pts.as<double>();
    const double* normals = ctx->normals_n == ctx->n ? ctx->normals.as<double>() : nullptr;
    const int* smp = ctx->scratch.as<int>();
    double* models = ctx->models.as<double>();
    int* perm = ctx->perm.as<int>();
    const dim3 gs((unsigned)((S + 63) / 64)), bs(64);                                            // one lane per sample
    const dim3 gm((unsigned)((Mpad + kSolveBlock - 1) / kSolveBlock)), bm(kSolveBlock);      // one lane per padded model
    if (mt == kFundamental) hipLaunchKernelGGL(solve_f7_kernel, gs, bs, 0, ctx->stream, pts, ctx->n, smp, S, ctx->fscale, models, perm, Mpad);
    else if (mt == kHomography) hipLaunchKernelGGL(solve_h4_kernel, gs, bs, 0, ctx->stream, pts, ctx->n, smp, S, ctx->fscale, models, perm, Mpad);
    else if (mt == kPnP) hipLaunchKernelGGL(solve_p3p_kernel, gs, bs, 0, ctx->stream, pts, ctx->n, smp, S, models, perm, Mpad);
    else if (mt == kPrimitive3D || mt == kOrientedPrimitive3D) {
        hipLaunchKernelGGL(solve_primitive_kernel, gs, bs, 0, ctx->stream, pts, normals, ctx->n, smp, S, ctx->prim_mask, ctx->rmin, ctx->rmax, ctx->prim_smin,
                           ctx->prim_smax, models, perm, Mpad);
        if (mt == kOrientedPrimitive3D)   // the slots that disagree with their own sample's normals become all-NaN rows
            hipLaunchKernelGGL(oriented_slots_kernel, dim3((unsigned)((4 * S + 63) / 64)), bs, 0, ctx->stream, pts, normals, smp, S, ctx->normal_cos2, models);
    }
    else   // the lane-per-model solvers: whatever else declares slots has a solve_minimal, or this does not compile
        with_model_type(mt, [&](auto t) {
            constexpr int MT = decltype(t)::value;
            if constexpr (Residual<MT>::slots > 0 && MT != kFundamental && MT != kHomography && MT != kPnP && MT != kPrimitive3D && MT != kOrientedPrimitive3D)
                hipLaunchKernelGGL((solve_kernel<MT>), gm, bm, 0, ctx->stream, pts, normals, ctx->n, smp, S, ctx->rmin, ctx->rmax, ctx->major_rmin, ctx->major_rmax, models,
                                   perm, Mpad);
        });
    PGX_HIP(ctx, hipGetLastError());
    if (models_out) {
        PGX_TRY(d2h(ctx, models_out, ctx->models.p, (size_t)Mtot * mi.P * sizeof(double)));
        PGX_TRY(sync_deliver(ctx));
    }
    // Device-generated batches stay in the caller's order (the kernels above wrote the identity permutation), so an uploaded batch's
    // locality order and the mirror of its launch end HERE - for pgx_solve_minimal and pgx_solve_minimal_sampled alike, and only once
    // the call has succeeded: a refused or failed call leaves the uploaded batch resident, and its order with it.  (The sampled entry
    // point used to keep the stale order: the next mirrored fetch came back shuffled by it.  tests/test_gpu_switches.py
    // test_device_generated_batches_come_back_in_sample_order_after_a_reordered_upload)
    ctx->batch.generated(Mtot, Mpad);
    return PGX_OK;
}

// pgx_solve_minimal_sampled: S minimal samples (uniform, NAPSAC on the resident graph, or PROSAC with the resident subset-size table) from the in-repo
// generator (key, batch), drawn by the device into the solvers' sample buffer - no host RNG, no index upload - then the solver of the resident model type as in pgx_solve_minimal.
int solve_minimal_sampled_launch(pgx_ctx* ctx, int sampler, uint64_t key, uint32_t batch, int S, int32_t* samples_out, double* models_out)
{
    if (sampler < 0 || sampler > 2) return fail(ctx, PGX_ERR_INVALID, "pgx_solve_minimal_sampled: sampler %d (0 uniform, 1 NAPSAC, 2 PROSAC)", sampler);
    if (sampler == 2 && (ctx->prosac_count < S || ctx->prosac_points_version != ctx->expansion.points_version))
        return fail(ctx, PGX_ERR_INVALID, "pgx_solve_minimal_sampled: PROSAC needs pgx_sampler_prosac_set for the resident points with at least %d entries (has %d)", S,
                    ctx->prosac_points_version == ctx->expansion.points_version ? ctx->prosac_count : 0);
    if (sampler == 1 && (ctx->gn != ctx->n || ctx->gE <= 0)) return fail(ctx, PGX_ERR_INVALID, "pgx_solve_minimal_sampled: NAPSAC needs the neighbourhood graph of the resident points (pgx_graph_build / pgx_set_graph)");
    if (ctx->n <= 0 || ctx->model_type < 0) return fail(ctx, PGX_ERR_INVALID, "pgx_solve_minimal_sampled: points not set");
    if (S <= 0) return fail(ctx, PGX_ERR_INVALID, "pgx_solve_minimal_sampled: empty sample batch");
    ModelInfo mi;
    if (!model_info(ctx->model_type, &mi) || mi.slots == 0) return fail(ctx, PGX_ERR_INVALID, "pgx_solve_minimal_sampled: no device solver for model type %d", ctx->model_type);
    const int m = mi.sample;
    if (ctx->n < m) return fail(ctx, PGX_ERR_INVALID, "pgx_solve_minimal_sampled: %lld points, the minimal sample needs %d", (long long)ctx->n, m);
    PGX_TRY(ensure(ctx, ctx->scratch, (size_t)S * m * sizeof(int32_t)));
    if (sampler == 0)
        hipLaunchKernelGGL(sample_uniform_kernel, dim3((unsigned)((S + 255) / 256)), dim3(256), 0, ctx->stream, (unsigned long long)key, batch, S, ctx->n, m,
                           ctx->scratch.as<int>());
    else if (sampler == 1)
        hipLaunchKernelGGL(sample_napsac_kernel, dim3((unsigned)((S + 255) / 256)), dim3(256), 0, ctx->stream, (unsigned long long)key, batch, S, ctx->n,
                           ctx->goff.as<int>(), ctx->gidx.as<int>(), m, ctx->scratch.as<int>());
    else
        hipLaunchKernelGGL(sample_prosac_kernel, dim3((unsigned)((S + 255) / 256)), dim3(256), 0, ctx->stream, (unsigned long long)key, batch, S, ctx->n,
                           ctx->prosac_tops.as<int>(), m, ctx->scratch.as<int>());
    PGX_HIP(ctx, hipGetLastError());
    if (samples_out) {
        PGX_TRY(d2h(ctx, samples_out, ctx->scratch.p, (size_t)S * m * sizeof(int32_t)));
        PGX_TRY(sync_deliver(ctx));
    }
    return solve_minimal_launch(ctx, nullptr, S, models_out, true);
}

}  // namespace pgx
