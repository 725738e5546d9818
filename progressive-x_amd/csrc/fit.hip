// fit.hip — accumulation pass of the non-minimal refits: weighted Gram matrices of per-point
// design rows over a subset of the resident points.  The small dense solve (2x2 .. 9x9 eigen / 6x6 linear) stays on the
// host, as SURVEY a9 prescribes ("GPU does bucketing + sums, CPU does the solve").
//
// Replaces the data pass of estimator.estimateModelNonminimal(...) as called by
//   pearl::PEARL::parameterEstimation   /root/reference/src/pyprogressivex/include/PEARL.h:374-380
//   GC-RANSAC's local optimisation      (graph-cut-ransac submodule, absent from the snapshot)
// for the five estimators of progressivex_python.cpp:119,252,343,489,616.  Only the vanishing-point rows have an in-tree
// specification (solver_vanishing_point_two_lines.h:212-218: A = [y0*mz-my, mx-x0*mz, x0*my-y0*mx] * w); the other
// solvers are absent upstream and restated from the literature (normalised DLT, normalised 8-point, total least squares
// line, Gauss-Newton on the reprojection error) — DESIGN.md §3.
//
//   out = sum over selected points i of  W_i * sum over the rows a of point i of  a a^T      (upper triangle, row-major)
//   W_i = w_i^wpow (weights optional).  Selection: an uploaded index list, or label == k on the resident labelling.
// Fixed reduction tree (lanes -> waves -> per-block partials -> one final block per item): bit-reproducible run to run.
//
// Each pass is written once.  accumulate() is the per-point body of every kernel; wave_sum / wave_tree / block_tree are the only
// trees.  gram_kernel + gram_final_kernel serve pgx_gram (one item: an index list or one label) and pgx_gram_labels (blockIdx.y =
// label), so "entry k of the all-labels call is bitwise the single-label call" - the contract nonminimal_labels rests on once per
// PEARL iteration - holds because there is no second kernel.  wave_gram() is the one-wave pass of gram_batch_kernel and of every
// Gauss-Newton step of pnp_refine_batch_kernel.  On the host, check_call / check_index / gram_row_length are the argument checks
// under the caller's name, carve() lays out fit_scratch, batch_upload() is the prologue of the two one-wave-per-selection calls.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <vector>

#include "pgx_internal.h"

namespace pgx {

namespace {

constexpr int kFitBlock = 256;
// pgx_gram: the longest index list that is uploaded in one command with the zeroed counters in front of it
// (65 536 | 65 537 | 70 001: tests/test_gpu_switches.py test_gram_index_lists_either_side_of_the_fused_upload)
constexpr int64_t kFusedIndexMax = 65536;
// pgx_gram_labels: the most labels of one call (4096 | 4097: tests/test_gpu_switches.py test_gram_labels_up_to_the_label_limit)
constexpr int kMaxGramLabels = 4096;

struct FitParams {
    double v[12];
};

template <int Q>
struct Acc {
    double s[Q * (Q + 1) / 2];
    __device__ __forceinline__ void zero()
    {
#pragma unroll
        for (int k = 0; k < Q * (Q + 1) / 2; ++k) s[k] = 0.0;
    }
    __device__ __forceinline__ void add(const double (&a)[Q], double w)
    {
        int k = 0;
#pragma unroll
        for (int r = 0; r < Q; ++r) {
            const double wa = w * a[r];
#pragma unroll
            for (int c = r; c < Q; ++c) s[k++] += wa * a[c];
        }
    }
};

// row generators: Q = row length, emit(pt, prm, acc, w, bad)
struct GenDltH { static constexpr int Q = 9, D = 4; };
struct GenEpiF { static constexpr int Q = 9, D = 4; };
struct GenVp { static constexpr int Q = 3, D = 4; };
struct GenPnpGn { static constexpr int Q = 7, D = 5; };
struct GenCylGn { static constexpr int Q = 6, D = 3; };
struct GenConeGn { static constexpr int Q = 7, D = 3; };
struct GenTorusGn { static constexpr int Q = 8, D = 3; };

// the affine row (1, p[0], .., p[DIM - 1]) of a DIM-D point: lines (2), planes (3) and the 4- and 5-D rows
template <int DIM> struct GenAffine {
    static constexpr int Q = DIM + 1, D = DIM;
    static __device__ __forceinline__ void row(const double* pt, const FitParams&, double (&a)[Q])
    {
        a[0] = 1.0;
#pragma unroll
        for (int k = 0; k < DIM; ++k) a[k + 1] = pt[k];
    }
};

// the round family, prm = (o[DIM], s): the algebraic circle (DIM = 2) / sphere (3) row (1, u[DIM], u . u) of u = (p - o) / s,
// the last entry a left fold: u u + v v, (u u + v v) + w w
template <int DIM> struct GenRound {
    static constexpr int Q = DIM + 2, D = DIM;
    static __device__ __forceinline__ void row(const double* pt, const FitParams& prm, double (&a)[Q])
    {
        a[0] = 1.0;
#pragma unroll
        for (int k = 0; k < DIM; ++k) a[k + 1] = (pt[k] - prm.v[k]) / prm.v[DIM];
        double q = a[1] * a[1];
#pragma unroll
        for (int k = 1; k < DIM; ++k) q = q + a[k + 1] * a[k + 1];
        a[Q - 1] = q;
    }
};

// one row per point for the templated generators above; the others are specialisations
template <class G>
__device__ __forceinline__ void emit(const double* pt, const FitParams& prm, Acc<G::Q>& acc, double w, int&)
{
    double a[G::Q];
    G::row(pt, prm, a);
    acc.add(a, w);
}

// prm = (s1, cx1, cy1, s2, cx2, cy2): Hartley-normalised coordinates
template <>
__device__ __forceinline__ void emit<GenDltH>(const double* pt, const FitParams& prm, Acc<9>& acc, double w, int&)
{
    const double x1 = (pt[0] - prm.v[1]) * prm.v[0], y1 = (pt[1] - prm.v[2]) * prm.v[0];
    const double x2 = (pt[2] - prm.v[4]) * prm.v[3], y2 = (pt[3] - prm.v[5]) * prm.v[3];
    const double r1[9] = {-x1, -y1, -1.0, 0.0, 0.0, 0.0, x2 * x1, x2 * y1, x2};
    const double r2[9] = {0.0, 0.0, 0.0, -x1, -y1, -1.0, y2 * x1, y2 * y1, y2};
    acc.add(r1, w);
    acc.add(r2, w);
}
template <>
__device__ __forceinline__ void emit<GenEpiF>(const double* pt, const FitParams& prm, Acc<9>& acc, double w, int&)
{
    const double x1 = (pt[0] - prm.v[1]) * prm.v[0], y1 = (pt[1] - prm.v[2]) * prm.v[0];
    const double x2 = (pt[2] - prm.v[4]) * prm.v[3], y2 = (pt[3] - prm.v[5]) * prm.v[3];
    const double a[9] = {x2 * x1, x2 * y1, x2, y2 * x1, y2 * y1, y2, x1, y1, 1.0};
    acc.add(a, w);
}
// solver_vanishing_point_two_lines.h:212-217
template <>
__device__ __forceinline__ void emit<GenVp>(const double* pt, const FitParams&, Acc<3>& acc, double w, int&)
{
    const double x0 = pt[0], y0 = pt[1], x1 = pt[2], y1 = pt[3];
    const double mx = (x0 + x1) / 2.0, my = (y0 + y1) / 2.0, mz = 1.0;
    const double a[3] = {y0 * mz - my, mx - x0 * mz, x0 * my - y0 * mx};
    acc.add(a, w);
}
// prm = P = [R | t] row-major 3x4; rows (J_u, r_u), (J_v, r_v) with J = d proj / d (omega, t) at omega = 0
template <>
__device__ __forceinline__ void emit<GenPnpGn>(const double* pt, const FitParams& prm, Acc<7>& acc, double w, int& bad)
{
    const double* P = prm.v;
    const double X = pt[2], Y = pt[3], Z = pt[4];
    const double rx = P[0] * X + P[1] * Y + P[2] * Z, ry = P[4] * X + P[5] * Y + P[6] * Z, rz = P[8] * X + P[9] * Y + P[10] * Z;
    const double xc = rx + P[3], yc = ry + P[7], zc = rz + P[11];
    if (!(fabs(zc) >= 1e-12)) { bad = 1; return; }
    const double inv = 1.0 / zc;
    const double du = xc * inv - pt[0], dv = yc * inv - pt[1];
    // d proj / d Xc = [[inv, 0, -xc inv^2], [0, inv, -yc inv^2]];  d Xc / d omega = -[R X]_x, d Xc / d t = I
    const double a = inv, b = -xc * inv * inv, c = -yc * inv * inv;
    // skew(RX) as used by the host restatement: rows (0, rz, -ry), (-rz, 0, rx), (ry, -rx, 0)
    const double ju[7] = {b * ry, a * rz + b * (-rx), a * (-ry), a, 0.0, b, du};
    const double jv[7] = {a * (-rz) + c * ry, c * (-rx), a * rx, 0.0, a, c, dv};
    acc.add(ju, w);
    acc.add(jv, w);
}
// The cylinder's Gauss-Newton row.  prm = (p[3], d[3], r, u[3]): a point on the axis, the unit direction, the radius and a unit vector
// orthogonal to d; v = d x u (cross3's component order) completes the frame here.  With e = x - p, c = e x d and s = |c| exactly as
// Residual<kLine3D> computes them (so |a[5]| is Residual<kCylinder3D>::plain bit for bit), t = (e0 d0 + e1 d1) + e2 d2,
// cv = (c0 v0 + c1 v1) + c2 v2 and cu = (c0 u0 + c1 u1) + c2 u2:
//   gu = cv / s,  gv = -(cu / s),  a = (gu, gv, t gu, t gv, -1, s - r)
// the derivatives of f = s - r by (alpha, beta, gamma, eta, rho) at 0 in p + alpha u + beta v, normalise(d + gamma u + eta v),
// r + rho, followed by f: d s / d p = -(d x c) / s and d x c = e - t d is the radial vector, whose u and v components are -cv and cu;
// a tilt of d by gamma u moves the axis at height t by t gamma u.  A point on the axis (!(s > 0)) or a non-finite s has no row.
template <>
__device__ __forceinline__ void emit<GenCylGn>(const double* pt, const FitParams& prm, Acc<6>& acc, double w, int& bad)
{
    const double* m = prm.v;
    const double* u = prm.v + 7;
    const double v0 = m[4] * u[2] - m[5] * u[1], v1 = -(m[3] * u[2] - m[5] * u[0]), v2 = m[3] * u[1] - m[4] * u[0];
    const double e0 = pt[0] - m[0], e1 = pt[1] - m[1], e2 = pt[2] - m[2];
    const double c0 = e1 * m[5] - e2 * m[4];
    const double c1 = -(e0 * m[5] - e2 * m[3]);
    const double c2 = e0 * m[4] - e1 * m[3];
    const double s = sqrt((c0 * c0 + c1 * c1) + c2 * c2);
    if (!(s > 0.0) || !isfinite(s)) { bad = 1; return; }
    const double t = (e0 * m[3] + e1 * m[4]) + e2 * m[5];
    const double gu = ((c0 * v0 + c1 * v1) + c2 * v2) / s;
    const double gv = -(((c0 * u[0] + c1 * u[1]) + c2 * u[2]) / s);
    const double a[6] = {gu, gv, t * gu, t * gv, -1.0, s - m[6]};
    acc.add(a, w);
}
// The cone's Gauss-Newton row.  prm = (a[3], d[3], c, s, u[3]): the apex, the unit direction, the cosine and sine of the half-angle and
// a unit vector orthogonal to d; v = d x u (cross3's component order) completes the frame here.  With e = x - a, cr = e x d and
// rho = |cr| exactly as Residual<kLine3D> computes them and h = (e0 d0 + e1 d1) + e2 d2 (so the last entry is Residual<kCone3D>'s
// c rho - s h before its fabs, bit for bit):
//   rh_k = (e_k - h d_k) / rho,  g_k = c rh_k - s d_k,  gu = (g0 u0 + g1 u1) + g2 u2, gv and gd likewise with v and d,
//   eu = (e0 u0 + e1 u1) + e2 u2, ev likewise,  k = (c h) / rho + s,
//   row = (-gu, -gv, -gd, -(eu k), -(ev k), -(rho s + h c), c rho - s h)
// the derivatives of f = c rho - s h by (alpha, beta, gamma, delta, eta, tau) at 0 in a + alpha u + beta v + gamma d,
// normalise(d + delta u + eta v), (c, s) <- normalise(c - tau s, s + tau c), followed by f: g = c rhohat - s d is the gradient of f in x,
// so moving the apex by t moves f by -g . t; a tilt of d by delta u changes h by delta (e . u) and rho by -delta h (e . u) / rho; a
// turn of the half-angle by tau changes (c, s) by tau (-s, c).  A point on the axis (!(rho > 0)) or a non-finite rho has no row.
template <>
__device__ __forceinline__ void emit<GenConeGn>(const double* pt, const FitParams& prm, Acc<7>& acc, double w, int& bad)
{
    const double* m = prm.v;
    const double* u = prm.v + 8;
    const double c = m[6], s = m[7];
    const double v0 = m[4] * u[2] - m[5] * u[1], v1 = -(m[3] * u[2] - m[5] * u[0]), v2 = m[3] * u[1] - m[4] * u[0];
    const double e0 = pt[0] - m[0], e1 = pt[1] - m[1], e2 = pt[2] - m[2];
    const double c0 = e1 * m[5] - e2 * m[4];
    const double c1 = -(e0 * m[5] - e2 * m[3]);
    const double c2 = e0 * m[4] - e1 * m[3];
    const double rho = sqrt((c0 * c0 + c1 * c1) + c2 * c2);
    if (!(rho > 0.0) || !isfinite(rho)) { bad = 1; return; }
    const double h = (e0 * m[3] + e1 * m[4]) + e2 * m[5];
    const double g0 = c * ((e0 - h * m[3]) / rho) - s * m[3];
    const double g1 = c * ((e1 - h * m[4]) / rho) - s * m[4];
    const double g2 = c * ((e2 - h * m[5]) / rho) - s * m[5];
    const double gu = (g0 * u[0] + g1 * u[1]) + g2 * u[2];
    const double gv = (g0 * v0 + g1 * v1) + g2 * v2;
    const double gd = (g0 * m[3] + g1 * m[4]) + g2 * m[5];
    const double eu = (e0 * u[0] + e1 * u[1]) + e2 * u[2];
    const double ev = (e0 * v0 + e1 * v1) + e2 * v2;
    const double k = (c * h) / rho + s;
    const double a[7] = {-gu, -gv, -gd, -(eu * k), -(ev * k), -(rho * s + h * c), c * rho - s * h};
    acc.add(a, w);
}
// The torus' Gauss-Newton row.  prm = (c[3], d[3], R, r, u[3]): the centre, the unit direction, the major and minor radius and a unit
// vector orthogonal to d; v = d x u (cross3's component order) completes the frame here.  With e = x - c, cr = e x d, rho = |cr| and
// h = (e0 d0 + e1 d1) + e2 d2 exactly as Residual<kTorus3D> computes them, t = rho - R and w = sqrt(t t + h h) (so the last entry is
// Residual<kTorus3D>'s w - r before its fabs, bit for bit):
//   tw = t / w,  hw = h / w,  rh_k = (e_k - h d_k) / rho,  g_k = tw rh_k + hw d_k,  gu = (g0 u0 + g1 u1) + g2 u2, gv and gd likewise
//   with v and d,  eu = (e0 u0 + e1 u1) + e2 u2, ev likewise,  k = (h R) / (w rho),
//   row = (-gu, -gv, -gd, eu k, ev k, -tw, -1, w - r)
// the derivatives of f = w - r by (alpha, beta, gamma, delta, eta, dR, dr) at 0 in c + alpha u + beta v + gamma d,
// normalise(d + delta u + eta v), R + dR, r + dr, followed by f: g = (t / w) rhohat + (h / w) d is the gradient of f in x, so moving
// the centre by z moves f by -g . z; a tilt of d by delta u changes h by delta (e . u) and rho by -delta h (e . u) / rho, together
// delta (e . u)(h / w)(1 - t / rho) = delta (e . u) h R / (w rho).  A point on the axis (!(rho > 0)), a point on the spine (!(w > 0)) or
// a non-finite rho or w has no row.
template <>
__device__ __forceinline__ void emit<GenTorusGn>(const double* pt, const FitParams& prm, Acc<8>& acc, double w8, int& bad)
{
    const double* m = prm.v;
    const double* u = prm.v + 8;
    const double R = m[6], r = m[7];
    const double v0 = m[4] * u[2] - m[5] * u[1], v1 = -(m[3] * u[2] - m[5] * u[0]), v2 = m[3] * u[1] - m[4] * u[0];
    const double e0 = pt[0] - m[0], e1 = pt[1] - m[1], e2 = pt[2] - m[2];
    const double c0 = e1 * m[5] - e2 * m[4];
    const double c1 = -(e0 * m[5] - e2 * m[3]);
    const double c2 = e0 * m[4] - e1 * m[3];
    const double rho = sqrt((c0 * c0 + c1 * c1) + c2 * c2);
    if (!(rho > 0.0) || !isfinite(rho)) { bad = 1; return; }
    const double h = (e0 * m[3] + e1 * m[4]) + e2 * m[5];
    const double t = rho - R;
    const double w = sqrt(t * t + h * h);
    if (!(w > 0.0) || !isfinite(w)) { bad = 1; return; }
    const double tw = t / w, hw = h / w;
    const double g0 = tw * ((e0 - h * m[3]) / rho) + hw * m[3];
    const double g1 = tw * ((e1 - h * m[4]) / rho) + hw * m[4];
    const double g2 = tw * ((e2 - h * m[5]) / rho) + hw * m[5];
    const double gu = (g0 * u[0] + g1 * u[1]) + g2 * u[2];
    const double gv = (g0 * v0 + g1 * v1) + g2 * v2;
    const double gd = (g0 * m[3] + g1 * m[4]) + g2 * m[5];
    const double eu = (e0 * u[0] + e1 * u[1]) + e2 * u[2];
    const double ev = (e0 * v0 + e1 * v1) + e2 * v2;
    const double k = (h * R) / (w * rho);
    const double a[8] = {-gu, -gv, -gd, eu * k, ev * k, -tw, -1.0, w - r};
    acc.add(a, w8);
}

// ---- the reduction passes, each written once ---------------------------------------------------------------------------------
// The operation order below IS the contract: the bits of every Gram call are pinned (tests/test_gpu_reductions.py).

// block k of a [items][12] device table of parameter blocks
__device__ __forceinline__ FitParams load_params(const double* __restrict__ table, int64_t k)
{
    FitParams p;
#pragma unroll
    for (int j = 0; j < 12; ++j) p.v[j] = table[k * 12 + j];
    return p;
}

// the rows of resident point i under prm into acc, weighted by (*w)^wpow (w null: 1); returns 1 for a point without rows (bad)
template <class G>
__device__ __forceinline__ int accumulate(const double* __restrict__ pts, int64_t i, const double* __restrict__ w, int wpow,
                                          const FitParams& prm, Acc<G::Q>& acc)
{
    double pt[G::D];
#pragma unroll
    for (int k = 0; k < G::D; ++k) pt[k] = pts[i * G::D + k];
    double wi = 1.0;
    if (w != nullptr) { wi = *w; if (wpow == 2) wi = wi * wi; }
    int bad = 0;
    emit<G>(pt, prm, acc, wi, bad);
    return bad;
}

// the 64 lanes of a wave by shuffle, off = 32, 16, .., 1; the sum is valid in lane 0
template <class T>
__device__ __forceinline__ T wave_sum(T x)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off, 64);
    return x;
}

// the wave tree over the NV accumulators: sink(k, sum k), the sum valid in lane 0.  (Each sum goes to its consumer before the next
// tree starts: all NV trees first keep NV more values live - 182 VGPRs instead of 140 on the 9-entry rows.)
template <int NV, class F>
__device__ __forceinline__ void wave_tree(const double (&s)[NV], F&& sink)
{
#pragma unroll
    for (int k = 0; k < NV; ++k) sink(k, wave_sum(s[k]));
}

// a block of kFitBlock threads: the wave tree, lane 0 of each wave to lds [kFitBlock / 64][NV], then the waves 0..3 in order into out[NV]
template <int NV>
__device__ __forceinline__ void block_tree(const double (&s)[NV], double* __restrict__ lds, double* __restrict__ out)
{
    double* const mine = lds + (threadIdx.x >> 6) * NV;
    wave_tree(s, [&](int k, double x) { if ((threadIdx.x & 63) == 0) mine[k] = x; });
    __syncthreads();
    for (int k = threadIdx.x; k < NV; k += kFitBlock) {
        double x = lds[k];
        for (int w2 = 1; w2 < kFitBlock / 64; ++w2) x += lds[w2 * NV + k];
        out[k] = x;
    }
}

// One wave, one selection of m resident points (the inner RANSAC of the local optimisation, DESIGN.md 5.8: m <= 64 in practice,
// 7 x the minimal sample size): lanes take the points t = lane, lane + 64, ..; sink(k, sum k) and the returned number of bad
// points are valid in lane 0.
template <class G, class F>
__device__ __forceinline__ int wave_gram(const double* __restrict__ pts, const int* __restrict__ index, const double* __restrict__ wsel,
                                         int m, int wpow, const FitParams& prm, F&& sink)
{
    Acc<G::Q> acc;
    acc.zero();
    int nbad = 0;
    for (int t = threadIdx.x; t < m; t += 64) nbad += accumulate<G>(pts, index[t], wsel != nullptr ? wsel + t : nullptr, wpow, prm, acc);
    wave_tree(acc.s, sink);
    return wave_sum(nbad);
}

// The selection pass.  blockIdx.y = item: with an index list the listed points (one item), otherwise the points whose resident label
// is label0 + item (PEARL::parameterEstimation refits every instance per iteration: all labels in one launch).  The parameters
// of item k are block k of prm_k, or prm for every item when prm_k is null.  Partials [item][block][NV], counters [2 * item]: the
// single-selection calls are gridDim.y = 1, so entry k of an all-labels call is bitwise the single-label call by construction.
template <class G>
__global__ __launch_bounds__(kFitBlock) void gram_kernel(const double* __restrict__ pts, int64_t n, FitParams prm,
                                                         const double* __restrict__ prm_k, const int* __restrict__ index, int64_t m,
                                                         const int* __restrict__ labels, int label0,
                                                         const double* __restrict__ weights, int wpow,
                                                         int blocks, double* __restrict__ partials, int* __restrict__ counters)
{
    constexpr int Q = G::Q, NV = Q * (Q + 1) / 2;
    __shared__ double lds[(kFitBlock / 64) * NV];
    __shared__ int s_cnt, s_bad;
    if (threadIdx.x == 0) { s_cnt = 0; s_bad = 0; }
    __syncthreads();
    const int item = (int)blockIdx.y;
    if (prm_k != nullptr) prm = load_params(prm_k, item);
    Acc<Q> acc;
    acc.zero();
    const int64_t t = (int64_t)blockIdx.x * kFitBlock + threadIdx.x;
    int64_t i = -1;
    if (index != nullptr) { if (t < m) i = index[t]; }
    else if (t < n && labels[t] == label0 + item) i = t;
    if (i >= 0) {
        const int bad = accumulate<G>(pts, i, weights != nullptr ? weights + i : nullptr, wpow, prm, acc);
        atomicAdd(&s_cnt, 1);
        if (bad) atomicAdd(&s_bad, 1);
    }
    block_tree<NV>(acc.s, lds, partials + ((int64_t)item * blocks + blockIdx.x) * NV);
    if (threadIdx.x == 0) {
        if (s_cnt) atomicAdd(&counters[2 * item], s_cnt);
        if (s_bad) atomicAdd(&counters[2 * item + 1], s_bad);
    }
}

// The final pass, one block per item: value k is summed by 16 lanes (lane j takes the blocks b = j mod 16 in order), then a fixed
// xor tree
__global__ __launch_bounds__(1024) void gram_final_kernel(const double* __restrict__ partials, int blocks, int nv,
                                                          double* __restrict__ out)
{
    const double* part = partials + (int64_t)blockIdx.x * blocks * nv;
    const int k = (int)threadIdx.x >> 4, j = (int)threadIdx.x & 15;
    double s = 0.0;
    if (k < nv)
        for (int b = j; b < blocks; b += 16) s += part[(int64_t)b * nv + k];
#pragma unroll
    for (int off = 8; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    if (k < nv && j == 0) out[(int64_t)blockIdx.x * nv + k] = s;
}

// B selections of m points each, one wave per selection, per-selection parameter blocks; fixed shuffle tree: bit-reproducible
template <class G>
__global__ __launch_bounds__(64) void gram_batch_kernel(const double* __restrict__ pts, const double* __restrict__ prm,
                                                        const int* __restrict__ index, int m,
                                                        const double* __restrict__ wsel, int wpow,
                                                        double* __restrict__ out, int* __restrict__ bad)
{
    constexpr int NV = G::Q * (G::Q + 1) / 2;
    const int64_t b = blockIdx.x;
    double* const mine = out + b * NV;
    const int nbad = wave_gram<G>(pts, index + b * m, wsel != nullptr ? wsel + b * m : nullptr, m, wpow, load_params(prm, b),
                                  [&](int k, double x) { if (threadIdx.x == 0) mine[k] = x; });
    if (threadIdx.x == 0) bad[b] = nbad;
}

// ---- Gauss-Newton pose refits of a whole batch in ONE launch --------------------------------------------------------------
// The local optimisation refits ~50 selections of 21 points per graph-cut round; each Gauss-Newton step used to be one
// gram_batch launch, a copy back, a stacked 6x6 pseudo-inverse on the host and a copy up (10 steps per round: a third of
// find6DPoses' proposal time at C4).  Here one wave owns one selection for all its steps: the normal equations by wave_gram(),
// the pass of gram_batch_kernel (bitwise the same sums by construction), broadcast to every lane, and each lane
// redundantly runs the small dense part - pseudo-inverse of the symmetric 6x6 through a cyclic Jacobi eigen-decomposition with
// numpy.linalg.pinv's cut-off (|lambda| <= rcond max|lambda| dropped), Rodrigues update of R, t += dt - exactly the iteration
// of pyprogressivex/_estimators.py PnPEstimator._fit_many, whose iterates it reproduces up to rounding (tests: 1e-9).

// x = pinv(A) b for symmetric A (6x6).  Cyclic Jacobi, fixed rotation order, at most 12 sweeps (it converges quadratically:
// 5-7 sweeps reach the rounding floor).
__device__ __forceinline__ void sym6_pinv_apply(const double (&A0)[6][6], const double (&b)[6], double rcond, double (&x)[6])
{
    double A[6][6], V[6][6];
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
        for (int c = 0; c < 6; ++c) { A[r][c] = A0[r][c]; V[r][c] = r == c ? 1.0 : 0.0; }
    for (int sweep = 0; sweep < 12; ++sweep) {
        double off = 0.0, dia = 0.0;
#pragma unroll
        for (int r = 0; r < 6; ++r) {
            dia += A[r][r] * A[r][r];
#pragma unroll
            for (int c = r + 1; c < 6; ++c) off += A[r][c] * A[r][c];
        }
        if (!(off > 1e-36 * dia)) break;   // (also leaves on NaN)
#pragma unroll
        for (int p = 0; p < 5; ++p)
#pragma unroll
            for (int q = p + 1; q < 6; ++q) {
                const double apq = A[p][q];
                if (apq == 0.0) continue;
                const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
                const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), sn = t * c;
#pragma unroll
                for (int k = 0; k < 6; ++k) {   // columns p, q
                    const double akp = A[k][p], akq = A[k][q];
                    A[k][p] = c * akp - sn * akq;
                    A[k][q] = sn * akp + c * akq;
                }
#pragma unroll
                for (int k = 0; k < 6; ++k) {   // rows p, q
                    const double apk = A[p][k], aqk = A[q][k];
                    A[p][k] = c * apk - sn * aqk;
                    A[q][k] = sn * apk + c * aqk;
                }
#pragma unroll
                for (int k = 0; k < 6; ++k) {
                    const double vkp = V[k][p], vkq = V[k][q];
                    V[k][p] = c * vkp - sn * vkq;
                    V[k][q] = sn * vkp + c * vkq;
                }
            }
    }
    double smax = 0.0;
#pragma unroll
    for (int i = 0; i < 6; ++i) smax = fmax(smax, fabs(A[i][i]));
#pragma unroll
    for (int k = 0; k < 6; ++k) x[k] = 0.0;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        const double lam = A[i][i];
        if (!(fabs(lam) > rcond * smax)) continue;
        double vb = 0.0;
#pragma unroll
        for (int k = 0; k < 6; ++k) vb += V[k][i] * b[k];
        const double f = vb / lam;
#pragma unroll
        for (int k = 0; k < 6; ++k) x[k] += f * V[k][i];
    }
}

__global__ __launch_bounds__(64) void pnp_refine_batch_kernel(const double* __restrict__ pts, const double* __restrict__ inits,
                                                              const int* __restrict__ index, int m, const double* __restrict__ wsel, int wpow,
                                                              int iterations, double* __restrict__ out, int* __restrict__ status)
{
    constexpr int NV = 28;
    const int64_t b = blockIdx.x;
    FitParams p = load_params(inits, b);
    bool failed = m < 4;
    for (int it = 0; it < iterations && !failed; ++it) {
        double g[NV];
        const int nbad = wave_gram<GenPnpGn>(pts, index + b * m, wsel != nullptr ? wsel + b * m : nullptr, m, wpow, p,
                                             [&](int k, double x) { g[k] = __shfl(x, 0, 64); });
        if (__shfl(nbad, 0, 64) > 0) { failed = true; break; }
        // upper triangle, row-major: (r, c) at r * 7 - r (r - 1) / 2 + (c - r)
        double A[6][6], rhs[6];
        bool fin = true;
#pragma unroll
        for (int r = 0; r < 6; ++r) {
#pragma unroll
            for (int c = r; c < 6; ++c) {
                const double v = g[r * 7 - r * (r - 1) / 2 + (c - r)];
                A[r][c] = v; A[c][r] = v;
                fin = fin && isfinite(v);
            }
            rhs[r] = -g[r * 7 - r * (r - 1) / 2 + (6 - r)];
            fin = fin && isfinite(rhs[r]);
        }
        if (!fin) { failed = true; break; }
        double d[6];
        sym6_pinv_apply(A, rhs, 6.0 * 2.220446049250313e-16, d);
        const double ang = sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
        if (ang > 0.0) {   // R <- exp([omega]_x) R
            const double kx = d[0] / ang, ky = d[1] / ang, kz = d[2] / ang;
            const double K[3][3] = {{0.0, -kz, ky}, {kz, 0.0, -kx}, {-ky, kx, 0.0}};
            const double sn = sin(ang), cs = 1.0 - cos(ang);
            double rot[3][3];
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    double kk = 0.0;
#pragma unroll
                    for (int j = 0; j < 3; ++j) kk += K[r][j] * K[j][c];
                    rot[r][c] = (r == c ? 1.0 : 0.0) + sn * K[r][c] + cs * kk;
                }
            double Rn[3][3];
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    double v = 0.0;
#pragma unroll
                    for (int j = 0; j < 3; ++j) v += rot[r][j] * p.v[j * 4 + c];
                    Rn[r][c] = v;
                }
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c < 3; ++c) p.v[r * 4 + c] = Rn[r][c];
        }
        p.v[3] += d[3]; p.v[7] += d[4]; p.v[11] += d[5];
        double nd = 0.0;
#pragma unroll
        for (int k = 0; k < 6; ++k) nd += d[k] * d[k];
        if (sqrt(nd) < 1e-12) break;
    }
    if (threadIdx.x == 0) {
        bool fin = true;
#pragma unroll
        for (int k = 0; k < 12; ++k) { out[(int64_t)b * 12 + k] = p.v[k]; fin = fin && isfinite(p.v[k]); }
        status[b] = (!failed && fin) ? 1 : 0;
    }
}

}  // namespace

// ---- host side: checks, scratch and uploads, each stated once ------------------------------------------------------------------

// what every Gram entry point asks first, under its own name: resident points, the weight power, a parameter block of at most 12
static int check_call(pgx_ctx* ctx, const char* who, int wpow, const double* params, int nparams)
{
    if (ctx->n <= 0 || ctx->model_type < 0) return fail(ctx, PGX_ERR_INVALID, "%s: points not set", who);
    if (wpow != 1 && wpow != 2) return fail(ctx, PGX_ERR_INVALID, "%s: weight power must be 1 or 2", who);
    if (nparams < 0 || nparams > 12 || (nparams > 0 && !params)) return fail(ctx, PGX_ERR_INVALID, "%s: bad parameter block", who);
    return PGX_OK;
}

// every index of a list names a resident point (checked before anything is enqueued: the kernels gather without a bound)
static int check_index(pgx_ctx* ctx, const char* who, const int32_t* index, int64_t count)
{
    for (int64_t t = 0; t < count; ++t)
        if (index[t] < 0 || index[t] >= ctx->n) return fail(ctx, PGX_ERR_INVALID, "%s: index %d out of range", who, index[t]);
    return PGX_OK;
}

// Regions of the given byte sizes one behind the other in ctx->fit_scratch, each from an 8-byte boundary: region[k] = start of
// region k.  Regions whose sizes are multiples of 8 are adjacent: the fused uploads and read-backs below rely on that.
template <size_t N>
static int carve(pgx_ctx* ctx, const size_t (&bytes)[N], char* (&region)[N])
{
    size_t off[N], total = 0;
    for (size_t k = 0; k < N; ++k) { off[k] = total; total += (bytes[k] + 7) & ~(size_t)7; }
    PGX_TRY(ensure(ctx, ctx->fit_scratch, total + 64));
    for (size_t k = 0; k < N; ++k) region[k] = (char*)ctx->fit_scratch.p + off[k];
    return PGX_OK;
}

static int gram_row_length(pgx_ctx* ctx, const char* who, int kind, int nparams, int* q)
{
    const int D = ctx->D;
    switch (kind) {
    case PGX_GRAM_AFFINE: *q = D + 1; if (D < 2 || D > 5) return fail(ctx, PGX_ERR_INVALID, "%s: affine rows need 2-, 3-, 4- or 5-D points", who); break;
    case PGX_GRAM_DLT_H: case PGX_GRAM_EPI_F: *q = 9; if (D != 4 || nparams != 6) return fail(ctx, PGX_ERR_INVALID, "%s: needs 4-D correspondences and 6 normalisation parameters", who); break;
    case PGX_GRAM_VP: *q = 3; if (D != 4) return fail(ctx, PGX_ERR_INVALID, "%s: needs 4-D segments", who); break;
    case PGX_GRAM_PNP_GN: *q = 7; if (D != 5 || nparams != 12) return fail(ctx, PGX_ERR_INVALID, "%s: needs 5-D 2D-3D rows and a 3x4 pose", who); break;
    case PGX_GRAM_SPHERE: *q = 5; if (D != 3 || nparams != 4) return fail(ctx, PGX_ERR_INVALID, "%s: needs 3-D points and 4 parameters (ox, oy, oz, s)", who); break;
    case PGX_GRAM_CIRCLE: *q = 4; if (D != 2 || nparams != 3) return fail(ctx, PGX_ERR_INVALID, "%s: needs 2-D points and 3 parameters (ox, oy, s)", who); break;
    case PGX_GRAM_CYL_GN: *q = 6; if (D != 3 || nparams != 10) return fail(ctx, PGX_ERR_INVALID, "%s: needs 3-D points and 10 parameters (p, d, r, u)", who); break;
    case PGX_GRAM_CONE_GN: *q = 7; if (D != 3 || nparams != 11) return fail(ctx, PGX_ERR_INVALID, "%s: needs 3-D points and 11 parameters (a, d, c, s, u)", who); break;
    case PGX_GRAM_TORUS_GN: *q = 8; if (D != 3 || nparams != 11) return fail(ctx, PGX_ERR_INVALID, "%s: needs 3-D points and 11 parameters (c, d, R, r, u)", who); break;
    default: return fail(ctx, PGX_ERR_INVALID, "%s: unknown row kind %d", who, kind);
    }
    return PGX_OK;
}

// the row generator of a kind that gram_row_length accepted: calls f(Gen{})
template <class F>
static void with_gram_generator(int kind, int D, F&& f)
{
    switch (kind) {
    case PGX_GRAM_AFFINE:
        if (D == 2) f(GenAffine<2>{});
        else if (D == 3) f(GenAffine<3>{});
        else if (D == 4) f(GenAffine<4>{});
        else f(GenAffine<5>{});
        break;
    case PGX_GRAM_DLT_H: f(GenDltH{}); break;
    case PGX_GRAM_EPI_F: f(GenEpiF{}); break;
    case PGX_GRAM_VP: f(GenVp{}); break;
    case PGX_GRAM_SPHERE: f(GenRound<3>{}); break;
    case PGX_GRAM_CIRCLE: f(GenRound<2>{}); break;
    case PGX_GRAM_CYL_GN: f(GenCylGn{}); break;
    case PGX_GRAM_CONE_GN: f(GenConeGn{}); break;
    case PGX_GRAM_TORUS_GN: f(GenTorusGn{}); break;
    default: f(GenPnpGn{}); break;
    }
}

// Per-point weights are RESIDENT (pgx_set_weights checks their length against n and uploads them once): the Gram calls only
// say whether to use them.  (They used to take a host pointer without a length and copied n doubles from it on every call.)
static int resident_weights(pgx_ctx* ctx, const char* who, int use_weights, const double** ww)
{
    *ww = nullptr;
    if (!use_weights) return PGX_OK;
    if (ctx->weights_n != ctx->n || !ctx->weights.p)
        return fail(ctx, PGX_ERR_INVALID, "%s: use_weights set but no weights are resident for the current points (pgx_set_weights)", who);
    *ww = ctx->weights.as<double>();
    return PGX_OK;
}

// the selection pass over blocks x K workgroups and the final pass of its K items: partials -> out [K][nv]
static int launch_gram(pgx_ctx* ctx, int kind, int K, int blocks, const FitParams& prm, const double* prm_k, const int* index, int64_t m,
                       int label0, const double* ww, int wpow, double* partials, int* counters, int nv, double* out)
{
    with_gram_generator(kind, ctx->D, [&](auto gen) {
        hipLaunchKernelGGL((gram_kernel<decltype(gen)>), dim3((unsigned)blocks, (unsigned)K), dim3(kFitBlock), 0, ctx->stream,
                           ctx->pts.as<double>(), ctx->n, prm, prm_k, index, m, ctx->labels.as<int>(), label0, ww, wpow, blocks, partials, counters);
    });
    PGX_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(gram_final_kernel, dim3((unsigned)K), dim3(1024), 0, ctx->stream, partials, blocks, nv, out);
    PGX_HIP(ctx, hipGetLastError());
    return PGX_OK;
}

// result [K][nv] | counters [2K], the counters cnt_off bytes behind the result: ONE copy back, into pinned memory
static int fetch_gram(pgx_ctx* ctx, const void* d_out, size_t cnt_off, int K, int nv, double* out, int64_t* count, int64_t* bad)
{
    const size_t bytes = cnt_off + (size_t)2 * K * sizeof(int);
    void* hs = nullptr;
    PGX_TRY(host_staging(ctx, bytes, &hs));
    PGX_TRY(d2h(ctx, hs, d_out, bytes));
    PGX_TRY(sync_deliver(ctx));
    memcpy(out, hs, (size_t)K * nv * sizeof(double));
    const int* cnt = (const int*)((const char*)hs + cnt_off);
    for (int k = 0; k < K; ++k) {
        if (count) count[k] = cnt[2 * k];
        if (bad) bad[k] = cnt[2 * k + 1];
    }
    return PGX_OK;
}

// The one-wave-per-selection calls: scratch prm[B][12] | out[B][out_doubles] | wsel[B][m] | index[B][m] | flags[B], and the uploads
// of the parameter blocks (host, [B][12]), the index lists and the selections' weights (wsel null: none, d->w null)
struct BatchBuffers {
    double *prm, *out, *w;
    int *index, *flags;
};

static int batch_upload(pgx_ctx* ctx, const double* prm, int B, int m, const int32_t* index, const double* wsel, size_t out_doubles,
                        BatchBuffers* d)
{
    const size_t tot = (size_t)B * m, prm_bytes = (size_t)B * 12 * 8, w_bytes = wsel ? tot * 8 : 0;
    char* r[5];
    PGX_TRY(carve(ctx, {prm_bytes, (size_t)B * out_doubles * 8, w_bytes, tot * 4, (size_t)B * 4}, r));
    *d = {(double*)r[0], (double*)r[1], wsel ? (double*)r[2] : nullptr, (int*)r[3], (int*)r[4]};
    PGX_HIP(ctx, hipMemcpyAsync(d->prm, prm, prm_bytes, hipMemcpyHostToDevice, ctx->stream));
    if (tot > 0) PGX_HIP(ctx, hipMemcpyAsync(d->index, index, tot * 4, hipMemcpyHostToDevice, ctx->stream));
    if (w_bytes) PGX_HIP(ctx, hipMemcpyAsync(d->w, wsel, w_bytes, hipMemcpyHostToDevice, ctx->stream));
    return PGX_OK;
}

int pnp_refine_batch_launch(pgx_ctx* ctx, const double* inits, const int32_t* index, int B, int m, const double* wsel, int wpow,
                            int iterations, double* out, int32_t* status)
{
    PGX_TRY(check_call(ctx, "pgx_pnp_refine_batch", wpow, nullptr, 0));
    if (ctx->D != 5) return fail(ctx, PGX_ERR_INVALID, "pgx_pnp_refine_batch: needs 5-D 2D-3D rows");
    if (!inits || !out || !status || B < 0 || m < 0 || iterations < 0 || ((int64_t)B * m > 0 && !index))
        return fail(ctx, PGX_ERR_INVALID, "pgx_pnp_refine_batch: bad argument");
    if (B == 0) return PGX_OK;
    PGX_TRY(check_index(ctx, "pgx_pnp_refine_batch", index, (int64_t)B * m));
    BatchBuffers d;
    PGX_TRY(batch_upload(ctx, inits, B, m, index, wsel, 12, &d));
    hipLaunchKernelGGL(pnp_refine_batch_kernel, dim3((unsigned)B), dim3(64), 0, ctx->stream, ctx->pts.as<double>(), d.prm, d.index, m,
                       d.w, wpow, iterations, d.out, d.flags);
    PGX_HIP(ctx, hipGetLastError());
    PGX_TRY(d2h(ctx, out, d.out, (size_t)B * 12 * 8));
    PGX_TRY(d2h(ctx, status, d.flags, (size_t)B * 4));
    PGX_TRY(sync_deliver(ctx));
    return PGX_OK;
}

int gram_batch_launch(pgx_ctx* ctx, int kind, const double* params, int nparams, const int32_t* index, int B, int m,
                      const double* wsel, int wpow, double* out, int32_t* bad)
{
    PGX_TRY(check_call(ctx, "pgx_gram_batch", wpow, params, nparams));
    if (!out || B < 0 || m < 0 || ((int64_t)B * m > 0 && !index)) return fail(ctx, PGX_ERR_INVALID, "pgx_gram_batch: bad argument");
    int q = 0;
    PGX_TRY(gram_row_length(ctx, "pgx_gram_batch", kind, nparams, &q));
    const int nv = q * (q + 1) / 2;
    if (B == 0) return PGX_OK;
    PGX_TRY(check_index(ctx, "pgx_gram_batch", index, (int64_t)B * m));
    std::vector<double> hp((size_t)B * 12, 0.0);
    for (int b = 0; b < B; ++b)
        for (int k = 0; k < nparams; ++k) hp[(size_t)b * 12 + k] = params[(size_t)b * nparams + k];
    BatchBuffers d;
    PGX_TRY(batch_upload(ctx, hp.data(), B, m, index, wsel, (size_t)nv, &d));
    with_gram_generator(kind, ctx->D, [&](auto gen) {
        hipLaunchKernelGGL((gram_batch_kernel<decltype(gen)>), dim3((unsigned)B), dim3(64), 0, ctx->stream, ctx->pts.as<double>(), d.prm,
                           d.index, m, d.w, wpow, d.out, d.flags);
    });
    PGX_HIP(ctx, hipGetLastError());
    PGX_TRY(d2h(ctx, out, d.out, (size_t)B * nv * 8));
    if (bad) PGX_TRY(d2h(ctx, bad, d.flags, (size_t)B * 4));
    PGX_TRY(sync_deliver(ctx));
    return PGX_OK;
}

int gram_labels_launch(pgx_ctx* ctx, int kind, const double* params, int nparams, int K, int use_weights, int wpow,
                       double* out, int64_t* count, int64_t* bad)
{
    PGX_TRY(check_call(ctx, "pgx_gram_labels", wpow, params, nparams));
    if (ctx->labels_n != ctx->n) return fail(ctx, PGX_ERR_INVALID, "pgx_gram_labels: labels not set");
    if (!out || K <= 0 || K > kMaxGramLabels) return fail(ctx, PGX_ERR_INVALID, "pgx_gram_labels: bad argument");
    int q = 0;
    PGX_TRY(gram_row_length(ctx, "pgx_gram_labels", kind, nparams, &q));
    const int nv = q * (q + 1) / 2;
    const int blocks = (int)((ctx->n + kFitBlock - 1) / kFitBlock);
    const double* ww = nullptr;
    PGX_TRY(resident_weights(ctx, "pgx_gram_labels", use_weights, &ww));
    // scratch: partials[K][blocks][nv] | out[K][nv] | counters[2K] | prm[K][12]
    const size_t out_bytes = (size_t)K * nv * 8, cnt_bytes = ((size_t)K * 8 + 15) & ~(size_t)15, prm_bytes = (size_t)K * 12 * 8;
    char* r[4];
    PGX_TRY(carve(ctx, {(size_t)K * blocks * nv * 8, out_bytes, cnt_bytes, prm_bytes}, r));
    // counters (zero) | parameter blocks are adjacent: ONE upload clears the first and fills the second; result | counters are
    // adjacent too (fetch_gram).  (A fill, two uploads' worth of commands and two blocking copies into pageable
    // memory before: a third of the call on a 300-point scene, scripts/bench_small_calls.py.)
    std::vector<double> hp(cnt_bytes / 8 + (size_t)K * 12, 0.0);
    for (int k = 0; k < K; ++k)
        for (int j = 0; j < nparams; ++j) hp[cnt_bytes / 8 + (size_t)k * 12 + j] = params[(size_t)k * nparams + j];
    PGX_HIP(ctx, hipMemcpyAsync(r[2], hp.data(), cnt_bytes + prm_bytes, hipMemcpyHostToDevice, ctx->stream));
    PGX_TRY(launch_gram(ctx, kind, K, blocks, FitParams{}, (const double*)r[3], nullptr, 0, 0, ww, wpow, (double*)r[0], (int*)r[2], nv,
                        (double*)r[1]));
    return fetch_gram(ctx, r[1], out_bytes, K, nv, out, count, bad);
}

int gram_launch(pgx_ctx* ctx, int kind, const double* params, int nparams, int sel, const int32_t* index, int64_t m,
                int label, int use_weights, int wpow, double* out, int64_t* count, int64_t* bad)
{
    PGX_TRY(check_call(ctx, "pgx_gram", wpow, params, nparams));
    if (!out) return fail(ctx, PGX_ERR_INVALID, "pgx_gram: out is NULL");
    int q = 0;
    PGX_TRY(gram_row_length(ctx, "pgx_gram", kind, nparams, &q));
    const int nv = q * (q + 1) / 2;
    int64_t work = 0;
    if (sel == PGX_SEL_INDEX) {
        if (m < 0 || (m > 0 && !index)) return fail(ctx, PGX_ERR_INVALID, "pgx_gram: index list missing");
        PGX_TRY(check_index(ctx, "pgx_gram", index, m));
        work = m;
    } else if (sel == PGX_SEL_LABEL) {
        if (ctx->labels_n != ctx->n) return fail(ctx, PGX_ERR_INVALID, "pgx_gram: labels not set");
        work = ctx->n;
    } else {
        return fail(ctx, PGX_ERR_INVALID, "pgx_gram: unknown selection %d", sel);
    }
    const double* ww = nullptr;
    PGX_TRY(resident_weights(ctx, "pgx_gram", use_weights, &ww));
    FitParams prm;
    for (int k = 0; k < 12; ++k) prm.v[k] = k < nparams ? params[k] : 0.0;
    const int blocks = (int)((work + kFitBlock - 1) / kFitBlock);
    if (blocks == 0) {
        for (int k = 0; k < nv; ++k) out[k] = 0.0;
        if (count) *count = 0;
        if (bad) *bad = 0;
        return PGX_OK;
    }
    // scratch: partials | out (64 doubles) | counters (64 bytes) | index
    const size_t idx_bytes = sel == PGX_SEL_INDEX ? (size_t)m * sizeof(int32_t) : 0;
    char* r[4];
    PGX_TRY(carve(ctx, {(size_t)blocks * nv * 8, 64 * sizeof(double), (size_t)64, idx_bytes}, r));
    int* d_cnt = (int*)r[2];
    // counters (zero) | index list are adjacent: a short list is uploaded together with the zeros (one command instead of two)
    std::vector<int32_t> up;   // (alive until the stream has been synchronised below)
    if (idx_bytes && m <= kFusedIndexMax) {
        up.assign(16 + (size_t)m, 0);
        memcpy(up.data() + 16, index, idx_bytes);
        PGX_HIP(ctx, hipMemcpyAsync(d_cnt, up.data(), 64 + idx_bytes, hipMemcpyHostToDevice, ctx->stream));
    } else {
        PGX_HIP(ctx, hipMemsetAsync(d_cnt, 0, 8, ctx->stream));
        if (idx_bytes) PGX_HIP(ctx, hipMemcpyAsync(r[3], index, idx_bytes, hipMemcpyHostToDevice, ctx->stream));
    }
    PGX_TRY(launch_gram(ctx, kind, 1, blocks, prm, nullptr, sel == PGX_SEL_INDEX ? (const int*)r[3] : nullptr, m, label, ww, wpow,
                        (double*)r[0], d_cnt, nv, (double*)r[1]));
    return fetch_gram(ctx, r[1], 64 * sizeof(double), 1, nv, out, count, bad);
}


// ---- smallest eigenpair of small symmetric matrices: the dense solve of the non-minimal refits behind the C ABI (round 6) -------
// Replaces: Eigen::SelfAdjointEigenSolver as the refit solvers use it (solver_vanishing_point_two_lines.h:227 in-tree; the DLT /
// 8-point solvers of the absent submodule on A^T A), so far numpy's LAPACK on the host.  Cyclic Jacobi in FP64, ONE LANE PER
// MATRIX in the operation order of the CPU restatement the tests hold (no contraction, IEEE division and square root): the
// device and that restatement return the same bits (tests), and both agree with LAPACK to ~1e-13 on the eigenvector (tests, tolerance
// stated there).  B is tens of matrices per call (one local-optimisation round): latency, not throughput.
__global__ __launch_bounds__(64) void eigh_smallest_kernel(const double* __restrict__ A, int q, int64_t B, double* __restrict__ vec,
                                                            double* __restrict__ val)
{
    const int64_t b = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    double a[9][9], v[9][9];
    for (int i = 0; i < 9; ++i)
        for (int j = 0; j < 9; ++j) {
            a[i][j] = (i < q && j < q) ? A[b * q * q + (int64_t)i * q + j] : 0.0;
            v[i][j] = i == j ? 1.0 : 0.0;
        }
    for (int sweep = 0; sweep < 50; ++sweep) {
        double off = 0.0, dg = 0.0;
        for (int p = 0; p < q; ++p) {
            dg = dg + a[p][p] * a[p][p];
            for (int r = p + 1; r < q; ++r) off = off + a[p][r] * a[p][r];
        }
        if (!(off > 4.930380657631324e-32 * dg)) break;
        for (int p = 0; p < q - 1; ++p)
            for (int r = p + 1; r < q; ++r) {
                const double apr = a[p][r];
                if (apr == 0.0) continue;
                const double theta = (a[r][r] - a[p][p]) / (2.0 * apr);
                const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), sn = t * c;
                for (int k = 0; k < q; ++k) {
                    const double akp = a[k][p], akr = a[k][r];
                    a[k][p] = c * akp - sn * akr;
                    a[k][r] = sn * akp + c * akr;
                }
                for (int k = 0; k < q; ++k) {
                    const double apk = a[p][k], ark = a[r][k];
                    a[p][k] = c * apk - sn * ark;
                    a[r][k] = sn * apk + c * ark;
                }
                for (int k = 0; k < q; ++k) {
                    const double vkp = v[k][p], vkr = v[k][r];
                    v[k][p] = c * vkp - sn * vkr;
                    v[k][r] = sn * vkp + c * vkr;
                }
            }
    }
    int best = 0;
    for (int p = 1; p < q; ++p)
        if (a[p][p] < a[best][best]) best = p;
    for (int k = 0; k < q; ++k) vec[b * q + k] = v[k][best];
    val[b] = a[best][best];
}

int eigh_smallest_launch(pgx_ctx* ctx, const double* A, int q, int64_t B, double* vec, double* val)
{
    if (!A || !vec || !val) return fail(ctx, PGX_ERR_INVALID, "pgx_eigh_smallest_batch: NULL argument");
    if (q < 1 || q > 9) return fail(ctx, PGX_ERR_INVALID, "pgx_eigh_smallest_batch: q = %d (1..9)", q);
    if (B <= 0) return PGX_OK;
    if (B > (1 << 20)) return fail(ctx, PGX_ERR_INVALID, "pgx_eigh_smallest_batch: at most 2^20 matrices per call");
    const size_t in_bytes = (size_t)B * q * q * sizeof(double), out_bytes = (size_t)B * (q + 1) * sizeof(double);
    PGX_TRY(ensure(ctx, ctx->fit_scratch, in_bytes + out_bytes + 256));
    double* d_A = (double*)ctx->fit_scratch.p;
    double* d_vec = (double*)((char*)ctx->fit_scratch.p + ((in_bytes + 255) & ~(size_t)255));
    double* d_val = d_vec + (size_t)B * q;
    PGX_HIP(ctx, hipMemcpyAsync(d_A, A, in_bytes, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(eigh_smallest_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, ctx->stream, d_A, q, B, d_vec, d_val);
    PGX_HIP(ctx, hipGetLastError());
    PGX_TRY(d2h(ctx, vec, d_vec, (size_t)B * q * sizeof(double)));
    PGX_TRY(d2h(ctx, val, d_val, (size_t)B * sizeof(double)));
    PGX_TRY(sync_deliver(ctx));
    return PGX_OK;
}

}  // namespace pgx
