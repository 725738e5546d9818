// normals.hip — pgx_estimate_normals: per-point surface normals from the resident neighbourhood graph (include/pgx.h states the
// definition; tests/normals_model.py restates it in numpy and the device returns its bits).
//
// No reference counterpart: the reference has no oriented-point model.  The cylinder's minimal solver (solve.hip) reads one normal per
// point, and until now the only source of them was the dataset generator's own radial vectors.
//
// ONE LANE PER POINT, both passes over the row sequential in row order: the definition's summation order is the loop, and a result is
// a pure function of the point's neighbourhood - which lane computes it does not matter.  Lane t serves site gorder[t] (the sites in
// the Morton order of the coordinates the graph was built on) when that order is resident, so that the lanes of a wave gather from
// neighbouring rows of `points` and share their cache lines; without it (pgx_set_graph) lane t serves site t.  Pass 2 gathers the row
// again instead of keeping it: a row has no length cap (ball graphs, hubs of the symmetric k-NN graph), and a runtime-indexed register
// array would live in scratch memory.  The 3 x 3 Jacobi is eigh_smallest_kernel's (fit.hip) operation order at q = 3 with every index
// a compile-time constant, so the matrices stay in registers.
#include <cmath>

#include "pgx_internal.h"

namespace pgx {

namespace {

constexpr int kNormalsBlock = 256;

__device__ __forceinline__ bool finite3(double x, double y, double z)
{
    return isfinite(x) && isfinite(y) && isfinite(z);
}

// one rotation of the cyclic sweep on the pair (P, R): the three k-loops of eigh_smallest_kernel, in their order
template <int P, int R>
__device__ __forceinline__ void jacobi_rotate(double (&a)[3][3], double (&v)[3][3])
{
    const double apr = a[P][R];
    if (apr == 0.0) return;
    const double theta = (a[R][R] - a[P][P]) / (2.0 * apr);
    const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double c = 1.0 / sqrt(t * t + 1.0), sn = t * c;
#define PGX_NRM_COLS(k) { const double akp = a[k][P], akr = a[k][R]; a[k][P] = c * akp - sn * akr; a[k][R] = sn * akp + c * akr; }
#define PGX_NRM_ROWS(k) { const double apk = a[P][k], ark = a[R][k]; a[P][k] = c * apk - sn * ark; a[R][k] = sn * apk + c * ark; }
#define PGX_NRM_VECS(k) { const double vkp = v[k][P], vkr = v[k][R]; v[k][P] = c * vkp - sn * vkr; v[k][R] = sn * vkp + c * vkr; }
    PGX_NRM_COLS(0) PGX_NRM_COLS(1) PGX_NRM_COLS(2)
    PGX_NRM_ROWS(0) PGX_NRM_ROWS(1) PGX_NRM_ROWS(2)
    PGX_NRM_VECS(0) PGX_NRM_VECS(1) PGX_NRM_VECS(2)
#undef PGX_NRM_COLS
#undef PGX_NRM_ROWS
#undef PGX_NRM_VECS
}

__global__ __launch_bounds__(kNormalsBlock) void estimate_normals_kernel(const double* __restrict__ pts, const int* __restrict__ off,
                                                                         const int* __restrict__ idx, const int* __restrict__ order,
                                                                         int64_t n, double v0, double v1, double v2, int has_view,
                                                                         double* __restrict__ nrm, double* __restrict__ curv,
                                                                         unsigned long long* __restrict__ undefined)
{
    const int64_t t = (int64_t)blockIdx.x * kNormalsBlock + threadIdx.x;
    if (t >= n) return;
    const int64_t i = order ? (int64_t)order[t] : t;
    const int beg = off[i], end = off[i + 1];
    const double m = (double)(1 + (end - beg));
    const double x0 = pts[3 * i], x1 = pts[3 * i + 1], x2 = pts[3 * i + 2];
    bool ok = (end - beg) >= 2 && finite3(x0, x1, x2);
    // pass 1: the offsets' sums, the self term (e = 0) first
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    for (int a = beg; a < end; ++a) {
        const int64_t j = idx[a];
        const double y0 = pts[3 * j], y1 = pts[3 * j + 1], y2 = pts[3 * j + 2];
        ok = ok && finite3(y0, y1, y2);
        s0 = s0 + (y0 - x0);
        s1 = s1 + (y1 - x1);
        s2 = s2 + (y2 - x2);
    }
    const double mu0 = s0 / m, mu1 = s1 / m, mu2 = s2 / m;
    // pass 2: the centred second moments, the self term first
    double d0 = 0.0 - mu0, d1 = 0.0 - mu1, d2 = 0.0 - mu2;
    double c00 = d0 * d0, c01 = d0 * d1, c02 = d0 * d2, c11 = d1 * d1, c12 = d1 * d2, c22 = d2 * d2;
    for (int a = beg; a < end; ++a) {
        const int64_t j = idx[a];
        d0 = (pts[3 * j] - x0) - mu0;
        d1 = (pts[3 * j + 1] - x1) - mu1;
        d2 = (pts[3 * j + 2] - x2) - mu2;
        c00 = c00 + d0 * d0;
        c01 = c01 + d0 * d1;
        c02 = c02 + d0 * d2;
        c11 = c11 + d1 * d1;
        c12 = c12 + d1 * d2;
        c22 = c22 + d2 * d2;
    }
    ok = ok && isfinite(c00) && isfinite(c01) && isfinite(c02) && isfinite(c11) && isfinite(c12) && isfinite(c22);
    if (!ok) {
        const double nan = __builtin_nan("");
        nrm[3 * i] = nan;
        nrm[3 * i + 1] = nan;
        nrm[3 * i + 2] = nan;
        if (curv) curv[i] = nan;
        atomicAdd(undefined, 1ull);
        return;
    }
    const double trace = (c00 + c11) + c22;
    double a[3][3] = {{c00, c01, c02}, {c01, c11, c12}, {c02, c12, c22}};
    double v[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
    for (int sweep = 0; sweep < 50; ++sweep) {
        double offd = 0.0, dg = 0.0;
        dg = dg + a[0][0] * a[0][0];
        offd = offd + a[0][1] * a[0][1];
        offd = offd + a[0][2] * a[0][2];
        dg = dg + a[1][1] * a[1][1];
        offd = offd + a[1][2] * a[1][2];
        dg = dg + a[2][2] * a[2][2];
        if (!(offd > 4.930380657631324e-32 * dg)) break;
        jacobi_rotate<0, 1>(a, v);
        jacobi_rotate<0, 2>(a, v);
        jacobi_rotate<1, 2>(a, v);
    }
    // best: the first smallest diagonal entry.  Every entry is read into a scalar first and the selection is made among the scalars: a
    // conditional read of v[k][best] becomes a read through a selected address, and the matrix then lives in scratch memory after all
    const double l0 = a[0][0], l1 = a[1][1], l2 = a[2][2];
    const double v00 = v[0][0], v01 = v[0][1], v02 = v[0][2], v10 = v[1][0], v11 = v[1][1], v12 = v[1][2], v20 = v[2][0], v21 = v[2][1],
                 v22 = v[2][2];
    const bool b1 = l1 < l0;
    double lam = b1 ? l1 : l0, n0 = b1 ? v01 : v00, n1 = b1 ? v11 : v10, n2 = b1 ? v21 : v20;
    const bool b2 = l2 < lam;
    lam = b2 ? l2 : lam;
    n0 = b2 ? v02 : n0;
    n1 = b2 ? v12 : n1;
    n2 = b2 ? v22 : n2;
    // sign: the entry of largest magnitude (lowest index on ties) positive, then towards the viewpoint
    double big = n0;
    if (fabs(n1) > fabs(big)) big = n1;
    if (fabs(n2) > fabs(big)) big = n2;
    if (big < 0.0) { n0 = -n0; n1 = -n1; n2 = -n2; }
    if (has_view) {
        const double tv = ((v0 - x0) * n0 + (v1 - x1) * n1) + (v2 - x2) * n2;
        if (tv < 0.0) { n0 = -n0; n1 = -n1; n2 = -n2; }
    }
    nrm[3 * i] = n0;
    nrm[3 * i + 1] = n1;
    nrm[3 * i + 2] = n2;
    if (curv) curv[i] = lam / trace;
}

}  // namespace

int estimate_normals_launch(pgx_ctx* ctx, const double* points, int64_t n, const double* viewpoint, double* normals_out,
                            double* curvature_out, int64_t* undefined)
{
    if (n < 0) return fail(ctx, PGX_ERR_INVALID, "pgx_estimate_normals: n = %lld", (long long)n);
    if (n == 0) {
        if (undefined) *undefined = 0;
        return PGX_OK;
    }
    if (!points || !normals_out) return fail(ctx, PGX_ERR_INVALID, "pgx_estimate_normals: NULL argument");
    if (viewpoint && !(std::isfinite(viewpoint[0]) && std::isfinite(viewpoint[1]) && std::isfinite(viewpoint[2])))
        return fail(ctx, PGX_ERR_INVALID, "pgx_estimate_normals: non-finite viewpoint");
    if (ctx->gn <= 0)
        return fail(ctx, PGX_ERR_INVALID, "pgx_estimate_normals: needs a neighbourhood graph of the points (pgx_graph_build / pgx_set_graph)");
    if (ctx->gn != n)
        return fail(ctx, PGX_ERR_INVALID, "pgx_estimate_normals: %lld points for a graph of %lld sites", (long long)n, (long long)ctx->gn);
    // scratch: points | normals | curvature | counter, each from a 256-byte boundary (the resident problem's buffers are not touched)
    const size_t row = ((size_t)n * 3 * sizeof(double) + 255) & ~(size_t)255, col = ((size_t)n * sizeof(double) + 255) & ~(size_t)255;
    PGX_TRY(ensure(ctx, ctx->fit_scratch, 2 * row + col + 256));
    char* base = (char*)ctx->fit_scratch.p;
    double* d_pts = (double*)base;
    double* d_nrm = (double*)(base + row);
    double* d_curv = curvature_out ? (double*)(base + 2 * row) : nullptr;
    unsigned long long* d_cnt = (unsigned long long*)(base + 2 * row + col);
    PGX_HIP(ctx, hipMemcpyAsync(d_pts, points, (size_t)n * 3 * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    PGX_HIP(ctx, hipMemsetAsync(d_cnt, 0, sizeof(unsigned long long), ctx->stream));
    const int* order = ctx->gorder_n == n ? ctx->gorder.as<int>() : nullptr;
    hipLaunchKernelGGL(estimate_normals_kernel, dim3((unsigned)((n + kNormalsBlock - 1) / kNormalsBlock)), dim3(kNormalsBlock), 0, ctx->stream,
                       d_pts, ctx->goff.as<int>(), ctx->gidx.as<int>(), order, n, viewpoint ? viewpoint[0] : 0.0,
                       viewpoint ? viewpoint[1] : 0.0, viewpoint ? viewpoint[2] : 0.0, viewpoint ? 1 : 0, d_nrm, d_curv, d_cnt);
    PGX_HIP(ctx, hipGetLastError());
    unsigned long long cnt = 0;
    PGX_TRY(d2h(ctx, normals_out, d_nrm, (size_t)n * 3 * sizeof(double)));
    if (curvature_out) PGX_TRY(d2h(ctx, curvature_out, d_curv, (size_t)n * sizeof(double)));
    PGX_TRY(d2h(ctx, &cnt, d_cnt, sizeof(cnt)));
    PGX_TRY(sync_deliver(ctx));
    if (undefined) *undefined = (int64_t)cnt;
    return PGX_OK;
}

}  // namespace pgx
