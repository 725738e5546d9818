// graph.hip — neighbourhood graph on the GPU: points -> symmetric CSR with multiplicities, left
// resident for the expansion moves.
//
// Replaces: gcransac::neighborhood::FlannNeighborhoodGraph(&points, radius) + getNeighbors(i)
//           (/root/reference/src/pyprogressivex/src/progressivex_python.cpp:104,207,339,458,571) and the
//           setNeighbors loop of pearl::PEARL::labeling (/root/reference/src/pyprogressivex/include/PEARL.h:532-536).
//           The FLANN implementation is absent from the snapshot [U-7]: the deterministic restatement is "the k nearest
//           neighbours inside the ball" (k = 5 by default, the list length upstream's checks = 6 search can return),
//           or plain k-NN; one CSR entry per directed list element [U-6] => multiplicity 1 or 2 per undirected pair.
//
// Exact arithmetic contract (the parity tests require bit-identical neighbour sets): squared distance
//   s = (a0-b0)*(a0-b0); s = s + (a1-b1)*(a1-b1); ... in dimension order, double, no contraction; a neighbour needs
//   s <= radius*radius; candidates are ranked by (s, index) ascending; the point itself is skipped by index.
//
// Method: uniform grid over the first two coordinates with cell size >= radius (so the ball lies in the 3x3 block of
// cells), counting sort of the points by cell, then one workgroup per (cell, slice of 256 of its points): the points
// of the nine cells are streamed through LDS tiles and every thread keeps the K best of its own query in registers
// (LDS reads are broadcasts: all lanes look at the same candidate).  FP64-VALU/LDS bound: N * (points per 3x3 block)
// pair tests of 3d flops.  Lists -> CSR: reciprocity test, degree scan, fill with atomically placed reverse entries,
// per-row sort (rows come out sorted, so the result does not depend on atomic order).
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include "pgx_internal.h"

namespace pgx {

namespace {

constexpr int kGBlock = 256;
constexpr int kMaxCells = 1 << 22;   // (a grid beyond it: tests/test_gpu_switches.py test_graph_grid_is_coarsened_beyond_the_cell_limit)
constexpr int kTile = 256;

struct GridSpec {
    double min0, min1, inv_cell;
    int W, H;
};

__device__ __forceinline__ int cell_of(const GridSpec& g, double x, double y)
{
    int cx = (int)floor((x - g.min0) * g.inv_cell);
    int cy = (int)floor((y - g.min1) * g.inv_cell);
    cx = cx < 0 ? 0 : (cx >= g.W ? g.W - 1 : cx);
    cy = cy < 0 ? 0 : (cy >= g.H ? g.H - 1 : cy);
    return cy * g.W + cx;
}

__global__ __launch_bounds__(kGBlock) void g_key_kernel(const double* __restrict__ pts, int64_t n, int d, GridSpec g,
                                                        int* __restrict__ key, int* __restrict__ count)
{
    const int64_t i = (int64_t)blockIdx.x * kGBlock + threadIdx.x;
    if (i >= n) return;
    const int c = cell_of(g, pts[i * d], pts[i * d + 1]);
    key[i] = c;
    atomicAdd(&count[c], 1);
}

// exclusive scan of `in[0..m)` into `out[0..m]` (out[m] = total), one workgroup; `per` = ceil-division applied to the
// inputs first when > 0 (number of query slices of a cell)
__global__ __launch_bounds__(1024) void g_scan_kernel(const int* __restrict__ in, int* __restrict__ out, int64_t m, int per)
{
    __shared__ int s_wave[16];
    __shared__ int s_carry;
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) s_carry = 0;
    __syncthreads();
    for (int64_t base = 0; base < m; base += 1024 * 4) {
        int v[4], sum = 0;
        const int64_t i0 = base + (int64_t)tid * 4;
        for (int j = 0; j < 4; ++j) {
            int x = (i0 + j < m) ? in[i0 + j] : 0;
            if (per > 0) x = (x + per - 1) / per;
            v[j] = sum;
            sum += x;
        }
        int incl = sum;
        for (int o = 1; o < 64; o <<= 1) {
            const int t = __shfl_up(incl, o, 64);
            if (lane >= o) incl += t;
        }
        if (lane == 63) s_wave[wave] = incl;
        __syncthreads();
        int wbase = 0;
        for (int w = 0; w < wave; ++w) wbase += s_wave[w];
        const int carry = s_carry;
        const int excl = carry + wbase + incl - sum;
        for (int j = 0; j < 4; ++j)
            if (i0 + j < m) out[i0 + j] = excl + v[j];
        __syncthreads();
        if (tid == 1023) s_carry = carry + wbase + incl;
        __syncthreads();
    }
    if (tid == 0) out[m] = s_carry;
}

__global__ __launch_bounds__(kGBlock) void g_scatter_kernel(const double* __restrict__ pts, int64_t n, int d,
                                                            const int* __restrict__ key, const int* __restrict__ start,
                                                            int* __restrict__ cursor, int* __restrict__ sidx,
                                                            double* __restrict__ spts)
{
    const int64_t i = (int64_t)blockIdx.x * kGBlock + threadIdx.x;
    if (i >= n) return;
    const int c = key[i];
    const int pos = start[c] + atomicAdd(&cursor[c], 1);
    sidx[pos] = (int)i;
    for (int k = 0; k < d; ++k) spts[(int64_t)pos * d + k] = pts[i * d + k];
}

// K best candidates of one query, ascending by (s, index); slot K-1 is the current worst
template <int K>
struct Best {
    double s[K];
    int id[K];
    __device__ __forceinline__ void init()
    {
#pragma unroll
        for (int j = 0; j < K; ++j) { s[j] = __builtin_inf(); id[j] = 0x7fffffff; }
    }
    __device__ __forceinline__ void offer(double v, int c)
    {
        if (!(v < s[K - 1] || (v == s[K - 1] && c < id[K - 1]))) return;
        s[K - 1] = v;
        id[K - 1] = c;
#pragma unroll
        for (int j = K - 1; j > 0; --j) {
            const bool sw = s[j] < s[j - 1] || (s[j] == s[j - 1] && id[j] < id[j - 1]);
            const double ts = sw ? s[j - 1] : s[j];
            const int ti = sw ? id[j - 1] : id[j];
            s[j - 1] = sw ? s[j] : s[j - 1];
            id[j - 1] = sw ? id[j] : id[j - 1];
            s[j] = ts;
            id[j] = ti;
        }
    }
};

// One workgroup per (cell, slice of 256 queries).  blk_start[c] = first workgroup of cell c (scan of ceil(cnt/256)).
// knn_mode: the radius is the guaranteed search radius of a plain k-NN pass; a query whose K-th neighbour lies
// beyond it (or that found fewer than K) stays pending for a pass with a larger cell.
template <int D, int K>
__global__ __launch_bounds__(kGBlock) void g_search_kernel(const double* __restrict__ spts, const int* __restrict__ sidx,
                                                           const int* __restrict__ start, const int* __restrict__ blk_start,
                                                           GridSpec g, int cells, double r2, int k, int knn_mode,
                                                           int* __restrict__ done, int* __restrict__ nbr,
                                                           int* __restrict__ pending)
{
    __shared__ double t_pts[kTile * D];
    __shared__ int t_idx[kTile];
    __shared__ int s_cell;
    if (threadIdx.x == 0) {  // which cell does this workgroup belong to: last c with blk_start[c] <= blockIdx.x
        int lo = 0, hi = cells;
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (blk_start[mid] <= (int)blockIdx.x) lo = mid; else hi = mid;
        }
        s_cell = lo;
    }
    __syncthreads();
    const int c = s_cell;
    const int slice = (int)blockIdx.x - blk_start[c];
    const int cs = start[c], ce = start[c + 1];
    const int q = cs + slice * kGBlock + (int)threadIdx.x;
    bool live = q < ce;
    int qi = -1;
    double qp[D];
    if (live) {
        qi = sidx[q];
        if (done != nullptr && done[qi]) live = false;
#pragma unroll
        for (int j = 0; j < D; ++j) qp[j] = spts[(int64_t)q * D + j];
    }
    if (__syncthreads_count(live ? 1 : 0) == 0) return;
    Best<K> best;
    best.init();
    const int cx = c % g.W, cy = c / g.W;
    for (int dy = -1; dy <= 1; ++dy) {
        const int yy = cy + dy;
        if (yy < 0 || yy >= g.H) continue;
        // the three cells of a grid row are contiguous in the sorted order
        const int x0 = cx > 0 ? cx - 1 : 0, x1 = cx + 1 < g.W ? cx + 1 : g.W - 1;
        const int s0 = start[yy * g.W + x0], s1 = start[yy * g.W + x1 + 1];
        for (int t0 = s0; t0 < s1; t0 += kTile) {
            const int m = s1 - t0 < kTile ? s1 - t0 : kTile;
            __syncthreads();
            for (int e = (int)threadIdx.x; e < m * D; e += kGBlock) t_pts[e] = spts[(int64_t)t0 * D + e];
            for (int e = (int)threadIdx.x; e < m; e += kGBlock) t_idx[e] = sidx[t0 + e];
            __syncthreads();
            if (live)
                for (int e = 0; e < m; ++e) {
                    double df = qp[0] - t_pts[e * D];
                    double s = df * df;
#pragma unroll
                    for (int j = 1; j < D; ++j) {
                        df = qp[j] - t_pts[e * D + j];
                        s = s + df * df;
                    }
                    const int ci = t_idx[e];
                    // a squared distance that overflowed (coordinates ~1e155 and beyond) ranks nothing: no neighbour, as in the oracle
                    if (s <= r2 && s < __builtin_inf() && ci != qi) best.offer(s, ci);
                }
        }
    }
    if (!live) return;
    int found = 0;
#pragma unroll
    for (int j = 0; j < K; ++j)
        if (j < k) {
            const bool ok = best.id[j] != 0x7fffffff;
            nbr[(int64_t)qi * k + j] = ok ? best.id[j] : -1;
            found += ok ? 1 : 0;
        }
    if (knn_mode) {
        if (found == k) done[qi] = 1;   // the k-th lies within the radius every candidate of which was seen
        else atomicAdd(pending, 1);
    }
}

// Exhaustive ball (PGX_GRAPH_BALL): every point with squared distance <= r2, variable degree.  Same tiling as the search
// kernel, run twice: phase 0 counts (deg[qi]), phase 1 writes the neighbours to idx[off[qi] ..] in the order met (rows
// are sorted afterwards).  (a-b)^2 == (b-a)^2 and the sum runs over the coordinates in the same order, so the lists are
// symmetric by construction: every arc gets multiplicity 2 (both directed entries exist, U-6).
template <int D>
__global__ __launch_bounds__(kGBlock) void g_ball_kernel(const double* __restrict__ spts, const int* __restrict__ sidx,
                                                         const int* __restrict__ start, const int* __restrict__ blk_start,
                                                         GridSpec g, int cells, double r2, int phase, int* __restrict__ deg,
                                                         const int* __restrict__ off, int* __restrict__ idx,
                                                         int* __restrict__ mult, unsigned long long* __restrict__ total)
{
    __shared__ double t_pts[kTile * D];
    __shared__ int t_idx[kTile];
    __shared__ int s_cell;
    if (threadIdx.x == 0) {
        int lo = 0, hi = cells;
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (blk_start[mid] <= (int)blockIdx.x) lo = mid; else hi = mid;
        }
        s_cell = lo;
    }
    __syncthreads();
    const int c = s_cell;
    const int slice = (int)blockIdx.x - blk_start[c];
    const int cs = start[c], ce = start[c + 1];
    const int q = cs + slice * kGBlock + (int)threadIdx.x;
    const bool live = q < ce;
    int qi = -1;
    double qp[D];
    if (live) {
        qi = sidx[q];
#pragma unroll
        for (int j = 0; j < D; ++j) qp[j] = spts[(int64_t)q * D + j];
    }
    int cnt = 0;
    int w = (live && phase == 1) ? off[qi] : 0;
    const int cx = c % g.W, cy = c / g.W;
    for (int dy = -1; dy <= 1; ++dy) {
        const int yy = cy + dy;
        if (yy < 0 || yy >= g.H) continue;
        const int x0 = cx > 0 ? cx - 1 : 0, x1 = cx + 1 < g.W ? cx + 1 : g.W - 1;
        const int s0 = start[yy * g.W + x0], s1 = start[yy * g.W + x1 + 1];
        for (int t0 = s0; t0 < s1; t0 += kTile) {
            const int m = s1 - t0 < kTile ? s1 - t0 : kTile;
            __syncthreads();
            for (int e = (int)threadIdx.x; e < m * D; e += kGBlock) t_pts[e] = spts[(int64_t)t0 * D + e];
            for (int e = (int)threadIdx.x; e < m; e += kGBlock) t_idx[e] = sidx[t0 + e];
            __syncthreads();
            if (live)
                for (int e = 0; e < m; ++e) {
                    double df = qp[0] - t_pts[e * D];
                    double s = df * df;
#pragma unroll
                    for (int j = 1; j < D; ++j) {
                        df = qp[j] - t_pts[e * D + j];
                        s = s + df * df;
                    }
                    const int ci = t_idx[e];
                    if (s <= r2 && ci != qi) {
                        if (phase == 1) { idx[w] = ci; mult[w] = 2; ++w; }
                        ++cnt;
                    }
                }
        }
    }
    if (phase == 0) {
        if (live) deg[qi] = cnt;
        unsigned long long t = (unsigned long long)cnt;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) t += __shfl_down(t, o, 64);
        if ((threadIdx.x & 63) == 0 && t) atomicAdd(total, t);
    }
}

// ---- lists -> CSR ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kGBlock) void g_recip_kernel(const int* __restrict__ nbr, int64_t n, int k,
                                                          int* __restrict__ m1, int* __restrict__ outdeg,
                                                          int* __restrict__ extra)
{
    const int64_t i = (int64_t)blockIdx.x * kGBlock + threadIdx.x;
    if (i >= n) return;
    int deg = 0;
    for (int s = 0; s < k; ++s) {
        const int j = nbr[i * k + s];
        if (j < 0) { m1[i * k + s] = 0; continue; }
        bool rec = false;
        for (int t = 0; t < k; ++t) rec |= nbr[(int64_t)j * k + t] == (int)i;
        m1[i * k + s] = rec ? 2 : 1;
        if (!rec) atomicAdd(&extra[j], 1);
        ++deg;
    }
    outdeg[i] = deg;
}

__global__ __launch_bounds__(kGBlock) void g_degree_kernel(const int* __restrict__ outdeg, const int* __restrict__ extra,
                                                           int64_t n, int* __restrict__ deg)
{
    const int64_t i = (int64_t)blockIdx.x * kGBlock + threadIdx.x;
    if (i < n) deg[i] = outdeg[i] + extra[i];
}

__global__ __launch_bounds__(kGBlock) void g_fill_kernel(const int* __restrict__ nbr, const int* __restrict__ m1, int64_t n,
                                                         int k, const int* __restrict__ off, const int* __restrict__ outdeg,
                                                         int* __restrict__ cursor, int* __restrict__ idx,
                                                         int* __restrict__ mult)
{
    const int64_t i = (int64_t)blockIdx.x * kGBlock + threadIdx.x;
    if (i >= n) return;
    int w = off[i];
    for (int s = 0; s < k; ++s) {
        const int j = nbr[i * k + s];
        if (j < 0) continue;
        idx[w] = j;
        mult[w] = m1[i * k + s];
        ++w;
        if (m1[i * k + s] == 1) {  // j does not list i: the pair still needs its entry in row j
            const int pos = off[j] + outdeg[j] + atomicAdd(&cursor[j], 1);
            idx[pos] = (int)i;
            mult[pos] = 1;
        }
    }
}

// rows sorted by neighbour index (insertion sort: rows hold k + a few entries); also row statistics
__global__ __launch_bounds__(kGBlock) void g_rowsort_kernel(int64_t n, const int* __restrict__ off, int* __restrict__ idx,
                                                            int* __restrict__ mult, int* __restrict__ stats)
{
    const int64_t i = (int64_t)blockIdx.x * kGBlock + threadIdx.x;
    if (i >= n) return;
    const int a = off[i], b = off[i + 1];
    int rowm = 0;
    for (int p = a; p < b; ++p) {
        const int vi = idx[p], vm = mult[p];
        rowm += vm;
        int qq = p - 1;
        while (qq >= a && idx[qq] > vi) { idx[qq + 1] = idx[qq]; mult[qq + 1] = mult[qq]; --qq; }
        idx[qq + 1] = vi;
        mult[qq + 1] = vm;
    }
    atomicMax(&stats[0], b - a);
    atomicMax(&stats[1], rowm);
}

struct GraphScratch {
    DevBuf key, count, start, cursor, sidx, spts, blk, nbr, m1, outdeg, extra, deg, done, small, dpts;
};

template <int D>
void launch_search(pgx_ctx* ctx, GraphScratch& gs, const GridSpec& g, int cells, int nblocks, double r2, int k, int knn_mode)
{
    int* done = knn_mode ? gs.done.as<int>() : nullptr;
    int* pending = gs.small.as<int>();
    if (k <= 8)
        hipLaunchKernelGGL((g_search_kernel<D, 8>), dim3((unsigned)nblocks), dim3(kGBlock), 0, ctx->stream, gs.spts.as<double>(),
                           gs.sidx.as<int>(), gs.start.as<int>(), gs.blk.as<int>(), g, cells, r2, k, knn_mode, done,
                           gs.nbr.as<int>(), pending);
    else
        hipLaunchKernelGGL((g_search_kernel<D, 16>), dim3((unsigned)nblocks), dim3(kGBlock), 0, ctx->stream, gs.spts.as<double>(),
                           gs.sidx.as<int>(), gs.start.as<int>(), gs.blk.as<int>(), g, cells, r2, k, knn_mode, done,
                           gs.nbr.as<int>(), pending);
}

template <int D>
void launch_ball(pgx_ctx* ctx, GraphScratch& gs, const GridSpec& g, int cells, int nblocks, double r2, int phase, int* off,
                 int* idx, int* mult)
{
    hipLaunchKernelGGL((g_ball_kernel<D>), dim3((unsigned)nblocks), dim3(kGBlock), 0, ctx->stream, gs.spts.as<double>(),
                       gs.sidx.as<int>(), gs.start.as<int>(), gs.blk.as<int>(), g, cells, r2, phase, gs.deg.as<int>(), off, idx, mult,
                       (unsigned long long*)(gs.small.as<int>() + 2));
}

// ---- site order for the tile-resident min-cut (maxflow_tile.hip): Morton code of the coordinates the graph was built on,
// quantised with ONE cell size for all coordinates (the ball's radius: neighbours are at most one cell apart in every
// coordinate), most significant bits first, coordinates with fewer cells contributing fewer bits
struct MortonSpec {
    double mn[5];
    double inv_cell;
    int bits[5];
    int d, maxb;
};

__global__ __launch_bounds__(kGBlock) void g_morton_kernel(const double* __restrict__ pts, int64_t n, MortonSpec m,
                                                           unsigned long long* __restrict__ keys, int* __restrict__ vals)
{
    const int64_t i = (int64_t)blockIdx.x * kGBlock + threadIdx.x;
    if (i >= n) return;
    int q[5];
    for (int k = 0; k < m.d; ++k) {
        const double x = (pts[i * m.d + k] - m.mn[k]) * m.inv_cell;
        int c = x > 0.0 ? (x < 2147483000.0 ? (int)x : 2147483000) : 0;   // NaN -> 0
        const int top = (1 << m.bits[k]) - 1;
        q[k] = c > top ? top : c;
    }
    unsigned long long key = 0;
    for (int level = m.maxb - 1; level >= 0; --level)
        for (int k = 0; k < m.d; ++k)
            if (level < m.bits[k]) key = (key << 1) | (unsigned long long)((q[k] >> level) & 1);
    keys[i] = key;
    vals[i] = (int)i;
}

int graph_site_order(pgx_ctx* ctx, const double* d_pts, int64_t n, int d, const double* mn, const double* mx, double cell)
{
    ctx->gorder_n = 0;
    MortonSpec m;
    m.d = d;
    double ext = 0.0;
    for (int k = 0; k < d; ++k) { m.mn[k] = mn[k]; ext = std::fmax(ext, mx[k] - mn[k]); }
    if (!(cell > 0.0) || !std::isfinite(cell)) cell = ext / 1024.0;
    if (!(cell > 0.0) || !std::isfinite(ext)) return PGX_OK;   // all points identical (or not finite): the caller's order
    const int cap = 62 / d;
    int total = 0;
    for (;;) {
        total = 0;
        m.maxb = 0;
        bool fits = true;
        for (int k = 0; k < d; ++k) {
            const double cells = std::floor((mx[k] - mn[k]) / cell) + 1.0;
            int b = 0;
            while (b < 31 && (double)(1u << b) < cells) ++b;
            if (b > cap) fits = false;
            m.bits[k] = b;
            total += b;
            m.maxb = b > m.maxb ? b : m.maxb;
        }
        if (fits) break;
        cell *= 2.0;
    }
    if (total == 0) return PGX_OK;
    m.inv_cell = 1.0 / cell;
    size_t tmp_bytes = 0;
    unsigned long long* nullk = nullptr;
    int* nullv = nullptr;
    PGX_HIP(ctx, rocprim::radix_sort_pairs(nullptr, tmp_bytes, nullk, nullk, nullv, nullv, (size_t)n, 0, (unsigned)total, ctx->stream));
    const size_t ka = ((size_t)n * 8 + 255) & ~(size_t)255, va = ((size_t)n * 4 + 255) & ~(size_t)255;
    PGX_TRY(ensure(ctx, ctx->fit_scratch, 2 * ka + va + tmp_bytes + 256));
    PGX_TRY(ensure(ctx, ctx->gorder, (size_t)n * sizeof(int)));
    char* base = (char*)ctx->fit_scratch.p;
    unsigned long long* k_in = (unsigned long long*)base;
    unsigned long long* k_out = (unsigned long long*)(base + ka);
    int* v_in = (int*)(base + 2 * ka);
    void* tmp = base + 2 * ka + va;
    hipLaunchKernelGGL(g_morton_kernel, dim3((unsigned)((n + kGBlock - 1) / kGBlock)), dim3(kGBlock), 0, ctx->stream, d_pts, n, m, k_in, v_in);
    PGX_HIP(ctx, hipGetLastError());
    PGX_HIP(ctx, rocprim::radix_sort_pairs(tmp, tmp_bytes, k_in, k_out, v_in, ctx->gorder.as<int>(), (size_t)n, 0, (unsigned)total, ctx->stream));
    ctx->gorder_n = n;
    return PGX_OK;
}

void free_scratch(GraphScratch& gs)
{
    DevBuf* all[] = {&gs.key, &gs.count, &gs.start, &gs.cursor, &gs.sidx, &gs.spts, &gs.blk, &gs.nbr, &gs.m1,
                     &gs.outdeg, &gs.extra, &gs.deg, &gs.done, &gs.small, &gs.dpts};
    for (DevBuf* b : all) release(*b);
}

// one grid pass: sort by cell of size `cell`, search.  Returns the number of pending queries (knn mode) in *pending.
int grid_pass(pgx_ctx* ctx, GraphScratch& gs, int64_t n, int d, const double mn[2], const double mx[2], double cell,
              double r2, int k, int knn_mode, int* pending_out, GridSpec* grid_out = nullptr, int* nblocks_out = nullptr)
{
    GridSpec g;
    g.min0 = mn[0]; g.min1 = mn[1];
    for (;;) {
        const double w = std::floor((mx[0] - mn[0]) / cell) + 1.0, h = std::floor((mx[1] - mn[1]) / cell) + 1.0;
        if (w * h <= (double)kMaxCells) { g.W = (int)w; g.H = (int)h; break; }
        cell *= 1.5;  // coarser cells keep the 3x3 block a superset of the ball
    }
    g.inv_cell = 1.0 / cell;
    const int cells = g.W * g.H;
    const unsigned nb = (unsigned)((n + kGBlock - 1) / kGBlock);
    PGX_TRY(ensure(ctx, gs.count, (size_t)cells * sizeof(int)));
    PGX_TRY(ensure(ctx, gs.cursor, (size_t)cells * sizeof(int)));
    PGX_TRY(ensure(ctx, gs.start, (size_t)(cells + 1) * sizeof(int)));
    PGX_TRY(ensure(ctx, gs.blk, (size_t)(cells + 1) * sizeof(int)));
    PGX_HIP(ctx, hipMemsetAsync(gs.count.p, 0, (size_t)cells * sizeof(int), ctx->stream));
    PGX_HIP(ctx, hipMemsetAsync(gs.cursor.p, 0, (size_t)cells * sizeof(int), ctx->stream));
    PGX_HIP(ctx, hipMemsetAsync(gs.small.p, 0, 16, ctx->stream));
    hipLaunchKernelGGL(g_key_kernel, dim3(nb), dim3(kGBlock), 0, ctx->stream, gs.dpts.as<double>(), n, d, g, gs.key.as<int>(),
                       gs.count.as<int>());
    hipLaunchKernelGGL(g_scan_kernel, dim3(1), dim3(1024), 0, ctx->stream, gs.count.as<int>(), gs.start.as<int>(), (int64_t)cells, 0);
    hipLaunchKernelGGL(g_scan_kernel, dim3(1), dim3(1024), 0, ctx->stream, gs.count.as<int>(), gs.blk.as<int>(), (int64_t)cells, kGBlock);
    hipLaunchKernelGGL(g_scatter_kernel, dim3(nb), dim3(kGBlock), 0, ctx->stream, gs.dpts.as<double>(), n, d, gs.key.as<int>(),
                       gs.start.as<int>(), gs.cursor.as<int>(), gs.sidx.as<int>(), gs.spts.as<double>());
    int nblocks = 0;
    PGX_TRY(d2h(ctx, &nblocks, gs.blk.as<int>() + cells, sizeof(int)));
    PGX_TRY(sync_deliver(ctx));
    if (grid_out) {  // the caller runs its own kernels over the sorted grid (exhaustive ball)
        *grid_out = g;
        *nblocks_out = nblocks;
        *pending_out = 0;
        return PGX_OK;
    }
    if (nblocks > 0) {
        switch (d) {
        case 2: launch_search<2>(ctx, gs, g, cells, nblocks, r2, k, knn_mode); break;
        case 3: launch_search<3>(ctx, gs, g, cells, nblocks, r2, k, knn_mode); break;
        case 4: launch_search<4>(ctx, gs, g, cells, nblocks, r2, k, knn_mode); break;
        case 5: launch_search<5>(ctx, gs, g, cells, nblocks, r2, k, knn_mode); break;
        default: return fail(ctx, PGX_ERR_INVALID, "pgx_graph_build: dimension %d not supported (2..5)", d);
        }
    }
    PGX_HIP(ctx, hipGetLastError());
    int pend = 0;
    if (knn_mode) {
        PGX_TRY(d2h(ctx, &pend, gs.small.p, sizeof(int)));
        PGX_TRY(sync_deliver(ctx));
    }
    *pending_out = pend;
    return PGX_OK;
}

}  // namespace

int graph_build_launch(pgx_ctx* ctx, const double* pts, int64_t n, int d, int kind, double radius, int k, int64_t* arcs)
{
    if (n <= 0 || !pts) return fail(ctx, PGX_ERR_INVALID, "pgx_graph_build: no points");
    if (n >= (int64_t)1 << 30) return fail(ctx, PGX_ERR_INVALID, "pgx_graph_build: too many points");
    if (d < 2 || d > 5) return fail(ctx, PGX_ERR_INVALID, "pgx_graph_build: dimension %d not supported (2..5)", d);
    if (kind != PGX_GRAPH_KNN_IN_BALL && kind != PGX_GRAPH_KNN && kind != PGX_GRAPH_BALL)
        return fail(ctx, PGX_ERR_INVALID, "pgx_graph_build: unknown graph kind %d", kind);
    if (k < 1 || k > 16) return fail(ctx, PGX_ERR_INVALID, "pgx_graph_build: k = %d outside 1..16", k);
    if (kind == PGX_GRAPH_BALL) k = 1;  // unused
    if (kind != PGX_GRAPH_KNN && !(radius > 0.0)) return fail(ctx, PGX_ERR_INVALID, "pgx_graph_build: radius must be > 0");
    if (k > n - 1) k = (int)(n - 1);
    // extent of the two grid coordinates (host pass: the caller's buffer is in host memory anyway)
    double mn[5] = {pts[0], pts[1], 0, 0, 0}, mx[5] = {pts[0], pts[1], 0, 0, 0};
    for (int c = 2; c < d; ++c) mn[c] = mx[c] = pts[c];
    for (int64_t i = 0; i < n; ++i)
        for (int c = 0; c < d; ++c) {
            const double v = pts[i * d + c];
            if (c < 2 && (!(v == v) || std::isinf(v))) return fail(ctx, PGX_ERR_INVALID, "pgx_graph_build: non-finite coordinate in row %lld", (long long)i);
            if (v < mn[c]) mn[c] = v;
            if (v > mx[c]) mx[c] = v;
        }
    GraphScratch gs;
    int rc = PGX_OK;
    // exhaustive ball: count, scan, fill, sort rows — the lists are symmetric, the CSR is written directly
    auto ball_csr = [&](pgx_ctx* c, GraphScratch& g_s, int64_t nn, int dd, const double* lo, const double* hi, double rad,
                        int64_t* arcs_out) -> int {
        GridSpec g;
        int nblocks = 0, pend = 0;
        const double cell = rad * (1.0 + 1e-9);
        PGX_TRY(grid_pass(c, g_s, nn, dd, lo, hi, cell, rad * rad, 1, 0, &pend, &g, &nblocks));
        const int cells = g.W * g.H;
        const unsigned nb = (unsigned)((nn + kGBlock - 1) / kGBlock);
        PGX_TRY(ensure(c, c->goff, (size_t)(nn + 1) * sizeof(int32_t)));
        PGX_HIP(c, hipMemsetAsync(g_s.small.p, 0, 32, c->stream));
        PGX_HIP(c, hipMemsetAsync(g_s.deg.p, 0, (size_t)nn * sizeof(int), c->stream));
        auto run = [&](int phase, int* off, int* idx, int* mult) {
            switch (dd) {
            case 2: launch_ball<2>(c, g_s, g, cells, nblocks, rad * rad, phase, off, idx, mult); break;
            case 3: launch_ball<3>(c, g_s, g, cells, nblocks, rad * rad, phase, off, idx, mult); break;
            case 4: launch_ball<4>(c, g_s, g, cells, nblocks, rad * rad, phase, off, idx, mult); break;
            default: launch_ball<5>(c, g_s, g, cells, nblocks, rad * rad, phase, off, idx, mult); break;
            }
        };
        if (nblocks > 0) run(0, nullptr, nullptr, nullptr);
        PGX_HIP(c, hipGetLastError());
        unsigned long long total = 0;
        PGX_TRY(d2h(c, &total, g_s.small.as<int>() + 2, sizeof(total)));
        PGX_TRY(sync_deliver(c));
        if (total >= (1ull << 31)) return fail(c, PGX_ERR_INVALID, "pgx_graph_build: %llu arcs inside the ball (limit 2^31 - 1): choose a smaller radius", total);
        hipLaunchKernelGGL(g_scan_kernel, dim3(1), dim3(1024), 0, c->stream, g_s.deg.as<int>(), c->goff.as<int>(), nn, 0);
        const int E = (int)total;
        PGX_TRY(ensure(c, c->gidx, (size_t)(E > 0 ? E : 1) * sizeof(int32_t)));
        PGX_TRY(ensure(c, c->gmult, (size_t)(E > 0 ? E : 1) * sizeof(int32_t)));
        PGX_TRY(ensure(c, c->grev, (size_t)(E > 0 ? E : 1) * sizeof(int32_t)));
        int stats[2] = {0, 0};
        if (E > 0) {
            run(1, c->goff.as<int>(), c->gidx.as<int>(), c->gmult.as<int>());
            PGX_HIP(c, hipMemsetAsync(g_s.small.p, 0, 16, c->stream));
            hipLaunchKernelGGL(g_rowsort_kernel, dim3(nb), dim3(kGBlock), 0, c->stream, nn, c->goff.as<int>(), c->gidx.as<int>(),
                               c->gmult.as<int>(), g_s.small.as<int>());
            PGX_TRY(d2h(c, stats, g_s.small.p, sizeof(stats)));
            PGX_TRY(sync_deliver(c));
        }
        PGX_HIP(c, hipGetLastError());
        c->gn = nn; c->gE = E; c->max_degree = stats[0]; c->max_row_mult = stats[1];
        if (arcs_out) *arcs_out = E;
        return graph_build_reverse(c);
    };
    auto body = [&]() -> int {
        const size_t nk = (size_t)n * (size_t)(k > 0 ? k : 1);
        PGX_TRY(ensure(ctx, gs.dpts, (size_t)n * d * sizeof(double)));
        PGX_TRY(ensure(ctx, gs.spts, (size_t)n * d * sizeof(double)));
        PGX_TRY(ensure(ctx, gs.key, (size_t)n * sizeof(int)));
        PGX_TRY(ensure(ctx, gs.sidx, (size_t)n * sizeof(int)));
        PGX_TRY(ensure(ctx, gs.nbr, nk * sizeof(int)));
        PGX_TRY(ensure(ctx, gs.m1, nk * sizeof(int)));
        PGX_TRY(ensure(ctx, gs.outdeg, (size_t)n * sizeof(int)));
        PGX_TRY(ensure(ctx, gs.extra, (size_t)n * sizeof(int)));
        PGX_TRY(ensure(ctx, gs.deg, (size_t)n * sizeof(int)));
        PGX_TRY(ensure(ctx, gs.done, (size_t)n * sizeof(int)));
        PGX_TRY(ensure(ctx, gs.small, 64));
        PGX_HIP(ctx, hipMemcpyAsync(gs.dpts.p, pts, (size_t)n * d * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
        PGX_HIP(ctx, hipMemsetAsync(gs.nbr.p, 0xff, nk * sizeof(int), ctx->stream));
        PGX_HIP(ctx, hipMemsetAsync(gs.done.p, 0, (size_t)n * sizeof(int), ctx->stream));
        int pend = 0;
        if (kind == PGX_GRAPH_BALL) return ball_csr(ctx, gs, n, d, mn, mx, radius, arcs);
        if (k == 0) {
            // a single point: no neighbours
        } else if (kind == PGX_GRAPH_KNN_IN_BALL) {
            const double cell = radius * (1.0 + 1e-9);  // strictly larger than the ball: rounding cannot skip a cell
            PGX_TRY(grid_pass(ctx, gs, n, d, mn, mx, cell, radius * radius, k, 0, &pend));
        } else {
            // plain k-NN: passes with growing cells; a query is final once its k-th neighbour lies within the cell size
            const double ext0 = mx[0] - mn[0], ext1 = mx[1] - mn[1];
            const double area = (ext0 > 0 ? ext0 : 1.0) * (ext1 > 0 ? ext1 : 1.0);
            double cell = std::sqrt(4.0 * (double)(k + 1) * area / (double)n);
            const double span = (ext0 > ext1 ? ext0 : ext1) * (1.0 + 1e-9) + 1e-300;
            for (int pass = 0; pass < 64; ++pass) {
                const bool whole = cell >= span;  // one cell block covers everything: the search is exhaustive
                const double r = whole ? __builtin_inf() : cell / (1.0 + 1e-9);
                PGX_TRY(grid_pass(ctx, gs, n, d, mn, mx, whole ? span : cell, whole ? __builtin_inf() : r * r, k, 1, &pend));
                if (pend == 0 || whole) break;
                cell *= 2.0;
            }
        }
        // ---- lists -> CSR
        const unsigned nb = (unsigned)((n + kGBlock - 1) / kGBlock);
        PGX_TRY(ensure(ctx, ctx->goff, (size_t)(n + 1) * sizeof(int32_t)));
        PGX_HIP(ctx, hipMemsetAsync(gs.extra.p, 0, (size_t)n * sizeof(int), ctx->stream));
        if (k == 0) {
            PGX_HIP(ctx, hipMemsetAsync(ctx->goff.p, 0, (size_t)(n + 1) * sizeof(int32_t), ctx->stream));
        } else {
            hipLaunchKernelGGL(g_recip_kernel, dim3(nb), dim3(kGBlock), 0, ctx->stream, gs.nbr.as<int>(), n, k, gs.m1.as<int>(),
                               gs.outdeg.as<int>(), gs.extra.as<int>());
            hipLaunchKernelGGL(g_degree_kernel, dim3(nb), dim3(kGBlock), 0, ctx->stream, gs.outdeg.as<int>(), gs.extra.as<int>(), n,
                               gs.deg.as<int>());
            hipLaunchKernelGGL(g_scan_kernel, dim3(1), dim3(1024), 0, ctx->stream, gs.deg.as<int>(), ctx->goff.as<int>(), n, 0);
        }
        int E = 0;
        PGX_TRY(d2h(ctx, &E, ctx->goff.as<int>() + n, sizeof(int)));
        PGX_TRY(sync_deliver(ctx));
        PGX_TRY(ensure(ctx, ctx->gidx, (size_t)(E > 0 ? E : 1) * sizeof(int32_t)));
        PGX_TRY(ensure(ctx, ctx->gmult, (size_t)(E > 0 ? E : 1) * sizeof(int32_t)));
        PGX_TRY(ensure(ctx, ctx->grev, (size_t)(E > 0 ? E : 1) * sizeof(int32_t)));
        int stats[2] = {0, 0};
        if (E > 0) {
            PGX_HIP(ctx, hipMemsetAsync(gs.extra.p, 0, (size_t)n * sizeof(int), ctx->stream));  // reused as the fill cursor
            PGX_HIP(ctx, hipMemsetAsync(gs.small.p, 0, 16, ctx->stream));
            hipLaunchKernelGGL(g_fill_kernel, dim3(nb), dim3(kGBlock), 0, ctx->stream, gs.nbr.as<int>(), gs.m1.as<int>(), n, k,
                               ctx->goff.as<int>(), gs.outdeg.as<int>(), gs.extra.as<int>(), ctx->gidx.as<int>(),
                               ctx->gmult.as<int>());
            hipLaunchKernelGGL(g_rowsort_kernel, dim3(nb), dim3(kGBlock), 0, ctx->stream, n, ctx->goff.as<int>(), ctx->gidx.as<int>(),
                               ctx->gmult.as<int>(), gs.small.as<int>());
            PGX_TRY(d2h(ctx, stats, gs.small.p, sizeof(stats)));
            PGX_TRY(sync_deliver(ctx));
        }
        PGX_HIP(ctx, hipGetLastError());
        ctx->gn = n; ctx->gE = E; ctx->max_degree = stats[0]; ctx->max_row_mult = stats[1];
        if (arcs) *arcs = E;
        return graph_build_reverse(ctx);
    };
    rc = body();
    ctx->gorder_n = 0;
    if (rc == PGX_OK && ctx->tile_order)   // (gs.dpts still holds the caller's rows)
        rc = graph_site_order(ctx, gs.dpts.as<double>(), n, d, mn, mx, kind == PGX_GRAPH_KNN ? 0.0 : radius);
    (void)hipStreamSynchronize(ctx->stream);
    free_scratch(gs);
    if (rc != PGX_OK) { ctx->gn = 0; ctx->gE = 0; }
    return rc;
}

int graph_fetch_launch(pgx_ctx* ctx, int32_t* off, int32_t* idx, int32_t* mult)
{
    if (ctx->gn <= 0) return fail(ctx, PGX_ERR_INVALID, "pgx_graph_fetch: no graph resident");
    if (!off) return fail(ctx, PGX_ERR_INVALID, "pgx_graph_fetch: off is NULL");
    PGX_TRY(d2h(ctx, off, ctx->goff.p, (size_t)(ctx->gn + 1) * sizeof(int32_t)));
    if (ctx->gE > 0 && idx) PGX_TRY(d2h(ctx, idx, ctx->gidx.p, (size_t)ctx->gE * sizeof(int32_t)));
    if (ctx->gE > 0 && mult) PGX_TRY(d2h(ctx, mult, ctx->gmult.p, (size_t)ctx->gE * sizeof(int32_t)));
    PGX_TRY(sync_deliver(ctx));
    return PGX_OK;
}

}  // namespace pgx
