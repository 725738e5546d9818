// components.hip — pgx_label_components: the connected components of a labelling in the resident neighbourhood graph (include/pgx.h
// states the definition; tests/components_model.py restates it as a breadth-first search and the device returns its integers).
//
// No reference counterpart: the reference returns models of infinite extent and never asks which of a model's inliers hang together.
//
// A lock-free union-find on parent[n] in the manner of ECL-CC (Jaiganesh & Burtscher, HPDC 2018), the find / link statements in
// components_uf.h.  Five launches on the ctx stream, and every launch that consumes another's parent[] is a launch of its own: what a
// launch wrote is visible to the next one because of the kernel boundary, and nothing inside a launch hands data from one workgroup to
// another through a fence or a flag.
//   init      parent[i] = i, counters zero
//   hook      every arc (i, j) with j < i and equal live labels: uf_unite(i, j).  The resident graph is symmetric and has no self arcs
//             (pgx_set_graph refuses any other), so each undirected arc is met once, from its larger end.  The larger root goes below the
//             smaller one, so the root of a finished tree is its smallest member - whatever order the hardware runs the lanes in.
//   flatten   root[i] = the root of i (parent[] is only read now), one integer atomicAdd per site on its root's counter
//   scan      rocprim exclusive scan of the root flags: a root's rank is its component's number, roots ascending = smallest members ascending
//   fill      comp[i] = rank[root[i]]; first[] and sizes[] from the roots
//
// MEMORY MODEL of the hook launch: every access to parent[] - load, compare-and-swap, path-halving store - is a relaxed agent-scope atomic
// on global memory (AgentMem below), so each is performed where the word is coherent for the whole device and none is served from a CU's
// L1.  No ordering between them is needed; components_uf.h says why a stale value can only cost a retry.  labels[], off[] and idx[] are
// written before the launch and only read in it.
//
// FORWARD PROGRESS: no kernel here waits for another lane, wave or workgroup - no spin, no flag, no barrier across workgroups, no
// persistent launch.  The one loop that repeats (uf_unite) repeats only after another lane's compare-and-swap has succeeded.
//
// WORK MAPPING: lane t serves site gorder[t] (the Morton order pgx_graph_build left) or site t (after pgx_set_graph), as in normals.hip:
// the lanes of a wave then walk neighbouring rows and mostly meet the same few roots.  A row has no length cap (ball graphs, hubs of the
// symmetric k-NN graph); a lane walks its own row only up to kLongRow arcs.  Longer rows are taken afterwards by the whole wave, one row
// at a time, lane l serving arcs l, l + 64, ... of it: no lane walks a 10^5-arc row alone.  The hand-over is a ballot and four shuffles
// inside the wave.  Consecutive arcs of one site hand the root they ended at to the next arc (uf_unite's return value), whose walk is
// then a single load while nobody else links that root.
#include <cstdint>
#include <cstring>

#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include "components_uf.h"
#include "pgx_internal.h"

namespace pgx {

namespace {

constexpr int kCcBlock = 256;
constexpr int kLongRow = PGX_COMPONENTS_LONG_ROW;   // rows beyond this many arcs go to a whole wave (include/pgx.h)
constexpr int kWave = 64;
static_assert(kCcBlock % kWave == 0, "whole waves");

struct AgentMem {   // components_uf.h's accesses as relaxed agent-scope atomics on global memory
    int* parent;
    __device__ __forceinline__ int load(int x) const { return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    __device__ __forceinline__ void store(int x, int v) { __hip_atomic_store(parent + x, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    __device__ __forceinline__ int cas(int x, int expected, int v)
    {
        __hip_atomic_compare_exchange_strong(parent + x, &expected, v, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return expected;   // what parent[x] held
    }
};

struct PlainMem {   // after the hook launch parent[] is read-only: plain loads
    const int* parent;
    __device__ __forceinline__ int load(int x) const { return parent[x]; }
};

__device__ __forceinline__ bool live_label(int l, int first_ignored) { return l >= 0 && l < first_ignored; }

__global__ __launch_bounds__(kCcBlock) void cc_init_kernel(int64_t n, int* __restrict__ parent, int* __restrict__ cnt, int* __restrict__ flag)
{
    const int64_t i = (int64_t)blockIdx.x * kCcBlock + threadIdx.x;
    if (i < n) {
        parent[i] = (int)i;
        cnt[i] = 0;
    }
    if (i == n) flag[n] = 0;   // the scan runs over n + 1 entries: its last output is the number of roots
}

// No early return: every lane of a wave reaches the ballot, lanes beyond n with an empty row.
__global__ __launch_bounds__(kCcBlock) void cc_hook_kernel(const int* __restrict__ off, const int* __restrict__ idx,
                                                           const int* __restrict__ order, const int* __restrict__ labels, int first_ignored,
                                                           int64_t n, int* parent)
{
    const int64_t t = (int64_t)blockIdx.x * kCcBlock + threadIdx.x;
    AgentMem m{parent};
    int i = -1, beg = 0, end = 0, li = -1;
    if (t < n) {
        i = order ? order[t] : (int)t;
        li = labels[i];
        if (live_label(li, first_ignored)) {
            beg = off[i];
            end = off[i + 1];
        }
    }
    const bool long_row = end - beg > kLongRow;
    if (!long_row) {
        int r = i;   // an ancestor of i: each arc's walk starts where the last one ended
        for (int a = beg; a < end; ++a) {
            const int j = idx[a];
            if (j < i && labels[j] == li) r = uf_unite(m, r, j);
        }
    }
    // the long rows of this wave, one after the other, by all 64 lanes
    const int lane = threadIdx.x & (kWave - 1);
    unsigned long long todo = __ballot(long_row);
    while (todo) {
        const int src = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        const int ri = __shfl(i, src, kWave), rbeg = __shfl(beg, src, kWave), rend = __shfl(end, src, kWave), rl = __shfl(li, src, kWave);
        int r = ri;
        for (int a = rbeg + lane; a < rend; a += kWave) {
            const int j = idx[a];
            if (j < ri && labels[j] == rl) r = uf_unite(m, r, j);
        }
    }
}

// root[i] (-1: not live), the root flags of the scan, and the sizes: one atomicAdd per site on its root's counter - or one per wave where
// every live lane of the wave has the root of the first one, the common case under the Morton order.
__global__ __launch_bounds__(kCcBlock) void cc_flatten_kernel(const int* __restrict__ order, const int* __restrict__ labels, int first_ignored,
                                                              int64_t n, const int* __restrict__ parent, int* __restrict__ root,
                                                              int* __restrict__ flag, int* cnt)
{
    const int64_t t = (int64_t)blockIdx.x * kCcBlock + threadIdx.x;
    const PlainMem m{parent};
    int r = -1;
    if (t < n) {
        const int i = order ? order[t] : (int)t;
        if (live_label(labels[i], first_ignored)) r = uf_root(m, i);
        root[i] = r;
        flag[i] = r == i ? 1 : 0;
    }
    const unsigned long long alive = __ballot(r >= 0);
    if (!alive) return;
    const int lead = __ffsll((long long)alive) - 1;
    const int r0 = __shfl(r, lead, kWave);
    const unsigned long long same = __ballot(r == r0);   // (r0 >= 0: only live lanes)
    const int lane = threadIdx.x & (kWave - 1);
    if (lane == lead) atomicAdd(&cnt[r0], __popcll(same));
    else if (r >= 0 && r != r0) atomicAdd(&cnt[r], 1);
}

__global__ __launch_bounds__(kCcBlock) void cc_fill_kernel(int64_t n, const int* __restrict__ root, const int* __restrict__ rank,
                                                           const int* __restrict__ cnt, int* __restrict__ comp, int* __restrict__ first,
                                                           long long* __restrict__ sizes)
{
    const int64_t i = (int64_t)blockIdx.x * kCcBlock + threadIdx.x;
    if (i >= n) return;
    const int r = root[i];
    comp[i] = r >= 0 ? rank[r] : -1;
    if (r == (int)i) {   // rank[i] < number of roots <= n
        first[rank[i]] = (int)i;
        sizes[rank[i]] = cnt[i];
    }
}

inline size_t pad256(size_t bytes) { return (bytes + 255) & ~(size_t)255; }

}  // namespace

int label_components_launch(pgx_ctx* ctx, const int32_t* labels, int64_t n, int32_t first_ignored, int32_t* comp_out, int32_t* first_out,
                            int64_t* sizes_out, int64_t* components)
{
    if (n < 0) return fail(ctx, PGX_ERR_INVALID, "pgx_label_components: n = %lld", (long long)n);
    if (!components) return fail(ctx, PGX_ERR_INVALID, "pgx_label_components: NULL argument");
    if (n == 0) {
        *components = 0;
        return PGX_OK;
    }
    if (!labels || !comp_out) return fail(ctx, PGX_ERR_INVALID, "pgx_label_components: NULL argument");
    if (ctx->gn <= 0)
        return fail(ctx, PGX_ERR_INVALID, "pgx_label_components: needs a neighbourhood graph of the points (pgx_graph_build / pgx_set_graph)");
    if (ctx->gn != n)
        return fail(ctx, PGX_ERR_INVALID, "pgx_label_components: %lld labels for a graph of %lld sites", (long long)n, (long long)ctx->gn);
    // the call's own buffer (the resident problem's are not touched): labels | parent | root | cnt | comp | first, n ints each;
    // flag | rank, n + 1 ints each; sizes, n int64; the scan's workspace - each from a 256-byte boundary
    size_t tmp_bytes = 0;
    int* const nulli = nullptr;
    PGX_HIP(ctx, rocprim::exclusive_scan(nullptr, tmp_bytes, nulli, nulli, 0, (size_t)(n + 1), rocprim::plus<int>(), ctx->stream));
    const size_t col = pad256((size_t)n * sizeof(int)), col1 = pad256((size_t)(n + 1) * sizeof(int)), wide = pad256((size_t)n * sizeof(long long));
    PGX_TRY(ensure(ctx, ctx->cc_buf, 6 * col + 2 * col1 + wide + pad256(tmp_bytes)));
    char* base = (char*)ctx->cc_buf.p;
    int* d_labels = (int*)base;
    int* d_parent = (int*)(base + col);
    int* d_root = (int*)(base + 2 * col);
    int* d_cnt = (int*)(base + 3 * col);
    int* d_comp = (int*)(base + 4 * col);
    int* d_first = (int*)(base + 5 * col);
    int* d_flag = (int*)(base + 6 * col);
    int* d_rank = (int*)(base + 6 * col + col1);
    long long* d_sizes = (long long*)(base + 6 * col + 2 * col1);
    void* d_tmp = base + 6 * col + 2 * col1 + wide;
    PGX_HIP(ctx, hipMemcpyAsync(d_labels, labels, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    const int* order = ctx->gorder_n == n ? ctx->gorder.as<int>() : nullptr;
    const int* off = ctx->goff.as<int>();
    const int* idx = ctx->gidx.as<int>();
    const dim3 block(kCcBlock), grid((unsigned)((n + kCcBlock - 1) / kCcBlock)), grid1((unsigned)((n + 1 + kCcBlock - 1) / kCcBlock));
    hipLaunchKernelGGL(cc_init_kernel, grid1, block, 0, ctx->stream, n, d_parent, d_cnt, d_flag);
    PGX_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(cc_hook_kernel, grid, block, 0, ctx->stream, off, idx, order, d_labels, first_ignored, n, d_parent);
    PGX_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(cc_flatten_kernel, grid, block, 0, ctx->stream, order, d_labels, first_ignored, n, d_parent, d_root, d_flag, d_cnt);
    PGX_HIP(ctx, hipGetLastError());
    PGX_HIP(ctx, rocprim::exclusive_scan(d_tmp, tmp_bytes, d_flag, d_rank, 0, (size_t)(n + 1), rocprim::plus<int>(), ctx->stream));
    hipLaunchKernelGGL(cc_fill_kernel, grid, block, 0, ctx->stream, n, d_root, d_rank, d_cnt, d_comp, d_first, d_sizes);
    PGX_HIP(ctx, hipGetLastError());
    int C = 0;
    PGX_TRY(d2h(ctx, &C, d_rank + n, sizeof(int)));
    PGX_TRY(d2h(ctx, comp_out, d_comp, (size_t)n * sizeof(int32_t)));
    PGX_TRY(sync_deliver(ctx));
    if (C < 0 || C > n) return fail(ctx, PGX_ERR_RANGE, "pgx_label_components: %d components of %lld sites", C, (long long)n);
    if (C > 0 && (first_out || sizes_out)) {   // C entries each: the count had to come back first
        if (first_out) PGX_TRY(d2h(ctx, first_out, d_first, (size_t)C * sizeof(int32_t)));
        if (sizes_out) PGX_TRY(d2h(ctx, sizes_out, d_sizes, (size_t)C * sizeof(int64_t)));
        PGX_TRY(sync_deliver(ctx));
    }
    *components = C;
    return PGX_OK;
}

}  // namespace pgx
