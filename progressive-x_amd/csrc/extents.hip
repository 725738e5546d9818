// extents.hip — pgx_instance_extents: per-instance bounds, sector masks, occupancy and counts of a labelled 3-D point cloud, each point
// measured in its instance's frame (include/pgx.h states the definition; tests/extents_model.py restates it in numpy and the device
// returns its bits).
//
// No reference counterpart: the reference returns models of infinite extent and never says how far along them the points reach.
//
// The per-point arithmetic is extents_point.h's, shared with a CPU driver.  Every word of the result is an integer reduction - add, max
// or or, identity 0 - so the table is one hipMemsetAsync and the result does not depend on the order of the lanes.  Three launches on
// the ctx stream, each consuming what the one before it finished; the hand-overs are the kernel boundaries, no workgroup waits for
// another, and nothing in a kernel loops on another lane's progress:
//   bounds     one lane per point, grid-stride: the point's contribution (count 1, two keys per linear coordinate, one sector bit per
//              angular one) into its instance's row.  A wave whose live lanes share one label - the common case for labels that follow
//              the scan order - merges inside the wave first (shuffles) and its leader sends one atomic per non-zero slot.  For
//              K <= PGX_EXTENTS_LDS_INSTANCES the row lives in a workgroup's LDS table (ds atomics) and the workgroup ends by sending
//              its non-zero words to the global table; above it the lanes go to the global table directly.  Same operations, same bits.
//   finalise   one lane per instance: keys -> lo / hi, count and sectors into the layout handed back
//   occupancy  one lane per point again: its cell between the FINISHED bounds, or-ed into the instance's word the same two ways
//
// ATOMICS (Guideline 12 of the HIP guide): a global atomic per point per slot would put every lane of a uniform wave on one address;
// the wave merge makes that one per wave, the LDS table one per workgroup and touched word.  The grid is capped (kExtMaxBlocks) so
// the flush - at most 7 K words per workgroup - stays small next to the points a workgroup serves.  All of them are relaxed,
// device-scope, returnless read-modify-writes performed at L2; the next launch reads them across a kernel boundary.
#include <cstdint>

#include <hip/hip_runtime.h>

#include "extents_point.h"
#include "pgx_internal.h"

namespace pgx {

namespace {

constexpr int kExtBlock = 256;
constexpr int kExtWave = 64;
constexpr int kExtLdsK = PGX_EXTENTS_LDS_INSTANCES;
constexpr int kExtMaxBlocks = 1024;   // 4 workgroups per CU: a lane serves ceil(n / 262144) points
static_assert(kExtBlock % kExtWave == 0, "whole waves");
static_assert((size_t)kExtLdsK * EXT_SLOTS * sizeof(unsigned long long) <= 32 * 1024, "the workgroup's table takes at most half of 64 KiB");

typedef unsigned long long u64;
static_assert(sizeof(u64) == sizeof(uint64_t), "one word");

struct AtomicTab {   // extents_point.h's three updates as relaxed atomics; `w` is an LDS or a global table
    u64* w;
    __device__ __forceinline__ void add(int64_t i, uint64_t x) { atomicAdd(w + i, (u64)x); }
    __device__ __forceinline__ void max(int64_t i, uint64_t x) { atomicMax(w + i, (u64)x); }
    __device__ __forceinline__ void bor(int64_t i, uint64_t x) { atomicOr(w + i, (u64)x); }
};

__device__ __forceinline__ u64 shfl_xor_u64(u64 x, int mask)
{
    const int lo = __shfl_xor((int)(unsigned)(x & 0xffffffffull), mask, kExtWave);
    const int hi = __shfl_xor((int)(unsigned)(x >> 32), mask, kExtWave);
    return ((u64)(unsigned)hi << 32) | (u64)(unsigned)lo;
}

template <class Op>
__device__ __forceinline__ u64 wave_reduce(u64 x, Op op)   // every lane of the wave takes part; all end with the result
{
    for (int m = kExtWave / 2; m >= 1; m >>= 1) x = op(x, shfl_xor_u64(x, m));
    return x;
}

struct OpAdd { __device__ u64 operator()(u64 a, u64 b) const { return a + b; } };
struct OpMax { __device__ u64 operator()(u64 a, u64 b) const { return a > b ? a : b; } };
struct OpOr { __device__ u64 operator()(u64 a, u64 b) const { return a | b; } };

// the wave's contributions to ONE row as one; a slot nobody fills is left alone (the ballot is uniform across the wave)
__device__ __forceinline__ void wave_combine(ExtAcc& a)
{
    a.v[EXT_COUNT] = wave_reduce((u64)a.v[EXT_COUNT], OpAdd());
    for (int s = EXT_HI_A; s <= EXT_LO_B; ++s)
        if (__ballot(a.v[s] != 0)) a.v[s] = wave_reduce((u64)a.v[s], OpMax());
    for (int s = EXT_SEC_A; s <= EXT_SEC_B; ++s)
        if (__ballot(a.v[s] != 0)) a.v[s] = wave_reduce((u64)a.v[s], OpOr());
}

// The label of lane's point and, when it is live, its coordinates: j = the instance, or -1.  `dead` counts in-range labels that are not live.
__device__ __forceinline__ int load_point(const double* __restrict__ pts, const int* __restrict__ labels, const double* __restrict__ frames,
                                          int K, int64_t n, int64_t i, ExtPoint& p, u64& dead)
{
    if (i >= n) return -1;
    const int l = labels[i];
    if (l < 0 || l >= K) return -1;
    if (ext_point(frames + (int64_t)l * kExtFrame, pts[3 * i], pts[3 * i + 1], pts[3 * i + 2], p)) return l;
    ++dead;
    return -1;
}

// No early return before the loop's ballots: `base` is the same for the whole workgroup, so every lane of a wave makes every trip.
template <bool kLds>
__global__ __launch_bounds__(kExtBlock) void extents_bounds_kernel(const double* __restrict__ pts, const int* __restrict__ labels,
                                                                   const double* __restrict__ frames, int K, int64_t n, u64* table,
                                                                   u64* skipped)
{
    __shared__ u64 lds[kLds ? kExtLdsK * EXT_SLOTS : 1];
    const int words = K * EXT_SLOTS;   // kLds: K <= kExtLdsK, the launcher's test
    if (kLds) {
        for (int w = threadIdx.x; w < words; w += kExtBlock) lds[w] = 0;
        __syncthreads();
    }
    AtomicTab tab{kLds ? lds : table};
    const int lane = threadIdx.x & (kExtWave - 1);
    u64 dead = 0;
    const int64_t stride = (int64_t)gridDim.x * kExtBlock;
    for (int64_t base = (int64_t)blockIdx.x * kExtBlock; base < n; base += stride) {
        ExtPoint p;
        const int j = load_point(pts, labels, frames, K, n, base + threadIdx.x, p, dead);
        const u64 alive = __ballot(j >= 0);
        if (!alive) continue;
        ExtAcc a;
        if (j >= 0) a = ext_contribution(p);
        else
            for (int s = 0; s < EXT_SLOTS; ++s) a.v[s] = 0;
        const int lead = __ffsll((long long)alive) - 1;
        const int j0 = __shfl(j, lead, kExtWave);
        if (__ballot(j == j0) == alive && __popcll(alive) > 1) {   // one row for the whole wave
            wave_combine(a);
            if (lane == lead) ext_merge(tab, j0, a);
        } else if (j >= 0) {
            ext_merge(tab, j, a);
        }
    }
    dead = wave_reduce(dead, OpAdd());
    if (lane == 0 && dead) atomicAdd(skipped, dead);
    if (kLds) {
        __syncthreads();
        AtomicTab out{table};
        for (int w = threadIdx.x; w < words; w += kExtBlock) ext_merge_word(out, w, lds[w]);
    }
}

__global__ __launch_bounds__(kExtBlock) void extents_finalise_kernel(int K, const u64* __restrict__ table, long long* __restrict__ count,
                                                                     double* __restrict__ lo, double* __restrict__ hi,
                                                                     u64* __restrict__ sectors)
{
    const int j = blockIdx.x * kExtBlock + threadIdx.x;
    if (j >= K) return;
    uint64_t row[EXT_SLOTS];
    for (int s = 0; s < EXT_SLOTS; ++s) row[s] = table[(int64_t)j * EXT_SLOTS + s];
    double l[2], h[2];
    ext_finalise(row, l, h);
    count[j] = (long long)row[EXT_COUNT];
    for (int w = 0; w < 2; ++w) {
        lo[2 * j + w] = l[w];
        hi[2 * j + w] = h[w];
        sectors[2 * j + w] = row[EXT_SEC_A + w];
    }
}

template <bool kLds>
__global__ __launch_bounds__(kExtBlock) void extents_occupancy_kernel(const double* __restrict__ pts, const int* __restrict__ labels,
                                                                      const double* __restrict__ frames, int K, int64_t n,
                                                                      const double* __restrict__ lo, const double* __restrict__ hi, u64* occ)
{
    __shared__ u64 lds[kLds ? kExtLdsK : 1];
    if (kLds) {
        for (int w = threadIdx.x; w < K; w += kExtBlock) lds[w] = 0;
        __syncthreads();
    }
    u64* const tab = kLds ? lds : occ;
    const int lane = threadIdx.x & (kExtWave - 1);
    u64 dead = 0;   // counted by the bounds launch
    const int64_t stride = (int64_t)gridDim.x * kExtBlock;
    for (int64_t base = (int64_t)blockIdx.x * kExtBlock; base < n; base += stride) {
        ExtPoint p;
        const int j = load_point(pts, labels, frames, K, n, base + threadIdx.x, p, dead);
        const u64 alive = __ballot(j >= 0);
        if (!alive) continue;
        u64 bit = 0;
        if (j >= 0) bit = ext_occupancy_bit(p, lo + 2 * (int64_t)j, hi + 2 * (int64_t)j);
        const int lead = __ffsll((long long)alive) - 1;
        const int j0 = __shfl(j, lead, kExtWave);
        if (__ballot(j == j0) == alive && __popcll(alive) > 1) {
            bit = wave_reduce(bit, OpOr());
            if (lane == lead) atomicOr(tab + j0, bit);
        } else if (j >= 0) {
            atomicOr(tab + j, bit);
        }
    }
    if (kLds) {
        __syncthreads();
        for (int w = threadIdx.x; w < K; w += kExtBlock)
            if (lds[w]) atomicOr(occ + w, lds[w]);
    }
}

inline size_t pad256(size_t bytes) { return (bytes + 255) & ~(size_t)255; }

}  // namespace

int instance_extents_launch(pgx_ctx* ctx, const double* points, int64_t n, const int32_t* labels, const double* frames, int32_t K,
                            int64_t* count_out, double* lo_out, double* hi_out, uint64_t* sectors_out, uint64_t* occupancy_out,
                            int64_t* skipped)
{
    if (n < 0) return fail(ctx, PGX_ERR_INVALID, "pgx_instance_extents: n = %lld", (long long)n);
    if (K < 0) return fail(ctx, PGX_ERR_INVALID, "pgx_instance_extents: K = %d", (int)K);
    if (K > PGX_EXTENTS_MAX_INSTANCES)
        return fail(ctx, PGX_ERR_INVALID, "pgx_instance_extents: %d instances, at most %d", (int)K, (int)PGX_EXTENTS_MAX_INSTANCES);
    if (!skipped) return fail(ctx, PGX_ERR_INVALID, "pgx_instance_extents: NULL argument");
    if (K > 0 && (!frames || !count_out || !lo_out || !hi_out || !sectors_out || !occupancy_out))
        return fail(ctx, PGX_ERR_INVALID, "pgx_instance_extents: NULL argument");
    if (n > 0 && (!points || !labels)) return fail(ctx, PGX_ERR_INVALID, "pgx_instance_extents: NULL argument");
    *skipped = 0;
    if (K == 0) return PGX_OK;   // no label is in range
    if (n == 0) {
        for (int32_t j = 0; j < K; ++j) {
            count_out[j] = 0;
            occupancy_out[j] = 0;
            for (int w = 0; w < 2; ++w) {
                lo_out[2 * j + w] = __builtin_inf();
                hi_out[2 * j + w] = -__builtin_inf();
                sectors_out[2 * j + w] = 0;
            }
        }
        return PGX_OK;
    }
    // the call's own buffer (nothing resident is touched): points | labels | frames | zeroed: table, occupancy, skipped | count | lo | hi |
    // sectors - each from a 256-byte boundary
    const size_t b_pts = pad256((size_t)n * 3 * sizeof(double)), b_lab = pad256((size_t)n * sizeof(int32_t));
    const size_t b_frm = pad256((size_t)K * kExtFrame * sizeof(double));
    const size_t zero_bytes = ((size_t)K * EXT_SLOTS + (size_t)K + 1) * sizeof(u64), b_zero = pad256(zero_bytes);
    const size_t b_one = pad256((size_t)K * sizeof(u64)), b_two = pad256((size_t)K * 2 * sizeof(u64));
    PGX_TRY(ensure(ctx, ctx->ext_buf, b_pts + b_lab + b_frm + b_zero + b_one + 3 * b_two));
    char* base = (char*)ctx->ext_buf.p;
    double* d_pts = (double*)base;
    int* d_lab = (int*)(base + b_pts);
    double* d_frm = (double*)(base + b_pts + b_lab);
    u64* d_table = (u64*)(base + b_pts + b_lab + b_frm);
    u64* d_occ = d_table + (size_t)K * EXT_SLOTS;
    u64* d_skip = d_occ + K;
    char* out = base + b_pts + b_lab + b_frm + b_zero;
    long long* d_count = (long long*)out;
    double* d_lo = (double*)(out + b_one);
    double* d_hi = (double*)(out + b_one + b_two);
    u64* d_sec = (u64*)(out + b_one + 2 * b_two);
    PGX_HIP(ctx, hipMemcpyAsync(d_pts, points, (size_t)n * 3 * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    PGX_HIP(ctx, hipMemcpyAsync(d_lab, labels, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    PGX_HIP(ctx, hipMemcpyAsync(d_frm, frames, (size_t)K * kExtFrame * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    PGX_HIP(ctx, hipMemsetAsync(d_table, 0, zero_bytes, ctx->stream));
    const int64_t need = (n + kExtBlock - 1) / kExtBlock;
    const dim3 block(kExtBlock), grid((unsigned)(need < kExtMaxBlocks ? need : kExtMaxBlocks)), gridK((unsigned)((K + kExtBlock - 1) / kExtBlock));
    const bool lds = K <= kExtLdsK;
    if (lds) hipLaunchKernelGGL(extents_bounds_kernel<true>, grid, block, 0, ctx->stream, d_pts, d_lab, d_frm, (int)K, n, d_table, d_skip);
    else hipLaunchKernelGGL(extents_bounds_kernel<false>, grid, block, 0, ctx->stream, d_pts, d_lab, d_frm, (int)K, n, d_table, d_skip);
    PGX_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(extents_finalise_kernel, gridK, block, 0, ctx->stream, (int)K, d_table, d_count, d_lo, d_hi, d_sec);
    PGX_HIP(ctx, hipGetLastError());
    if (lds) hipLaunchKernelGGL(extents_occupancy_kernel<true>, grid, block, 0, ctx->stream, d_pts, d_lab, d_frm, (int)K, n, d_lo, d_hi, d_occ);
    else hipLaunchKernelGGL(extents_occupancy_kernel<false>, grid, block, 0, ctx->stream, d_pts, d_lab, d_frm, (int)K, n, d_lo, d_hi, d_occ);
    PGX_HIP(ctx, hipGetLastError());
    u64 dead = 0;
    PGX_TRY(d2h(ctx, count_out, d_count, (size_t)K * sizeof(int64_t)));
    PGX_TRY(d2h(ctx, lo_out, d_lo, (size_t)K * 2 * sizeof(double)));
    PGX_TRY(d2h(ctx, hi_out, d_hi, (size_t)K * 2 * sizeof(double)));
    PGX_TRY(d2h(ctx, sectors_out, d_sec, (size_t)K * 2 * sizeof(uint64_t)));
    PGX_TRY(d2h(ctx, occupancy_out, d_occ, (size_t)K * sizeof(uint64_t)));
    PGX_TRY(d2h(ctx, &dead, d_skip, sizeof(dead)));
    PGX_TRY(sync_deliver(ctx));
    *skipped = (int64_t)dead;
    return PGX_OK;
}

}  // namespace pgx
