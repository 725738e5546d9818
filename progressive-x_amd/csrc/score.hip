// score.hip — batched MSAC-with-compound-model scoring of M hypotheses over N points (gfx950).
//
// Replaces: progx::MSACScoringFunctionWithCompoundModel::getScore,
//           /root/reference/src/pyprogressivex/include/scoring_function_with_compound_model.h:61-125,
//           called once per hypothesis by the GC-RANSAC proposal loop (progressive_x.h:294).
//
// Mapping: ONE HYPOTHESIS PER LANE, points streamed through the scalar unit.
//   * a lane keeps its hypothesis (3..18 doubles) in VGPRs for the whole kernel;
//   * the point row (2..5 doubles) is wave-uniform, so it is fetched with s_load into SGPRs and used as the
//     scalar operand of v_mul_f64/v_add_f64 — no LDS, no cross-lane traffic, no per-pair reduction;
//   * inlier count / truncated-quadratic score / shared support accumulate in registers of the owning lane;
//   * grid = (ceil(M/256) hypothesis groups) x (point chunks); every block writes one partial triple per
//     hypothesis, a second tiny kernel adds the chunk partials in a fixed order (bit-reproducible run to run,
//     which keeps multi-GPU replicas identical without communication).
// The kernel is FP64-VALU bound (≈0.02 algorithmic bytes per pair); MFMA is deliberately unused: there is no
// dense contraction, every pair is a projective map + divide + compare.
#include <cmath>
#include <cstdlib>

#include "pgx_internal.h"
#include "score_filters.hip.h"
#include "score_runs.h"

namespace pgx {

// (kScoreBlock = 256, hypotheses per workgroup of the chunked kernel: score_plan.h)

// FILT: 0 = no filter, 1 = FP64 filter, 2 = FP32 pre-filter
template <int MT, bool MASK, int FILT>
__global__ __launch_bounds__(kScoreBlock) void score_kernel(
    const double* __restrict__ pts, int64_t n, const double* __restrict__ models, int M, int Mpad,
    double T2, const double* __restrict__ comp, int has_comp, int64_t chunk,
    const double* __restrict__ pmax, double guard, const float* __restrict__ pts32, double guard32,
    unsigned* __restrict__ pcnt, double* __restrict__ pval, double* __restrict__ psh,
    unsigned long long* __restrict__ masks, int64_t words, const int* __restrict__ perm, int chunks, int xcd_map,
    const float* __restrict__ gbounds)
{
    using R = Residual<MT>;
    // (hypothesis group, point chunk) of this block.  Workgroups are handed to the 8 XCDs round-robin by linear id and
    // every XCD has its own L2: with the plain 2-D grid (group fastest, 8 groups) XCD x ran group x over ALL chunks,
    // i.e. every XCD streamed the whole point set from HBM (PMC: ~1.3 GB fetched per launch for ~0.09 GB of inputs).
    // The 1-D mapping below gives each XCD its own chunks and runs the groups of one chunk back to back on it.
    int gx = (int)blockIdx.x, gy = (int)blockIdx.y;
    if (xcd_map) {
        const int groups = Mpad / kScoreBlock;
        const int slot = (int)(blockIdx.x >> 3);
        gx = slot % groups;
        gy = (int)(blockIdx.x & 7u) + 8 * (slot / groups);
        if (gy >= chunks) return;
    }
    const int m = gx * kScoreBlock + threadIdx.x;
    const bool live = m < M;
    const int64_t i0 = (int64_t)gy * chunk;
    const int64_t i1 = (i0 + chunk < n) ? (i0 + chunk) : n;

    double mdl[R::P];
#pragma unroll
    for (int k = 0; k < R::P; ++k)
        mdl[k] = live ? models[(int64_t)m * R::P + k] : __builtin_nan("");  // NaN model: never an inlier

    using F = Filter<MT>;
    using F32 = Filter32<MT>;
    const typename F::Lane flane = F::prep(mdl, guard);
    const typename F32::Lane flane32 = F32::prep(mdl, guard32, T2);
    const double T2d = T2 * (1.0 + kFilterDelta);
    const float T2d32 = f32_up(T2 * (1.0 + kFilter32Delta));
    const float Tup32 = f32_up(sqrt(T2) * (1.0 + 1.0 / 64.0));  // group test

    unsigned cnt = 0;
    double val = 0.0, sh = 0.0;
    unsigned long long word = 0;
    const double kappa = oriented_kappa<MT>(pts, n);   // (an oriented type's normals and kappa lie behind its rows: residuals.hip.h)

    // One point per step; the body is written once and instantiated for a group of kUnroll points whose scalar loads
    // are all issued before the first use, so one s_waitcnt covers kUnroll points (SMEM returns out of order: the
    // only usable wait is lgkmcnt(0), which makes per-point prefetching impossible).
    auto step = [&](int64_t i, const double (&pt)[R::D], const Normal<MT>& nr, double pm, const float* p32) {
        bool inl = false;
        bool rejected = false;
        if (FILT == 1 && F::enabled) rejected = F::reject(pt, mdl, flane, pm, T2d);
        if (FILT == 2 && F32::enabled) rejected = F32::reject(p32, flane32, T2d32);
        if (live && !rejected) {  // exact path: oracle operation order, no contraction
            const double sq = squared_at<MT>(pt, nr, mdl, T2, kappa);
            inl = sq < T2;  // strict, scoring_function_with_compound_model.h:85
            if (inl) {
                ++cnt;                                        // :91
                const double s = cv_max(0.0, 1.0 - sq / T2);  // :94
                val += s;                                     // :97
                if (has_comp) sh += cv_min(comp[i], s);       // :115-117 (pref = 0 for non-inliers adds +0)
            }
        }
        if (MASK) {
            word |= (unsigned long long)(inl ? 1 : 0) << (i & 63);
            if ((i & 63) == 63 || i == i1 - 1) {
                if (live) masks[(int64_t)perm[m] * words + (i >> 6)] = word;  // :88 inlier list as a bit mask (row = caller's index)
                word = 0;
            }
        }
    };
    constexpr int kUnroll = 4;
    int64_t i = i0;
    while (i < i1) {
        // one 64-point group at a time (chunks start at multiples of 64)
        const int64_t gend = ((i | 63) + 1 < i1) ? (i | 63) + 1 : i1;
        if (FILT == 2 && F32::enabled && gbounds != nullptr) {
            const float* __restrict__ g = gbounds + (i >> 6) * kGroupRow;  // wave-uniform -> scalar loads
            float gr[kGroupRow];
#pragma unroll
            for (int k = 0; k < 9; ++k) gr[k] = g[k];
            const bool keep = live && !F32::group_reject(gr, flane32, Tup32);
            if (__ballot(keep) == 0) {  // none of this wave's hypotheses can have an inlier in the group
                if (MASK && live) masks[(int64_t)perm[m] * words + (i >> 6)] = 0;
                i = gend;
                continue;
            }
        }
        for (; i + kUnroll <= gend; i += kUnroll) {
            const double* __restrict__ prow = pts + i * R::D;  // wave-uniform address -> scalar loads
            double pt[kUnroll][R::D];
            Normal<MT> nr[kUnroll];
            double pm[kUnroll];
            float p32[kUnroll][8];
#pragma unroll
            for (int u = 0; u < kUnroll; ++u) {
#pragma unroll
                for (int k = 0; k < R::D; ++k) pt[u][k] = prow[u * R::D + k];
                nr[u] = load_normal<MT>(pts, n, i + u);   // wave-uniform as well
                pm[u] = (FILT == 1 && F::enabled) ? pmax[i + u] : 1.0;
                if (FILT == 2 && F32::enabled) {
#pragma unroll
                    for (int k = 0; k < 8; ++k) p32[u][k] = pts32[(i + u) * 8 + k];
                }
            }
#pragma unroll
            for (int u = 0; u < kUnroll; ++u) step(i + u, pt[u], nr[u], pm[u], p32[u]);
        }
        for (; i < gend; ++i) {
            const double* __restrict__ prow = pts + i * R::D;
            double pt[R::D];
            float p32[8];
#pragma unroll
            for (int k = 0; k < R::D; ++k) pt[k] = prow[k];
            if (FILT == 2 && F32::enabled) {
#pragma unroll
                for (int k = 0; k < 8; ++k) p32[k] = pts32[i * 8 + k];
            }
            step(i, pt, load_normal<MT>(pts, n, i), (FILT == 1 && F::enabled) ? pmax[i] : 1.0, p32);
        }
    }
    const int64_t o = (int64_t)gy * Mpad + m;
    pcnt[o] = cnt;
    pval[o] = val;
    psh[o] = sh;
}

// ---- cull, then score group-major ------------------------------------------------------------------
// Skipping rejected groups inside the chunked kernel needs a whole wave of 64 hypotheses to agree (74 % of the (wave,
// group) pairs) although 93 % of the (hypothesis, group) pairs are rejected, and leaves the surviving work badly
// distributed (instructions 39 %, time 65 %); scoring the survivors hypothesis-major still runs the pre-filter for 64
// hypotheses at a time and the FP64 exact path with ~3 of 64 lanes busy (the union of the wave's candidates).  So the
// surviving pairs are scored the other way round:
//   score_cull_kernel   one wave per (64 hypotheses, segment of groups): the group test; bit h of keep[g][w] = hypothesis
//                       64 w + h may have inliers in group g.  Also stores every hypothesis' f32 filter constants.
//   score_group_kernel  one wave per GROUP, one point per lane (rows loaded once, coalesced); the surviving hypotheses
//                       stream through the scalar unit: 17-op pre-filter for 64 points, then the exact FP64 path with
//                       the group's actual candidates as active lanes; per (hypothesis, group): count = popcount, the
//                       two sums by a fixed shuffle tree, added to the hypothesis' accumulators as integers (count) and
//                       as 2^-q fixed point (sums) with integer atomics: exact and order-free, so results are
//                       bit-reproducible although the accumulation order is not fixed.  q = 62 - ceil(log2 n): the
//                       quantisation error of a sum is < (#groups with inliers) * 2^-(q+1), ~1e-13 relative.
//   score_finish_kernel accumulators -> counts / values / shared in the caller's hypothesis order.
// Three independent trims of the group-major kernel, each behind one bit so that two builds of the library can be compared
// (make EXTRA=-DPGX_SCORE_TRIM=<mask>; docs/lab-notebook.md, "Trimming the group-major step loop"):
//   1  a hypothesis' row holds the staged form only (StagedVals: the floats reject() reads) instead of the whole lane
//   2  drain() carries count and value in one word and takes the run boundaries from one head mask (score_runs.h)
//   4  direct() leaves out the tree and the atomic of the shared sum when no lane shares anything with the compound instance
// Four more, of the way into the step loop and of the filter step (docs/lab-notebook.md, "A shorter prologue and filter step").  Only
// 64 is on by default: the three prologue bits take the dependent memory round trips before the first step from about 14 to 5 and
// measured nothing (the other waves of the SIMD hide them) - they stay for the next A/B.
//   8   a listed workgroup fetches its XCD's four counts in one round trip and finds its (class, position) by selects
//       (wl_locate_select) - wl_locate's early exits let the loads sink into its branches, one round trip each
//   16  the kernel arguments are all requested right after entry: one batch instead of five lazy ones
//   32  what the item determines is requested together: its (up to) four keep words, the point rows, the compound value
//   64  the filter runs in every lane and the tail group's lanes beyond n are taken out of the ballot by one mask computed once:
//       no exec region around the filter in every step, no bool between the comparison and the ballot, and a lane's candidate flag
//       is its bit of the surviving mask as it stands
// Four of the cull kernel, all on (docs/lab-notebook.md, "Cull kernel: keep words per tile, one generation, a shorter way in"):
//   128 a wave keeps the tile's keep words in registers - lane i holds the word of group t0 + i - and they are stored once per tile
//       instead of once per bound test (and once more per culled super-group); an item's weight is the popcount of its four words
//   256 the pose instances are held to 64 registers, 8 waves per SIMD: all 2 048 workgroups of the metric launch resident at once
//   512 the first tile's bound rows are requested together with the model and staged before the FP64 preparation (one barrier
//       instead of two dependent round trips), and a workgroup whose segment lies behind the last group leaves after its zeroing
//   1024 a bound row is read from LDS as a whole before its test begins: one LDS round trip per test instead of two dependent ones
#ifndef PGX_SCORE_TRIM
#define PGX_SCORE_TRIM 1991
#endif
constexpr bool kTrimRows = (PGX_SCORE_TRIM & 1) != 0, kTrimDrain = (PGX_SCORE_TRIM & 2) != 0, kTrimDirect = (PGX_SCORE_TRIM & 4) != 0;
constexpr bool kTrimLocate = (PGX_SCORE_TRIM & 8) != 0, kTrimArgs = (PGX_SCORE_TRIM & 16) != 0, kTrimItem = (PGX_SCORE_TRIM & 32) != 0,
               kTrimTail = (PGX_SCORE_TRIM & 64) != 0;
// An oriented type's normal in the group-major kernel (score_group_kernel): by default the lane loads it next to its point row and drain()
// shuffles it; with -DPGX_ORIENTED_GATHER a candidate's normal is gathered from the sorted copy on the exact path only.
#ifdef PGX_ORIENTED_GATHER
constexpr bool kOrientedGather = true;
#else
constexpr bool kOrientedGather = false;
#endif
constexpr bool kTrimKeepTile = (PGX_SCORE_TRIM & 128) != 0, kTrimResident = (PGX_SCORE_TRIM & 256) != 0, kTrimEarly = (PGX_SCORE_TRIM & 512) != 0,
               kTrimRowFirst = (PGX_SCORE_TRIM & 1024) != 0;

// A hypothesis' f32 constants as the cull kernel stores them (hyp32) and the group kernel stages them (LDS): the first kVals
// floats of Filter32<MT>::Lane in float4 chunks.  Rows of hyp32 are kStride floats apart - 16-byte aligned, 64 bytes for the pose
// family (14 floats: one cache-line sector per hypothesis).
template <int MT> struct HypRow {
    using LaneT = typename Filter32<MT>::Lane;
    static_assert(sizeof(LaneT) % sizeof(float) == 0, "Filter32 lane constants are floats");
    static constexpr int kLaneVals = (int)(sizeof(LaneT) / sizeof(float));
    static constexpr int kVals = kTrimRows ? StagedVals<Filter32<MT>>::value : kLaneVals;
    static_assert(kVals <= kLaneVals, "the staged form is a prefix of the lane");
    static constexpr int kChunks = (kVals + 3) / 4;
    static constexpr int kStride = 4 * kChunks;

    static __device__ __forceinline__ void store(const LaneT& ln, float* __restrict__ row)   // the cull kernel
    {
        const float* src = reinterpret_cast<const float*>(&ln);
#pragma unroll
        for (int k = 0; k < kVals; ++k) row[k] = src[k];
    }
    // The rest of the lane stays unset: reject() does not read it (StagedVals).
    static __device__ __forceinline__ LaneT load(const float* __restrict__ row)              // the verify kernel
    {
        LaneT ln;
        float* dst = reinterpret_cast<float*>(&ln);
#pragma unroll
        for (int k = 0; k < kVals; ++k) dst[k] = row[k];
        return ln;
    }
    // LDS image of a word's 64 hypotheses: [chunk][hypothesis][4].  The owning lanes write consecutive 16-byte slots (rows 80 bytes
    // apart collided on the banks), the step loop reads chunk c of hypothesis h at the same address in every lane.
    static __device__ __forceinline__ void stage(const float* __restrict__ row0, float (*lds)[64][4], int lane)
    {
        const float* __restrict__ row = static_cast<const float*>(__builtin_assume_aligned(row0, 16));
#pragma unroll
        for (int c = 0; c < kChunks; ++c) {
            if (4 * c + 4 <= kVals) {
                *reinterpret_cast<float4*>(&lds[c][lane][0]) = *reinterpret_cast<const float4*>(row + 4 * c);
            } else {
#pragma unroll
                for (int k = 0; k < kVals - 4 * c; ++k) lds[c][lane][k] = row[4 * c + k];
            }
        }
    }
    static __device__ __forceinline__ LaneT staged(const float (*lds)[64][4], int h)
    {
        LaneT ln;
        float* dst = reinterpret_cast<float*>(&ln);
#pragma unroll
        for (int c = 0; c < kChunks; ++c) {
            if (4 * c + 4 <= kVals) {
                const float4 v = *reinterpret_cast<const float4*>(&lds[c][h][0]);
                dst[4 * c] = v.x; dst[4 * c + 1] = v.y; dst[4 * c + 2] = v.z; dst[4 * c + 3] = v.w;
            } else {
#pragma unroll
                for (int k = 0; k < kVals - 4 * c; ++k) dst[4 * c + k] = lds[c][h][k];
            }
        }
        return ln;
    }
};

constexpr int kCullWaves = 4;   // hypothesis words (waves) per workgroup of the cull kernel
constexpr int kCullTile = 64;   // group bounds staged in LDS per step

// The group bounds of a segment are staged in LDS by the whole workgroup (coalesced vector loads, one round trip per 64
// groups) and read back as broadcasts: with scalar loads a wave paid one ~1 us scalar-cache miss per four groups, and the
// kernel took as long as that latency chain (43 us for 27 VALU instructions per test).
// (waves per SIMD: the budget the kernel had before it weighed items - 72 registers for the two 12-parameter filters, 64 for the rest;
// the compiler meets it without scratch, and left alone it gives a wave away on four of the nine types.  At 7 waves per SIMD a CU
// holds 7 workgroups and the chip 1 792: the metric launch - 2 048 workgroups, 1 960 of them with a tile - is NOT one generation of
// waves, its last 168 working workgroups start as others retire.  Bit 256 asks 8 of the pose instances.)
template <int MT> constexpr int kCullWavesPerSimd = ((MT == kPnP && !kTrimResident) || MT == kHomographySym) ? 7 : 8;
static_assert(kCullWaves == kWlItemWords && kCullTile * kGroupRow == 3 * 64 * kCullWaves && kCullTile / kSuper * kGroupRow <= 64 * kCullWaves,
              "an item is a workgroup's words; a tile's rows are three loads per thread, its super-group rows less than one");
// LISTS: also weigh the tile's (group, 4-word) items and append the non-empty ones to the work lists (without: the kernel as it was)
template <int MT, bool LISTS>
__global__ __launch_bounds__(64 * kCullWaves) __attribute__((amdgpu_waves_per_eu(kCullWavesPerSimd<MT>))) void score_cull_kernel(
    const double* __restrict__ models, int M, double T2, double guard32, const float* __restrict__ gbounds, int groups,
    int gps /* groups per segment */, int W, unsigned long long* __restrict__ keep, float* __restrict__ hyp32,
    double* __restrict__ models_t /* [P][W * 64]: component-major copy for the gathers of the group kernel */,
    unsigned long long* __restrict__ zero /* the accumulators of the group kernel, zeroed here (one fill command less) */, int64_t zero_words,
    unsigned* __restrict__ wl /* LISTS: the work lists of the group kernel, counts | items (score_worklist.h) */, int wl_xb, unsigned wl_cap,
    unsigned wl_t1, unsigned wl_t2, unsigned wl_t3)
{
    using R = Residual<MT>;
    using F32 = Filter32<MT>;
    __shared__ __attribute__((aligned(16))) float s_gb[kCullTile + kCullTile / kSuper][kGroupRow];  // groups | their super-groups
    // work lists: surviving steps per (word of this workgroup, group of the tile) - with bit 128 the keep words themselves, [group][word]
    __shared__ unsigned s_wt[(LISTS && !kTrimKeepTile) ? kCullWaves : 1][kCullTile];
    __shared__ __attribute__((aligned(16))) unsigned long long s_kw[(LISTS && kTrimKeepTile) ? kCullTile : 1][kCullWaves];
    {
        const int64_t nthreads = (int64_t)gridDim.x * gridDim.y * (64 * kCullWaves);
        for (int64_t i = ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * (64 * kCullWaves) + threadIdx.x; i < zero_words; i += nthreads) zero[i] = 0ull;
    }
    const int lane = (int)(threadIdx.x & 63);
    const int w = (int)blockIdx.x * kCullWaves + (int)(threadIdx.x >> 6), seg = (int)blockIdx.y;
    const int g0 = seg * gps, g1 = g0 + gps < groups ? g0 + gps : groups;
    // a segment behind the last group (the metric launch has 11 of 256) has no tile, and only segment 0 stores the hypotheses' rows
    if (kTrimEarly && seg != 0 && g0 >= groups) return;
    const int m = w * 64 + lane;
    const bool live = w < W && m < M;
    // T'' of the group test depends on the launch alone.  Bit 256: computed before anything is loaded and handed to the scalar unit,
    // so that its FP64 root is not in flight among the preparation's and it takes no vector register in the tile loop.
    float Tup32 = 0.0f;
    if constexpr (kTrimResident) Tup32 = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(f32_up(sqrt(T2) * (1.0 + 1.0 / 64.0)))));
    // Bit 512: a tile's rows as straight-line code - every thread requests its three floats of the group rows and its float of the
    // super-group rows under a clamped index instead of a loop bound (request), and writes them to LDS (commit); what a thread behind
    // the tile's rows writes is a copy of the last float, into a row no test reads.
    float rv[3], sv;
    auto request = [&](int t0, int cnt, int scnt) {
        const int last = cnt > 0 ? cnt * kGroupRow - 1 : 0, slast = scnt > 0 ? scnt * kGroupRow - 1 : 0;
        const float* __restrict__ rows = gbounds + (int64_t)t0 * kGroupRow;
        const float* __restrict__ srows = gbounds + ((int64_t)groups + t0 / kSuper) * kGroupRow;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int e = (int)threadIdx.x + k * 64 * kCullWaves;
            rv[k] = rows[e < last ? e : last];
        }
        sv = srows[(int)threadIdx.x < slast ? (int)threadIdx.x : slast];
    };
    auto commit = [&]() {
#pragma unroll
        for (int k = 0; k < 3; ++k) (&s_gb[0][0])[(int)threadIdx.x + k * 64 * kCullWaves] = rv[k];
        if (threadIdx.x < kCullTile / kSuper * kGroupRow) (&s_gb[kCullTile][0])[threadIdx.x] = sv;
    };
    // Bit 1024: the whole row is in registers before the test begins.  Left alone the compiler turns the test's three comparisons
    // into nested exec regions and sinks the reads of the row's second half into the second one: two dependent LDS round trips per
    // test, on the one chain the longest wave of the kernel is made of.  (Code motion only: the operations and their order stay.)
    auto row_first = [](float* row) {
        if constexpr (kTrimRowFirst) {
#pragma unroll
            for (int k = 0; k < F32::kGroupVals; ++k) asm volatile("" : "+v"(row[k]));
        }
    };
    double mdl[R::P];
    if constexpr (kTrimEarly) {
        // The first tile's rows do not depend on the model: requested together with it, they are in LDS before the FP64 preparation,
        // and one barrier behind it replaces two dependent round trips.  The model's loads are unconditional too (row 0 for a lane
        // behind M, which then takes its NaNs), so that nothing stands between the two requests.
        const double* __restrict__ row = models + (int64_t)(live ? m : 0) * R::P;
#pragma unroll
        for (int k = 0; k < R::P; ++k) mdl[k] = row[k];
        const int cnt = g1 - g0 < kCullTile ? g1 - g0 : kCullTile;
        request(g0, cnt, (cnt + kSuper - 1) / kSuper);
#pragma unroll
        for (int k = 0; k < R::P; ++k) mdl[k] = live ? mdl[k] : __builtin_nan("");
        if (seg == 0 && w < W) {
#pragma unroll
            for (int k = 0; k < R::P; ++k) models_t[(int64_t)k * W * 64 + m] = mdl[k];
        }
        commit();
    } else {
#pragma unroll
        for (int k = 0; k < R::P; ++k) mdl[k] = live ? models[(int64_t)m * R::P + k] : __builtin_nan("");
    }
    const typename F32::Lane flane32 = F32::prep(mdl, guard32, T2);
    if (seg == 0 && w < W) {
        HypRow<MT>::store(flane32, hyp32 + (int64_t)m * HypRow<MT>::kStride);
        if constexpr (!kTrimEarly) {
#pragma unroll
            for (int k = 0; k < R::P; ++k) models_t[(int64_t)k * W * 64 + m] = mdl[k];
        }
    }
    if constexpr (!kTrimResident) Tup32 = f32_up(sqrt(T2) * (1.0 + 1.0 / 64.0));
    for (int t0 = g0; t0 < g1; t0 += kCullTile) {
        const int cnt = g1 - t0 < kCullTile ? g1 - t0 : kCullTile;
        const int scnt = (cnt + kSuper - 1) / kSuper;  // t0 is a multiple of kSuper (gps is)
        if constexpr (kTrimEarly) {
            if (t0 != g0) {
                __syncthreads();  // the previous tile has been read
                request(t0, cnt, scnt);
                commit();
            }
        } else {
            __syncthreads();  // the previous tile has been read
            for (int e = (int)threadIdx.x; e < cnt * kGroupRow; e += 64 * kCullWaves)
                (&s_gb[0][0])[e] = gbounds[(int64_t)t0 * kGroupRow + e];
            for (int e = (int)threadIdx.x; e < scnt * kGroupRow; e += 64 * kCullWaves)
                (&s_gb[kCullTile][0])[e] = gbounds[((int64_t)groups + t0 / kSuper) * kGroupRow + e];
        }
        __syncthreads();
        unsigned steps = 0;   // work lists: lane i holds the surviving steps of (this wave's word, group t0 + i)
        unsigned long long kw = 0;       // bit 128: lane i holds the keep word of (group t0 + i, this wave's word); 0 where nothing was tested
        if (w < W)
            for (int sgi = 0; sgi < scnt; ++sgi) {
                const int i0 = sgi * kSuper, i1 = i0 + kSuper < cnt ? i0 + kSuper : cnt;
                float sr[kGroupRow];
#pragma unroll
                for (int k = 0; k < F32::kGroupVals; ++k) sr[k] = s_gb[kCullTile + sgi][k];  // same address in every lane: LDS broadcast
                row_first(sr);
                if (__ballot(live && !F32::group_reject(sr, flane32, Tup32)) == 0) {  // no hypothesis of the word reaches these 512 points
                    if (!kTrimKeepTile && lane < i1 - i0) keep[(int64_t)(t0 + i0 + lane) * W + w] = 0;
                    continue;
                }
                for (int i = i0; i < i1; ++i) {
                    float gr[kGroupRow];
#pragma unroll
                    for (int k = 0; k < F32::kGroupVals; ++k) gr[k] = s_gb[i][k];
                    row_first(gr);
                    const unsigned long long bm = __ballot(live && !F32::group_reject(gr, flane32, Tup32));
                    if constexpr (kTrimKeepTile) {
                        kw = lane == i ? bm : kw;
                    } else {
                        if (lane == 0) keep[(int64_t)(t0 + i) * W + w] = bm;
                        if (LISTS) steps = lane == i ? (unsigned)__popcll(bm) : steps;
                    }
                }
            }
        if constexpr (kTrimKeepTile && !LISTS) {
            if (w < W && lane < cnt) keep[(int64_t)(t0 + lane) * W + w] = kw;   // one store per wave and tile, from registers
        }
        if (!LISTS) continue;
        // ---- the tile's items (group t0 + i, this workgroup's words) onto the work lists: lane i of the first wave weighs item i -
        // the surviving steps of its live words - and the non-empty ones are appended to list [g & 7][class of the weight].  One
        // returning atomic per (XCD, class) pair that occurs in the tile: lanes with equal lane & 7 have equal g & 7, so the pair's
        // lanes are the class' ballot under one byte-lane mask; positions inside the pair's block follow from the lanes below.
        unsigned wt = 0;
        if constexpr (kTrimKeepTile) {
            // the four waves' words meet in LDS; behind the barrier every thread stores one word of the tile (four neighbouring lanes
            // an item's 32 bytes), and an item's weight is the popcount of its words - zero for a wave past W or a lane past cnt
            s_kw[lane][threadIdx.x >> 6] = kw;
            __syncthreads();
            const int64_t at = wl_tile_store_index((int)threadIdx.x, t0, cnt, (int)blockIdx.x, W);
            if (at >= 0) keep[at] = s_kw[threadIdx.x / kCullWaves][threadIdx.x % kCullWaves];
            if (threadIdx.x >= 64) continue;
#pragma unroll
            for (int v = 0; v < kCullWaves; ++v) wt += (unsigned)__popcll(s_kw[lane][v]);
        } else {
            s_wt[threadIdx.x >> 6][lane] = steps;
            __syncthreads();
            if (threadIdx.x >= 64) continue;
            const int nlive = W - (int)blockIdx.x * kCullWaves < kCullWaves ? W - (int)blockIdx.x * kCullWaves : kCullWaves;
            if (lane < cnt)
                for (int v = 0; v < nlive; ++v) wt += s_wt[v][lane];
        }
        const int cls = wt != 0 ? wl_class(wt, wl_t1, wl_t2, wl_t3) : -1;
        unsigned long long mine = 0;   // the lanes of this lane's (XCD, class) pair
#pragma unroll
        for (int c = 0; c < kWlClasses; ++c) {
            const unsigned long long bc = __ballot(cls == c);
            if (cls == c) mine = bc & (0x0101010101010101ull << (lane & 7));
        }
        const int first = cls >= 0 ? __builtin_ctzll(mine) : lane;
        const unsigned g = (unsigned)(t0 + lane);
        const int list = (int)(g & 7u) * kWlClasses + (cls >= 0 ? cls : 0);
        unsigned base = 0;
        if (cls >= 0 && lane == first) base = atomicAdd(&wl[list * kWlCountStride], (unsigned)__popcll(mine));
        base = (unsigned)__shfl((int)base, first, 64);
        if (cls >= 0) {
            const unsigned pos = base + __builtin_amdgcn_mbcnt_hi((unsigned)(mine >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mine, 0u));
            if (pos < wl_cap)   // (always: a list holds every item of its XCD's groups, and the counts start from zero)
                wl[kWlCountWords + (size_t)list * wl_cap + pos] = wl_item(g, blockIdx.x, wl_xb);
        }
    }
}

// round-to-nearest-even of 0 <= x < 2^51 as an integer: one FP64 add against 1.5 * 2^52 and an integer subtraction (the
// generic double -> int64 conversion is ~20 instructions and ran twice per evaluated pair)
__device__ __forceinline__ long long to_fixed(double x)
{
    const double magic = 6755399441055744.0;
    return __double_as_longlong(x + magic) - __double_as_longlong(magic);
}

constexpr int kGroupWaves = 1;  // waves per workgroup of the group-major kernel

template <int MT, bool MASK, bool STATS = false>
__global__ __launch_bounds__(64 * kGroupWaves) void score_group_kernel(
    const double* __restrict__ pts, const float* __restrict__ pts32, const double* __restrict__ comp, int64_t n, int groups,
    const double* __restrict__ models, int W, double T2, int has_comp, const unsigned long long* __restrict__ keep,
    const float* __restrict__ hyp32, double qscale, unsigned long long* __restrict__ acc /* [3][Mpad]: count, value, shared */,
    int Mpad, unsigned long long* __restrict__ masks, int64_t words, const int* __restrict__ perm, int split, int xcd_local, const double* __restrict__ models_t,
    unsigned long long* __restrict__ stats /* STATS: [0] surviving (hypothesis, group) steps, [1] exact evaluations, [2] inlier pairs */,
    const double* __restrict__ pts_g /* [groups][D][64]: group-blocked SoA copy of the rows (nullptr: AoS) */,
    const float* __restrict__ p32_g /* [groups][8][64] */, int nrep, int dense_min,
    const unsigned* __restrict__ wl /* the cull kernel's work lists (score_worklist.h), or nullptr: (group, part) from the workgroup id */,
    int wl_xb, unsigned wl_cap)
{
    // split: waves per group, each takes every split-th word of 64 hypotheses (shorter waves: better tail)
    // Work lists: workgroup b takes item b >> 3 of the lists of XCD b & 7 instead, the heaviest class first - a group and 4 adjacent
    // words - and walks exactly the non-empty words the parts would have walked: the same steps, the same integers.  The grid is the
    // lists' worst case; a workgroup past its XCD's total leaves after four scalar loads, and those come last in dispatch order.
    using R = Residual<MT>;
    using F32 = Filter32<MT>;
    using LaneT = typename F32::Lane;
    using Row = HypRow<MT>;
    const int lane = (int)(threadIdx.x & 63);
    // One item (group, part) per wave, one wave per workgroup.  Measured alternatives at M = 2048, N = 1e6: 4-wave workgroups
    // (a workgroup retires with its slowest wave; 0.32 ms), 2-wave (0.30), persistent waves striding over the items
    // (0.31-0.38), workgroups that hand out 8-64 items to their 4 waves from an LDS counter (0.29-0.32), placing a
    // group's workgroups on one XCD (FETCH_SIZE 165 -> 45 MiB but 0.51 ms); one wave per workgroup with 8 parts per
    // group: 0.28 ms (16 parts: 250 k workgroups, the dispatcher limits at ~1.3 ns per workgroup).
    const int wv = 0;
    if constexpr (kTrimArgs) {
        // Left alone the compiler fetches an argument where it is first used: a listed wave waited for five batches of them, one
        // after the other, between its entry and its first step.  One empty statement that every path needs the result of (W, groups)
        // and that reads the others makes them one batch of scalar loads.  Not volatile: a statement with side effects counts as a
        // store, and the uniform loads behind it (counts, item, keep words) would leave the scalar unit.  keep and wl are not named:
        // a pointer an asm statement has seen counts as escaped, its loads inside the word loop could then alias the atomics and
        // would leave the scalar unit as well; they sit between named arguments and arrive with them.
        asm("" : "+s"(W), "+s"(groups) : "s"(wl_xb), "s"(wl_cap), "s"(n), "s"(pts_g), "s"(p32_g), "s"(pts), "s"(pts32),
            "s"(comp), "s"(has_comp), "s"(nrep), "s"(acc), "s"(Mpad), "s"(hyp32), "s"(dense_min), "s"(models), "s"(models_t), "s"(T2), "s"(qscale), "s"(split), "s"(xcd_local));
    }
    int g, w0, w1 = W, wstep = 1;   // this wave's words of group g: w0, w0 + wstep, ... below w1
    if (wl != nullptr) {
        const int xcd = (int)(blockIdx.x & 7u);
        unsigned lc[kWlClasses];
#pragma unroll
        for (int c = 0; c < kWlClasses; ++c) lc[c] = wl[wl_count_index(xcd, c)];   // wave-uniform -> scalar loads
        int cls;
        unsigned pos;
        if constexpr (kTrimLocate) {
            // all four counts are in registers before the first is looked at: one round trip, and a workgroup past its lists leaves
            // after it.  (The never-taken guard on the position shares the exit.)
            asm("" : "+s"(lc[0]), "+s"(lc[1]), "+s"(lc[2]), "+s"(lc[3]));
            const bool found = wl_locate_select(lc[0], lc[1], lc[2], lc[3], blockIdx.x >> 3, &cls, &pos);
            if (!found | (pos >= wl_cap)) return;
        } else {
            if (!wl_locate(lc[0], lc[1], lc[2], lc[3], blockIdx.x >> 3, &cls, &pos)) return;   // past this XCD's lists
            if (pos >= wl_cap) return;            // (never: a list holds at most its XCD's items)
        }
        const unsigned item = wl[kWlCountWords + (size_t)(xcd * kWlClasses + cls) * wl_cap + pos];
        if (wl_item_group(item, wl_xb) >= (unsigned)groups || wl_item_column(item, wl_xb) * kWlItemWords >= (unsigned)W) return;   // (never either)
        g = (int)wl_item_group(item, wl_xb);
        w0 = (int)wl_item_column(item, wl_xb) * kWlItemWords;
        w1 = w0 + kWlItemWords < W ? w0 + kWlItemWords : W;
    } else {
        if (xcd_local) {  // workgroup ids go round-robin over the 8 XCDs: all parts of a group on one XCD (its L2 fetches the rows once)
            const int slot = (int)(blockIdx.x >> 3);
            g = (slot / split) * 8 + (int)(blockIdx.x & 7u);
            w0 = slot % split;
            if (g >= groups) return;
        } else {
            g = (int)blockIdx.x / split;
            w0 = (int)blockIdx.x % split;
        }
        wstep = split;
        // nothing survived the cull for this wave's hypotheses: leave before the point rows are requested (a listed item has survivors)
        unsigned long long any = 0;
        for (int w = w0; w < W; w += split) any |= keep[(int64_t)g * W + w];
        if (any == 0) return;
    }
    g = __builtin_amdgcn_readfirstlane(g);
    w0 = __builtin_amdgcn_readfirstlane(w0);
    w1 = __builtin_amdgcn_readfirstlane(w1);
    const int64_t j = (int64_t)g * 64 + lane;
    const bool valid = j < n;
    const int64_t jj = valid ? j : n - 1;
    // Lanes at or past n exist in the last group only and hold a COPY OF THE LAST POINT on both layouts (AoS: row jj = n - 1; SoA: the
    // tail group is padded with its last row), so their filter arithmetic is that of a real row.  kTrimTail relies on it: the filter
    // runs in every lane and these lanes are taken out of each step's ballot by valid_mask.
    const unsigned long long valid_mask = __ballot(valid);
    // kTrimItem: a listed item's keep words (adjacent: w0 .. w0 + 3), its point rows and its compound value are requested together
    // here - one memory round trip; the word loop takes its words from registers.  The four words are ONE 32-byte scalar load
    // (four loads share their address registers and wait for each other) that stays inside the group's row, also where the row's
    // last item is short (score_worklist.h wl_words_begin / wl_words_shift): a word at or past W is 0 and is never read.  Rows
    // shorter than one item (W < 4) keep the word loop's own loads.
    static_assert(kWlItemWords == 4, "the item's keep words are one 4-word load");
    typedef unsigned long long keep4_t __attribute__((ext_vector_type(4), aligned(8)));
    const bool item_words = kTrimItem && wl != nullptr && W >= kWlItemWords;
    uint64_t kw[kWlItemWords] = {};
    double cmp = 0.0;
    const int kwb = wl_words_begin(w0, W);   // (wave-uniform)
    keep4_t kwv = {};
    if (item_words) kwv = *reinterpret_cast<const keep4_t*>(keep + (int64_t)g * W + kwb);   // wave-uniform -> one scalar load
    if (kTrimItem && has_comp) cmp = comp[jj];   // (ahead of the rows: its address and value in registers of their own)
    double pt[R::D];
    float p32[8];
    if (pts_g != nullptr) {
        // group-blocked SoA copies: every load instruction of the wave reads one contiguous 512 B (256 B) run instead of 64
        // rows 40 B (32 B) apart - 13 loads touch 17 cache lines instead of ~100 (the tail group is padded with its last row)
#pragma unroll
        for (int q = 0; q < R::D; ++q) pt[q] = pts_g[((int64_t)g * R::D + q) * 64 + lane];
#pragma unroll
        for (int q = 0; q < 8; ++q) p32[q] = 0.0f;
        if constexpr (R::in1 >= R::in0) {
            // the generic f32 row (sp_prep_kernel) recomputed from the f64 row just loaded - the same operations, the same bits -
            // instead of a second 24-byte row per point from memory (24 MB of 89 fetched per launch at 10^6 points)
#pragma unroll
            for (int q = 0; q < R::D; ++q) p32[q] = (float)pt[q];
            double pm = 1.0;
#pragma unroll
            for (int q = R::in0; q <= R::in1; ++q) { const double a = fabs(pt[q]); if (!(a <= pm)) pm = a; }
            p32[5] = (float)(pm * 1.000001);
        } else {
#pragma unroll
            for (int q = 0; q < F32::kRowVals; ++q) p32[q] = p32_g[((int64_t)g * 8 + q) * 64 + lane];
        }
    } else {
#pragma unroll
        for (int q = 0; q < R::D; ++q) pt[q] = pts[jj * R::D + q];
#pragma unroll
        for (int q = 0; q < 8; ++q) p32[q] = pts32[jj * 8 + q];
    }
    // An oriented type (residuals.hip.h): the lane's normal next to its row, from the copy its row came from - the tail group's lanes at
    // or past n see the last point's normal, as they see its row - and kappa from behind the same copy.  drain() shuffles the normal
    // with the row.  (The other design, a gather of the candidate's normal from the sorted copy inside drain() and direct():
    // -DPGX_ORIENTED_GATHER, docs/lab-notebook.md "Oriented primitives: where the group-major kernel takes the normal from".)
    Normal<MT> nrm;
    double kappa = 0.0;
    if constexpr (kOriented<MT>) {
        if (pts_g != nullptr) {
            kappa = oriented_kappa<MT>(pts_g, (int64_t)groups * 64);
            if constexpr (!kOrientedGather) nrm = load_normal_blocked<MT>(pts_g, groups, g, lane);
        } else {
            kappa = oriented_kappa<MT>(pts, n);
            if constexpr (!kOrientedGather) nrm = load_normal<MT>(pts, n, jj);
        }
    }
    if (!kTrimItem && has_comp) cmp = comp[jj];
    if (item_words) wl_words_shift(kwv.x, kwv.y, kwv.z, kwv.w, w0 - kwb, kw);   // (first use of the keep words: behind the requests for the rows)
    // nrep replicas of the integer accumulators, chosen by workgroup id: workgroup ids go round-robin over the XCDs, so with
    // nrep a multiple of 8 a replica is only ever updated from one XCD (its atomics stay in that L2), and the hot
    // hypotheses (thousands of updates) do not serialise on three addresses.  score_finish_kernel adds the replicas (exact).
    acc += (size_t)(blockIdx.x % (unsigned)nrep) * 3 * (size_t)Mpad;
    const float T2d32 = f32_up(T2 * (1.0 + kFilter32Delta));
    // The f32 constants of a word's surviving hypotheses are staged in LDS by the lanes that own them (one vector-load
    // round trip per 64 hypotheses) and read back as broadcasts: one scalar-memory round trip per hypothesis (~1 us
    // when the scalar cache misses) left the kernel latency-bound (37 % VALU utilisation).  The f64 model is fetched
    // only by pairs that have candidates (staging it as well costs occupancy or compaction work: measured slower).
    __shared__ __attribute__((aligned(16))) float s_h32[kGroupWaves][Row::kChunks][64][4];
    __shared__ unsigned s_queue[kGroupWaves][128];
    int qn = 0;  // queued candidate pairs of this wave (wave-uniform)
    unsigned long long st_steps = 0, st_exact = 0, st_inl = 0;  // STATS only (wave-uniform / per-lane partials)
    // Exact evaluation of up to 64 queued (hypothesis, point) pairs, one per lane.  A pair's point lives in the registers
    // of lane `src` of this wave (shuffles), its model is gathered from global memory.  Every contribution is converted to
    // 2^-q fixed point BEFORE any summation, so the accumulated integers do not depend on how pairs were batched:
    // results are bit-reproducible and independent of the launch geometry.  Equal hypotheses are adjacent in the queue
    // (pairs are appended hypothesis by hypothesis): a segmented shuffle reduction leaves one atomic set per run.
    auto drain = [&](int c) __attribute__((always_inline)) {
        const bool act = lane < c;
        const unsigned e = act ? s_queue[wv][lane] : 0u;
        const int m = act ? (int)(e >> 6) : -1 - lane;
        const int src = act ? (int)(e & 63u) : lane;
        double q_pt[R::D];
#pragma unroll
        for (int k = 0; k < R::D; ++k) q_pt[k] = __shfl(pt[k], src, 64);
        const double q_cmp = has_comp ? __shfl(cmp, src, 64) : 0.0;
        Normal<MT> q_nrm;
        if constexpr (kOriented<MT> && !kOrientedGather) {
#pragma unroll
            for (int k = 0; k < 3; ++k) q_nrm.v[k] = __shfl(nrm.v[k], src, 64);
        }
        long long cnt = 0, val = 0, shq = 0;  // (kTrimDrain: val = run_pack(count, value), cnt is only the lane's own 0 / 1)
        if (act) {  // exact path: oracle operation order, no contraction
            double mdl[R::P];
#pragma unroll
            for (int k = 0; k < R::P; ++k) mdl[k] = models_t[(int64_t)k * Mpad + m];  // neighbours in m share cache lines
            if constexpr (kOriented<MT> && kOrientedGather) q_nrm = load_normal<MT>(pts, n, (int64_t)g * 64 + src);   // (a candidate is a valid lane: < n)
            const double sq = squared_at<MT>(q_pt, q_nrm, mdl, T2, kappa);
            if (STATS) ++st_exact;
            if (sq < T2) {  // strict, scoring_function_with_compound_model.h:85
                const double sc = cv_max(0.0, 1.0 - sq / T2);                       // :94
                cnt = 1;
                if (STATS) ++st_inl;
                val = to_fixed(sc * qscale);
                if (has_comp) shq = to_fixed(cv_min(q_cmp, sc) * qscale);           // :115-117
            }
        }
        const int mp = __shfl_up(m, 1, 64);
        const bool head = lane == 0 || mp != m;
        if constexpr (kTrimDrain) {
            // Runs are contiguous, so the mask of their first lanes says how far every lane's run reaches (score_runs.h): no
            // shuffle of m per round; and the count rides in the top bits of the value word (a drain's value sum is < 2^57):
            // two 64-bit shuffles per round (one without a compound instance) where there were an int and three.  The fields
            // are split again below - the same integers go into the same atomics.
            const int dist = run_dist(__ballot(head), lane);
            unsigned long long pv = run_pack((unsigned)cnt, (unsigned long long)val);
#pragma unroll 1   // (unrolled, the six rounds cost the pose instance 6 VGPRs and with them a wave per SIMD)
            for (int off = 1; off < 64; off <<= 1) {  // segmented sums: lane i ends with the total of i .. end of its run
                const bool same = off < dist;
                if (__ballot(same) == 0) break;  // none reaches `off` lanes, none reaches further
                const unsigned long long p2 = __shfl_down(pv, off, 64);
                if (same) pv += p2;
                if (has_comp) {
                    const long long s2 = __shfl_down(shq, off, 64);
                    if (same) shq += s2;
                }
            }
            cnt = (long long)run_count(pv);
            val = (long long)run_value(pv);
        } else {
            for (int off = 1; off < 64; off <<= 1) {  // segmented sums: lane i ends with the total of i .. end of its run
                const int mo = __shfl_down(m, off, 64);
                const bool same = lane + off < 64 && mo == m;
                if (__ballot(same) == 0) break;  // runs are contiguous: none reaches `off` lanes, none reaches further
                const long long c2 = __shfl_down(cnt, off, 64), v2 = __shfl_down(val, off, 64), s2 = __shfl_down(shq, off, 64);
                if (same) { cnt += c2; val += v2; shq += s2; }
            }
        }
        if (act && head && cnt > 0) {
            atomicAdd(&acc[m], (unsigned long long)cnt);
            atomicAdd(&acc[(int64_t)Mpad + m], (unsigned long long)val);
            if (has_comp) atomicAdd(&acc[2 * (int64_t)Mpad + m], (unsigned long long)shq);
        }
    };
    // Exact evaluation IN PLACE for one hypothesis: the candidates of this group are the active lanes (point in registers,
    // the f64 model at a wave-uniform address), per-lane fixed point, one integer shuffle tree, one set of atomics.  Used by
    // the mask-producing variant for every step and by the queued variant for DENSE steps (>= dense_min candidates of 64):
    // through the queue such a step would pay the shuffles, the model gather and the segmented reduction per pair for
    // nothing - its 64 pairs already sit in 64 lanes.  The same per-pair integers as the queued path: bitwise equal sums.
    auto direct = [&](int m, bool cand) __attribute__((always_inline)) {
        double sc = 0.0, shv = 0.0;
        bool inl = false;
        if (cand) {  // exact path: oracle operation order, no contraction
            double mdl[R::P];
#pragma unroll
            for (int k = 0; k < R::P; ++k) mdl[k] = models[(int64_t)m * R::P + k];
            if constexpr (kOriented<MT> && kOrientedGather) nrm = load_normal<MT>(pts, n, jj);
            const double sq = squared_at<MT>(pt, nrm, mdl, T2, kappa);
            inl = sq < T2;  // strict, scoring_function_with_compound_model.h:85
            if (STATS) { ++st_exact; if (inl) ++st_inl; }
            if (inl) {
                sc = cv_max(0.0, 1.0 - sq / T2);      // :94
                if (has_comp) shv = cv_min(cmp, sc);  // :115-117
            }
        }
        const unsigned long long bm = __ballot(inl);
        if (bm == 0) return;
        // per-lane fixed point first (the same integers the queued path adds up), then an exact integer tree
        long long val = inl ? to_fixed(sc * qscale) : 0, shq = (inl && has_comp) ? to_fixed(shv * qscale) : 0;
        // Nothing shared with the compound instance (no instance, or min(compound, score) is 0 in every inlier lane - most
        // hypotheses of a batch): every shq is to_fixed(0) = 0, the tree would add zeros and the atomic would add 0.
        // (shv != 0 holds for NaN: such a step takes the full path.)
        const bool shares = kTrimDirect ? (has_comp && __ballot(inl && shv != 0.0) != 0) : (has_comp != 0);
        if (shares) {
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                val += __shfl_down(val, off, 64);
                shq += __shfl_down(shq, off, 64);
            }
        } else {
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) val += __shfl_down(val, off, 64);
        }
        if (lane == 0) {
            atomicAdd(&acc[m], (unsigned long long)__popcll(bm));
            atomicAdd(&acc[(int64_t)Mpad + m], (unsigned long long)val);
            if (shares) atomicAdd(&acc[2 * (int64_t)Mpad + m], (unsigned long long)shq);
            if (MASK) masks[(int64_t)perm[m] * words + g] = bm;  // rows start zeroed
        }
    };
    for (int w = w0; w < w1; w += wstep) {
        unsigned long long todo;
        if (item_words) {  // the item's next word: fetched with the rows
            todo = kw[0];
#pragma unroll
            for (int k = 0; k + 1 < kWlItemWords; ++k) kw[k] = kw[k + 1];
        } else {
            todo = keep[(int64_t)g * W + w];  // wave-uniform -> scalar load
        }
        if (todo == 0) continue;
        if (STATS) st_steps += (unsigned long long)__popcll(todo);
        __builtin_amdgcn_wave_barrier();  // the previous word's reads are done (LDS ops of a wave execute in order)
        if ((todo >> lane) & 1ull) {
            const int64_t ml = (int64_t)w * 64 + lane;
            Row::stage(hyp32 + ml * Row::kStride, s_h32[wv], lane);
        }
        __builtin_amdgcn_wave_barrier();
        while (todo != 0) {
            const int h = __builtin_ctzll(todo);
            todo &= todo - 1;
            const int m = w * 64 + h;
            const LaneT ln = Row::staged(s_h32[wv], h);  // same address in every lane: LDS broadcast
            bool cand;
            unsigned long long cm;
            if constexpr (kTrimTail) {
                // every lane runs the filter (the lanes past n on a copy of the last point, see valid_mask); the comparison's lane
                // mask is the ballot, and a lane is a candidate when its bit survives the mask
                cm = RejectTerms<F32>::passed(p32, ln, T2d32) & valid_mask;
                if (cm == 0) continue;
                cand = __builtin_amdgcn_inverse_ballot_w64(cm);   // lane i: bit i of cm - the mask itself, no shift and compare per lane
            } else {
                cand = valid && !F32::reject(p32, ln, T2d32);
                cm = __ballot(cand);
                if (cm == 0) continue;
            }
            if (!MASK && __popcll(cm) < dense_min) {
                // the exact path with ~3 of 64 lanes busy per (hypothesis, group) was most of this kernel: candidates
                // are queued instead and evaluated 64 at a time
                if (cand) s_queue[wv][qn + __builtin_amdgcn_mbcnt_hi((unsigned)(cm >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)cm, 0u))] =
                    ((unsigned)m << 6) | (unsigned)lane;
                qn += __popcll(cm);
                if (qn >= 64) {
                    __builtin_amdgcn_wave_barrier();
                    drain(64);
                    __builtin_amdgcn_wave_barrier();
                    const unsigned mv = s_queue[wv][64 + lane];
                    __builtin_amdgcn_wave_barrier();
                    s_queue[wv][lane] = mv;
                    qn -= 64;
                }
                continue;
            }
            direct(m, cand);
        }
    }
    if (!MASK && qn > 0) {
        __builtin_amdgcn_wave_barrier();
        drain(qn);
    }
    if (STATS) {  // one set of atomics per wave
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            st_exact += __shfl_down(st_exact, off, 64);
            st_inl += __shfl_down(st_inl, off, 64);
        }
        if (lane == 0) {
            atomicAdd(&stats[0], st_steps);
            atomicAdd(&stats[1], st_exact);
            atomicAdd(&stats[2], st_inl);
        }
    }
}

// ---- PGX_VERIFY=1: every decision of the bound / filter chain against the exact residual -----------------------------------
// The correctness of counts and masks rests on inequalities with hand-derived error budgets (score_filters.hip.h): a group bound
// that removes (hypothesis, 64-point group) pairs and an f32 filter that removes single pairs may only ever remove outliers.
// This kernel re-decides EVERY pair of the batch with the exact FP64 residual (the reference's operation order) and counts the
// pairs the chain discarded although they are inliers: out[0] removed by the group bound, out[1] by the f32 filter; out[2] =
// inlier pairs.  Any non-zero out[0] / out[1] is a hole in a proof.  Run inside pgx_score_stats only (never timed).
template <int MT>
__global__ __launch_bounds__(64) void score_verify_kernel(const double* __restrict__ pts, const float* __restrict__ pts32, int64_t n,
                                                          const double* __restrict__ models, int M, int W, double T2,
                                                          const unsigned long long* __restrict__ keep, const float* __restrict__ hyp32,
                                                          unsigned long long* __restrict__ out)
{
    using R = Residual<MT>;
    using F32 = Filter32<MT>;
    using LaneT = typename F32::Lane;
    const int lane = (int)threadIdx.x, g = (int)blockIdx.x, w = (int)blockIdx.y;
    const int64_t j = (int64_t)g * 64 + lane;
    const bool valid = j < n;
    const int64_t jj = valid ? j : n - 1;
    double pt[R::D];
    float p32[8];
#pragma unroll
    for (int q = 0; q < R::D; ++q) pt[q] = pts[jj * R::D + q];
#pragma unroll
    for (int q = 0; q < 8; ++q) p32[q] = pts32[jj * 8 + q];
    const Normal<MT> nrm = load_normal<MT>(pts, n, jj);
    const double kappa = oriented_kappa<MT>(pts, n);
    const float T2d32 = f32_up(T2 * (1.0 + kFilter32Delta));
    const unsigned long long todo = keep[(int64_t)g * W + w];
    unsigned long long c_cull = 0, c_filt = 0, c_inl = 0;
    for (int h = 0; h < 64; ++h) {
        const int m = w * 64 + h;
        if (m >= M) break;
        double mdl[R::P];
#pragma unroll
        for (int k = 0; k < R::P; ++k) mdl[k] = models[(int64_t)m * R::P + k];
        const bool inl = valid && squared_at<MT>(pt, nrm, mdl, T2, kappa) < T2;
        const bool kept = (todo >> h) & 1ull;
        const LaneT ln = HypRow<MT>::load(hyp32 + (int64_t)m * HypRow<MT>::kStride);
        const bool rej = F32::reject(p32, ln, T2d32);
        c_inl += inl;
        c_cull += inl && !kept;
        c_filt += inl && kept && rej;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        c_cull += __shfl_down(c_cull, off, 64);
        c_filt += __shfl_down(c_filt, off, 64);
        c_inl += __shfl_down(c_inl, off, 64);
    }
    if (lane == 0) {
        if (c_cull) atomicAdd(&out[0], c_cull);
        if (c_filt) atomicAdd(&out[1], c_filt);
        if (c_inl) atomicAdd(&out[2], c_inl);
    }
}

__global__ __launch_bounds__(256) void score_finish_kernel(const unsigned long long* __restrict__ acc, int M, int Mpad, double qscale,
                                                           const int* __restrict__ perm, long long* __restrict__ counts,
                                                           double* __restrict__ values, double* __restrict__ shared, int nrep,
                                                           long long* __restrict__ mirror /* pinned host memory or nullptr */,
                                                           unsigned* __restrict__ wl /* the work lists' counts or nullptr */)
{
    // the work lists' counts back to zero for the next launch's cull kernel: nothing reads them after the group kernel (a copy stays
    // in the next word of each count's line for pgx_score_debug_fetch(6))
    if (wl != nullptr && blockIdx.x == 0 && threadIdx.x < kWlXcds * kWlClasses) {
        wl[threadIdx.x * kWlCountStride + 1] = wl[threadIdx.x * kWlCountStride];
        wl[threadIdx.x * kWlCountStride] = 0u;
    }
    const int m = (int)(blockIdx.x * 256 + threadIdx.x);
    if (m >= M) return;
    const int o = perm[m];  // hypotheses were scored in locality order: results go back to the caller's order
    // nrep per-XCD replicas of the integer accumulators (co-located groups): integer sums, exact in any order
    unsigned long long c = 0, v = 0, sh = 0;
    for (int r = 0; r < nrep; ++r) {
        const unsigned long long* a = acc + (size_t)r * 3 * (size_t)Mpad;
        c += a[m];
        v += a[(int64_t)Mpad + m];
        sh += a[2 * (int64_t)Mpad + m];
    }
    const double val = (double)(long long)v / qscale, shv = (double)(long long)sh / qscale;
    counts[o] = (long long)c;
    values[o] = val;
    shared[o] = shv;
    if (mirror != nullptr) {  // the same triples in device order, contiguous per wave: pgx_score_fetch reads them without a copy
        mirror[m] = (long long)c;
        reinterpret_cast<double*>(mirror)[(int64_t)Mpad + m] = val;
        reinterpret_cast<double*>(mirror)[2 * (int64_t)Mpad + m] = shv;
    }
}

// ---- point-sharded jobs (comm.hip pgx_score_allreduce): the integer accumulators leave / enter here ---------------------------
// Counts are integers and both sums are 2^-q fixed point, so the accumulators of ranks that scored DIFFERENT points against the
// same hypotheses add exactly in any order: ncclAllReduce(sum, uint64) of 3 x Mpad words gives bitwise the accumulators of one
// GPU scoring all the points (given one q: pgx_score_set_global_n).  Hypotheses are in locality order on the device and the
// order may differ between ranks (it depends on nothing but the models today, but the exchange must not rely on that): the
// block travels in the CALLER's order.
__global__ __launch_bounds__(256) void score_acc_export_kernel(const unsigned long long* __restrict__ acc, int M, int Mpad, int nrep,
                                                               const int* __restrict__ perm, unsigned long long* __restrict__ out)
{
    const int m = (int)(blockIdx.x * 256 + threadIdx.x);
    if (m >= Mpad) return;
    if (m >= M) {   // the padding is nobody's target: zero
        out[m] = 0; out[(size_t)Mpad + m] = 0; out[2 * (size_t)Mpad + m] = 0;
        return;
    }
    unsigned long long c = 0, v = 0, sh = 0;
    for (int r = 0; r < nrep; ++r) {
        const unsigned long long* a = acc + (size_t)r * 3 * (size_t)Mpad;
        c += a[m];
        v += a[(size_t)Mpad + m];
        sh += a[2 * (size_t)Mpad + m];
    }
    const int o = perm[m];
    out[o] = c; out[(size_t)Mpad + o] = v; out[2 * (size_t)Mpad + o] = sh;
}

__global__ __launch_bounds__(256) void score_acc_import_kernel(const unsigned long long* __restrict__ in, int M, int Mpad, double qscale,
                                                               long long* __restrict__ counts, double* __restrict__ values,
                                                               double* __restrict__ shared)
{
    const int m = (int)(blockIdx.x * 256 + threadIdx.x);
    if (m >= M) return;
    counts[m] = (long long)in[m];                                                // as score_finish_kernel
    values[m] = (double)(long long)in[(size_t)Mpad + m] / qscale;
    shared[m] = (double)(long long)in[2 * (size_t)Mpad + m] / qscale;
}

int score_acc_export(pgx_ctx* ctx, unsigned long long* out, hipStream_t stream)
{
    const ScoreBatch& b = ctx->batch;
    if (b.acc_stale())
        return fail(ctx, PGX_ERR_INVALID, "integer accumulators are stale: the batch changed (upload / solve) since the last launch");
    if (!b.acc_exportable())
        return fail(ctx, PGX_ERR_INVALID, "point-sharded exchange: the last launch did not run the group-major path (integer accumulators); "
                                          "it needs sorted points, the f32 filter and the cull (the defaults)");
    hipLaunchKernelGGL(score_acc_export_kernel, dim3((unsigned)((b.resident.Mpad + 255) / 256)), dim3(256), 0, stream, b.last.acc, b.resident.M, b.resident.Mpad,
                       b.last.nrep, ctx->perm.as<int>(), out);
    PGX_HIP(ctx, hipGetLastError());
    return PGX_OK;
}

int score_acc_import(pgx_ctx* ctx, const unsigned long long* in, int M, int Mpad, double qscale, long long* counts, double* values,
                     double* shared, hipStream_t stream)
{
    hipLaunchKernelGGL(score_acc_import_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, stream, in, M, Mpad, qscale, counts, values, shared);
    PGX_HIP(ctx, hipGetLastError());
    return PGX_OK;
}

// Adds the chunk partials of each hypothesis in a FIXED order (bit-reproducible): 64 hypotheses per block, 16 waves
// each summing the chunks k = wave, wave+16, ... sequentially, then the 16 wave sums are added in wave order.
constexpr int kReduceWaves = 16;
__global__ __launch_bounds__(64 * kReduceWaves) void score_reduce_kernel(
    const unsigned* __restrict__ pcnt, const double* __restrict__ pval, const double* __restrict__ psh,
    int chunks, int Mpad, int M, const int* __restrict__ perm, long long* __restrict__ counts,
    double* __restrict__ values, double* __restrict__ shared)
{
    __shared__ long long lc[kReduceWaves][64];
    __shared__ double lv[kReduceWaves][64], ls[kReduceWaves][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int m = blockIdx.x * 64 + lane;
    long long c = 0;
    double v = 0.0, s = 0.0;
    if (m < M)
        for (int k = wave; k < chunks; k += kReduceWaves) {
            const int64_t o = (int64_t)k * Mpad + m;
            c += pcnt[o];
            v += pval[o];
            s += psh[o];
        }
    lc[wave][lane] = c; lv[wave][lane] = v; ls[wave][lane] = s;
    __syncthreads();
    if (wave == 0 && m < M) {
        for (int w = 1; w < kReduceWaves; ++w) { c += lc[w][lane]; v += lv[w][lane]; s += ls[w][lane]; }
        const int o = perm[m];  // hypotheses were scored in locality order: results go back to the caller's order
        counts[o] = c;
        values[o] = v;
        shared[o] = s;
    }
}

// What plan_score (score_plan.h) needs to know of a model type.
template <int MT>
constexpr ScoreTraits score_traits()
{
    return ScoreTraits{Filter<MT>::enabled, Filter32<MT>::enabled, Residual<MT>::bound, std::is_base_of_v<Filter32<kHomography>, Filter32<MT>>};
}

// the planner tells the types apart by these traits alone (the automatic split: poses 5, vanishing points and Sampson 16)
static_assert(score_traits<kPnP>().bound == kBoundBox && !score_traits<kPnP>().homography, "the only box-bounded type outside the homography family");
static_assert(score_traits<kHomography>().homography && score_traits<kHomographySym>().homography && !score_traits<kLine2D>().homography, "");
static_assert(score_traits<kVanishingPoint>().bound == kBoundVanishing && score_traits<kFundamental>().bound == kBoundBoxAll, "");

template <int MT, bool MASK, int FILT>
static void score_launch_one(pgx_ctx* ctx, const ScorePlan& pl, double T2, int has_compound)
{
    const ScoreBatch::Resident& rb = ctx->batch.resident;
    const unsigned groups = (unsigned)(rb.Mpad / kScoreBlock);
    dim3 grid(groups, (unsigned)pl.chunks);
    if (kScoreXcdMap) grid = dim3(groups * (((unsigned)pl.chunks + 7u) / 8u * 8u), 1);
    const bool srt = ctx->point_sort != 0;  // spatially sorted copies (score_sort_points); masks come out in sorted bit order
    hipLaunchKernelGGL((score_kernel<MT, MASK, FILT>), grid, dim3(kScoreBlock), 0, ctx->stream,
                       (srt ? ctx->pts_s : ctx->pts).as<double>(), ctx->n, ctx->models.as<double>(), rb.M, rb.Mpad, T2,
                       (srt ? ctx->comp_s : ctx->comp).as<double>(), has_compound, pl.chunk,
                       (srt ? ctx->pmax_s : ctx->pmax).as<double>(), pl.guard, (srt ? ctx->pts32_s : ctx->pts32).as<float>(), FILT == 2 ? pl.guard32 : 0.0,
                       ctx->pcnt.as<unsigned>(), ctx->pval.as<double>(), ctx->psh.as<double>(),
                       MASK ? (srt ? ctx->masks_s : ctx->masks).as<unsigned long long>() : (unsigned long long*)nullptr,
                       pl.words, ctx->perm.as<int>(), pl.chunks, kScoreXcdMap,
                       (srt && FILT == 2) ? ctx->gbounds.as<float>() : (const float*)nullptr);
}

// cull, then score group-major, then finish: the plan's path 2.  *acc_out: the integer accumulators the launch leaves behind
template <int MT>
static int score_group_path(pgx_ctx* ctx, const ScorePlan& pl, double T2, int has_compound, int want_masks, unsigned long long** acc_out)
{
    const int M = ctx->batch.resident.M, Mpad = ctx->batch.resident.Mpad;
    const int groups = pl.groups, W = pl.W, nrep = pl.nrep, split = pl.split, xcd_local = pl.group_xcd ? 1 : 0;
    PGX_TRY(ensure(ctx, ctx->cull_lists, (size_t)groups * W * sizeof(unsigned long long)));             // keep[g][w]
    PGX_TRY(ensure(ctx, ctx->cull_counts, (size_t)Mpad * (HypRow<MT>::kStride * sizeof(float) + (size_t)nrep * 3 * sizeof(long long) + Residual<MT>::P * sizeof(double))));  // hyp32 | acc[nrep] | models_t
    float* hyp32 = ctx->cull_counts.as<float>();
    unsigned long long* acc = (unsigned long long*)(ctx->cull_counts.as<char>() + (size_t)Mpad * HypRow<MT>::kStride * sizeof(float));
    double* models_t = (double*)(acc + (size_t)nrep * 3 * (size_t)Mpad);
    const double* pts_g = ctx->pts_g.p ? ctx->pts_g.as<double>() : (const double*)nullptr;   // group-blocked SoA copies of the rows
    const float* p32_g = ctx->pts_g.p ? ctx->p32_g.as<float>() : (const float*)nullptr;
    unsigned long long* stats = nullptr;
    if (pl.counters) {
        PGX_TRY(ensure(ctx, ctx->stats_buf, 8 * sizeof(unsigned long long)));
        stats = ctx->stats_buf.as<unsigned long long>();
    }
    long long* mirror = nullptr;
    if (pl.mirror) {
        const size_t need = (size_t)Mpad * 24;
        if (ctx->h_mirror.cap < need) PGX_HIP(ctx, hipStreamSynchronize(ctx->stream));   // an earlier launch may still be writing the old one
        PGX_TRY(grow_pinned(ctx, ctx->h_mirror, need, hipHostMallocMapped | hipHostMallocCoherent));
        mirror = (long long*)ctx->h_mirror.p;
    }
    // The work lists: counts | 8 x 4 lists of wl_cap items.  The counts are zero whenever a cull kernel starts: zeroed when the buffer is
    // allocated, put back to zero by every finish kernel, and cleared here after a launch that did not get as far as its finish kernel.
    unsigned* wl = nullptr;
    if (pl.worklist) {
        const void* before = ctx->score_wl.p;
        PGX_TRY(ensure(ctx, ctx->score_wl, ((size_t)kWlCountWords + (size_t)kWlXcds * kWlClasses * pl.wl_cap) * sizeof(unsigned)));
        if (ctx->score_wl.p != before || ctx->score_wl_dirty) PGX_HIP(ctx, hipMemsetAsync(ctx->score_wl.p, 0, kWlCountWords * sizeof(unsigned), ctx->stream));
        ctx->score_wl_dirty = 1;   // until the finish kernel is enqueued
        wl = ctx->score_wl.as<unsigned>();
    }
    if (ctx->score_profile >= 2) PGX_HIP(ctx, hipEventRecord(ctx->kev[0], ctx->stream));
    // (the accumulators are zeroed by the cull kernel, which runs before their first use)
    auto cull_launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3((unsigned)((W + kCullWaves - 1) / kCullWaves), pl.cull_segs), dim3(64 * kCullWaves), 0,
                           ctx->stream, ctx->models.as<double>(), M, T2, pl.guard32, ctx->gbounds.as<float>(), groups, pl.gps, W,
                           ctx->cull_lists.as<unsigned long long>(), hyp32, models_t, acc, pl.zero_words, wl, pl.wl_xbits, pl.wl_cap, pl.wl_t[0],
                           pl.wl_t[1], pl.wl_t[2]);
    };
    if (pl.worklist) cull_launch(score_cull_kernel<MT, true>);
    else cull_launch(score_cull_kernel<MT, false>);
    PGX_HIP(ctx, hipGetLastError());
    if (ctx->score_profile) PGX_HIP(ctx, hipEventRecord(ctx->kev[1], ctx->stream));
    auto group_launch = [&](auto kernel, unsigned long long* masks_s) {
        hipLaunchKernelGGL(kernel, dim3(pl.worklist ? pl.wl_grid : pl.gblocks), dim3(64 * kGroupWaves), 0, ctx->stream,
                           ctx->pts_s.as<double>(), ctx->pts32_s.as<float>(), ctx->comp_s.as<double>(), ctx->n, groups,
                           ctx->models.as<double>(), W, T2, has_compound, ctx->cull_lists.as<unsigned long long>(), hyp32,
                           pl.qscale, acc, Mpad, masks_s, pl.words, ctx->perm.as<int>(), split, xcd_local, models_t,
                           stats, pts_g, p32_g, nrep, pl.dense_min, (const unsigned*)wl, pl.wl_xbits, pl.wl_cap);
    };
    if (want_masks) {
        PGX_HIP(ctx, hipMemsetAsync(ctx->masks_s.p, 0, (size_t)M * (size_t)pl.words * sizeof(uint64_t), ctx->stream));
        group_launch(score_group_kernel<MT, true>, ctx->masks_s.as<unsigned long long>());
    } else if (pl.counters) {  // pgx_score_stats: the same launch with work counters (never timed)
        PGX_HIP(ctx, hipMemsetAsync(ctx->stats_buf.p, 0, 8 * sizeof(unsigned long long), ctx->stream));
        group_launch(score_group_kernel<MT, false, true>, nullptr);
        if (pl.verify)   // PGX_VERIFY=1: stats_buf[4..6] = inliers the group bound removed / the f32 filter removed / all inlier pairs
            hipLaunchKernelGGL((score_verify_kernel<MT>), dim3((unsigned)groups, (unsigned)W), dim3(64), 0, ctx->stream,
                               ctx->pts_s.as<double>(), ctx->pts32_s.as<float>(), ctx->n, ctx->models.as<double>(), M, W, T2,
                               ctx->cull_lists.as<unsigned long long>(), hyp32, stats + 4);
    } else {
        group_launch(score_group_kernel<MT, false>, nullptr);
    }
    PGX_HIP(ctx, hipGetLastError());
    if (ctx->score_profile) PGX_HIP(ctx, hipEventRecord(ctx->kev[2], ctx->stream));
    if (ctx->score_profile >= 2) PGX_HIP(ctx, hipEventRecord(ctx->kev[4], ctx->stream));
    hipLaunchKernelGGL(score_finish_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, ctx->stream, acc, M,
                       Mpad, pl.qscale, ctx->perm.as<int>(), ctx->counts.as<long long>(), ctx->values.as<double>(),
                       ctx->shared.as<double>(), nrep, mirror, wl);
    PGX_HIP(ctx, hipGetLastError());
    ctx->score_wl_dirty = 0;
    ctx->score_wl_last = pl.worklist ? 1 : 0;
    if (ctx->score_profile >= 2) PGX_HIP(ctx, hipEventRecord(ctx->kev[3], ctx->stream));
    *acc_out = acc;
    return PGX_OK;
}

// the chunked kernel, then the reduction of its partials: the plan's path 1
template <int MT>
static int score_chunked_path(pgx_ctx* ctx, const ScorePlan& pl, double T2, int has_compound, int want_masks)
{
    const int M = ctx->batch.resident.M, Mpad = ctx->batch.resident.Mpad;
    if (ctx->score_profile) PGX_HIP(ctx, hipEventRecord(ctx->kev[0], ctx->stream));
    if constexpr (Filter<MT>::enabled) {
        if (want_masks) {
            if (pl.filter == 2) score_launch_one<MT, true, 2>(ctx, pl, T2, has_compound);
            else if (pl.filter == 1) score_launch_one<MT, true, 1>(ctx, pl, T2, has_compound);
            else score_launch_one<MT, true, 0>(ctx, pl, T2, has_compound);
        } else {
            if (pl.filter == 2) score_launch_one<MT, false, 2>(ctx, pl, T2, has_compound);
            else if (pl.filter == 1) score_launch_one<MT, false, 1>(ctx, pl, T2, has_compound);
            else score_launch_one<MT, false, 0>(ctx, pl, T2, has_compound);
        }
    } else {
        if (want_masks) score_launch_one<MT, true, 0>(ctx, pl, T2, has_compound);
        else score_launch_one<MT, false, 0>(ctx, pl, T2, has_compound);
    }
    PGX_HIP(ctx, hipGetLastError());
    if (ctx->score_profile) PGX_HIP(ctx, hipEventRecord(ctx->kev[1], ctx->stream));
    if (ctx->score_profile >= 2) { PGX_HIP(ctx, hipEventRecord(ctx->kev[2], ctx->stream)); PGX_HIP(ctx, hipEventRecord(ctx->kev[4], ctx->stream)); }
    hipLaunchKernelGGL(score_reduce_kernel, dim3((unsigned)((M + 63) / 64)), dim3(64 * kReduceWaves), 0,
                       ctx->stream, ctx->pcnt.as<unsigned>(), ctx->pval.as<double>(), ctx->psh.as<double>(),
                       pl.chunks, Mpad, M, ctx->perm.as<int>(), ctx->counts.as<long long>(),
                       ctx->values.as<double>(), ctx->shared.as<double>());
    PGX_HIP(ctx, hipGetLastError());
    if (ctx->score_profile >= 2) PGX_HIP(ctx, hipEventRecord(ctx->kev[3], ctx->stream));
    return PGX_OK;
}

// ---- spatially sorted copies of the point data (group test) ----------------------------------------------------------
__global__ __launch_bounds__(256) void gather_f64_kernel(const double* __restrict__ src, const int* __restrict__ pperm, int64_t n,
                                                         double* __restrict__ dst)
{
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j < n) dst[j] = src[pperm[j]];
}

// masks written in sorted bit order -> the caller's point order: one thread per (row, sorted word), set bits scattered
__global__ __launch_bounds__(256) void mask_unpermute_kernel(const unsigned long long* __restrict__ ms, const int* __restrict__ pperm,
                                                             int64_t n, int64_t words, int M, unsigned long long* __restrict__ out)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (int64_t)M * words) return;
    const int64_t row = t / words, w = t % words;
    unsigned long long bits = ms[t];
    while (bits) {
        const int b = __ffsll((long long)bits) - 1;
        bits &= bits - 1;
        const int64_t j = w * 64 + b;
        if (j < n) {
            const int i = pperm[j];
            atomicOr(&out[row * words + (i >> 6)], 1ull << (i & 63));
        }
    }
}

// Host: Morton order of all coordinates, sorted copies, per-group bounds (rows of kGroupRow floats, see above).
int score_sort_points(pgx_ctx* ctx, const ModelInfo& mi, const double* points, const float* p32, const double* pmax)
{
    const int64_t n = ctx->n;
    const int d = ctx->D;
    const int bits = 30 / d;
    std::vector<double> lo((size_t)d), inv((size_t)d);
    for (int k = 0; k < d; ++k) {
        double a = points[k], b = points[k];
        for (int64_t i = 1; i < n; ++i) { const double v = points[i * d + k]; if (v < a) a = v; if (v > b) b = v; }
        if (!std::isfinite(a) || !std::isfinite(b)) return PGX_OK;  // non-finite data: no sorted copies, no group test
        lo[(size_t)k] = a;
        inv[(size_t)k] = b > a ? (double)(1u << bits) / (b - a) : 0.0;
    }
    std::vector<uint64_t> kv((size_t)n), tmp((size_t)n);
    const uint32_t qmax = (1u << bits) - 1u;
    // spread[k][v]: the bits of v placed where coordinate k's bits sit in the interleaved key (bit b -> b*d + d-1-k)
    std::vector<std::vector<uint32_t>> spread((size_t)d, std::vector<uint32_t>((size_t)qmax + 1));
    for (int k = 0; k < d; ++k)
        for (uint32_t v = 0; v <= qmax; ++v) {
            uint32_t out = 0;
            for (int b = 0; b < bits; ++b) out |= ((v >> b) & 1u) << (b * d + d - 1 - k);
            spread[(size_t)k][v] = out;
        }
    for (int64_t i = 0; i < n; ++i) {
        uint32_t key = 0;
        for (int k = 0; k < d; ++k) {
            const double t = (points[i * d + k] - lo[(size_t)k]) * inv[(size_t)k];
            uint32_t v = t > 0.0 ? (uint32_t)t : 0u;
            key |= spread[(size_t)k][v > qmax ? qmax : v];
        }
        kv[(size_t)i] = ((uint64_t)key << 32) | (uint32_t)i;
    }
    for (int pass = 0; pass < 4; ++pass) {  // LSD radix sort on the key's four bytes (stable: ties keep index order)
        size_t cnt[257] = {0};
        const int sh = 32 + 8 * pass;
        for (int64_t i = 0; i < n; ++i) ++cnt[((kv[(size_t)i] >> sh) & 0xff) + 1];
        for (int b = 0; b < 256; ++b) cnt[b + 1] += cnt[b];
        for (int64_t i = 0; i < n; ++i) tmp[cnt[(kv[(size_t)i] >> sh) & 0xff]++] = kv[(size_t)i];
        kv.swap(tmp);
    }
    const int64_t groups = (n + 63) / 64;
    std::vector<int> pperm((size_t)n);
    std::vector<double> sp((size_t)n * d), spm((size_t)n);
    const int64_t supers = (groups + kSuper - 1) / kSuper;
    std::vector<float> sp32((size_t)n * 8), gb((size_t)(groups + supers) * kGroupRow, 0.0f);
    for (int64_t j = 0; j < n; ++j) {
        const int64_t i = (int64_t)(uint32_t)kv[(size_t)j];
        pperm[(size_t)j] = (int)i;
        for (int k = 0; k < d; ++k) sp[(size_t)j * d + k] = points[i * d + k];
        for (int k = 0; k < 8; ++k) sp32[(size_t)j * 8 + k] = p32[i * 8 + k];
        spm[(size_t)j] = pmax[i];
    }
    // which coordinates the projective map multiplies / which are observed (a kBoundBox model type: pgx_set_points)
    const int in0 = mi.in0, in1 = mi.box1, ob0 = mi.obs0;
    auto bounds = [&](int64_t a, int64_t b, float* row) {  // bounds of the sorted points [a, b)
        // centre = box centre of the f32 rows (the values the kernel's per-point filter sees are not needed here: the
        // bound is about the exact f64 points; extents are inflated below)
        double cmin[3] = {0, 0, 0}, cmax[3] = {0, 0, 0}, omin[2], omax[2];
        for (int k = in0; k <= in1; ++k) { cmin[k - in0] = cmax[k - in0] = sp[(size_t)a * d + k]; }
        for (int k = 0; k < 2; ++k) omin[k] = omax[k] = sp[(size_t)a * d + ob0 + k];
        for (int64_t j = a; j < b; ++j) {
            for (int k = in0; k <= in1; ++k) { const double v = sp[(size_t)j * d + k]; if (v < cmin[k - in0]) cmin[k - in0] = v; if (v > cmax[k - in0]) cmax[k - in0] = v; }
            for (int k = 0; k < 2; ++k) { const double v = sp[(size_t)j * d + ob0 + k]; if (v < omin[k]) omin[k] = v; if (v > omax[k]) omax[k] = v; }
        }
        float cf[3] = {0, 0, 0};
        double scale = 1.0;
        for (int k = 0; k <= in1 - in0; ++k) { cf[k] = (float)(0.5 * (cmin[k] + cmax[k])); if (std::fabs((double)cf[k]) > scale) scale = std::fabs((double)cf[k]); }
        double rho2 = 0.0;  // radius about the f32 centre actually stored
        for (int64_t j = a; j < b; ++j) {
            double s2 = 0.0;
            for (int k = in0; k <= in1; ++k) { const double df = sp[(size_t)j * d + k] - (double)cf[k - in0]; s2 += df * df; }
            if (s2 > rho2) rho2 = s2;
        }
        const float ub = (float)(0.5 * (omin[0] + omax[0])), vb = (float)(0.5 * (omin[1] + omax[1]));
        double ru = 0.0, rv = 0.0;
        for (int64_t j = a; j < b; ++j) {
            const double du = std::fabs(sp[(size_t)j * d + ob0] - (double)ub), dv = std::fabs(sp[(size_t)j * d + ob0 + 1] - (double)vb);
            if (du > ru) ru = du;
            if (dv > rv) rv = dv;
        }
        row[0] = cf[0]; row[1] = cf[1]; row[2] = cf[2];
        row[3] = (float)(std::sqrt(rho2) * kGroupInflate + 1e-30);
        row[4] = ub; row[5] = vb;
        row[6] = (float)(ru * kGroupInflate + 1e-30);
        row[7] = (float)(rv * kGroupInflate + 1e-30);
        row[8] = (float)(scale * 1.000001);
    };
    for (int64_t g = 0; g < groups; ++g) bounds(g * 64, g * 64 + 64 < n ? g * 64 + 64 : n, gb.data() + (size_t)g * kGroupRow);
    // super-groups of kSuper consecutive groups (512 points): the cull kernel tests them first; rows behind the group rows
    for (int64_t sg = 0; sg < supers; ++sg)
        bounds(sg * kSuper * 64, (sg + 1) * kSuper * 64 < n ? (sg + 1) * kSuper * 64 : n, gb.data() + (size_t)(groups + sg) * kGroupRow);
    {   // group-blocked SoA copies for the group-major kernel: [group][coordinate][64]; the tail group repeats its last row
        std::vector<double> pg((size_t)groups * d * 64);
        std::vector<float> p32g((size_t)groups * 8 * 64, 0.0f);
        for (int64_t g = 0; g < groups; ++g)
            for (int l = 0; l < 64; ++l) {
                const int64_t j = g * 64 + l < n ? g * 64 + l : n - 1;
                for (int k = 0; k < d; ++k) pg[((size_t)g * d + k) * 64 + l] = sp[(size_t)j * d + k];
                for (int k = 0; k < 8; ++k) p32g[((size_t)g * 8 + k) * 64 + l] = sp32[(size_t)j * 8 + k];
            }
        PGX_TRY(ensure(ctx, ctx->pts_g, pg.size() * sizeof(double)));
        PGX_TRY(ensure(ctx, ctx->p32_g, p32g.size() * sizeof(float)));
        PGX_HIP(ctx, hipMemcpyAsync(ctx->pts_g.p, pg.data(), pg.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
        PGX_HIP(ctx, hipMemcpyAsync(ctx->p32_g.p, p32g.data(), p32g.size() * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
        PGX_HIP(ctx, hipStreamSynchronize(ctx->stream));  // the staging vectors die at the end of this block
    }
    PGX_TRY(ensure(ctx, ctx->pts_s, (size_t)n * d * sizeof(double)));
    PGX_TRY(ensure(ctx, ctx->pts32_s, (size_t)n * 8 * sizeof(float)));
    PGX_TRY(ensure(ctx, ctx->pmax_s, (size_t)n * sizeof(double)));
    PGX_TRY(ensure(ctx, ctx->comp_s, (size_t)n * sizeof(double)));
    PGX_TRY(ensure(ctx, ctx->pperm, (size_t)n * sizeof(int)));
    PGX_TRY(ensure(ctx, ctx->gbounds, (size_t)(groups + supers) * kGroupRow * sizeof(float)));
    PGX_HIP(ctx, hipMemcpyAsync(ctx->pts_s.p, sp.data(), (size_t)n * d * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    PGX_HIP(ctx, hipMemcpyAsync(ctx->pts32_s.p, sp32.data(), (size_t)n * 8 * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    PGX_HIP(ctx, hipMemcpyAsync(ctx->pmax_s.p, spm.data(), (size_t)n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    PGX_HIP(ctx, hipMemcpyAsync(ctx->pperm.p, pperm.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    PGX_HIP(ctx, hipMemcpyAsync(ctx->gbounds.p, gb.data(), (size_t)(groups + supers) * kGroupRow * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    PGX_HIP(ctx, hipMemsetAsync(ctx->comp_s.p, 0, (size_t)n * sizeof(double), ctx->stream));
    PGX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ctx->point_sort = 1;
    ctx->comp_dirty = 1;
    return PGX_OK;
}

// plan (score_plan.h) -> buffers -> launches -> one event on the batch's owner.  A refused call changes nothing; an accepted one that
// fails midway (an allocation) tells the owner so.
template <int MT>
static int score_launch_typed(pgx_ctx* ctx, double T2, int has_compound, int want_masks, bool want_counters)
{
    const ScoreBatch::Resident& rb = ctx->batch.resident;
    const ScorePlan pl = plan_score(score_traits<MT>(), ctx->score_sw, ctx->cu_count, ctx->n, rb.M, rb.Mpad, rb.ordered, ctx->point_sort != 0, T2,
                                    ctx->umax, ctx->fscale, ctx->score_global_n, want_masks != 0, want_counters);
    const size_t np = (size_t)pl.chunks * (size_t)rb.Mpad;
    PGX_TRY(ensure(ctx, ctx->pcnt, np * sizeof(unsigned)));
    PGX_TRY(ensure(ctx, ctx->pval, np * sizeof(double)));
    PGX_TRY(ensure(ctx, ctx->psh, np * sizeof(double)));
    // counts | values | shared live in ONE allocation (values / shared are views into it): pgx_score_fetch brings all three
    // back with a single copy (three small copies cost ~5 us each on the critical path of a 0.3 ms step)
    PGX_TRY(ensure(ctx, ctx->counts, (size_t)3 * rb.Mpad * sizeof(long long)));
    ctx->values.p = ctx->counts.as<char>() + (size_t)rb.Mpad * 8;
    ctx->shared.p = ctx->counts.as<char>() + (size_t)2 * rb.Mpad * 8;
    ctx->values.cap = ctx->shared.cap = 0;  // not owned
    const size_t mask_bytes = (size_t)rb.M * (size_t)pl.words * sizeof(uint64_t);
    if (want_masks) PGX_TRY(ensure(ctx, ctx->masks, mask_bytes));
    if (ctx->point_sort) {
        if (has_compound && ctx->comp_dirty) {  // the kernel reads the compound vector in sorted point order
            hipLaunchKernelGGL(gather_f64_kernel, dim3((unsigned)((ctx->n + 255) / 256)), dim3(256), 0, ctx->stream,
                               ctx->comp.as<double>(), ctx->pperm.as<int>(), ctx->n, ctx->comp_s.as<double>());
            PGX_HIP(ctx, hipGetLastError());
            ctx->comp_dirty = 0;
        }
        if (want_masks) PGX_TRY(ensure(ctx, ctx->masks_s, mask_bytes));
    }
    unsigned long long* acc = nullptr;
    if constexpr (Filter32<MT>::enabled) {
        if (pl.path == 2) PGX_TRY(score_group_path<MT>(ctx, pl, T2, has_compound, want_masks, &acc));
    }
    if (pl.path != 2) PGX_TRY(score_chunked_path<MT>(ctx, pl, T2, has_compound, want_masks));
    if (ctx->point_sort && want_masks) {
        const int64_t total = (int64_t)rb.M * pl.words;
        PGX_HIP(ctx, hipMemsetAsync(ctx->masks.p, 0, mask_bytes, ctx->stream));
        hipLaunchKernelGGL(mask_unpermute_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ctx->stream,
                           ctx->masks_s.as<unsigned long long>(), ctx->pperm.as<int>(), ctx->n, pl.words, rb.M,
                           ctx->masks.as<unsigned long long>());
        PGX_HIP(ctx, hipGetLastError());
    }
    ctx->batch.launched(pl, has_compound != 0, want_masks != 0, acc);
    return PGX_OK;
}

int score_launch(pgx_ctx* ctx, double T2, int has_compound, int want_masks, bool want_counters)
{
    if (ctx->n <= 0 || ctx->model_type < 0) return fail(ctx, PGX_ERR_INVALID, "pgx_score: points not set");
    if (ctx->batch.resident.M <= 0) return fail(ctx, PGX_ERR_INVALID, "pgx_score: no hypotheses uploaded");
    PGX_TRY(need_oriented_normals(ctx, "pgx_score"));
    int rc = PGX_OK;
    if (!with_model_type(ctx->model_type, [&](auto mt) { rc = score_launch_typed<decltype(mt)::value>(ctx, T2, has_compound, want_masks, want_counters); }))
        return fail(ctx, PGX_ERR_INVALID, "pgx_score: bad model type %d", ctx->model_type);
    if (rc != PGX_OK) ctx->batch.launch_failed();
    return rc;
}

}  // namespace pgx
