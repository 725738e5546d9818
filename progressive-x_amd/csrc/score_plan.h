// score_plan.h — what a scoring launch looks like (plan_score) and who owns the hypothesis batch and the last launch's results
// (ScoreBatch); DESIGN.md 4.1, "What a launch looks like".  No HIP in here: libpgx.so and the CPU tests (tests/emu/mf_emu.cpp,
// tests/test_score_plan.py) compile the same code.  score.hip turns a plan into buffers and launches; the limits and windows of
// the decision live in this file and nowhere else.
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

#include "score_worklist.h"

namespace pgx {

// What the group bound of the sorted points is made of (setpoints.hip builds the rows, score.hip's cull kernel tests them).
enum GroupBound : int {
    kBoundBox,        // box of the observed pair + box and ball of the coordinates the projective map multiplies
    kBoundBoxAll,     // box of all coordinates (Sampson)
    kBoundBall,       // ball of all coordinates about the box centre (D = 2 or 3)
    kBoundVanishing   // rows of the normalised segment features
};

constexpr int kScoreBlock = 256;        // hypotheses per workgroup of the chunked kernel; Mpad is a multiple of it
constexpr int kSuper = 8;               // groups per super-group (512 points): first level of the cull kernel
constexpr int kScoreBlocksPerCu = 64;   // grid over-decomposition of the chunked kernel (no switch sets it)
constexpr int kScoreXcdMap = 1;         // XCD-aware block mapping of the chunked kernel (no switch sets it)
constexpr int kScoreMaxChunk = 65472;   // queue entries of the deferred kernel are 16-bit offsets into the chunk
constexpr int kScoreMaxChunks = 65535;  // gridDim.y limit
constexpr int kScoreCullSegs = 256;     // the cull kernel's segments per hypothesis word unless pgx_score_debug_geometry(4) says otherwise
constexpr int64_t kWlMaxItems = (int64_t)1 << 22;   // (group, item column) pairs beyond which the work lists are not built (16 bytes each)

// What the planner needs to know of a model type (score.hip score_traits<MT>() fills it from Residual / Filter / Filter32).
struct ScoreTraits {
    bool filter64 = false;     // Filter<MT>::enabled: the f64 rejection filter with its global guard
    bool filter32 = false;     // Filter32<MT>::enabled: the f32 pre-filter, and with it the cull + group-major path
    int bound = kBoundBox;     // Residual<MT>::bound
    bool homography = false;   // Filter32<MT> is Filter32<kHomography> or derives from it: explicit per-pair error terms
};

struct ScoreSwitches {
    int filter_enabled{1};   // pgx_create, PGX_NO_FILTER: =1 -> 0 no rejection filter, =2 -> 2 the FP64 filter only (A/B, debugging)
    int cull{1};             // pgx_create, PGX_SCORE_NO_CULL=1 -> 0: the chunked kernel with in-kernel group skipping (A/B)
    int mirror{1};           // pgx_create, PGX_SCORE_MIRROR=0: the triples come back with a copy, not through the host mirror
    int verify{0};           // pgx_create, PGX_VERIFY=1: pgx_score_stats also re-decides every pair exactly and counts contradictions
    int split{0};            // pgx_score_debug_geometry(0): waves per 64-point group of the group-major kernel; 0 = automatic (below)
    int group_xcd{-1};       // pgx_score_debug_geometry(1): 1 = a group's workgroups on one XCD (8x less row fetch, per-XCD accumulator
                             // replicas), 0 = part p on XCD p; -1 = 1 for a locality-ordered batch, else 0
    int nrep{0};             // pgx_score_debug_geometry(2): replicas of the integer accumulators (multiple of 8); 0 = 8 when a group's
                             // waves share an XCD, else 1
    int dense_min{32};       // pgx_score_debug_geometry(3): steps with at least this many candidates of 64 are evaluated in place, not
                             // queued (65 = never)
    int cull_segs{kScoreCullSegs};   // pgx_score_debug_geometry(4): segments of groups per hypothesis word in the cull kernel
    int worklist{-1};        // pgx_create, PGX_SCORE_WORKLIST=0 | 1 and pgx_score_debug_geometry(5): the group-major kernel takes (group, 4-word)
                             // items from the cull kernel's work lists; -1 = automatic (pose problems on the co-located mapping), 0 = never,
                             // 1 = on the co-located mapping for every model type (A/B)
    int wl_t1{24}, wl_t2{64}, wl_t3{160};   // pgx_score_debug_geometry(6 .. 8): weight thresholds of the four classes (t2 = t3 = 2^30: two classes)
};

struct ScorePlan {
    int path = 1;              // 1 = chunked kernel + reduce (every pair visited), 2 = cull + group-major + finish
    int filter = 0;            // 0 none, 1 the f64 filter, 2 the f32 pre-filter (in front of the f64 one where the type has it)
    double guard = 0.0;        // Filter<MT>::prep
    double guard32 = 0.0;      // Filter32<MT>::prep: the global guard, or the overflow guard of the types with per-pair error terms
    int64_t chunk = 0;         // points per block of the chunked kernel (multiple of 64: mask words never straddle blocks)
    int chunks = 0;
    int64_t words = 0;         // 64-bit words of a mask row
    // path 2 only (0 on path 1)
    int groups = 0;            // 64-point groups
    int cull_segs = 0, gps = 0;   // segments per hypothesis word, groups per segment (whole super-groups)
    int W = 0;                 // hypothesis words
    int group_xcd = 0;         // a group's waves share an XCD (then the accumulators have per-XCD replicas)
    int nrep = 0;
    int split = 0;             // waves per group
    unsigned gblocks = 0;      // workgroups of the group-major kernel
    double qscale = 0.0;       // 2^q of the fixed-point sums
    int64_t zero_words = 0;    // accumulator words the cull kernel clears
    int dense_min = 0;
    bool counters = false;     // the group-major instance with work counters (pgx_score_stats)
    bool verify = false;       // ... followed by the exhaustive verification kernel
    bool mirror = false;       // the finish kernel also writes the triples to the host mirror
    // the work lists (score_worklist.h); all 0 when off: split and gblocks above then describe the launch
    bool worklist = false;     // the cull kernel appends the non-empty (group, 4-word) items, the group kernel takes them heaviest first
    int wl_columns = 0;        // items per group: ceil(W / kWlItemWords)
    int wl_xbits = 0;          // bits of the item column in an item record
    unsigned wl_cap = 0;       // capacity of each of the 8 x 4 lists: its worst case, every item of the XCD's groups (no overflow path)
    unsigned wl_t[3] = {0, 0, 0};   // class thresholds
    unsigned wl_grid = 0;      // workgroups of the group kernel: 8 * wl_cap, slot b >> 3 of XCD b & 7
};

// The floating-point expressions keep the operation order they always had: guard, guard32 and qscale are compared by their bits.
// `ordered`: the resident batch is in locality order (ScoreBatch) - the planner's only coupling to the batch.
inline ScorePlan plan_score(const ScoreTraits& tr, const ScoreSwitches& sw, int cu_count, int64_t n, int M, int Mpad, bool ordered,
                            bool point_sort, double T2, double umax, double fscale, int64_t score_global_n, bool want_masks,
                            bool want_counters, int blocks_per_cu = kScoreBlocksPerCu)
{
    (void)M;
    ScorePlan p;
    // ---- filter level.  f64 filter guard (score_filters.hip.h Filter<>): usable iff Umax / T <= 2^28 and everything is finite
    const double T = std::sqrt(T2);
    bool filt = tr.filter64 && sw.filter_enabled && T > 0.0 && std::isfinite(T) && std::isfinite(umax) && umax <= T * 268435456.0;
    if (filt) {
        p.guard = 4.5 * 1.1102230246251565e-16 * (1.0 + umax + T) * 16777216.0 / T;
        filt = std::isfinite(p.guard);
    }
    // FP32 pre-filter: tau = 2^-10, needs Umax / T <= tau * 2^24 = 2^14
    bool filt32 = filt && sw.filter_enabled == 1 && umax <= T * 16384.0;
    if (filt32) {
        p.guard32 = 5.5 * 5.9604644775390625e-8 * (1.0 + umax + T) * 1024.0 / T;
        filt32 = std::isfinite(p.guard32) && p.guard32 < 1e30;
    }
    if (tr.bound == kBoundVanishing)   // its own trust test per pair, no global guard (Filter32<kVanishingPoint>)
        filt32 = sw.filter_enabled == 1 && T > 0.0 && std::isfinite(T) && T2 < 1e30;
    if (tr.homography)                 // explicit per-pair error terms, no global guard (Filter32<kHomography>)
        filt32 = sw.filter_enabled == 1 && T2 > 1e-24 && T2 < 1e24;
    if (tr.bound == kBoundBall) {      // per-pair error term, no global guard; T'' must be an ordinary f32
        filt32 = sw.filter_enabled == 1 && T2 > 1e-24 && T2 < 1e24 && std::isfinite(fscale);
        p.guard32 = fscale;            // Filter32<kLine2D / kPlane3D / kSphere3D / kCircle2D>::prep: overflow guard (fscale >= 1);
                                       // the plan keys on `bound`: a ball-bounded type needs no line of its own here
    }
    if (tr.bound == kBoundBoxAll) {    // likewise; the bounds on T keep T2 * D~^2 (D~ >= 1e-12) inside the f32 normal range
        filt32 = sw.filter_enabled == 1 && T2 > 1e-12 && T2 < 1e12 && std::isfinite(fscale);
        p.guard32 = fscale * fscale;   // Filter32<kFundamental>::prep: overflow guard of the f32 terms (fscale >= 1)
    }
    // every filter's proof takes the exact path's f64 arithmetic as overflow-free: coordinates up to 1e30 with the
    // per-hypothesis band of pow2_normaliser keep it so
    if (!(fscale <= 1e30)) filt = filt32 = false;
    p.filter = filt32 ? 2 : (filt ? 1 : 0);

    // ---- the chunked kernel's grid: >= ~blocks_per_cu blocks per CU (work per pair is data dependent - the exact path only for
    // candidates - so the grid is over-decomposed to keep the tail behind the slowest block short), chunks multiples of 64 points
    const int hyp_blocks = Mpad >= kScoreBlock ? Mpad / kScoreBlock : 1;   // (Mpad is a multiple of kScoreBlock wherever a batch comes from)
    const int target_blocks = (cu_count > 0 ? cu_count : 256) * blocks_per_cu;
    int64_t chunks = (target_blocks + hyp_blocks - 1) / hyp_blocks;
    int64_t chunk = (n + chunks - 1) / chunks;
    chunk = ((chunk + 63) / 64) * 64;
    if (chunk < 64) chunk = 64;
    if (chunk > kScoreMaxChunk) chunk = kScoreMaxChunk;
    chunks = (n + chunk - 1) / chunk;
    if (chunks > kScoreMaxChunks) {
        chunks = kScoreMaxChunks;
        chunk = (((n + chunks - 1) / chunks + 63) / 64) * 64;
        chunks = (n + chunk - 1) / chunk;
    }
    p.chunk = chunk;
    p.chunks = (int)chunks;
    p.words = (n + 63) / 64;

    if (!(tr.filter32 && filt32 && point_sort && sw.cull)) return p;
    // ---- cull, then score group-major
    p.path = 2;
    p.groups = (int)((n + 63) / 64);
    p.cull_segs = sw.cull_segs;
    p.gps = ((p.groups + p.cull_segs - 1) / p.cull_segs + kSuper - 1) / kSuper * kSuper;   // whole super-groups per segment
    p.W = Mpad / 64;
    // Where the waves of a group run.  Part p of every group on XCD p spreads a group's work over the chip but makes every
    // XCD fetch every row; all parts of a group on one XCD fetches a row once (FETCH_SIZE 8x lower) and needs a replica of
    // the accumulators per XCD.  Measured on the final code: the co-located mapping is 9 % faster (group kernel 215 -> 196 us)
    // on a locality-ordered batch, where only a few of a group's hypothesis words have survivors, and 19 % slower (step
    // 0.42 -> 0.50 ms) on a batch in arbitrary order, where all of them do - so the order of the batch decides.
    p.group_xcd = sw.group_xcd >= 0 ? sw.group_xcd : (ordered ? 1 : 0);
    p.nrep = sw.nrep > 0 ? sw.nrep : (p.group_xcd ? 8 : 1);
    int lg = 0;
    const int64_t n_scale = score_global_n > n ? score_global_n : n;   // pgx_score_set_global_n
    while (((int64_t)1 << lg) < n_scale + 1) ++lg;
    p.qscale = std::ldexp(1.0, 62 - lg < 50 ? 62 - lg : 50);   // every sum is <= n < 2^lg; terms < 2^51 (to_fixed)
    p.zero_words = (int64_t)p.nrep * Mpad * 3;                 // the cull kernel zeroes the accumulators before their first use
    // waves per group.  Spread mapping: 8 (part p = XCD p).  Co-located mapping: 5 - fewer, longer waves load a group's rows
    // less often, and an ODD count keeps the heavy workgroups (a locality-ordered batch puts a group's survivors into two or
    // three neighbouring hypothesis words) from falling into a period of the dispatch order: group kernel 169 (8), 157 (4),
    // 146 (6), 140 (2) against 135-140 us (1, 3, 5, 7) on the metric batch.
    // (pose problems take 5 with the spread mapping as well: RANSAC-like batch 0.371 -> 0.353 ms; Sampson and vanishing-point
    // batches lose 15-20 % there and keep 8)
    // Round 6 (scripts/sweep_vp_geometry.py, after the Hough ordering of the segments): vanishing-point and Sampson batches take 16 -
    // group kernel 301 -> 280 us and 123 -> 114 us against 8 (12: 284 / 118, 24: 284 / 115, 32: 296 / 119).
    const bool pose = tr.bound == kBoundBox && !tr.homography;
    const int split_cfg = sw.split > 0 ? sw.split
                          : ((p.group_xcd || pose) ? 5 : ((tr.bound == kBoundVanishing || tr.bound == kBoundBoxAll) ? 16 : 8));
    p.split = split_cfg < p.W ? split_cfg : p.W;
    p.gblocks = p.group_xcd ? (unsigned)((int64_t)((p.groups + 7) / 8) * 8 * p.split) : (unsigned)((int64_t)p.groups * p.split);
    p.dense_min = want_masks ? 65 : sw.dense_min;
    p.counters = want_counters && !want_masks;   // pgx_score_stats: the same launch with work counters (never timed)
    p.verify = p.counters && sw.verify;
    p.mirror = sw.mirror && !want_masks;
    // ---- the work lists.  On for pose problems on the co-located mapping (the step bench.py measures: group kernel, tail and sweep in
    // docs/lab-notebook.md, "A heavy-first work list"); the other types keep the strided parts until somebody measures them
    // (sw.worklist = 1 is the switch for that).  Off whenever a debug switch asks for a geometry of its own (split, cull_segs; a forced
    // spread mapping is not co-located), and for the mask-producing launch, which evaluates every step in place and was not measured.
    const int columns = (p.W + kWlItemWords - 1) / kWlItemWords;
    const int64_t cap = (int64_t)((p.groups + kWlXcds - 1) / kWlXcds) * columns;
    if (p.group_xcd && sw.split == 0 && sw.cull_segs == kScoreCullSegs && !want_masks && (sw.worklist == 1 || (sw.worklist < 0 && pose)) &&
        wl_fits(p.groups, columns) && (int64_t)p.groups * columns <= kWlMaxItems) {
        p.worklist = true;
        p.wl_columns = columns;
        p.wl_xbits = wl_xbits(columns);
        p.wl_cap = (unsigned)cap;
        p.wl_t[0] = (unsigned)sw.wl_t1; p.wl_t[1] = (unsigned)sw.wl_t2; p.wl_t[2] = (unsigned)sw.wl_t3;
        p.wl_grid = (unsigned)kWlXcds * p.wl_cap;
    }
    return p;
}

// ---- the batch and the last launch: one owner, changed only by its events ------------------------------------------------------
// An event fires after the fallible work of its call has succeeded: a refused or failed upload / solve leaves both records as they
// were.  comm.hip's exchange slots keep their own copies of M, Mpad and has_compound - they outlive the batch by design.
enum class ScoreTable { Ready, None, Changed };   // the last launch scored the resident batch | nothing launched (or no batch) |
                                                  // the batch or the points changed since the launch: its rows belong to nothing
struct ScoreBatch {
    struct Resident {
        int M = 0, Mpad = 0;
        bool ordered = false;          // locality order (pgx_score_upload); perm[device position] = the caller's index
        std::vector<int> perm;
        int64_t generation = 0;        // bumped by every event that changes the batch
    } resident;
    struct Launch {
        int64_t generation = -1;       // the batch it scored; -1: nothing was ever launched
        bool has_compound = false, masks = false;
        int64_t words = 0;
        int path = 0, filter = 0;      // ScorePlan's (0: no launch yet); they outlive the batch - pgx_score_kernel_times reads them
        unsigned long long* acc = nullptr;   // integer accumulators [nrep][3][Mpad] of a group-major launch (device order), or nullptr
        int nrep = 0;
        double qscale = 0.0;
        bool mirror = false;           // the host mirror holds this launch's triples, in device order
    } last;

    // ---- events
    void points_changed() { resident.M = 0; resident.Mpad = 0; resident.ordered = false; resident.generation += 1; }
    void uploaded(int M, int Mpad, const int* perm)   // pgx_score_upload; perm = nullptr: the caller's order
    {
        resident.M = M; resident.Mpad = Mpad; resident.ordered = perm != nullptr;
        if (perm) resident.perm.assign(perm, perm + M);
        resident.generation += 1;
    }
    void generated(int M, int Mpad) { uploaded(M, Mpad, nullptr); }   // pgx_solve_minimal(_sampled): device batches keep the sample order
    void launched(const ScorePlan& p, bool has_compound, bool masks, unsigned long long* acc)
    {
        last.generation = resident.generation;
        last.has_compound = has_compound; last.masks = masks; last.words = p.words;
        last.path = p.path; last.filter = p.filter;
        last.acc = p.path == 2 ? acc : nullptr; last.nrep = p.nrep; last.qscale = p.qscale;
        last.mirror = p.path == 2 && p.mirror;
    }
    void launch_failed() { last.mirror = false; }   // an accepted launch that ran out of memory midway: nothing wrote the mirror
    void table_reduced() { last.mirror = false; }   // pgx_score_allreduce: the device table is the job's, the mirror this rank's part

    // ---- questions
    bool current() const { return last.generation == resident.generation; }
    ScoreTable table() const   // pgx_score_fetch, pgx_score_allgather(_begin), pgx_score_fetch_all
    {
        if (resident.M <= 0 || last.generation < 0) return ScoreTable::None;
        return current() ? ScoreTable::Ready : ScoreTable::Changed;
    }
    ScoreTable mask_rows() const   // pgx_score_inliers, the masks of pgx_score_fetch
    {
        if (resident.M <= 0 || last.generation < 0 || !last.masks) return ScoreTable::None;
        return current() ? ScoreTable::Ready : ScoreTable::Changed;
    }
    bool from_mirror() const { return last.mirror; }                                        // of a Ready table: the mirror, else the device copy
    const int* unpermute() const { return resident.ordered ? resident.perm.data() : nullptr; }   // ... and the mirror's order (nullptr: the caller's)
    bool acc_exportable() const { return current() && last.path == 2 && last.acc != nullptr; }   // pgx_score_allreduce, pgx_score_debug_fetch(5)
    bool acc_stale() const { return !current() && last.path == 2 && last.acc != nullptr; }       // (only the wording of the refusal)
};

}  // namespace pgx
