// pgx_internal.h — context layout and helpers shared by the translation units of libpgx.so (not part of the ABI).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "../../include/pgx.h"
#include "expansion_cycle.h"
#include "move_route.h"
#include "residuals.hip.h"
#include "score_plan.h"

namespace pgx {

// growable device buffer
struct StagedCopy { void* dst; size_t off, bytes; };
struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    template <class T> T* as() const { return reinterpret_cast<T*>(p); }
};

// growable pinned host buffer (grow_pinned) / ... used as the staging of an asynchronous upload: the caller's array is consumed before
// the call returns, the copies need no synchronisation, and an event guards the buffer against the next call
struct PinnedBuf { void* p = nullptr; size_t cap = 0; };
struct PinnedStage {
    PinnedBuf buf;
    hipEvent_t ev = nullptr;
    int busy = 0;
    int acquire(pgx_ctx* ctx, size_t bytes);       // waits for the copies of the last submission, then buf.p holds at least `bytes`
    int submitted(pgx_ctx* ctx, hipStream_t stream);   // the copies out of buf.p are enqueued on `stream`
    void free();
};

struct MaxflowState;  // maxflow.hip
struct TileState;     // maxflow_tile.hip
struct CommState;     // comm.cpp

}  // namespace pgx

struct pgx_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    hipEvent_t kev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};  // pgx_score_profile: [0] start, [1] after cull, [2] after group-major, [4] after exact, [3] after finish
    int score_profile = 0;
    std::string err;
    int cu_count = 0;

    // resident problem data
    int model_type = -1, D = 0, P = 0;
    int64_t n = 0;
    pgx::DevBuf pts, comp;
    pgx::DevBuf pmax;        // per point max(|coords the filter scales by|, 1)  (score filter)
    pgx::DevBuf pts32;       // N x 8 f32: coordinates + filter scale (FP32 pre-filter)
    double umax = 0.0;       // max |observed image coordinate| over all points
    double fscale = 0.0;     // max(1, max |coordinate|) over all points: isotropic pre-scaling of the minimal solvers
    double rmin = 0.0, rmax = __builtin_inf();   // pgx_set_radius_range: the radii the sphere, the circle and the cylinder solver accept, the sines of the cone's (context state)
    int prim_mask = 15;                          // pgx_set_primitive_classes: the classes the mixed-primitive solver makes (bit j = slot j) and the
    double major_rmin = 0.0, major_rmax = __builtin_inf();   // pgx_set_major_radius_range: the major radii the torus solver accepts (context state; its tube radii read rmin, rmax)
    double prim_smin = 0.0, prim_smax = 1.0;     // sines its cones may have (context state; its spheres and cylinders read rmin, rmax)
    pgx::ScoreSwitches score_sw;   // PGX_NO_FILTER, PGX_SCORE_NO_CULL, PGX_SCORE_MIRROR, PGX_VERIFY and pgx_score_debug_geometry: what plan_score reads (score_plan.h)
    pgx::DevBuf stats_buf;         // work counters of a pgx_score_stats launch
    // spatially sorted copies for the score kernel (group-level rejection); aliases of the originals
    // when point_sort is off
    int point_sort = 0;          // 1: pts_s / pts32_s / pmax_s / comp_s hold the points in Morton order, pperm maps back
    int group_filter = 1;        // PGX_NO_GROUP=1 disables the sorted copies and the group test (A/B)
    int comp_dirty = 0;          // comp changed since comp_s was gathered
    pgx::DevBuf pts_s, pts32_s, pmax_s, comp_s, pperm, gbounds, masks_s;
    pgx::DevBuf pts_g, p32_g;    // group-blocked SoA copies of the sorted rows: [group][coordinate][64] (group-major kernel)
    int setpoints_host = 0;      // PGX_SETPOINTS_HOST=1: round 1's host preprocessing in pgx_set_points (A/B, cross-check)
    double sp_kd_weight = 0.25;  // weight of the 3-D part against the observed pair in the k-d order (1 = box normalisation); no switch sets it
    int sp_kd = 1;               // PGX_SP_KD=0: Morton order of the points of a pose problem instead of the k-d order (setpoints.hip)
    pgx::DevBuf weights_scratch; // scratch of the k-d build (64-bit keys, sort workspace, per-node extents)
    pgx::DevBuf cull_lists, cull_counts;
    pgx::DevBuf score_wl;        // work lists of the group-major kernel (score_worklist.h): counts | 8 x 4 lists of (group, 4-word) items
    int score_wl_last = 0;       // the last group-major launch took its items from the lists (their counts: pgx_score_debug_fetch(6))
    int score_wl_dirty = 0;      // a launch got past its cull kernel but not to its finish kernel: the counts may not be zero
    pgx::DevBuf gc;          // inlier/outlier graph cut: e[n] | dq[2][n] | wq[E] | labels[n]
    pgx::DevBuf gc_sel;      // ... the inliers' indices (pgx_gc_inliers): index[n] | count | select scratch

    // scoring
    // The resident hypothesis batch and what the last launch produced of it: one owner, changed only by its events (score_plan.h
    // ScoreBatch; compiled into the CPU tests too).  Every entry point that reads results asks it whether they belong to the batch.
    pgx::ScoreBatch batch;
    int64_t score_global_n = 0;  // pgx_score_set_global_n: the fixed-point scale of the sums is taken from max(n, this) - the ranks of a
                                 // point-sharded job (pgx_score_allreduce) then add integers of the SAME scale: bitwise the unsharded sums
    pgx::DevBuf models, pcnt, pval, psh, counts, values, shared, masks;
    pgx::DevBuf perm;        // perm[sorted position] = caller's hypothesis index (locality ordering, capi.hip)
    int score_sort = 1;      // PGX_NO_SORT=1 keeps the caller's order (A/B)
    pgx::DevBuf g_counts, g_values, g_shared;  // all-gathered results (multi-GPU)

    // preference slots + reductions
    std::vector<pgx::DevBuf> slots;
    pgx::DevBuf red_partials, red_out;

    // PEARL
    int L = 0;          // labels of the resident unary table
    int64_t dq_n = 0;   // sites of the resident unary table
    pgx::DevBuf dq;     // label-major [L][n] int64
    int64_t dq_max = 0; // upper bound of the table's entries (pgx_pearl_unary: 2^33; pgx_set_unary_q: the actual maximum)
    pgx::DevBuf kmodels;
    pgx::DevBuf labels; // int32 [n]
    int64_t labels_n = 0;
    // Everything pgx_expansion remembers between calls - the first-cycle memo, the last fixed point, the labels' version, the unary
    // columns' identities - and the events that change it (expansion_cycle.h ExpansionState: one owner, compiled into the CPU tests too).
    pgx::ExpansionState expansion;
    struct MemoSnapshots {        // the memo's device side (expansion.hip): [rows][n] int32, the labels after first-cycle move alpha
        pgx::DevBuf buf;
        int rows = 0;
        int64_t n = 0;
    } memo_snaps;
    // graph (symmetric CSR)
    int64_t gn = 0, gE = 0;
    int max_degree = 0;
    int64_t max_row_mult = 0;
    pgx::DevBuf goff, gidx, gmult, grev;
    pgx::MaxflowState* mf = nullptr;
    // tile-resident min-cut (maxflow_tile.hip), the default path of an expansion move
    pgx::TileState* tile = nullptr;
    int64_t graph_version = 0;   // bumped whenever the resident graph changes (graph_build_reverse)
    pgx::DevBuf gorder;          // sites in the Morton order of the coordinates the graph was built on (graph.hip); gorder_n == gn when valid
    int64_t gorder_n = 0;
    pgx::RouteSwitches route;    // PGX_MF_TILE, PGX_MF_TILE_BATCH, PGX_MF_REGION, PGX_GC_FLIP, PGX_TILE_EXPANSION_MAX: which solver takes a move (move_route.h)
    int tile_order = 1;          // sites of the tile path in the Morton order of the graph's coordinates (0: the caller's order)
    int mf_xcd = 1;              // PGX_MF_XCD=0: no persistent one-XCD rounds (maxflow_xcd.hip.h); read at pgx_create like the switches above
    int mf_xcd_search = 1;       // PGX_MF_XCD_SEARCH=0: no one-launch global relabels
    int mf_xcd_min_depth = 24;   // PGX_MF_XCD_MIN_DEPTH: a search runs as one launch when the previous search of its kind was deeper than this
    long long mf_xcd_max_n = 300000;   // PGX_MF_XCD_MAXN: graphs beyond this stay on level launches (measured: maxflow.hip)
    int mf_sweeps = 0;           // PGX_MF_SWEEPS: sweeps per round, list mode and all-sites alike (0 = the measured defaults; tests shorten the rounds)
    int tile_sweeps = 24;        // push-relabel sweeps per discharge launch
    int tile_mini = 1;           // PGX_TILE_MINI=0: graphs of <= 1024 sites and <= 8192 arcs go through t_move_kernel too (A/B; default: the LDS-resident t_mini_kernel)
    int64_t tile_launches[2] = {0, 0};   // pgx_one_workgroup_launches: whole-graph moves enqueued on t_mini_kernel / on t_move_kernel
    int tile_mini_sweeps = 24;   // PGX_TILE_MINI_SWEEPS: sweeps between two exact searches of t_mini_kernel
    int64_t paths[6] = {0, 0, 0, 0, 0, 0};   // pgx_expansion_paths
    int64_t tile_fallbacks = 0;  // moves the tile path handed back to maxflow.hip
    int tile_debug = 0;          // PGX_MF_DEBUG: one stderr line per global relabel
    int64_t stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    pgx::DevBuf scratch;  // misc small device scratch (bucket, energy, ...)
    pgx::DevBuf prosac_tops;              // pgx_sampler_prosac_set: subset size per sample number (int32 x prosac_count)
    int prosac_count = 0;
    int64_t prosac_points_version = -1;   // the table belongs to these points
    void* h_rb = nullptr;       // pinned ring of d2h() / sync_deliver()
    size_t h_rb_used = 0;
    std::vector<pgx::StagedCopy> rb;
    pgx::PinnedBuf h_res;       // pinned host staging for result read-backs (pageable targets make the copies synchronous): host_staging
    pgx::PinnedStage h_models;  // pgx_score_upload's (reordered) batch + permutation
    pgx::PinnedStage h_samples; // pgx_solve_minimal's sample indices (solve.hip upload_samples)
    // Host mirror of the score triples: score_finish_kernel also writes (count, value, shared) in the batch's device order
    // straight into this pinned, device-mapped allocation (coalesced 512 B runs over PCIe), so pgx_score_fetch needs no
    // copy command on the stream - it waits for the kernel and un-permutes on the host (batch.unpermute()).
    pgx::PinnedBuf h_mirror;
    pgx::DevBuf fit_scratch;  // pgx_gram: partials | result | counters | index list
    pgx::DevBuf weights;      // resident per-point weights of the weighted refits (pgx_set_weights), weights_n == n when valid
    int64_t weights_n = 0;
    pgx::DevBuf normals;      // resident per-point normals n x 3, caller's order (pgx_set_normals), normals_n == n when valid: only the
    int64_t normals_n = 0;    // cylinder's, the cone's and the mixed-primitive minimal solvers read them - and an ORIENTED type's residual:
    int oriented = 0;         // the resident type is one (Residual<MT>::oriented).  Its normals and kappa also lie behind the rows of pts, pts_s
    double normal_cos2 = 0.0; // and pts_g (residuals.hip.h; place_oriented_normals).  kappa = cos^2(tolerance), pgx_set_normal_tolerance (context state)
    int64_t oriented_version = 0;   // bumped when an oriented type's normals or kappa change: part of a unary column's identity
    pgx::DevBuf cc_buf;       // pgx_label_components: its labels, parent[], counters, ranks and results (components.hip); nothing resident reads it
    pgx::DevBuf ext_buf;      // pgx_instance_extents: its points, labels, frames, table and results (extents.hip); nothing resident reads it

    pgx::CommState* comm = nullptr;
};

namespace pgx {

int fail(pgx_ctx* ctx, int code, const char* fmt, ...);
int ensure(pgx_ctx* ctx, DevBuf& b, size_t bytes);
// An oriented type's squared residual reads the resident normals: every entry point that evaluates it refuses without them (PGX_OK for
// every other type).
int need_oriented_normals(pgx_ctx* ctx, const char* who);
// Small read-backs go through pinned memory: a copy into a pageable target is a BLOCKING command (14 us against 4 for one into pinned
// memory, scripts/micro/small_copy_bench.hip), and an entry point that returns three small arrays paid it three times.  d2h() enqueues the
// copy into a slice of a pinned ring and remembers where the bytes belong; sync_deliver() synchronises the stream once and hands them
// over.  (Copies beyond 32 KB, or when the ring is full, go straight to the target as before.)  Pairs live inside one function body;
// every entry point starts with an empty list (CTX_GUARD).
int d2h(pgx_ctx* ctx, void* dst, const void* src, size_t bytes);
int sync_deliver(pgx_ctx* ctx);
int grow_pinned(pgx_ctx* ctx, PinnedBuf& b, size_t bytes, unsigned flags = hipHostMallocDefault);   // b.p holds at least `bytes` (twice that when it grows; the old contents are not kept)
void release(PinnedBuf& b);
int host_staging(pgx_ctx* ctx, size_t bytes, void** p);   // ctx->h_res grown to at least `bytes` (pinned: a copy into it is one asynchronous command; a pageable target makes every copy a blocking one)
void release(DevBuf& b);

#define PGX_HIP(ctx, call)                                                                        \
    do {                                                                                          \
        hipError_t e_ = (call);                                                                   \
        if (e_ != hipSuccess)                                                                     \
            return pgx::fail(ctx, PGX_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), \
                             __FILE__, __LINE__);                                                 \
    } while (0)

#define PGX_TRY(call)               \
    do {                            \
        int r_ = (call);            \
        if (r_ != PGX_OK) return r_; \
    } while (0)

inline int64_t quantize(double x) { return (int64_t)__builtin_nearbyint(x * 4294967296.0); }
// weight of one directed neighbour entry, forced even so that w/2 is exact in the expansion graph
inline int64_t quantize_lambda(double lambda) { return 2 * (int64_t)__builtin_nearbyint(lambda * 2147483648.0); }

// group bounds of the score path (score.hip consumes them, setpoints.hip / score_sort_points build them)
constexpr double kGroupInflate = 1.00001;
constexpr int kGroupRow = 12;  // floats per group: c[3], rho, ub, vb, ru, rv, scale, pad[3]

// launchers implemented in the .hip translation units
int set_points_device(pgx_ctx* ctx, const ModelInfo& mi, const double* points, int64_t n);  // setpoints.hip: upload + all preprocessing
int score_launch(pgx_ctx* ctx, double T2, int has_compound, int want_masks, bool want_counters = false);   // score.hip: plan_score -> buffers -> launches -> batch.launched
int score_inliers_launch(pgx_ctx* ctx, int row, int32_t* index, int64_t* count);   // pointwise.hip
// point-sharded exchange (comm.hip): the last launch's integer accumulators, replicas summed, in the caller's hypothesis order
// ([3][Mpad] words) / counts | values | shared from such a block
int score_acc_export(pgx_ctx* ctx, unsigned long long* out, hipStream_t stream);
int score_acc_import(pgx_ctx* ctx, const unsigned long long* in, int M, int Mpad, double qscale, long long* counts, double* values,
                     double* shared, hipStream_t stream);
int score_sort_points(pgx_ctx* ctx, const ModelInfo& mi, const double* points, const float* p32, const double* pmax);  // builds the sorted copies
int preference_launch(pgx_ctx* ctx, const double* model, double T2, double* d_pref, double out3[3]);
int compound_launch(pgx_ctx* ctx, const int32_t* slots, int K);
int unary_launch(pgx_ctx* ctx, int K, double threshold, double lambda);
int residual_sum_launch(pgx_ctx* ctx, const double* model, int label, double* sum);
int bucket_launch(pgx_ctx* ctx, int L, int64_t* counts, int32_t* order);
int energy_launch(pgx_ctx* ctx, int64_t lambda_q, int64_t h_q, int64_t* energy_q);
int greedy_labeling_launch(pgx_ctx* ctx, int64_t h_q, int64_t* energy_q, int* opened);
int epipolar_support_launch(pgx_ctx* ctx, const double* F, double T2, double S2, int64_t counts[2]);
int gc_labeling_launch(pgx_ctx* ctx, const double* model, double T2, double lambda, int32_t* flags, int64_t* count, bool want_index = false);
int graph_build_reverse(pgx_ctx* ctx);
int graph_build_launch(pgx_ctx* ctx, const double* pts, int64_t n, int d, int kind, double radius, int k, int64_t* arcs);
int graph_fetch_launch(pgx_ctx* ctx, int32_t* off, int32_t* idx, int32_t* mult);
int solve_minimal_launch(pgx_ctx* ctx, const int32_t* samples, int S, double* models_out, bool resident = false);   // resident: the samples are in ctx->scratch already
int solve_minimal_sampled_launch(pgx_ctx* ctx, int sampler, uint64_t key, uint32_t batch, int S, int32_t* samples_out, double* models_out);
int sampler_prosac_set(pgx_ctx* ctx, const int32_t* tops, int count);
int gram_launch(pgx_ctx* ctx, int kind, const double* params, int nparams, int sel, const int32_t* index, int64_t m,
                int label, int use_weights, int wpow, double* out, int64_t* count, int64_t* bad);
int gram_labels_launch(pgx_ctx* ctx, int kind, const double* params, int nparams, int K, int use_weights, int wpow,
                       double* out, int64_t* count, int64_t* bad);
int residual_sums_launch(pgx_ctx* ctx, const double* models, int K, double* sums);
int gram_batch_launch(pgx_ctx* ctx, int kind, const double* params, int nparams, const int32_t* index, int B, int m,
                      const double* wsel, int wpow, double* out, int32_t* bad);
int pnp_refine_batch_launch(pgx_ctx* ctx, const double* inits, const int32_t* index, int B, int m, const double* wsel, int wpow,
                            int iterations, double* out, int32_t* status);
// One expansion move, as its caller states it and as the solvers report on it (maxflow.hip run_move walks the planner's list with it).
enum class MoveOutcome { Done, HandedBack, Pending };   // solved (`changed` set) | not solved, labels untouched: the next solver | enqueued in the batch: region_result
struct MoveRequest {
    int64_t n = 0;                  // the tables: dq [L][n] label-major, labels [n], optionally per-arc weights wq [E] (the inlier / outlier cut)
    int L = 0, alpha = 0;
    const long long *dq = nullptr, *wq = nullptr;
    int* labels = nullptr;
    int64_t lambda_q = 0, h_q = 0;
    bool source_reach = false;      // alpha goes to the sites the SOURCE reaches (the flipped cut; level-synchronous only)
    int batch_slot = -1;            // >= 0: enqueued in this slot of pgx_expansion's batch, no host round trip ...
    int skip_rel = -1;              // ... and skipped on the device if exactly this many moves of the batch before it relabelled something (-1: always runs)
    bool region_declined = false;   // the batch gave this move back: from scratch, without the region path
    // work enqueued BEHIND an unbatched whole-graph move and BEFORE its one synchronisation (the compaction of the cut's flags and its
    // copy back: one host round trip for both); pre_sync_ran: it was enqueued and the solver did not give the move up
    int (*pre_sync)(pgx_ctx*, const MoveRequest&) = nullptr;
    bool pre_sync_ran = false;
    int64_t changed = 0;            // results
    MoveOutcome outcome = MoveOutcome::Done;
};
int expand_alpha_launch(pgx_ctx* ctx, MoveRequest& rq);   // a move on the resident problem: fills in the tables (the caller gives lambda_q, h_q, alpha, the batch fields)
int expand_cycle_l0(pgx_ctx* ctx, int64_t h_q, int64_t* changed, int* evaluated);  // lambda = 0: all labels, one read-back
// expansion.hip: pgx_expansion on the resident problem, the cycles driven by expansion_cycle.h run_expansion.  allow_shortcut = false: the
// cycle runs even when the call could be answered from the last fixed point (what PGX_MF_DONE_VERIFY compares the answer with)
int expansion_launch(pgx_ctx* ctx, int64_t lambda_q, int64_t h_q, int max_cycles, bool allow_shortcut, int64_t* energy_q, int* cycles);
void expansion_points_changed(pgx_ctx* ctx);   // pgx_set_points: the event, and the memo's snapshots of the old point set released
int run_move(pgx_ctx* ctx, MoveRequest& rq);              // lambda > 0, any tables
void maxflow_free(pgx_ctx* ctx);
int maxflow_schedule_stats(pgx_ctx* ctx, int64_t out[8]);   // maxflow.hip
int eigh_smallest_launch(pgx_ctx* ctx, const double* A, int q, int64_t B, double* vec, double* val);   // fit.hip
int estimate_normals_launch(pgx_ctx* ctx, const double* points, int64_t n, const double* viewpoint, double* normals_out,
                            double* curvature_out, int64_t* undefined);   // normals.hip
int label_components_launch(pgx_ctx* ctx, const int32_t* labels, int64_t n, int32_t first_ignored, int32_t* comp_out, int32_t* first_out,
                            int64_t* sizes_out, int64_t* components);   // components.hip
int instance_extents_launch(pgx_ctx* ctx, const double* points, int64_t n, const int32_t* labels, const double* frames, int32_t K,
                            int64_t* count_out, double* lo_out, double* hi_out, uint64_t* sectors_out, uint64_t* occupancy_out,
                            int64_t* skipped);   // extents.hip
int expand_alpha_tile(pgx_ctx* ctx, MoveRequest& rq);   // maxflow_tile.hip: the whole graph in one workgroup, one launch
void tile_free(pgx_ctx* ctx);
struct MfView;
int region_batch_begin(pgx_ctx* ctx);
int region_batch_fetch(pgx_ctx* ctx, int slots);   // the batch's results to the host mirror (one copy), before the synchronisation
int region_result(pgx_ctx* ctx, int slot, int alpha, int* status, int64_t* changed);
int expand_alpha_region(pgx_ctx* ctx, MoveRequest& rq, const MfView& mv);   // maxflow_tile.hip: a move with few open sites, one workgroup
void comm_free(pgx_ctx* ctx);

}  // namespace pgx
