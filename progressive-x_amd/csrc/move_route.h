// move_route.h — which min-cut solver takes an expansion move, in which order the others follow, and whether pgx_expansion
// batches the cycle ("Which form takes a move").  No HIP in here: libpgx.so and the CPU tests (tests/emu/mf_emu.cpp,
// tests/test_move_route.py) compile the same function.  The size limits of the routing live in this file and nowhere else.
#pragma once
#include <cstdint>

namespace pgx {

enum class Solver : int { None = 0, Tile = 1, Region = 2, Level = 3 };   // one workgroup on the whole graph (maxflow_tile.hip expand_alpha_tile) |
                                                                          // one workgroup on the open sites (expand_alpha_region) | maxflow.hip's level-synchronous schedule
enum class MoveKind : int {
    Cycle = 0,    // a move of pgx_expansion's cycle on the resident problem: the only kind that may be batched
    Single = 1,   // pgx_expand_alpha: the same move with a host round trip of its own
    Cut = 2       // the inlier / outlier cut (per-arc weights, two labels): never a region move
};

constexpr int kTileMaxSites = 8192;                  // the whole-graph kernels: sites one workgroup takes
constexpr int kRegionMaxDegree = 32;                 // the region path's compact arc rows
constexpr int64_t kRegionMaxSites = (int64_t)1 << 30;
constexpr int kRouteMaxLabels = 64;                  // hub slots of the one-workgroup kernels; moves with more labels are refused before they are routed

struct RouteSwitches {               // read once, at pgx_create
    int mf_tile{1};                  // PGX_MF_TILE=0: no whole-graph one-workgroup moves (A/B)
    int mf_tile_batch{1};            // PGX_MF_TILE_BATCH=0: one host round trip per whole-graph move (A/B)
    int mf_region{1};                // PGX_MF_REGION=0: no region moves
    int gc_flip{1};                  // PGX_GC_FLIP=0: the inlier / outlier cut in its stated orientation (pointwise.hip gc_labeling_launch)
    int tile_expansion_max{1024};    // PGX_TILE_EXPANSION_MAX: expansion moves on larger graphs try the region path first.  1 024 = the LDS-resident
                                     // whole-graph kernel's limit: beyond it the region path with ITS LDS-resident solver is as fast or faster
                                     // (2 000 sites 1.99 vs 2.03 ms per expansion, 5 000 sites 6.2 vs 7.7; unihouse, 2 084 points: 74 -> 67 ms per call)
};

struct MoveRoute {
    Solver order[3] = {Solver::None, Solver::None, Solver::None};   // tried in this order; a solver that declines leaves the labels untouched
    bool flip = false;      // Cut: terminals swapped, alpha goes to the sites the SOURCE reaches (then Level only)
    bool batched = false;   // Cycle: the moves are enqueued back to back, one host round trip per batch
};

// `region_declined`: the move comes back from a batch whose region (or whole-graph) solver gave it up; it is solved from scratch
// without the region path.
inline MoveRoute plan_move(const RouteSwitches& sw, int64_t n, int max_degree, int64_t gn, MoveKind kind, bool region_declined)
{
    MoveRoute r;
    int k = 0;
    const bool tile_fits = sw.mf_tile && n <= kTileMaxSites;
    if (kind == MoveKind::Cut) {
        r.flip = sw.gc_flip && !tile_fits;
        if (!r.flip && tile_fits) r.order[k++] = Solver::Tile;
        r.order[k++] = Solver::Level;
        return r;
    }
    const bool region_ok = !region_declined && sw.mf_region && max_degree >= 1 && max_degree <= kRegionMaxDegree && gn < kRegionMaxSites;
    const bool region_first = region_ok && n > sw.tile_expansion_max;
    if (tile_fits && !region_first) {
        r.order[k++] = Solver::Tile;
        if (region_ok) r.order[k++] = Solver::Region;
    } else if (region_ok) {
        r.order[k++] = Solver::Region;
        if (region_first && tile_fits) r.order[k++] = Solver::Tile;
    }
    r.order[k++] = Solver::Level;
    r.batched = kind == MoveKind::Cycle && !region_declined &&
                (r.order[0] == Solver::Region || (r.order[0] == Solver::Tile && sw.mf_tile_batch));
    return r;
}

}  // namespace pgx
