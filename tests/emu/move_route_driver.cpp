// move_route_driver.cpp — walks the planner of csrc/move_route.h under AddressSanitizer + UndefinedBehaviorSanitizer (TEST
// INFRASTRUCTURE, scripts/sanitize.sh).  The routes themselves are checked against the predicates they replaced by
// tests/test_move_route.py; this run checks the shape of every answer (a list without holes or repeats that ends in Level,
// only a one-workgroup solver in front of a batched cycle) on that test's grid and at the ends of the argument types.
#include <cstdint>
#include <cstdio>

#include "../../progressive-x_amd/csrc/move_route.h"

int main()
{
    using namespace pgx;
    const int64_t ns[] = {INT64_MIN, -1, 0, 1, 1024, 1025, 4096, 8192, 8193, 300000, ((int64_t)1 << 30) - 1, (int64_t)1 << 30, INT64_MAX};
    const int degrees[] = {INT32_MIN, -1, 0, 1, 32, 33, INT32_MAX};
    const int limits[] = {INT32_MIN, 0, 1024, 8192, INT32_MAX};
    long long points = 0;
    for (int64_t n : ns) for (int deg : degrees) for (int tem : limits) for (int bits = 0; bits < 16; ++bits)
    for (int kind = 0; kind < 3; ++kind) for (int declined = 0; declined < 2; ++declined) {
        RouteSwitches sw;
        sw.mf_tile = bits & 1; sw.mf_tile_batch = (bits >> 1) & 1; sw.mf_region = (bits >> 2) & 1; sw.gc_flip = (bits >> 3) & 1;
        sw.tile_expansion_max = tem;
        const MoveRoute r = plan_move(sw, n, deg, n, (MoveKind)kind, declined != 0);
        int len = 0;
        while (len < 3 && r.order[len] != Solver::None) ++len;
        bool ok = len >= 1 && r.order[len - 1] == Solver::Level;
        for (int k = len; k < 3; ++k) ok = ok && r.order[k] == Solver::None;
        for (int k = 0; k < len; ++k) for (int j = 0; j < k; ++j) ok = ok && r.order[j] != r.order[k];
        if (r.batched) ok = ok && kind == (int)MoveKind::Cycle && !declined && (r.order[0] == Solver::Tile || r.order[0] == Solver::Region);
        if (r.flip) ok = ok && kind == (int)MoveKind::Cut && len == 1;
        if (kind == (int)MoveKind::Cut || declined) for (int k = 0; k < len; ++k) ok = ok && r.order[k] != Solver::Region;
        if (!ok) {
            std::fprintf(stderr, "plan_move: malformed route at n=%lld degree=%d limit=%d switches=%d kind=%d declined=%d\n",
                         (long long)n, deg, tem, bits, kind, declined);
            return 1;
        }
        ++points;
    }
    std::printf("move_route: %lld routes well-formed\n", points);
    return 0;
}
