// score_plan_driver.cpp — walks the planner and the batch owner of csrc/score_plan.h under AddressSanitizer +
// UndefinedBehaviorSanitizer (TEST INFRASTRUCTURE, scripts/sanitize.sh).  What the planner answers is checked against the decisions
// it replaced by tests/test_score_plan.py; this run checks the shape of every answer (a chunking that covers the points, a group-major
// geometry only on path 2, a split within the hypothesis words) on that test's grid and at the ends of the ranges pgx_set_points,
// pgx_score_upload and pgx_score_debug_geometry let through, and drives ScoreBatch through seeded random event scripts.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <random>
#include <vector>

#include "../../progressive-x_amd/csrc/score_plan.h"

int main()
{
    using namespace pgx;
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    const int64_t ns[] = {1, 63, 64, 65, 511, 512, 513, 4096, 1000000, ((int64_t)1 << 31) - 1};
    const int mpads[] = {64, 256, 320, 512, 2048, 1 << 20};
    const double t2s[] = {0.0, -1.0, 5e-324, 1e-24, 1e-12, 1.0, 1e12, 1e24, 1e30, 1e300, inf, nan};
    const double scales[] = {0.0, 1.0, 16384.0, 1e30, 1e300, inf, nan};
    long long points = 0;
    for (int type = 0; type < 16; ++type) for (int64_t n : ns) for (int Mpad : mpads) for (double T2 : t2s) for (double s : scales)
    for (int bits = 0; bits < 64; ++bits) {
        ScoreTraits tr;
        tr.filter64 = type & 1; tr.filter32 = (type >> 1) & 1; tr.bound = type >> 2; tr.homography = tr.bound == kBoundBox && (bits & 32);
        ScoreSwitches sw;
        sw.filter_enabled = bits % 3; sw.cull = (bits >> 2) & 1; sw.mirror = (bits >> 3) & 1; sw.verify = (bits >> 4) & 1;
        sw.split = (bits & 1) ? 1024 : 0; sw.group_xcd = bits % 3 - 1; sw.nrep = (bits & 2) ? 1024 : 0; sw.dense_min = 1 + bits;
        sw.cull_segs = (bits & 4) ? 65535 : 1;
        const bool masks = bits & 8, counters = bits & 16;
        const ScorePlan p = plan_score(tr, sw, bits & 1 ? 0 : 256, n, Mpad, Mpad, bits & 2, bits & 1, T2, s, s, bits & 4 ? 50000000 : 0, masks, counters,
                                       bits & 32 ? 1 : kScoreBlocksPerCu);
        bool ok = p.chunk >= 64 && p.chunk % 64 == 0 && p.chunk <= 65536 * 64 && p.chunks >= 1 && p.chunks <= kScoreMaxChunks &&
                  p.chunk * p.chunks >= n && p.words == (n + 63) / 64 && p.filter >= 0 && p.filter <= 2;
        if (p.path == 2)
            ok = ok && tr.filter32 && p.filter == 2 && sw.cull && p.groups == (int)p.words && p.W == Mpad / 64 && p.split >= 1 && p.split <= p.W &&
                 (int64_t)p.gps * p.cull_segs >= p.groups && p.gps % kSuper == 0 && p.nrep >= 1 &&
                 p.zero_words == (int64_t)3 * p.nrep * Mpad && p.qscale >= 1.0 && p.qscale <= 1125899906842624.0 && !(p.mirror && masks) &&
                 !(p.counters && masks) && (!p.verify || p.counters);
        else
            ok = ok && p.path == 1 && p.groups == 0 && p.gblocks == 0 && !p.mirror && !p.counters && p.qscale == 0.0;
        if (!ok) {
            std::fprintf(stderr, "plan_score: malformed plan at type=%d n=%lld Mpad=%d T2=%g scale=%g switches=%d\n", type, (long long)n, Mpad, T2, s, bits);
            return 1;
        }
        ++points;
    }
    // ScoreBatch: random events; the order handed out is the one uploaded, and a table is Ready only for the batch it was launched for
    std::mt19937 rng(7);
    long long events = 0;
    for (int script = 0; script < 200; ++script) {
        ScoreBatch sb;
        std::vector<int> perm;
        unsigned long long acc[4] = {0, 0, 0, 0};
        bool launched_current = false;
        for (int step = 0; step < 200; ++step, ++events) {
            const int e = (int)(rng() % 6);
            if (e == 0) { sb.points_changed(); launched_current = false; }
            else if (e == 1) {
                const int M = 1 + (int)(rng() % 3000);
                perm.resize((size_t)M);
                for (int m = 0; m < M; ++m) perm[(size_t)m] = M - 1 - m;
                sb.uploaded(M, (M + 255) / 256 * 256, (rng() & 1) ? perm.data() : nullptr);
                launched_current = false;
            } else if (e == 2) { sb.generated(1 + (int)(rng() % 3000), 3072); launched_current = false; }
            else if (e == 3 && sb.resident.M > 0) {
                ScorePlan p;
                p.path = 1 + (int)(rng() & 1); p.filter = (int)(rng() % 3); p.words = 9; p.nrep = 8; p.qscale = 1024.0; p.mirror = rng() & 1;
                sb.launched(p, rng() & 1, rng() & 1, acc);
                launched_current = true;
            } else if (e == 4) sb.launch_failed();
            else if (e == 5 && sb.acc_exportable()) sb.table_reduced();
            bool ok = (sb.table() == ScoreTable::Ready) == (launched_current && sb.resident.M > 0);
            ok = ok && (sb.mask_rows() != ScoreTable::Ready || sb.table() == ScoreTable::Ready) && !(sb.acc_exportable() && sb.acc_stale());
            if (const int* pm = sb.unpermute())
                for (int m = 0; m < sb.resident.M; ++m) ok = ok && pm[m] == sb.resident.M - 1 - m;
            if (!ok) {
                std::fprintf(stderr, "ScoreBatch: inconsistent answers in script %d at step %d\n", script, step);
                return 1;
            }
        }
    }
    std::printf("score_plan: %lld plans well-formed, %lld batch events consistent\n", points, events);
    return 0;
}
