// extents_driver.cpp — runs the per-point statements of csrc/extents_point.h on the CPU (TEST INFRASTRUCTURE,
// tests/test_extents_cpu.py): the lines the three launches of extents.hip run per lane, here point by point on a plain table - bounds,
// finalise, occupancy - in the order given.  Compiled with -ffp-contract=off like the library.
#include <cstdint>
#include <vector>

#include "../../progressive-x_amd/csrc/extents_point.h"

namespace {

struct PlainTab {   // the three updates without atomics
    uint64_t* w;
    void add(int64_t i, uint64_t x) { w[i] += x; }
    void max(int64_t i, uint64_t x) { w[i] = w[i] > x ? w[i] : x; }
    void bor(int64_t i, uint64_t x) { w[i] |= x; }
};

}  // namespace

extern "C" {

// group > 1: contributions of up to `group` consecutive points of one label are combined first (ext_combine), as a wave does, and the
// points go into a partial table that is merged word by word at the end (ext_merge_word), as a workgroup's LDS table is
int ext_emu_run(const double* points, int64_t n, const int32_t* labels, const double* frames, int32_t K, int group, int64_t* count,
                double* lo, double* hi, uint64_t* sectors, uint64_t* occupancy, int64_t* skipped)
{
    using namespace pgx;
    std::vector<uint64_t> table((size_t)K * EXT_SLOTS + 1, 0), partial((size_t)K * EXT_SLOTS + 1, 0);
    PlainTab tab{group > 1 ? partial.data() : table.data()};
    int64_t dead = 0;
    ExtAcc run = {};
    int run_label = -1, run_len = 0;
    for (int64_t i = 0; i < n; ++i) {
        const int l = labels[i];
        if (l < 0 || l >= K) continue;
        ExtPoint p;
        if (!ext_point(frames + (int64_t)l * kExtFrame, points[3 * i], points[3 * i + 1], points[3 * i + 2], p)) {
            ++dead;
            continue;
        }
        const ExtAcc a = ext_contribution(p);
        if (group <= 1) {
            ext_merge(tab, l, a);
        } else if (run_len && l == run_label && run_len < group) {
            ext_combine(run, a);
            ++run_len;
        } else {
            if (run_len) ext_merge(tab, run_label, run);
            run = a;
            run_label = l;
            run_len = 1;
        }
    }
    if (group > 1) {
        if (run_len) ext_merge(tab, run_label, run);
        PlainTab out{table.data()};
        for (int64_t w = 0; w < (int64_t)K * EXT_SLOTS; ++w) ext_merge_word(out, w, partial[(size_t)w]);
    }
    for (int32_t j = 0; j < K; ++j) {
        const uint64_t* row = table.data() + (size_t)j * EXT_SLOTS;
        ext_finalise(row, lo + 2 * j, hi + 2 * j);
        count[j] = (int64_t)row[EXT_COUNT];
        sectors[2 * j] = row[EXT_SEC_A];
        sectors[2 * j + 1] = row[EXT_SEC_B];
        occupancy[j] = 0;
    }
    for (int64_t i = 0; i < n; ++i) {
        const int l = labels[i];
        if (l < 0 || l >= K) continue;
        ExtPoint p;
        if (ext_point(frames + (int64_t)l * kExtFrame, points[3 * i], points[3 * i + 1], points[3 * i + 2], p))
            occupancy[l] |= ext_occupancy_bit(p, lo + 2 * l, hi + 2 * l);
    }
    *skipped = dead;
    return 0;
}

void ext_emu_sectors(const double* x, const double* y, int64_t n, int32_t* out)
{
    for (int64_t i = 0; i < n; ++i) out[i] = pgx::ext_sector(x[i], y[i]);
}

// key -> double -> key, and whether the keys order as the doubles do
int ext_emu_keys(const double* x, int64_t n, uint64_t* keys, double* back)
{
    int ordered = 1;
    for (int64_t i = 0; i < n; ++i) {
        keys[i] = pgx::ext_key(x[i]);
        back[i] = pgx::ext_unkey(keys[i]);
        if (keys[i] == 0 || ~keys[i] == 0) ordered = 0;
        if (i && ((x[i - 1] < x[i]) != (keys[i - 1] < keys[i]) || (x[i - 1] > x[i]) != (keys[i - 1] > keys[i]))) ordered = 0;
    }
    return ordered;
}

}
