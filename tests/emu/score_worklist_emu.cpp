// score_worklist_emu.cpp — csrc/score_worklist.h as libpgx.so compiles it, for tests/test_score_worklist_index.py: the header's
// functions one by one, and the two sides of the lists replayed on the CPU with the header driving them - the cull kernel's append
// of a table of item weights, and the group kernel's grid taking one item per workgroup.
#include <cstdint>
#include <vector>

#include "../../progressive-x_amd/csrc/score_plan.h"
#include "../../progressive-x_amd/csrc/score_worklist.h"

extern "C" {

int wl_consts(int what)
{
    const int v[] = {pgx::kWlXcds, pgx::kWlClasses, pgx::kWlItemWords, pgx::kWlCountStride, pgx::kWlCountWords};
    return v[what];
}
int wl_emu_class(unsigned weight, unsigned t1, unsigned t2, unsigned t3) { return pgx::wl_class(weight, t1, t2, t3); }
int wl_emu_xbits(int columns) { return pgx::wl_xbits(columns); }
int wl_emu_fits(int64_t groups, int columns) { return pgx::wl_fits(groups, columns) ? 1 : 0; }
uint32_t wl_emu_item(uint32_t g, uint32_t x, int xbits) { return pgx::wl_item(g, x, xbits); }
uint32_t wl_emu_item_group(uint32_t item, int xbits) { return pgx::wl_item_group(item, xbits); }
uint32_t wl_emu_item_column(uint32_t item, int xbits) { return pgx::wl_item_column(item, xbits); }
int wl_emu_count_index(int xcd, int cls) { return pgx::wl_count_index(xcd, cls); }
// returns the class (0 .. 3) and the position through *pos, or -1 when the slot is at or past the total
int wl_emu_locate(const uint32_t c[4], uint32_t slot, uint32_t* pos)
{
    int cls = -7;
    return pgx::wl_locate(c[0], c[1], c[2], c[3], slot, &cls, pos) ? cls : -1;
}

// weights [groups][columns] -> the buffer the cull kernel leaves (counts | 8 x 4 lists of `cap` items), appended tile by tile in the
// order tiles[] names them (a tile = 64 groups x one column), then the grid of 8 * cap workgroups: taken[g * columns + x] = how many
// workgroups ran item (g, x), order[b] = the weight workgroup b ran (0: it left).  Returns the number of workgroups that ran an item,
// or -1 if an append fell outside its list.
int64_t wl_emu_run(const uint32_t* weights, int groups, int columns, const uint32_t t[3], const int32_t* tiles, int ntiles,
                   uint32_t* counts_out, int32_t* taken, uint32_t* order)
{
    using namespace pgx;
    const int xbits = wl_xbits(columns);
    const uint32_t cap = (uint32_t)((groups + kWlXcds - 1) / kWlXcds) * (uint32_t)columns;
    std::vector<uint32_t> wl((size_t)kWlCountWords + (size_t)kWlXcds * kWlClasses * cap, 0u);
    const int tiles_per_column = (groups + 63) / 64;
    for (int k = 0; k < ntiles; ++k) {
        const int x = tiles[k] / tiles_per_column, t0 = (tiles[k] % tiles_per_column) * 64;
        for (int i = 0; i < 64 && t0 + i < groups; ++i) {
            const uint32_t g = (uint32_t)(t0 + i), wt = weights[(size_t)g * columns + x];
            if (wt == 0) continue;
            const int list = (int)(g & 7u) * kWlClasses + wl_class(wt, t[0], t[1], t[2]);
            const uint32_t pos = wl[(size_t)list * kWlCountStride]++;
            if (pos >= cap) return -1;
            wl[(size_t)kWlCountWords + (size_t)list * cap + pos] = wl_item(g, (uint32_t)x, xbits);
        }
    }
    for (int xcd = 0; xcd < kWlXcds; ++xcd)
        for (int c = 0; c < kWlClasses; ++c) counts_out[xcd * kWlClasses + c] = wl[(size_t)wl_count_index(xcd, c)];
    int64_t ran = 0;
    for (uint32_t b = 0; b < (uint32_t)kWlXcds * cap; ++b) {
        const int xcd = (int)(b & 7u);
        int cls;
        uint32_t pos;
        order[b] = 0;
        if (!wl_locate(wl[(size_t)wl_count_index(xcd, 0)], wl[(size_t)wl_count_index(xcd, 1)], wl[(size_t)wl_count_index(xcd, 2)],
                       wl[(size_t)wl_count_index(xcd, 3)], b >> 3, &cls, &pos))
            continue;
        const uint32_t item = wl[(size_t)kWlCountWords + (size_t)(xcd * kWlClasses + cls) * cap + pos];
        const uint32_t g = wl_item_group(item, xbits), x = wl_item_column(item, xbits);
        if (g >= (uint32_t)groups || x >= (uint32_t)columns || (int)(g & 7u) != xcd) return -1;
        ++taken[(size_t)g * columns + x];
        order[b] = weights[(size_t)g * columns + x];
        ++ran;
    }
    return ran;
}

// The planner's work-list decision (csrc/score_plan.h) for a type given by its traits on sorted points inside every filter window:
//   in = bound, homography, n, Mpad, ordered, want_masks, want_counters | switches split, group_xcd, cull_segs, worklist, t1, t2, t3
//   out = path, worklist, wl_columns, wl_xbits, wl_cap, wl_grid, t[3], split, gblocks, group_xcd
void wl_emu_plan(const int64_t in[14], int64_t out[12])
{
    pgx::ScoreTraits tr;
    tr.filter64 = true; tr.filter32 = true; tr.bound = (int)in[0]; tr.homography = in[1] != 0;
    pgx::ScoreSwitches sw;
    sw.split = (int)in[7]; sw.group_xcd = (int)in[8]; sw.cull_segs = (int)in[9]; sw.worklist = (int)in[10];
    sw.wl_t1 = (int)in[11]; sw.wl_t2 = (int)in[12]; sw.wl_t3 = (int)in[13];
    const pgx::ScorePlan p = pgx::plan_score(tr, sw, 256, in[2], (int)in[3], (int)in[3], in[4] != 0, true, 1.0, 1.0, 1.0, 0, in[5] != 0, in[6] != 0);
    const int64_t o[12] = {p.path, p.worklist, p.wl_columns, p.wl_xbits, p.wl_cap, p.wl_grid, p.wl_t[0], p.wl_t[1], p.wl_t[2], p.split,
                           (int64_t)p.gblocks, p.group_xcd};
    for (int k = 0; k < 12; ++k) out[k] = o[k];
}

}  // extern "C"
