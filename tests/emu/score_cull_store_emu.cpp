// score_cull_store_emu.cpp — csrc/score_worklist.h wl_tile_store_index, the thread -> keep word mapping of score_cull_kernel's tile
// store, compiled for the host as libpgx.so compiles it for the device (tests/test_score_cull_store.py).
#include <cstdint>

#include "../../progressive-x_amd/csrc/score_worklist.h"

extern "C" {

int wl_emu_item_words_per_workgroup() { return pgx::kWlItemWords; }

// every thread of workgroup x stores its word of the tile: keep[index] = value(group, word) where the index is not -1.
// Returns the number of stores, or -1 - a store outside keep[0, groups * W).
int64_t wl_emu_tile_store(uint64_t* keep, int64_t groups, int W, int t0, int cnt, int x)
{
    int64_t stores = 0;
    for (int t = 0; t < 64 * pgx::kWlItemWords; ++t) {
        const int64_t at = pgx::wl_tile_store_index(t, t0, cnt, x, W);
        if (at == -1) continue;
        if (at < 0 || at >= groups * W) return -1;
        keep[at] += ((uint64_t)(t / pgx::kWlItemWords) << 32) | (uint64_t)(t % pgx::kWlItemWords + 1);   // += : a word stored twice shows
        ++stores;
    }
    return stores;
}

}  // extern "C"
