// score_worklist_locate_emu.cpp — the two ways csrc/score_worklist.h finds the item of a slot, for tests/test_score_worklist_locate.py:
// wl_locate (early exits; the host replay and the existing tests) and wl_locate_select (no exits; score_group_kernel), side by side.
#include <cstdint>

#include "../../progressive-x_amd/csrc/score_worklist.h"

extern "C" {

// each returns the class (0 .. 3) and the position through *pos, or -1 when the slot is at or past the total
int wl_emu_locate(const uint32_t c[4], uint32_t slot, uint32_t* pos)
{
    int cls = -7;
    return pgx::wl_locate(c[0], c[1], c[2], c[3], slot, &cls, pos) ? cls : -1;
}
int wl_emu_locate_select(const uint32_t c[4], uint32_t slot, uint32_t* pos)
{
    int cls = -7;
    return pgx::wl_locate_select(c[0], c[1], c[2], c[3], slot, &cls, pos) ? cls : -1;
}

// slots [first, first + count) of one count vector: the number of slots on which the two disagree (found or not, class, position)
int64_t wl_emu_locate_mismatches(const uint32_t c[4], uint32_t first, uint32_t count)
{
    int64_t bad = 0;
    for (uint32_t k = 0; k < count; ++k) {
        const uint32_t slot = first + k;
        int ca = -7, cb = -7;
        uint32_t pa = 0, pb = 0;
        const bool fa = pgx::wl_locate(c[0], c[1], c[2], c[3], slot, &ca, &pa), fb = pgx::wl_locate_select(c[0], c[1], c[2], c[3], slot, &cb, &pb);
        if (fa != fb || (fa && (ca != cb || pa != pb))) ++bad;
    }
    return bad;
}

// an item's keep words the way score_group_kernel fetches them: one 4-word load inside the row [0, W) of `row`, then the shift.
// Returns the load's first word, or -1 if the load would leave the row.
int wl_emu_item_words(const uint64_t* row, int W, int w0, uint64_t out[4])
{
    const int b = pgx::wl_words_begin(w0, W);
    if (b < 0 || b + pgx::kWlItemWords > W) return -1;
    pgx::wl_words_shift(row[b], row[b + 1], row[b + 2], row[b + 3], w0 - b, out);
    return b;
}

}  // extern "C"
