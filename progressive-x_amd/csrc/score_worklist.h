// score_worklist.h — the index arithmetic of the group-major kernel's work lists (score.hip: score_cull_kernel appends, score_group_kernel
// takes): the class of an item's weight, the item record, and the (class, position) a workgroup's slot stands for given
// the four counts of its XCD.  No HIP in here: libpgx.so and the CPU test (tests/test_score_worklist_index.py) compile the same code.
//
// An item is a 64-point group x kWlItemWords adjacent hypothesis words - what one workgroup of the cull kernel decides per group of its
// tile.  Its weight is the number of surviving (hypothesis, group) steps in those words.  Non-empty items go to one of
// kWlXcds x kWlClasses lists, [g & 7][class]: a group's items all run on XCD g & 7 (workgroup ids go round-robin over the XCDs), and
// within an XCD the classes are handed out heaviest first, so that the long items start first and the short ones fill the tail.
// The class is scheduling only: every sum of the group kernel is an integer added by atomics, the order of the items cannot show.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define PGX_WL_FN __host__ __device__ inline
#else
#define PGX_WL_FN inline
#endif

namespace pgx {

constexpr int kWlXcds = 8;
constexpr int kWlClasses = 4;
constexpr int kWlItemWords = 4;      // hypothesis words per item = waves per workgroup of the cull kernel (score.hip kCullWaves)
constexpr int kWlCountStride = 32;   // 32-bit words between two counts: a cache line each (the appends of 2 000 cull workgroups meet here)
constexpr int kWlCountWords = kWlXcds * kWlClasses * kWlCountStride;   // the lists' items follow the counts

PGX_WL_FN int wl_count_index(int xcd, int cls) { return (xcd * kWlClasses + cls) * kWlCountStride; }

// class of a non-empty item: how many of the three thresholds (ascending; t2 = t3 = a value no weight reaches leaves two classes)
// its weight has reached.  0 = lightest.
PGX_WL_FN int wl_class(unsigned weight, unsigned t1, unsigned t2, unsigned t3)
{
    return (weight >= t1 ? 1 : 0) + (weight >= t2 ? 1 : 0) + (weight >= t3 ? 1 : 0);
}

// ---- the item record: group and item column (x = first word / kWlItemWords) in one 32-bit word, the column in the low xbits bits
PGX_WL_FN int wl_xbits(int columns)
{
    int b = 0;
    while (((int64_t)1 << b) < columns) ++b;
    return b;
}
PGX_WL_FN bool wl_fits(int64_t groups, int columns) { return columns >= 1 && groups >= 1 && groups <= ((int64_t)1 << (32 - wl_xbits(columns))); }
PGX_WL_FN uint32_t wl_item(uint32_t g, uint32_t x, int xbits) { return (g << xbits) | x; }
PGX_WL_FN uint32_t wl_item_group(uint32_t item, int xbits) { return item >> xbits; }
PGX_WL_FN uint32_t wl_item_column(uint32_t item, int xbits) { return item & (((uint32_t)1 << xbits) - 1u); }

// ---- which item a slot of an XCD stands for.  counts[c] = items of class c on this XCD; slots run through class 3, then 2, 1, 0.
// false: the slot is at or past the XCD's total.
PGX_WL_FN bool wl_locate(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t slot, int* cls, uint32_t* pos)
{
    if (slot < c3) { *cls = 3; *pos = slot; return true; }
    slot -= c3;
    if (slot < c2) { *cls = 2; *pos = slot; return true; }
    slot -= c2;
    if (slot < c1) { *cls = 1; *pos = slot; return true; }
    slot -= c1;
    if (slot < c0) { *cls = 0; *pos = slot; return true; }
    return false;
}

// wl_locate without early exits, for the group kernel: every comparison and subtraction is made, selects pick the result, so the
// four counts can be fetched in one round trip and nothing is loaded behind a branch.  A class' comparison only counts when no
// heavier class took the slot; then every subtraction before it was of a count <= slot and did not wrap - the same (class, position)
// as wl_locate for all 32-bit counts (tests/test_score_worklist_locate.py).  When false, *cls and *pos are written but mean nothing.
PGX_WL_FN bool wl_locate_select(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t slot, int* cls, uint32_t* pos)
{
    const uint32_t s3 = slot, s2 = s3 - c3, s1 = s2 - c2, s0 = s1 - c1;
    const bool in3 = s3 < c3, in2 = !in3 & (s2 < c2), in1 = !in3 & !in2 & (s1 < c1), in0 = !in3 & !in2 & !in1 & (s0 < c0);
    *cls = in3 ? 3 : in2 ? 2 : in1 ? 1 : 0;
    *pos = in3 ? s3 : in2 ? s2 : in1 ? s1 : s0;
    return in3 | in2 | in1 | in0;
}

// ---- an item's keep words (words w0 .. w0 + 3 of a group's row of W >= 4 words, those at or past W count as 0) as ONE load of four
// adjacent words that stays inside the row: it begins at wl_words_begin, d = w0 - begin words early when the row's last item is
// short, and wl_words_shift moves the words down by d.
PGX_WL_FN int wl_words_begin(int w0, int W) { return w0 + kWlItemWords <= W ? w0 : W - kWlItemWords; }
PGX_WL_FN void wl_words_shift(uint64_t v0, uint64_t v1, uint64_t v2, uint64_t v3, int d, uint64_t out[kWlItemWords])
{
    out[0] = d == 0 ? v0 : d == 1 ? v1 : d == 2 ? v2 : v3;
    out[1] = d == 0 ? v1 : d == 1 ? v2 : d == 2 ? v3 : 0;
    out[2] = d == 0 ? v2 : d == 1 ? v3 : 0;
    out[3] = d == 0 ? v3 : 0;
}

// ---- the cull kernel's tile store: the 64 * kWlItemWords threads of workgroup x (item column x) write the keep words of a tile of
// cnt <= 64 groups beginning at group t0.  Thread t takes group t0 + t / 4 and word 4 x + t % 4, so four neighbouring lanes write the
// 32 contiguous bytes of one item.  The word's index in keep[groups][W], or -1: nothing to store (a group behind the tile's last,
// a word at or past W).
PGX_WL_FN int64_t wl_tile_store_index(int t, int t0, int cnt, int x, int W)
{
    const int gi = t / kWlItemWords, w = x * kWlItemWords + t % kWlItemWords;
    return (gi < cnt && w < W) ? (int64_t)(t0 + gi) * W + w : -1;
}

}  // namespace pgx
