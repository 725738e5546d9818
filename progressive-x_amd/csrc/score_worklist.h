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

}  // namespace pgx
