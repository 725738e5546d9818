// score_runs.h — the two pure pieces of the queued exact path's segmented reduction (score.hip score_group_kernel, drain()):
// the (count, value) word a lane carries through the reduction, and a lane's distance to the end of its run of equal hypotheses.
// No HIP in here: libpgx.so and the CPU test (tests/test_score_runs.py) compile the same code.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define PGX_RUNS_FN __host__ __device__ inline
#else
#define PGX_RUNS_FN inline
#endif

namespace pgx {

// ---- count and value in one word ----------------------------------------------------------------------------------------------
// A drain reduces at most 64 pairs.  A pair contributes count 0 or 1 and the fixed-point value to_fixed(sc * qscale) with
// 0 <= sc <= 1 and qscale <= 2^50 (score_plan.h plan_score), an integer in [0, 2^50].  Any partial sum of a drain is therefore below
// 2^57 and its count at most 64 < 2^7: the value sits in bits 0-56, the count in bits 57-63 of one unsigned word, and adding packed
// words adds both fields without a carry from one into the other.  The fields are split again before the atomics, so the integers
// that reach the accumulators are those of two separate sums.
constexpr int kRunMaxTerms = 64;                           // lanes of a wave: pairs of one drain
constexpr int kRunTermBits = 50;                           // a term is <= 2^50
constexpr uint64_t kRunMaxTerm = (uint64_t)1 << kRunTermBits;
constexpr int kRunCountShift = 57;                         // first bit of the count
constexpr uint64_t kRunValueMask = ((uint64_t)1 << kRunCountShift) - 1;
static_assert((uint64_t)kRunMaxTerms * kRunMaxTerm <= kRunValueMask, "64 terms of 2^50 must fit below the count field");
static_assert(((uint64_t)kRunMaxTerms << kRunCountShift) >> kRunCountShift == (uint64_t)kRunMaxTerms, "a count of 64 must fit above the value field");

PGX_RUNS_FN uint64_t run_pack(unsigned count, uint64_t value) { return ((uint64_t)count << kRunCountShift) + value; }
PGX_RUNS_FN unsigned run_count(uint64_t packed) { return (unsigned)(packed >> kRunCountShift); }
PGX_RUNS_FN uint64_t run_value(uint64_t packed) { return packed & kRunValueMask; }

// ---- distance to the end of a run -----------------------------------------------------------------------------------------------
// Runs of equal hypotheses are contiguous in the queue.  heads: bit i set iff lane i starts a run (bit 0 always is).  Returns the
// number of lanes from `lane` to the end of its run, itself included (1 .. 64 - lane).  In round `off` of the reduction lane i adds
// what lane i + off holds iff that lane belongs to the same run: iff off < run_dist(heads, i).
PGX_RUNS_FN int run_dist(uint64_t heads, int lane)
{
    const uint64_t above = (heads >> lane) >> 1;   // the heads behind this lane (two shifts: lane = 63 must not shift by 64)
    return above != 0 ? __builtin_ctzll(above) + 1 : 64 - lane;
}

}  // namespace pgx
