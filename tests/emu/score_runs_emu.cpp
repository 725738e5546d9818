// score_runs_emu.cpp — csrc/score_runs.h as libpgx.so compiles it, for tests/test_score_runs.py: the header's functions one by
// one, and the segmented reduction of score_group_kernel's drain() replayed lane by lane on the CPU with the header driving it.
#include <cstdint>

#include "../../progressive-x_amd/csrc/score_runs.h"

extern "C" {

int sr_run_dist(uint64_t heads, int lane) { return pgx::run_dist(heads, lane); }
uint64_t sr_pack(unsigned count, uint64_t value) { return pgx::run_pack(count, value); }
unsigned sr_count(uint64_t packed) { return pgx::run_count(packed); }
uint64_t sr_value(uint64_t packed) { return pgx::run_value(packed); }
int sr_max_terms() { return pgx::kRunMaxTerms; }
uint64_t sr_max_term() { return pgx::kRunMaxTerm; }

// The reduction as the kernel runs it: every lane packs its own (count, value), then in rounds off = 1, 2, 4, ... lane i adds what
// lane i + off held BEFORE the round iff off < run_dist(heads, i); the loop ends with the first round in which no lane adds.
// out_count / out_value: per lane, the split total of lane .. end of its run.  Returns the number of rounds that added something.
int sr_segmented_sum(uint64_t heads, const unsigned* count, const uint64_t* value, unsigned* out_count, uint64_t* out_value)
{
    uint64_t pv[64], nx[64];
    int dist[64];
    for (int i = 0; i < 64; ++i) { pv[i] = pgx::run_pack(count[i], value[i]); dist[i] = pgx::run_dist(heads, i); }
    int rounds = 0;
    for (int off = 1; off < 64; off <<= 1) {
        bool any = false;
        for (int i = 0; i < 64; ++i) any |= off < dist[i];
        if (!any) break;
        for (int i = 0; i < 64; ++i) nx[i] = off < dist[i] ? pv[i] + pv[i + off] : pv[i];   // off < dist <= 64 - i: i + off is a lane
        for (int i = 0; i < 64; ++i) pv[i] = nx[i];
        ++rounds;
    }
    for (int i = 0; i < 64; ++i) { out_count[i] = pgx::run_count(pv[i]); out_value[i] = pgx::run_value(pv[i]); }
    return rounds;
}

}  // extern "C"
