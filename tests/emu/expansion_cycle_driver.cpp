// expansion_cycle_driver.cpp — the cycle driver of csrc/expansion_cycle.h under AddressSanitizer + UndefinedBehaviorSanitizer (TEST
// INFRASTRUCTURE, scripts/sanitize.sh).  What the driver computes is held against the oracle by tests/test_expansion_cycle.py; this run
// takes the same scripted backend (mf_emu.cpp) to the ends of the argument ranges - L = 1 and 64, n = 1, max_cycles = 0, every move
// declined - through memo, restore and identical call, and checks that every move of every cycle is accounted for exactly once.
#include "mf_emu.cpp"

int main()
{
    std::mt19937_64 rng(5);
    long long runs = 0, moves = 0;
    const int Ls[] = {1, 2, 3, 64};
    const int64_t ns[] = {1, 2, 17};
    const int cycles[] = {0, 1, 1000};
    for (int L : Ls) for (int64_t n : ns) for (int64_t lq : {(int64_t)0, (int64_t)4}) for (int max_cycles : cycles)
    for (int batched = 0; batched < 2; ++batched) for (int script = 0; script < (batched ? 4 : 1); ++script) {
        std::vector<int64_t> Dq((size_t)n * L), ids((size_t)L);
        for (int64_t& v : Dq) v = (int64_t)(rng() % 20);
        std::iota(ids.begin(), ids.end(), 0);
        std::vector<int32_t> off((size_t)n + 1, 0), idx, mult;   // a path over the sites
        for (int64_t i = 0; i < n; ++i) {
            if (i > 0) { idx.push_back((int32_t)(i - 1)); mult.push_back(1 + (int32_t)((i - 1) % 2)); }
            if (i + 1 < n) { idx.push_back((int32_t)(i + 1)); mult.push_back(1 + (int32_t)(i % 2)); }
            off[(size_t)i + 1] = (int32_t)idx.size();
        }
        if (idx.empty()) { idx.push_back(0); mult.push_back(1); }
        void* h = emu_cycle_new(1);
        // from zeros twice (the second restores the whole first cycle), the identical call, then from the labels left behind after an event
        std::vector<int32_t> labels((size_t)n, 0);
        for (int call = 0; call < 4; ++call) {
            if (call < 2) { std::fill(labels.begin(), labels.end(), 0); emu_cycle_event(h, 4, 0, ids.data(), L); emu_cycle_event(h, 1, 0, nullptr, 0); }
            if (call == 3) emu_cycle_event(h, 0, 0, nullptr, 0);
            int64_t e = 0, counts[10];
            int done = -1;
            const int rc = emu_cycle_run(h, n, L, Dq.data(), off.data(), idx.data(), mult.data(), lq, 3, labels.data(), max_cycles, batched, 1,
                                         script, (uint64_t)runs + 1, &e, &done, counts);
            const bool ok = rc == 0 && done >= 0 && done <= (max_cycles > 0 ? max_cycles : 0) &&
                            counts[0] + counts[1] + counts[2] + counts[3] == (int64_t)L * done && counts[4] == counts[6] && counts[2] == counts[7] &&
                            (script != 1 || lq <= 0 || counts[0] == counts[4]) && e == emu_cycle_energy(n, L, Dq.data(), off.data(), idx.data(), mult.data(), lq, 3, labels.data());
            if (!ok) {
                std::fprintf(stderr, "expansion_cycle: bookkeeping broken at L=%d n=%lld lq=%lld max_cycles=%d batched=%d script=%d call=%d (rc %d, %d cycles, "
                                     "%lld solved + %lld + %lld skipped + %lld restored)\n", L, (long long)n, (long long)lq, max_cycles, batched, script, call, rc, done,
                             (long long)counts[0], (long long)counts[1], (long long)counts[2], (long long)counts[3]);
                emu_cycle_free(h);
                return 1;
            }
            ++runs;
            moves += (long long)L * done;
        }
        emu_cycle_free(h);
    }
    std::printf("expansion_cycle: %lld runs, %lld moves accounted for\n", runs, moves);
    return 0;
}
