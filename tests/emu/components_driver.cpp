// components_driver.cpp — runs the find / link statements of csrc/components_uf.h on std::atomic (TEST INFRASTRUCTURE,
// tests/test_components_cpu.py): the lines the hook and flatten kernels of components.hip run on relaxed agent-scope atomics, here on
// relaxed std::atomic<int>, arc by arc in the order given or by several threads that each take a slice of the arc list.
#include <atomic>
#include <cstdint>
#include <thread>
#include <vector>

#include "../../progressive-x_amd/csrc/components_uf.h"

namespace {

struct StdMem {
    std::atomic<int>* parent;
    int load(int x) const { return parent[x].load(std::memory_order_relaxed); }
    void store(int x, int v) { parent[x].store(v, std::memory_order_relaxed); }
    int cas(int x, int expected, int v)
    {
        parent[x].compare_exchange_strong(expected, v, std::memory_order_relaxed, std::memory_order_relaxed);
        return expected;
    }
};

bool live(int l, int first_ignored) { return l >= 0 && l < first_ignored; }

// the hook launch's statement for the arcs [lo, hi)
void hook(StdMem m, const int32_t* a, const int32_t* b, int64_t lo, int64_t hi, const int32_t* labels, int first_ignored)
{
    int site = -1, r = -1;   // as the kernel does: consecutive arcs of one site start from where the last one ended
    for (int64_t e = lo; e < hi; ++e) {
        const int i = a[e], j = b[e];
        if (i != site) { site = i; r = i; }
        if (live(labels[i], first_ignored) && labels[j] == labels[i]) r = pgx::uf_unite(m, r, j);
    }
}

// the flatten launch: the root of every live site, -1 elsewhere; returns 0 when parent[x] <= x held everywhere
int flatten(const StdMem& m, int64_t n, const int32_t* labels, int first_ignored, int32_t* root)
{
    int bad = 0;
    for (int64_t i = 0; i < n; ++i) {
        if (m.load((int)i) > (int)i) bad = 1;
        root[i] = live(labels[i], first_ignored) ? pgx::uf_root(m, (int)i) : -1;
    }
    return bad;
}

}  // namespace

extern "C" {

// arcs (a[e], b[e]), e < m, in the given order by `threads` threads (1: sequentially, on the caller's thread)
int cc_emu_run(int64_t n, int64_t m, const int32_t* a, const int32_t* b, const int32_t* labels, int first_ignored, int threads, int32_t* root)
{
    for (int64_t e = 0; e < m; ++e)
        if (a[e] < 0 || a[e] >= n || b[e] < 0 || b[e] >= n) return -1;
    std::vector<std::atomic<int>> parent((size_t)n);
    for (int64_t i = 0; i < n; ++i) parent[(size_t)i].store((int)i, std::memory_order_relaxed);
    StdMem mem{parent.data()};
    if (threads <= 1) {
        hook(mem, a, b, 0, m, labels, first_ignored);
    } else {
        std::vector<std::thread> pool;
        for (int t = 0; t < threads; ++t)
            pool.emplace_back(hook, mem, a, b, m * t / threads, m * (t + 1) / threads, labels, first_ignored);
        for (std::thread& t : pool) t.join();
    }
    return flatten(mem, n, labels, first_ignored, root);
}

}
