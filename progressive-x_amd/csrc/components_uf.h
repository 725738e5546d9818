// components_uf.h — the find / link statements of pgx_label_components (components.hip), HIP-free: the kernels run them on relaxed
// agent-scope atomics of global memory, tests/emu/components_driver.cpp runs the same lines on std::atomic, sequentially and under
// threads.
//
// parent[] is a forest over the sites with parent[x] <= x everywhere, so it has no cycles and the root of a tree is its smallest member.
// `Mem` gives the three accesses, each ONE atomic operation on one word, in any (relaxed) order:
//   int  load(int x)                       parent[x]
//   void store(int x, int v)               parent[x] = v
//   int  cas(int x, int expected, int v)   if parent[x] == expected, parent[x] = v; returns what parent[x] held before
//
// WHY STALE VALUES ARE HARMLESS.  Three facts hold at every moment of a hook launch, whatever the lanes' order:
//   (a) a link is made only by uf_unite's cas(big, big, small): it succeeds only while big is a ROOT (parent[big] == big), at the one place
//       where the word is coherent, and small < big.  A site that has stopped being a root never becomes one again;
//   (b) uf_find's path-halving store writes parent[x] = g only after it has READ parent[x] = p != x and parent[p] = g: x is no root then
//       (and by (a) never again), and g is an ancestor of p, which is an ancestor of x;
//   (c) trees only ever gain links at their roots (a) or have a site re-hung below one of its own ancestors (b): a value once read as
//       parent[x] = p != x names an ancestor of x FOR EVER, however old the read.
// So every value a lane holds - fresh or stale - is an ancestor of the site it was read for, and smaller than it.  uf_find walks ancestors
// and stops at a site it read as a root; if that read was stale the site is merely an ancestor, and the cas on it fails and RETURNS its
// present parent, from which the walk goes on.  Linking big below a `small` that has meanwhile stopped being a root is still a link below
// a smaller site of the other tree: the forest property and the union both hold.  A stale read can cost a retry, never a wrong link.
//
// FORWARD PROGRESS.  Nothing here waits for another lane: the loop of uf_find descends strictly (every step goes to a smaller site), and
// uf_unite repeats only after its cas has failed, that is after ANOTHER lane's cas on the same root has succeeded - of which there are at
// most (sites - 1) in a launch.
#pragma once

#if defined(__HIPCC__)
#define PGX_UF_HD __host__ __device__ __forceinline__
#else
#define PGX_UF_HD inline
#endif

namespace pgx {

// the root of x as far as this lane can see, halving the path on the way
template <class Mem>
PGX_UF_HD int uf_find(Mem& m, int x)
{
    int p = m.load(x);
    while (p != x) {
        const int g = m.load(p);
        if (g != p) m.store(x, g);   // (b): x is no root, g is an ancestor of x
        x = p;
        p = g;
    }
    return x;
}

// joins the trees of a and b: the larger root goes below the smaller one.  `a` may be any ancestor of the site meant (a site is its own):
// the answer is an ancestor of both sites, to be handed in as `a` for the next arc of the same site, whose walk then starts near the root.
template <class Mem>
PGX_UF_HD int uf_unite(Mem& m, int a, int b)
{
    int ra = uf_find(m, a), rb = uf_find(m, b);
    while (ra != rb) {
        const int big = ra > rb ? ra : rb, small = ra > rb ? rb : ra;
        const int seen = m.cas(big, big, small);
        if (seen == big) return small;   // linked
        ra = uf_find(m, seen);           // big had a parent already: go on from it
        rb = small;
    }
    return ra;
}

// the root of x where nothing links or stores any more (the launches after the hook launch): reads only
template <class Mem>
PGX_UF_HD int uf_root(const Mem& m, int x)
{
    int p = m.load(x);
    while (p != x) {
        x = p;
        p = m.load(x);
    }
    return x;
}

}  // namespace pgx
