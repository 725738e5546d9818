"""pgx_label_components (include/pgx.h) and splitComponents' regrouping restated in plain Python: TEST INFRASTRUCTURE ONLY.

A breadth-first search over the CSR, written from the definition and sharing nothing with the product (no union-find, no scipy): a site
is live when 0 <= label < first_ignored; two live sites are joined when an arc of either row joins them and their labels are equal;
components are numbered in ascending order of their smallest member."""
from collections import deque

import numpy as np


def label_components(off, idx, labels, first_ignored):
    """(comp int32 [n], first int32 [C], sizes int64 [C]) of the CSR (off [n + 1], idx [E]); rows may be asymmetric and hold self arcs"""
    off = np.asarray(off, dtype=np.int64)
    idx = np.asarray(idx, dtype=np.int64)
    labels = np.asarray(labels, dtype=np.int64)
    n = len(off) - 1
    assert len(labels) == n
    nbr = [[] for _ in range(n)]                                 # an arc in either row joins in both directions
    for i in range(n):
        for j in idx[off[i]:off[i + 1]].tolist():
            nbr[i].append(j)
            nbr[j].append(i)
    live = (labels >= 0) & (labels < first_ignored)
    comp = np.full(n, -1, dtype=np.int32)
    first, sizes = [], []
    for s in range(n):                                           # ascending: s is the smallest member of the component it opens
        if not live[s] or comp[s] >= 0:
            continue
        c = len(first)
        comp[s] = c
        queue, size = deque([s]), 0
        while queue:
            u = queue.popleft()
            size += 1
            for v in nbr[u]:
                if comp[v] < 0 and live[v] and labels[v] == labels[u]:
                    comp[v] = c
                    queue.append(v)
        first.append(s)
        sizes.append(size)
    return comp, np.array(first, dtype=np.int32), np.array(sizes, dtype=np.int64)


def regroup(labels, model_number, comp, first, sizes, minimum_point_number, keep):
    """(new_labels int32 [n], parent int32 [K']): components -> instances, one Python statement per sentence of the definition"""
    assert keep in ("all", "largest")
    cands = [(int(labels[f]), int(s), int(f), c) for c, (f, s) in enumerate(zip(first, sizes))]
    assert all(0 <= m < model_number for m, _, _, _ in cands)
    if keep == "largest":
        best = {}
        for m, s, f, c in cands:                                 # the largest of each model, ties to the smaller first
            if m not in best or (s, -f) > (best[m][1], -best[m][2]):
                best[m] = (m, s, f, c)
        cands = list(best.values())
    cands = [t for t in cands if t[1] >= minimum_point_number]   # the size test applies either way
    cands.sort(key=lambda t: (t[0], -t[1], t[2]))               # (original label ascending, size descending, first ascending)
    k = len(cands)
    new = np.full(len(labels), k, dtype=np.int32)
    for j, (_, _, _, c) in enumerate(cands):
        new[np.asarray(comp) == c] = j
    return new, np.array([t[0] for t in cands], dtype=np.int32)


def path_graph(order):
    """CSR of the path order[0] - order[1] - ... (a permutation of 0 .. n-1), rows ascending"""
    n = len(order)
    rows = [[] for _ in range(n)]
    for a, b in zip(order[:-1], order[1:]):
        rows[a].append(int(b))
        rows[b].append(int(a))
    return from_rows(rows)


def from_rows(rows, rng=None):
    """(off, idx, mult) int32 of the neighbour lists, each row sorted; multiplicities 1, or 1 .. 3 drawn symmetrically with rng"""
    rows = [sorted(set(r)) for r in rows]
    off = np.zeros(len(rows) + 1, dtype=np.int32)
    off[1:] = np.cumsum([len(r) for r in rows])
    idx = np.array([j for r in rows for j in r], dtype=np.int32)
    mult = np.ones(len(idx), dtype=np.int32)
    if rng is not None:
        drawn = {}
        for i, r in enumerate(rows):
            for a, j in enumerate(r):
                key = (min(i, j), max(i, j))
                if key not in drawn:
                    drawn[key] = int(rng.integers(1, 4))
                mult[off[i] + a] = drawn[key]
    return off, idx, mult


def random_graph(n, mean_degree, rng, weighted=True):
    """a symmetric CSR without self arcs: n * mean_degree / 2 random pairs"""
    m = int(round(n * mean_degree / 2))
    a, b = rng.integers(0, n, m), rng.integers(0, n, m)
    rows = [[] for _ in range(n)]
    for i, j in zip(a.tolist(), b.tolist()):
        if i != j:
            rows[i].append(j)
            rows[j].append(i)
    return from_rows(rows, rng if weighted else None)


def hub_graph(n, hubs, leaves_of):
    """stars: hubs[h] joined to every site of leaves_of[h]"""
    rows = [[] for _ in range(n)]
    for h, leaves in zip(hubs, leaves_of):
        for v in leaves:
            rows[h].append(int(v))
            rows[int(v)].append(h)
    return from_rows(rows)


def grid_graph(w, h):
    rows = [[] for _ in range(w * h)]
    for y in range(h):
        for x in range(w):
            i = y * w + x
            if x + 1 < w:
                rows[i].append(i + 1)
                rows[i + 1].append(i)
            if y + 1 < h:
                rows[i].append(i + w)
                rows[i + w].append(i)
    return from_rows(rows)


# ---- the small graphs both test files run: (name, (off, idx, mult), labels, first_ignored, resident) ------------------------------------
LONG_ROW = 64          # the product's long-row threshold, restated (the tests compare it with the header's and _lib's)
PATH_SIZES = (1, 2, 3, 63, 64, 65, 257, 4097)
HUB_LEAVES = (LONG_ROW - 1, LONG_ROW, LONG_ROW + 1, 5000)
_reference = {}


def reference(name, graph, labels, first_ignored):
    """the model's answer for a named case, computed once and shared by every test that needs it"""
    if name not in _reference:
        _reference[name] = label_components(graph[0], graph[1], labels, first_ignored)
    return _reference[name]


def path_cases():
    for n in PATH_SIZES:
        along = np.arange(n)
        for tag, order in (("along", along), ("reversed", along[::-1]), ("permuted", np.random.default_rng(n).permutation(n))):
            yield f"path-{n}-{tag}", path_graph(order), np.zeros(n, dtype=np.int32), 1, True


def hub_cases():
    for m in HUB_LEAVES:
        n = m + 1
        yield f"hub-first-{m}", hub_graph(n, [0], [range(1, n)]), np.zeros(n, dtype=np.int32), 1, True
        yield f"hub-last-{m}", hub_graph(n, [n - 1], [range(0, n - 1)]), np.zeros(n, dtype=np.int32), 1, True
        # two hubs of different labels share the leaves, whose labels are drawn: each hub collects its own
        n = m + 2
        for tag, hubs, leaves in (("first", [0, 1], range(2, n)), ("last", [n - 2, n - 1], range(0, n - 2))):
            labels = np.random.default_rng(m).integers(0, 2, n).astype(np.int32)
            labels[hubs[0]], labels[hubs[1]] = 0, 1
            yield f"hubs-two-{tag}-{m}", hub_graph(n, hubs, [leaves, leaves]), labels, 2, True


def grid_cases():
    g = grid_graph(32, 32)
    y, x = np.divmod(np.arange(1024), 32)
    mixed = np.random.default_rng(32).integers(-2, 6, 1024).astype(np.int32)
    yield "grid-checkerboard", g, ((x + y) % 2).astype(np.int32), 2, True
    yield "grid-stripes", g, ((x // 4) % 2).astype(np.int32), 2, True
    yield "grid-one-label", g, np.zeros(1024, dtype=np.int32), 1, True
    yield "grid-all-ignored", g, np.full(1024, 7, dtype=np.int32), 7, True
    yield "grid-negatives-and-ignored", g, mixed, 3, True
    yield "grid-first-ignored-0", g, np.zeros(1024, dtype=np.int32), 0, True


def isolated_cases():
    empty = (np.zeros(11, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32))
    yield "isolated-sites", empty, np.array([0, 0, 1, -1, 2, 5, 0, 1, 1, 2], dtype=np.int32), 3, True
    rows = [[] for _ in range(9)]                               # empty rows between two joined pairs
    rows[2], rows[6], rows[3], rows[8] = [6], [2], [8], [3]
    yield "isolated-rows-between-pairs", from_rows(rows), np.zeros(9, dtype=np.int32), 1, True


def random_cases(degrees=(0.5, 2, 8), seeds=range(20)):
    for deg in degrees:
        for seed in seeds:
            rng = np.random.default_rng([seed, int(deg * 10)])
            g = random_graph(1000, deg, rng)
            yield f"random-{deg}-{seed}", g, rng.integers(0, 4, 1000).astype(np.int32), 4 if seed % 2 == 0 else 3, True


def unsymmetric_cases():
    """CSRs that cannot be resident - pgx_set_graph refuses a row that its neighbour does not return and a self arc - run through the
    same statements on the CPU"""
    rng = np.random.default_rng(77)
    rows = [[] for _ in range(1000)]
    for i, j in zip(rng.integers(0, 1000, 900).tolist(), rng.integers(0, 1000, 900).tolist()):
        if i != j:
            rows[i].append(j)                                   # in row i only
    yield "asymmetric", from_rows(rows), rng.integers(0, 3, 1000).astype(np.int32), 3, False
    off, idx, _ = random_graph(1000, 2, rng, weighted=False)
    rows = [idx[off[i]:off[i + 1]].tolist() + ([i] if i % 3 == 0 else []) for i in range(1000)]
    yield "self-arcs", from_rows(rows), rng.integers(0, 3, 1000).astype(np.int32), 3, False


def small_cases():
    for make in (path_cases, hub_cases, grid_cases, isolated_cases, random_cases, unsymmetric_cases):
        yield from make()
