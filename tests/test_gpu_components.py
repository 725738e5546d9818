"""splitComponents on the MI355X: pgx_label_components integer for integer against the breadth-first search of components_model.py on
the fetched CSR - paths (the deepest trees), hubs around the long-row threshold, grids, isolated sites, random graphs, both lane
mappings - its refusals, repeatability and absence of side effects, and the public call on a scene of two coplanar squares.

pgx_set_graph refuses a CSR that is not symmetric and one with a self arc, so neither can be resident: those two cases of
components_model.small_cases() run through the same find / link statements on the CPU (test_components_cpu.py), and here the refusal is
held."""
import ctypes as C

import numpy as np
import pytest

import components_model as CM
import pyprogressivex as px
from pyprogressivex import _lib, datasets

pytestmark = pytest.mark.gpu

T = _lib.COMPONENTS_LONG_ROW


def cases(make):
    return [pytest.param(c, id=c[0]) for c in make()]


def equal(got, ref):
    return all(g.dtype == r.dtype and np.array_equal(g, r) for g, r in zip(got, ref)) and len(got[1]) == len(got[2]) == len(ref[1])


def check_case(ctx, case):
    """a named case through pgx_set_graph (lane t serves site t) against the model on the CSR fetched back"""
    name, graph, labels, first_ignored, _ = case
    ctx.set_graph(*graph)
    fetched = ctx.graph_fetch()
    assert all(np.array_equal(a, b) for a, b in zip(fetched, graph))
    got = ctx.label_components(labels, first_ignored)
    ref = CM.reference(name, fetched, labels, first_ignored)
    assert equal(got, ref), name
    return got


@pytest.mark.parametrize("n", CM.PATH_SIZES)
def test_paths(gpu_ctx, n):
    for case in CM.path_cases():
        if case[0].startswith(f"path-{n}-"):
            comp, first, sizes = check_case(gpu_ctx, case)
            assert first.tolist() == [0] and sizes.tolist() == [n] and (comp == 0).all()


@pytest.mark.parametrize("m", CM.HUB_LEAVES)
def test_hubs_around_the_long_row_threshold(gpu_ctx, m):
    assert CM.HUB_LEAVES[:3] == (T - 1, T, T + 1)
    seen = 0
    for case in CM.hub_cases():
        if case[0].endswith(f"-{m}"):
            comp, first, sizes = check_case(gpu_ctx, case)
            if case[0].startswith("hub-"):
                assert len(first) == 1 and sizes[0] == m + 1
            seen += 1
    assert seen == 4


@pytest.mark.parametrize("case", cases(CM.grid_cases))
def test_grid_labellings(gpu_ctx, case):
    comp, first, sizes = check_case(gpu_ctx, case)
    if case[0] == "grid-checkerboard":
        assert len(first) == 1024 and np.array_equal(comp, np.arange(1024))
    if case[0] in ("grid-all-ignored", "grid-first-ignored-0"):
        assert len(first) == 0 and (comp == -1).all()


def raw_call(ctx, labels, n, first_ignored, comp, first, sizes, want_count=True):
    count = C.c_int64(-7)
    r = ctx._lib.pgx_label_components(ctx._h, _lib._ptr(labels, C.c_int32), C.c_int64(n), C.c_int32(first_ignored), _lib._ptr(comp, C.c_int32),
                                      _lib._ptr(first, C.c_int32), _lib._ptr(sizes, C.c_int64), C.byref(count) if want_count else None)
    return r, ctx._lib.pgx_last_error(ctx._h).decode(), count.value


def test_isolated_sites_no_sites_and_null_outputs(gpu_ctx):
    for case in CM.isolated_cases():
        check_case(gpu_ctx, case)
    name, graph, labels, first_ignored, _ = next(CM.isolated_cases())
    ref = CM.reference(name, graph, labels, first_ignored)
    gpu_ctx.set_graph(*graph)
    n = len(labels)
    comp, first, sizes = np.full(n, -7, np.int32), np.full(n, -7, np.int32), np.full(n, -7, np.int64)
    r, _, count = raw_call(gpu_ctx, labels, n, first_ignored, comp, None, None)                  # NULL first_out and sizes_out
    assert r == 0 and count == len(ref[1]) and np.array_equal(comp, ref[0])
    r, _, count = raw_call(gpu_ctx, labels, n, first_ignored, comp, first, None)
    assert r == 0 and np.array_equal(first[:count], ref[1]) and (first[count:] == -7).all()    # C entries are written, no more
    r, _, count = raw_call(gpu_ctx, labels, n, first_ignored, comp, None, sizes)
    assert r == 0 and np.array_equal(sizes[:count], ref[2]) and (sizes[count:] == -7).all()
    r, _, count = raw_call(gpu_ctx, None, 0, first_ignored, None, None, None)                   # n == 0: fine, whatever is resident
    assert (r, count) == (0, 0)
    got = gpu_ctx.label_components(np.zeros(0, np.int32), 3)
    assert [len(a) for a in got] == [0, 0, 0]


@pytest.mark.parametrize("degree", [0.5, 2, 8])
def test_random_symmetric_graphs(gpu_ctx, degree):
    seen = 0
    for case in CM.random_cases(degrees=(degree,)):
        assert case[1][2].max() == 3 and case[1][2].min() == 1                                   # multiplicities 1 to 3, ignored
        check_case(gpu_ctx, case)
        seen += 1
    assert seen == 20


def test_a_graph_that_cannot_be_resident_is_refused_as_before():
    with _lib.Context(0) as ctx:
        for name, graph, labels, first_ignored, resident in CM.unsymmetric_cases():
            assert not resident
            with pytest.raises(_lib.PgxError, match="not symmetric|bad neighbour"):
                ctx.set_graph(*graph)
        with pytest.raises(_lib.PgxError, match="needs a neighbourhood graph of the points"):
            ctx.label_components(labels, first_ignored)
        check_case(ctx, next(CM.grid_cases()))                                                   # the context is usable afterwards


# ---- both lane mappings -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cloud():
    rng = np.random.default_rng(21)
    pts = rng.uniform(0.0, 1.0, (5000, 3))
    pts[:120] = pts[0] + 1e-3 * rng.normal(size=(120, 3))                                        # a clump: rows beyond the threshold in the ball graph
    cell = (pts[:, 0] > 0.5).astype(np.int32) + 2 * (pts[:, 1] > 0.5).astype(np.int32)           # four regions ...
    noise = rng.uniform(size=5000)
    labels = np.where(noise < 0.1, rng.integers(0, 4, 5000), cell)                               # ... a tenth of the points relabelled ...
    labels = np.where(noise > 0.95, rng.choice([-1, 4, 9], 5000), labels).astype(np.int32)       # ... and a twentieth ignored
    return pts, labels


@pytest.mark.parametrize("kind, k, radius", [(_lib.GRAPH_KNN, 5, 0.0), (_lib.GRAPH_KNN, 16, 0.0), (_lib.GRAPH_BALL, 1, 0.12)])
def test_both_lane_mappings(gpu_ctx, cloud, kind, k, radius):
    pts, labels = cloud
    graph = gpu_ctx.graph_build(pts, kind, radius=radius, k=k)                                  # leaves the Morton order of the sites resident
    morton = gpu_ctx.label_components(labels, 4)
    ref = CM.label_components(graph[0], graph[1], labels, 4)
    assert equal(morton, ref)
    gpu_ctx.set_graph(*graph)                                                                   # the same CSR without an order: lane t serves site t
    assert equal(gpu_ctx.label_components(labels, 4), ref)
    rows = np.diff(graph[0])
    if kind == _lib.GRAPH_BALL:
        assert 24 <= rows.mean() <= 36 and rows.max() > T
    assert len(ref[1]) > 50 and ref[2].max() > 500


def test_repeatability(gpu_ctx, cloud):
    pts, labels = cloud
    gpu_ctx.graph_build(pts, _lib.GRAPH_KNN, k=16, fetch=False)
    a = gpu_ctx.label_components(labels, 4)
    b = gpu_ctx.label_components(labels, 4)
    with _lib.Context(0) as fresh:
        fresh.graph_build(pts, _lib.GRAPH_KNN, k=16, fetch=False)
        c = fresh.label_components(labels, 4)
    assert equal(a, b) and equal(a, c)


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    name, graph, labels, first_ignored, _ = next(CM.grid_cases())
    n = len(labels)
    comp, first, sizes = np.full(n, -7, np.int32), np.full(n, -7, np.int32), np.full(n, -7, np.int64)
    with _lib.Context(0) as ctx:
        r, msg, _ = raw_call(ctx, labels, n, first_ignored, comp, first, sizes)
        assert r == -1 and "pgx_label_components: needs a neighbourhood graph of the points" in msg         # no graph
        ctx.set_graph(*graph)
        r, msg, _ = raw_call(ctx, labels, n - 1, first_ignored, comp, first, sizes)
        assert r == -1 and f"pgx_label_components: {n - 1} labels for a graph of {n} sites" in msg
        with pytest.raises(_lib.PgxError, match=f"{n + 1} labels for a graph of {n} sites"):
            ctx.label_components(np.zeros(n + 1, np.int32), 1)
        for lab, out, want_count in ((None, comp, True), (labels, None, True), (labels, comp, False)):
            r, msg, _ = raw_call(ctx, lab, n, first_ignored, out, first, sizes, want_count)
            assert r == -1 and "pgx_label_components: NULL argument" in msg
        assert (comp == -7).all() and (first == -7).all() and (sizes == -7).all()                         # a refused call writes nothing
        assert equal(ctx.label_components(labels, first_ignored), CM.reference(name, graph, labels, first_ignored))   # still usable


# ---- side effects -----------------------------------------------------------------------------------------------------------------------
def test_label_components_leave_the_resident_problem_alone(gpu_ctx):
    pts, gen, gt = datasets.make_planes(n_per_plane=400, n_planes=3, n_outliers=400, seed=5)
    n = len(pts)
    rng = np.random.default_rng(6)
    hyps = np.vstack([gt, gt[rng.integers(0, 3, 61)] + 0.02 * rng.normal(size=(61, 4))])
    lam, h, T2 = 0.1, 6.0, 2.25 * 0.05 ** 2
    gpu_ctx.set_points(_lib.PLANE3D, pts)
    graph = gpu_ctx.graph_build(pts, _lib.GRAPH_KNN_IN_BALL, radius=0.5, k=5)
    gpu_ctx.pearl_unary(gt, 0.05, lam)
    gpu_ctx.score(hyps, T2)
    gpu_ctx.set_labels(np.zeros(n, np.int32))
    eq0 = gpu_ctx.expansion(lam, h)[0]
    labels = gpu_ctx.get_labels()
    energy = gpu_ctx.energy(lam, h)
    score = gpu_ctx.score_fetch()
    other = rng.integers(-1, 5, n).astype(np.int32)
    assert equal(gpu_ctx.label_components(other, 3), CM.label_components(graph[0], graph[1], other, 3))
    assert np.array_equal(gpu_ctx.get_labels(), labels) and gpu_ctx.energy(lam, h) == energy
    again = gpu_ctx.score_fetch()
    assert all(np.array_equal(score[key].view(np.int64), again[key].view(np.int64)) for key in ("counts", "values", "shared", "scores"))
    assert gpu_ctx.expansion(lam, h)[0] == eq0 and np.array_equal(gpu_ctx.get_labels(), labels)   # the memo and the fixed point too
    assert len(np.unique(labels)) > 1 and score["counts"].max() > 300


# ---- the public call ----------------------------------------------------------------------------------------------------------------------
SPACING = 0.05


@pytest.fixture(scope="module")
def squares():
    """two coplanar 40 x 40 point squares (z = 0) a gap of 5 spacings apart, a third on the parallel plane z = 1, 300 uniform outliers"""
    g = SPACING * np.stack(np.meshgrid(np.arange(40.0), np.arange(40.0), indexing="ij"), axis=-1).reshape(-1, 2)
    a = np.column_stack([g, np.zeros(1600)])
    b = a + [SPACING * (39 + 5), 0.0, 0.0]
    c = a + [0.0, 0.0, 1.0]
    out = np.random.default_rng(3).uniform([-0.5, -0.5, -0.5], [4.5, 2.5, 1.5], (300, 3))
    pts = np.vstack([a, b, c, out])
    labels = np.concatenate([np.zeros(3200), np.ones(1600), np.full(300, 2)]).astype(np.int32)
    order = np.random.default_rng(4).permutation(len(pts))
    return np.ascontiguousarray(pts[order]), labels[order], order


def test_split_components_on_two_coplanar_squares(squares):
    pts, labels, order = squares
    piece = np.repeat([0, 1, 2, 3], [1600, 1600, 1600, 300])[order]                              # 0, 1, 2: the squares; 3: the outliers
    new, parent = px.splitComponents(pts, labels, 2, radius=1.5 * SPACING, k=None)
    ctx = px._api._context()
    off, idx, _ = ctx.graph_fetch()
    comp, first, sizes = CM.label_components(off, idx, np.where(labels < 2, labels, -1), 2)
    ref = CM.regroup(labels, 2, comp, first, sizes, 10, "all")
    assert np.array_equal(new, ref[0]) and np.array_equal(parent, ref[1]) and new.dtype == parent.dtype == np.int32
    assert parent.tolist() == [0, 0, 1]
    a, b = sorted([0, 1], key=lambda s: int(np.flatnonzero(piece == s).min()))                   # equal sizes: the smaller first is instance 0
    assert (new[piece == a] == 0).all() and (new[piece == b] == 1).all()
    assert (new[piece == 2] == 2).all() and (new[piece == 3] == 3).all()
    largest, parent2 = px.splitComponents(pts, labels, 2, radius=1.5 * SPACING, k=None, keep="largest")
    ref2 = CM.regroup(labels, 2, comp, first, sizes, 10, "largest")
    assert np.array_equal(largest, ref2[0]) and parent2.tolist() == [0, 1] == ref2[1].tolist()
    assert (largest[piece == a] == 0).all() and (largest[piece == b] == 2).all() and (largest[piece == 2] == 1).all()
    # the k-NN graph inside the same ball, and the labels in another integer type with a large outlier label
    wide = np.where(labels == 2, 2 ** 40, labels.astype(np.int64))
    new3, parent3 = px.splitComponents(pts, wide, 2, k=8, radius=1.5 * SPACING)
    assert parent3.tolist() == [0, 0, 1] and np.array_equal(new3, new)


def test_split_components_after_find_planes(squares):
    pts, _, _ = squares
    pts = pts + np.random.default_rng(9).normal(scale=0.002, size=pts.shape)
    mpn = 50
    planes, labels = px.findPlanes(pts, threshold=0.02, minimum_point_number=200, neighborhood_ball_radius=0.2, seed=1)
    K = len(planes)
    assert K >= 1
    new, parent = px.splitComponents(pts, labels, K, radius=1.5 * SPACING, k=None, minimum_point_number=mpn)
    off, idx, _ = px._api._context().graph_fetch()
    comp, first, sizes = CM.label_components(off, idx, np.where((labels >= 0) & (labels < K), labels, -1), K)
    assert len(parent) >= 1 and (np.diff(parent) >= 0).all() and parent.min() >= 0 and parent.max() < K
    assert new.min() >= 0 and new.max() <= len(parent)
    for j, m in enumerate(parent):
        members = np.flatnonzero(new == j)
        assert len(members) >= mpn
        assert (labels[members] == m).all()
        assert len(np.unique(comp[members])) == 1 and sizes[comp[members[0]]] == len(members)    # one whole component of the model's graph
    kept = np.flatnonzero(sizes >= mpn)                                                           # every point of a kept component keeps its model
    for c in kept:
        members = np.flatnonzero(comp == c)
        assert (new[members] < len(parent)).all() and (parent[new[members]] == labels[members]).all()
    assert (new[comp < 0] == len(parent)).all()
    print(f"findPlanes returned {K} planes; splitComponents {len(parent)} instances of sizes {np.bincount(new)[:len(parent)].tolist()}")
