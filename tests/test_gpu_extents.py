"""instanceExtents on the MI355X: pgx_instance_extents bit for bit - every output array and skipped - against the numpy restatement of
include/pgx.h (extents_model.py) on the cases test_extents_cpu.py runs through the shared statements: sizes around the wave and the
workgroup, a scene with one instance of each kind, both sides of the LDS switch, uniform / mixed / empty label layouts, bad inputs;
its refusals, repeatability and absence of side effects, and the public call behind findPlanes and splitComponents."""
import ctypes as C

import numpy as np
import pytest

import extents_model as EM
import pyprogressivex as px
from pyprogressivex import _lib, datasets

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def references():
    """the model's answer to every case, computed once"""
    return {case[0]: (case, EM.extents(*case[1:])) for case in EM.all_cases()}


def check(ctx, references, name):
    (_, pts, labels, frames), ref = references[name]
    got = ctx.instance_extents(pts, labels, frames)
    assert EM.same(got, ref), name
    return got


def names(make):
    return [case[0] for case in make()]


@pytest.mark.parametrize("name", names(EM.size_cases))
def test_sizes(gpu_ctx, references, name):
    assert [int(n.split("-")[1]) for n in names(EM.size_cases)] == [1, 63, 64, 65, 129, 257]
    check(gpu_ctx, references, name)


@pytest.mark.parametrize("name", names(EM.scene_cases))
def test_scene_with_one_instance_of_each_kind(gpu_ctx, references, name):
    got = check(gpu_ctx, references, name)
    frames = references[name][0][3]
    assert sorted(frames[:, 0].tolist()) == [0, 1, 2, 2, 3, 4] and len(references[name][0][1]) == 2000
    assert (got["count"] > 150).all() and got["skipped"] == 0


@pytest.mark.parametrize("name", names(EM.switch_cases))
def test_both_sides_of_the_lds_switch(gpu_ctx, references, name):
    T = _lib.EXTENTS_LDS_INSTANCES
    assert [int(n.split("-")[1]) for n in names(EM.switch_cases)] == [1, T, T + 1]
    got = check(gpu_ctx, references, name)
    assert len(got["count"]) == int(name.split("-")[1]) and got["count"].sum() > 900


@pytest.mark.parametrize("name", names(EM.layout_cases))
def test_label_layouts(gpu_ctx, references, name):
    got = check(gpu_ctx, references, name)
    if name == "one-instance":
        assert got["count"].tolist() == [1500]
    if name == "instance-without-points":
        assert got["count"][2] == 0 and np.isposinf(got["lo"][2]).all() and np.isneginf(got["hi"][2]).all() and got["occupancy"][2] == 0
    if name == "all-out-of-range":
        assert got["count"].sum() == 0 and got["skipped"] == 0 and (got["occupancy"] == 0).all()


@pytest.mark.parametrize("name", names(EM.bad_cases) + names(EM.exact_cases))
def test_bad_inputs_and_exact_coordinates(gpu_ctx, references, name):
    got = check(gpu_ctx, references, name)
    assert got["skipped"] > 0
    if name == "frame-of-kind--1":
        assert got["count"][2] == 0
    if name == "exact":
        assert not np.signbit(got["lo"][0]).any() and got["hi"][0].tolist() == [0.0, 8.0] and got["occupancy"][0] == 0b11000011


def test_repeat_on_a_fresh_context(gpu_ctx, references):
    (_, pts, labels, frames), ref = references["scene-single-types"]
    a = gpu_ctx.instance_extents(pts, labels, frames)
    b = gpu_ctx.instance_extents(pts, labels, frames)
    with _lib.Context(0) as fresh:
        c = fresh.instance_extents(pts, labels, frames)
        (_, pts2, labels2, frames2), ref2 = references["instances-257"]
        d = fresh.instance_extents(pts2, labels2, frames2)       # the buffer grows, the other route runs
        e = fresh.instance_extents(pts, labels, frames)
    assert EM.same(a, ref) and EM.same(b, ref) and EM.same(c, ref) and EM.same(d, ref2) and EM.same(e, ref)


# ---- refusals and empty calls -------------------------------------------------------------------------------------------------------------
def raw_call(ctx, pts, n, labels, frames, K, outs, want_skipped=True):
    skipped = C.c_int64(-7)
    count, lo, hi, sectors, occupancy = outs
    r = ctx._lib.pgx_instance_extents(ctx._h, _lib._ptr(pts, C.c_double), C.c_int64(n), _lib._ptr(labels, C.c_int32), _lib._ptr(frames, C.c_double),
                                      C.c_int32(K), _lib._ptr(count, C.c_int64), _lib._ptr(lo, C.c_double), _lib._ptr(hi, C.c_double),
                                      _lib._ptr(sectors, C.c_uint64), _lib._ptr(occupancy, C.c_uint64), C.byref(skipped) if want_skipped else None)
    return r, ctx._lib.pgx_last_error(ctx._h).decode(), skipped.value


def buffers(K):
    return [np.full(K, -7, np.int64), np.full((K, 2), -7.0), np.full((K, 2), -7.0), np.full((K, 2), 7, np.uint64), np.full(K, 7, np.uint64)]


def untouched(outs):
    return all((a == (7 if a.dtype == np.uint64 else -7)).all() for a in outs)


def test_refusals_and_empty_calls(references):
    (_, pts, labels, frames), ref = references["size-65"]
    n, K = len(pts), len(frames)
    with _lib.Context(0) as ctx:
        outs = buffers(K)
        for args, sentence in (((pts, -1, labels, frames, K), "pgx_instance_extents: n = -1"),
                               ((pts, n, labels, frames, -2), "pgx_instance_extents: K = -2"),
                               ((pts, n, labels, frames, _lib.EXTENTS_MAX_INSTANCES + 1),
                                f"pgx_instance_extents: {_lib.EXTENTS_MAX_INSTANCES + 1} instances, at most {_lib.EXTENTS_MAX_INSTANCES}"),
                               ((None, n, labels, frames, K), "pgx_instance_extents: NULL argument"),
                               ((pts, n, None, frames, K), "pgx_instance_extents: NULL argument"),
                               ((pts, n, labels, None, K), "pgx_instance_extents: NULL argument")):
            r, msg, skipped = raw_call(ctx, *args, outs)
            assert r == -1 and sentence in msg and skipped == -7 and untouched(outs), sentence
        for missing in range(5):
            some = list(outs)
            some[missing] = None
            r, msg, skipped = raw_call(ctx, pts, n, labels, frames, K, some)
            assert r == -1 and "pgx_instance_extents: NULL argument" in msg and skipped == -7 and untouched(outs)
        r, msg, _ = raw_call(ctx, pts, n, labels, frames, K, outs, want_skipped=False)
        assert r == -1 and "pgx_instance_extents: NULL argument" in msg and untouched(outs)
        # K == 0: fine, whatever else is NULL; only *skipped is written
        r, _, skipped = raw_call(ctx, pts, n, labels, None, 0, [None] * 5)
        assert (r, skipped) == (0, 0)
        # n == 0: the empty results for all K instances
        r, _, skipped = raw_call(ctx, None, 0, None, frames, K, outs)
        assert (r, skipped) == (0, 0)
        assert (outs[0] == 0).all() and np.isposinf(outs[1]).all() and np.isneginf(outs[2]).all() and (outs[3] == 0).all() and (outs[4] == 0).all()
        empty = ctx.instance_extents(np.zeros((0, 3)), np.zeros(0, np.int32), frames)
        assert EM.same(empty, EM.extents(np.zeros((0, 3)), np.zeros(0, np.int32), frames))
        none = ctx.instance_extents(pts, labels, np.zeros((0, 15)))
        assert EM.same(none, EM.extents(pts, labels, np.zeros((0, 15))))
        assert EM.same(ctx.instance_extents(pts, labels, frames), ref)                     # still usable, and it needed no problem or graph


# ---- side effects -----------------------------------------------------------------------------------------------------------------------
def test_instance_extents_leave_the_resident_problem_alone(gpu_ctx, references):
    pts, gen, gt = datasets.make_planes(n_per_plane=400, n_planes=3, n_outliers=400, seed=5)
    n = len(pts)
    rng = np.random.default_rng(6)
    hyps = np.vstack([gt, gt[rng.integers(0, 3, 61)] + 0.02 * rng.normal(size=(61, 4))])
    lam, h, T2 = 0.1, 6.0, 2.25 * 0.05 ** 2
    gpu_ctx.set_points(_lib.PLANE3D, pts)
    graph = gpu_ctx.graph_build(pts, _lib.GRAPH_KNN_IN_BALL, radius=0.5, k=5)
    normals, _, _ = gpu_ctx.estimate_normals(pts)
    gpu_ctx.pearl_unary(gt, 0.05, lam)
    gpu_ctx.score(hyps, T2)
    gpu_ctx.set_labels(np.zeros(n, np.int32))
    eq0 = gpu_ctx.expansion(lam, h)[0]
    labels = gpu_ctx.get_labels()
    energy = gpu_ctx.energy(lam, h)
    score = gpu_ctx.score_fetch()
    for name in ("scene-single-types", "instances-257"):
        check(gpu_ctx, references, name)
    from pyprogressivex import _extents
    frames, _ = _extents.frames(gt, 6)
    other = rng.integers(-1, 5, n).astype(np.int32)
    assert EM.same(gpu_ctx.instance_extents(pts, other, frames), EM.extents(pts, other, frames))
    assert np.array_equal(gpu_ctx.get_labels(), labels) and gpu_ctx.energy(lam, h) == energy
    again = gpu_ctx.score_fetch()
    assert all(np.array_equal(score[key].view(np.int64), again[key].view(np.int64)) for key in ("counts", "values", "shared", "scores"))
    assert all(np.array_equal(a, b) for a, b in zip(gpu_ctx.graph_fetch(), graph))
    assert np.array_equal(gpu_ctx.estimate_normals(pts)[0].view(np.int64), normals.view(np.int64))   # the graph and the points answer the same
    assert gpu_ctx.expansion(lam, h)[0] == eq0 and np.array_equal(gpu_ctx.get_labels(), labels)     # the memo and the fixed point too
    assert len(np.unique(labels)) > 1 and score["counts"].max() > 300


# ---- the public call ----------------------------------------------------------------------------------------------------------------------
def test_public_call_equals_the_model_through_type_18_rows(references):
    pts, labels, models = EM.scene(2000, seed=4)
    rows = np.zeros((4, 9))
    for i, surface in enumerate((6, 8, 14, 16)):
        rows[i, 0], rows[i, 1:1 + len(models[surface])] = surface, models[surface]
    mine = np.array([0, 1, -1, 2, 3, -1, -1])[np.clip(labels, -1, 6)]        # the scene's instances 0, 1, 3, 4 on the four union rows
    mine = np.where((labels >= 0) & (labels < 6), mine, 2 ** 40)
    got = px.instanceExtents(pts, mine, rows, 18)
    from pyprogressivex import _extents
    frames, surface = _extents.frames(rows, 18)
    ref = EM.extents(pts, np.where(mine < 4, mine, -1), frames)
    assert EM.same(got, ref) and got["kind"].tolist() == [0, 3, 2, 2] and np.array_equal(got["surface"], surface)
    arc, area = _extents.derive(surface, frames, ref["lo"], ref["hi"], ref["sectors"], ref["occupancy"])
    assert np.array_equal(got["arc"], arc, equal_nan=True) and np.array_equal(got["area"], area)
    assert 32 <= got["arc"][2, 1, 1] / (2 * np.pi / 64) <= 34               # the half shell
    oriented = px.instanceExtents(pts, mine, rows, 20, parent=np.arange(4))
    assert EM.same(oriented, ref)


def test_extents_after_find_planes_and_split_components():
    pts, _, _ = datasets.make_planes(n_per_plane=500, n_planes=3, n_outliers=300, seed=11)
    planes, labels = px.findPlanes(pts, threshold=0.05, minimum_point_number=100, neighborhood_ball_radius=0.5, seed=1)
    K = len(planes)
    assert K >= 1
    new, parent = px.splitComponents(pts, labels, K, k=8, radius=0.5, minimum_point_number=20)
    assert len(parent) >= 1
    ext = px.instanceExtents(pts, new, planes, 6, parent=parent)
    assert np.array_equal(ext["count"], np.bincount(new, minlength=len(parent) + 1)[:len(parent)]) and ext["skipped"] == 0
    assert (ext["kind"] == 0).all() and (ext["sectors"] == 0).all() and np.isnan(ext["arc"]).all()
    for j in range(len(parent)):
        e = pts[new == j] - ext["origin"][j]
        a, b = e @ ext["u"][j], e @ ext["v"][j]
        slack = 4 * np.finfo(float).eps * np.abs(e).max()                   # numpy's dot product is not the left fold
        assert (a >= ext["lo"][j, 0] - slack).all() and (a <= ext["hi"][j, 0] + slack).all()
        assert (b >= ext["lo"][j, 1] - slack).all() and (b <= ext["hi"][j, 1] + slack).all()
        assert 0 < ext["area"][j] <= (ext["hi"][j, 0] - ext["lo"][j, 0]) * (ext["hi"][j, 1] - ext["lo"][j, 1]) * (1 + 1e-12)
        assert np.abs(np.cross(ext["axis"][j], planes[parent[j], :3])).max() < 1e-12 and ext["axis"][j] @ planes[parent[j], :3] > 0
    print(f"findPlanes {K} planes, splitComponents {len(parent)} instances, counts {ext['count'].tolist()}, areas {np.round(ext['area'], 3).tolist()}")
