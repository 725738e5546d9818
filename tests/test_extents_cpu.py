"""instanceExtents without a GPU: the frames the host builds (_extents.frames), the sector rule S against floor(atan2), the statements of
csrc/extents_point.h - the lines the kernels of extents.hip run per lane - on the CPU (tests/emu/extents_driver.cpp) bit for bit against
the numpy restatement of include/pgx.h (extents_model.py) on the cases the GPU test runs, mask -> arc, the areas against closed forms,
and the public function's argument checks."""
import ctypes as C
import inspect
import math
import os
import re
import subprocess

import numpy as np
import pytest

import extents_model as EM
import pyprogressivex as px
from pyprogressivex import _extents, _lib

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(os.path.dirname(HERE), "include", "pgx.h")
EPS = np.finfo(np.float64).eps
TWO_PI = 2.0 * math.pi


# ---- frames ---------------------------------------------------------------------------------------------------------------------------
def direction_of(surface, q):
    return None if surface == 8 else q[:3] if surface == 6 else q[3:6]


def rows_of(models, union):
    """(model_type, rows) for the six single models, or for the four that have a class as type 18 rows"""
    for surface, q in models.items():
        if union and surface in _extents.UNION_CLASSES:
            row = np.zeros(9)
            row[0], row[1:1 + len(q)] = surface, q
            yield 18, surface, q, row
        elif not union:
            yield surface, surface, q, q


@pytest.mark.parametrize("union", [False, True])
@pytest.mark.parametrize("scale", [1.0, 3.0, 1e-3])
def test_frames_are_orthonormal_and_follow_the_model(union, scale):
    rng = np.random.default_rng(17)
    seen = set()
    for _ in range(20):
        for model_type, surface, q, row in rows_of(EM.single_models(rng), union):
            row = row.copy()
            d = direction_of(surface, q)
            if d is not None:                                    # a direction that is not unit
                lo = 1 if model_type == 18 else 0
                at = lo + (0 if surface == 6 else 3)
                row[at:at + 3] *= scale
                if surface == 6:
                    row[at + 3] *= scale                          # (s n, s d): the same plane
            for mt in ((18, 20) if union else (model_type,)):
                f, s = _extents.frames(row[None], mt)
                assert f.shape == (1, 15) and s.tolist() == [surface]
                kind, o, g, u, v, radii = f[0, 0], f[0, 1:4], f[0, 4:7], f[0, 7:10], f[0, 10:13], f[0, 13:15]
                assert kind == {6: 0, 12: 1, 14: 2, 16: 2, 8: 3, 22: 4}[surface]
                m = np.array([g, u, v])
                assert np.abs(m @ m.T - np.eye(3)).max() <= 4 * EPS
                assert np.linalg.det(m) > 0.5                    # v = g x u: right-handed
                if d is None:
                    assert np.array_equal(m, [[0, 0, 1], [1, 0, 0], [0, 1, 0]]) and np.array_equal(o, q[:3])
                else:
                    assert np.abs(np.cross(g, d / np.linalg.norm(d))).max() <= 4 * EPS and g @ d > 0
                if surface == 6:
                    assert abs(q[:3] @ o + q[3]) <= 8 * EPS       # the origin lies on the plane
                elif surface != 8:
                    assert np.array_equal(o, q[:3])
                assert radii.tolist() == {6: [0, 0], 12: [0, 0], 14: [q[-1], 0], 8: [q[3], 0]}.get(surface, list(q[-2:]))
                seen.add((mt, surface))
    assert len(seen) == (8 if union else 6)


def test_frame_tie_rule_on_axis_aligned_directions():
    # k = the index of the smallest |g_k|, the lowest on ties; t = e_k - g_k g; u = t / |t|; v = g x u
    for d, u, v in [((0, 0, 1), (1, 0, 0), (0, 1, 0)), ((0, 0, -2), (1, 0, 0), (0, -1, 0)), ((1, 0, 0), (0, 1, 0), (0, 0, 1)),
                    ((0, 5, 0), (1, 0, 0), (0, 0, -1)), ((-1, 0, 0), (0, 1, 0), (0, 0, -1))]:
        f, _ = _extents.frames(np.array([[0.0, 0.0, 0.0, *d]], dtype=np.float64), 12)
        assert np.array_equal(f[0, 4:7], np.array(d) / np.linalg.norm(d)) and np.array_equal(f[0, 7:10], u) and np.array_equal(f[0, 10:13], v)
    g, u, v = _extents.triad([1.0, 1.0, 1.0])                    # a three-way tie: k = 0
    assert u[0] > 0 and u[1] == u[2] < 0
    g, u, v = _extents.triad([2.0, 1.0, 1.0])                    # a tie between 1 and 2: k = 1
    assert u[1] > 0 and u[0] < 0 and u[2] < 0


@pytest.mark.parametrize("model_type, row", [
    (6, [0.0, 0.0, 0.0, 1.0]), (6, [np.nan, 0.0, 1.0, 0.0]), (6, [0.0, 0.0, 1.0, np.inf]),
    (8, [0.0, 0.0, np.nan, 1.0]), (8, [0.0, 0.0, 0.0, np.inf]),
    (12, [0.0, 0.0, 0.0, 0.0, 0.0, 0.0]), (12, [0.0, 0.0, 0.0, 1e-200, 0.0, 0.0]), (12, [0.0, 0.0, 0.0, 1e200, 1e200, 0.0]),
    (14, [0.0, 0.0, 0.0, 0.0, 0.0, 1.0, np.nan]), (16, [0.0, np.inf, 0.0, 0.0, 0.0, 1.0, 0.9, 0.4]), (22, [0.0] * 8),
    (18, [7.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0]), (18, [np.nan, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0]),
    (18, [12.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0]), (20, [22.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 1.0, 0.2]),
    (20, [6.5, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0]), (18, [14.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0]),
])
def test_bad_rows_and_bad_classes_have_no_frame(model_type, row):
    f, s = _extents.frames(np.array([row], dtype=np.float64), model_type)
    assert f[0, 0] == -1 and np.isnan(f[0, 1:]).all() and s.tolist() == [-1]
    pts = np.random.default_rng(0).normal(size=(10, 3))
    out = EM.extents(pts, np.zeros(10, np.int32), f)             # all its points are skipped, its count is 0 and its bounds are empty
    assert out["skipped"] == 10 and out["count"].tolist() == [0] and np.isposinf(out["lo"]).all() and np.isneginf(out["hi"]).all()
    assert out["sectors"].tolist() == [[0, 0]] and out["occupancy"].tolist() == [0]


def test_union_padding_is_not_a_parameter():
    row = np.array([[6.0, 0.0, 0.0, 1.0, 0.5, np.nan, np.nan, np.nan, np.nan]])   # a plane reads q0 .. q3 only
    f, s = _extents.frames(row, 18)
    assert f[0, 0] == 0 and s.tolist() == [6]


def test_frames_follow_the_parent():
    rng = np.random.default_rng(3)
    models = np.array([EM.single_models(rng)[14] for _ in range(4)])
    parent = np.array([2, 2, 0, 3, 3, 3], dtype=np.int32)
    f, s = _extents.frames(models, 14, parent)
    g, _ = _extents.frames(models, 14)
    assert np.array_equal(f, g[parent]) and s.tolist() == [14] * 6
    f, s = _extents.frames(models, 14, np.zeros(0, np.int32))
    assert f.shape == (0, 15) and s.shape == (0,)


# ---- S ----------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("extents") / "libextents_driver.so")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-o", so,
                           os.path.join(HERE, "emu", "extents_driver.cpp")])
    return C.CDLL(so)


def ptr(a):
    return C.c_void_p(a.ctypes.data)


def emu_sectors(emu, x, y):
    x, y = np.ascontiguousarray(x, dtype=np.float64), np.ascontiguousarray(y, dtype=np.float64)
    out = np.empty(len(x), dtype=np.int32)
    emu.ext_emu_sectors(ptr(x), ptr(y), C.c_int64(len(x)), ptr(out))
    return out


def test_the_thresholds_are_the_tangents():
    header = open(HEADER).read()
    for k, t in enumerate(EM.TAN, start=1):
        assert repr(float(t)) in header
        assert abs(t - math.tan(k * math.pi / 32)) <= 2 * EPS * t
    assert EM.TAN[3] == math.sqrt(2.0) - 1.0 or abs(EM.TAN[3] - (math.sqrt(2.0) - 1.0)) <= EPS


def test_sector_rule_against_floor_atan2(emu):
    rng = np.random.default_rng(2026)
    n = 100000
    x, y = rng.normal(size=n), rng.normal(size=n) * np.exp(rng.uniform(-8, 8, n))
    angle = np.mod(np.arctan2(y, x), TWO_PI) / (TWO_PI / 64)
    near = np.abs(angle - np.round(angle)) * (TWO_PI / 64) < 1e-9
    assert near.sum() <= n // 10000
    ref = np.floor(angle).astype(np.int64)
    got = EM.sector(x, y)
    assert np.array_equal(got[~near], ref[~near])
    assert np.array_equal(emu_sectors(emu, x, y), got)           # the header's lines and the model agree everywhere, boundaries included
    print(f"{int(near.sum())} of {n} directions within 1e-9 rad of a boundary")


def test_sector_table_of_axes_and_diagonals(emu):
    # |x| == |y| is not a swap, t = 1 and q = 7: the diagonals fall into 7, 24, 39 and 56, where floor(atan2) would say 8, 24, 40, 56
    z = 0.0
    table = [((1, z), 0), ((1, 1), 7), ((z, 1), 15), ((-1, 1), 24), ((-1, z), 31), ((-1, -1), 39), ((z, -1), 48), ((1, -1), 56),
             ((1, -z), 0), ((-z, 1), 15), ((-1, -z), 31), ((-z, -1), 63 - 15), ((1, -1e-300), 63), ((-1e-300, 1), 16), ((-1, -1e-300), 32),
             ((-1e-300, -1), 47), ((1e-300, -1), 48), ((1e308, 1e308), 7), ((1e-310, 1e-310), 7), ((3.0, 3.0 * float(EM.TAN[0])), None)]
    xy = np.array([p for p, _ in table], dtype=np.float64)
    got = EM.sector(xy[:, 0], xy[:, 1])
    want = [s for _, s in table]
    assert all(w is None or g == w for g, w in zip(got.tolist(), want)), got.tolist()
    assert np.array_equal(emu_sectors(emu, xy[:, 0], xy[:, 1]), got)
    # every boundary k pi / 32 of the first quadrant as the literals place it: t >= T_k counts the boundary into the upper sector
    for k, t in enumerate(EM.TAN, start=1):
        assert EM.sector(np.array([1.0]), np.array([float(t)]))[0] == k
        assert EM.sector(np.array([1.0]), np.array([np.nextafter(float(t), 0.0)]))[0] == k - 1
        assert EM.sector(np.array([float(t)]), np.array([1.0]))[0] == 15 - k
        assert EM.sector(np.array([np.nextafter(float(t), 0.0)]), np.array([1.0]))[0] == 16 - k


def test_keys_preserve_the_order(emu):
    rng = np.random.default_rng(4)
    x = np.concatenate([[-np.inf, -1.7976931348623157e308, -1.0, -5e-324, 0.0, 5e-324, 1.0, 1.7976931348623157e308, np.inf],
                        rng.normal(size=2000) * np.exp(rng.uniform(-600, 600, 2000))])
    x = np.sort(x)
    keys, back = np.empty(len(x), np.uint64), np.empty(len(x))
    assert emu.ext_emu_keys(ptr(x), C.c_int64(len(x)), ptr(keys), ptr(back)) == 1
    assert np.array_equal(back.view(np.uint64), x.view(np.uint64)) and (np.diff(keys.astype(object)) >= 0).all()


# ---- the statements against the model -------------------------------------------------------------------------------------------------------
def run_emu(emu, pts, labels, frames, group=1):
    pts = np.ascontiguousarray(pts, dtype=np.float64)
    labels = np.ascontiguousarray(labels, dtype=np.int32)
    frames = np.ascontiguousarray(frames, dtype=np.float64).reshape(-1, 15)
    K = len(frames)
    count, lo, hi = np.empty(K, np.int64), np.empty((K, 2)), np.empty((K, 2))
    sectors, occupancy, skipped = np.empty((K, 2), np.uint64), np.empty(K, np.uint64), C.c_int64(-7)
    r = emu.ext_emu_run(ptr(pts), C.c_int64(len(pts)), ptr(labels), ptr(frames), C.c_int32(K), C.c_int(group), ptr(count), ptr(lo), ptr(hi),
                        ptr(sectors), ptr(occupancy), C.byref(skipped))
    assert r == 0
    return dict(count=count, lo=lo, hi=hi, sectors=sectors, occupancy=occupancy, skipped=skipped.value)


@pytest.fixture(scope="module")
def references():
    return {case[0]: (case, EM.extents(*case[1:])) for case in EM.all_cases()}


CASE_NAMES = [case[0] for case in EM.all_cases()]


@pytest.mark.parametrize("name", CASE_NAMES)
def test_the_statements_equal_the_model(emu, references, name):
    (_, pts, labels, frames), ref = references[name]
    assert EM.same(run_emu(emu, pts, labels, frames), ref)
    assert EM.same(run_emu(emu, pts, labels, frames, group=64), ref)          # merged in runs and through a partial table: the same bits
    assert EM.same(run_emu(emu, pts, labels, frames, group=7), ref)
    order = np.random.default_rng(len(name)).permutation(len(pts))
    assert EM.same(run_emu(emu, pts[order], labels[order], frames, group=3), ref)   # in any order


def test_the_cases_cover_what_they_are_meant_to(references):
    assert len(CASE_NAMES) == len(set(CASE_NAMES)) == 6 + 2 + 3 + 6 + 3 + 2
    ref = references["scene-single-types"][1]
    assert EM.same(ref, references["scene-type-18-rows"][1]) and (ref["count"] > 150).all()
    assert np.array_equal(references["scene-single-types"][0][3], references["scene-type-18-rows"][0][3])   # one frame, either way
    assert np.isfinite(ref["lo"][:, 0]).sum() == 5 and (ref["sectors"][5] != 0).all() and ref["sectors"][0].tolist() == [0, 0]
    assert references["nan-and-inf-rows"][1]["skipped"] == 4 - int((references["nan-and-inf-rows"][0][2][[5, 17, 40, 41]] == -1).sum()
                                                                   + (references["nan-and-inf-rows"][0][2][[5, 17, 40, 41]] >= 6).sum())
    assert references["axis-and-centre"][1]["skipped"] >= 3
    assert references["frame-of-kind--1"][1]["count"][2] == 0 and references["frame-of-kind--1"][1]["skipped"] > 50
    assert references["instance-without-points"][1]["count"][2] == 0
    assert references["all-out-of-range"][1]["count"].sum() == 0 and references["all-out-of-range"][1]["skipped"] == 0
    assert references["one-live-point"][1]["count"].tolist() == [0, 0, 0, 0, 1, 0]
    for K in EM.SWITCH:
        assert len(references[f"instances-{K}"][0][3]) == K
    exact = references["exact"][1]
    assert exact["count"].tolist() == [8, 3, 2, 2] and exact["skipped"] == 5
    assert exact["lo"][0].tolist() == [0.0, 0.0] and exact["hi"][0].tolist() == [0.0, 8.0]           # hi == lo in a: bin 0 throughout
    assert not np.signbit(exact["lo"][0]).any() and not np.signbit(exact["hi"][0]).any()             # -0 never arrives
    assert exact["occupancy"][0] == sum(1 << b for b in (0, 1, 6, 7))                                # b: 0, 0.999 | 1 | 6.999 | 7, 8
    assert exact["lo"][2, 0] == exact["hi"][2, 0] == 4.0 and exact["occupancy"][2] == 1              # a line, one place twice
    assert EM.same(exact, references["exact-reversed"][1])


# ---- mask -> arc --------------------------------------------------------------------------------------------------------------------------
def test_mask_to_arc():
    sector = TWO_PI / 64
    assert all(math.isnan(v) for v in _extents.mask_to_arc(0))
    assert _extents.mask_to_arc(1 << 5) == (5 * sector, sector)
    assert _extents.mask_to_arc((1 << 62) | (1 << 63) | 1 | 2) == (62 * sector, 4 * sector)          # a run across the seam
    assert _extents.mask_to_arc(2 ** 64 - 1) == (0.0, TWO_PI)
    assert _extents.mask_to_arc(np.uint64(2 ** 64 - 1)) == (0.0, TWO_PI)
    two = (0b111 << 10) | (0b11 << 40)                                                               # gaps of 27 and 32 sectors: the longer is left out
    assert _extents.mask_to_arc(two) == (10 * sector, 32 * sector)
    assert _extents.mask_to_arc((1 << 0) | (1 << 32)) == (32 * sector, 33 * sector)                  # equal gaps: the first one, 1 .. 31, is left out
    assert _extents.mask_to_arc((2 ** 64 - 1) ^ (1 << 20)) == (21 * sector, 63 * sector)


# ---- areas ----------------------------------------------------------------------------------------------------------------------------------
FULL = 2 ** 64 - 1


def test_areas_against_closed_forms():
    close = lambda got, want: abs(got - want) <= 1e-12 * abs(want)
    inf = math.inf
    assert close(_extents.area(8, (0.7, 0.0), (-1.0, inf), (1.0, -inf), (0, FULL), FULL), 4 * math.pi * 0.7 ** 2)
    assert close(_extents.area(22, (1.5, 0.3), (inf, inf), (-inf, -inf), (FULL, FULL), FULL), 4 * math.pi ** 2 * 1.5 * 0.3)
    assert close(_extents.area(14, (0.4, 0.0), (-0.25, inf), (1.75, -inf), (0, FULL), FULL), TWO_PI * 0.4 * 2.0)
    assert close(_extents.area(6, (0.0, 0.0), (-1.0, 2.0), (3.0, 2.5), (0, 0), FULL), 4.0 * 0.5)
    # half a cylinder: the sectors 0 .. 31, the angular bins 0 .. 3 of every height
    half_cells = sum(1 << (8 * a + b) for a in range(8) for b in range(4))
    assert close(_extents.area(14, (0.4, 0.0), (-0.25, inf), (1.75, -inf), (0, 2 ** 32 - 1), half_cells), math.pi * 0.4 * 2.0)
    # a cone between the heights 0.5 and 1.5: pi (r0 + r1) times the slant length
    half = math.radians(25.0)
    c, s = math.cos(half), math.sin(half)
    frustum = math.pi * (0.5 * s / c + 1.5 * s / c) * (1.0 / c)
    assert close(_extents.area(16, (c, s), (0.5, inf), (1.5, -inf), (0, FULL), FULL), frustum)
    assert close(_extents.area(16, (c, s), (-1.5, inf), (-0.5, -inf), (0, FULL), FULL), frustum)     # the other nappe
    both = math.pi * (s / c) * (1.0 / c) * (1.0 + 4.0)                                                # heights -1 .. 2: two cones
    assert close(_extents.area(16, (c, s), (-1.0, inf), (2.0, -inf), (0, FULL), FULL), both)
    # part of a surface: one cell of a plane, the outer half of a torus, a sphere cap
    assert close(_extents.area(6, (0.0, 0.0), (0.0, 0.0), (8.0, 16.0), (0, 0), 1 << 9), 2.0)
    outer = (2 ** 16 - 1) | ((2 ** 16 - 1) << 48)                                                     # theta in (-pi/2, pi/2)
    outer_cells = sum(1 << (8 * a + b) for a in range(8) for b in (0, 1, 6, 7))
    assert close(_extents.area(22, (1.5, 0.3), (inf, inf), (-inf, -inf), (FULL, outer), outer_cells),
                 TWO_PI * 0.3 * (1.5 * math.pi + 2 * 0.3))
    cap = sum(1 << (8 * 7 + b) for b in range(8))                                                     # the top eighth of the cosine range
    assert close(_extents.area(8, (2.0, 0.0), (-1.0, inf), (1.0, -inf), (0, FULL), cap), TWO_PI * 4.0 * 0.25)
    assert math.isnan(_extents.area(12, (0.0, 0.0), (0.0, inf), (1.0, -inf), (0, 0), 1))
    assert math.isnan(_extents.area(-1, (math.nan, math.nan), (inf, inf), (-inf, -inf), (0, 0), 0))
    assert _extents.area(14, (0.4, 0.0), (inf, inf), (-inf, -inf), (0, 0), 0) == 0.0


def test_areas_of_sampled_surfaces_through_the_model():
    """densely sampled surfaces through the numpy model and the host's derivation: what the public call returns but for the device"""
    rng = np.random.default_rng(8)
    models = EM.single_models(rng)
    # sampled bounds lie inside the true ones (1 % allowed); the half shell starts anywhere in a sector, so it occupies 33 of them
    for surface, want, tol, over in ((8, 4 * math.pi * 0.7 ** 2, 0.01, 0.0), (22, 4 * math.pi ** 2 * 1.5 * 0.3, 1e-9, 1e-9),
                                     (14, math.pi * 0.4 * 2.0, 0.01, 1.0 / 32), (6, 2.0 * 1.0, 0.01, 0.0),
                                     (16, math.pi * math.tan(math.radians(25.0)) / math.cos(math.radians(25.0)) * 2.0, 0.01, 0.0)):
        pts = EM.sample_surface(surface, models[surface], 40000, rng, noise=0.0)
        f, s = _extents.frames(models[surface][None], surface)
        if surface == 6:                                         # a rectangle along the frame's own u and v: the grid's cells are whole
            pts = f[0, 1:4] + rng.uniform(-1, 1, (40000, 1)) * f[0, 7:10] + rng.uniform(-0.5, 0.5, (40000, 1)) * f[0, 10:13]
        out = EM.extents(pts, np.zeros(len(pts), np.int32), f)
        arc, area = _extents.derive(s, f, out["lo"], out["hi"], out["sectors"], out["occupancy"])
        assert -tol * want <= area[0] - want <= (over + 1e-12) * want, (surface, area[0], want)
        if surface == 14:                                        # the half shell: 32 or 33 sectors of an arbitrary start
            assert 32 * TWO_PI / 64 <= arc[0, 1, 1] <= 33 * TWO_PI / 64 and math.isnan(arc[0, 0, 0])
        if surface in (8, 16, 22):
            assert arc[0, 1].tolist() == [0.0, TWO_PI]


# ---- the public function ------------------------------------------------------------------------------------------------------------------
class ModelContext:
    """Context.instance_extents by the numpy model"""
    def instance_extents(self, points, labels, frames):
        return EM.extents(points, labels, frames)


@pytest.fixture
def model_context(monkeypatch):
    from pyprogressivex import _api
    monkeypatch.setattr(_api, "_context", lambda: ModelContext())


def test_instance_extents_is_exported_with_its_signature():
    assert "instanceExtents" in px.__all__
    sig = inspect.signature(px.instanceExtents)
    assert list(sig.parameters) == ["points", "labels", "models", "model_type", "parent"]
    assert sig.parameters["parent"].default is None
    doc = " ".join(px.instanceExtents.__doc__.split())
    for phrase in ("models[parent[j]]", "64 sectors", "changes nothing about how the find* calls score", "skipped"):
        assert phrase in doc, phrase


POINTS = np.arange(30.0).reshape(10, 3)
LABELS = np.zeros(10, dtype=np.int32)
PLANE = np.array([[0.0, 0.0, 1.0, 0.0]])


@pytest.mark.parametrize("args, kw, match", [
    ((np.zeros((10, 2)), LABELS, PLANE, 6), {}, r"points should be an array with dims \[n,3\]"),
    ((np.zeros(10), LABELS, PLANE, 6), {}, "points should be"),
    ((POINTS, np.zeros(9, dtype=np.int32), PLANE, 6), {}, "labels should be an array with dims"),
    ((POINTS, np.zeros((10, 1), dtype=np.int32), PLANE, 6), {}, "labels should be an array with dims"),
    ((POINTS, np.zeros(10), PLANE, 6), {}, "labels should be integers"),
    ((POINTS, np.zeros(10, dtype=bool), PLANE, 6), {}, "labels should be integers"),
    ((POINTS, LABELS, PLANE, 0), {}, "model_type should be one of the 3-D surface types"),       # 2-D lines
    ((POINTS, LABELS, PLANE, 10), {}, "model_type should be"),                                   # circles
    ((POINTS, LABELS, np.zeros((1, 9)), 1), {}, "model_type should be"),                         # homographies
    ((POINTS, LABELS, PLANE, 7), {}, "model_type should be"),
    ((POINTS, LABELS, PLANE, 6.0), {}, "model_type should be"),
    ((POINTS, LABELS, PLANE, True), {}, "model_type should be"),
    ((POINTS, LABELS, np.zeros((1, 5)), 6), {}, r"models should be an array with dims \[K,4\]"),
    ((POINTS, LABELS, np.zeros(4), 6), {}, "models should be"),
    ((POINTS, LABELS, np.zeros((1, 8)), 18), {}, r"models should be an array with dims \[K,9\]"),
    ((POINTS, LABELS, PLANE, 6), dict(parent=np.zeros((1, 1), dtype=np.int32)), "parent should be None or an array"),
    ((POINTS, LABELS, PLANE, 6), dict(parent=np.zeros(1)), "parent should be integers"),
    ((POINTS, LABELS, PLANE, 6), dict(parent=np.array([1])), "parent should index the rows of models"),
    ((POINTS, LABELS, PLANE, 6), dict(parent=np.array([-1])), "parent should index the rows of models"),
])
def test_instance_extents_rejects_bad_arguments_before_it_touches_the_context(args, kw, match, monkeypatch):
    from pyprogressivex import _api

    def no_context():
        raise AssertionError("the context was touched before the arguments were checked")
    monkeypatch.setattr(_api, "_context", no_context)
    with pytest.raises(ValueError, match=match):
        px.instanceExtents(*args, **kw)


def test_label_sentences_are_those_of_split_components(monkeypatch):
    from pyprogressivex import _api
    monkeypatch.setattr(_api, "_context", lambda: pytest.fail("the context was touched"))
    for labels in (np.zeros(9, dtype=np.int32), np.zeros(10), np.zeros(10, dtype=bool)):
        with pytest.raises(ValueError) as a:
            px.splitComponents(POINTS, labels, 1)
        with pytest.raises(ValueError) as b:
            px.instanceExtents(POINTS, labels, PLANE, 6)
        assert str(a.value) == str(b.value)


def test_parent_none_is_the_identity_parent(model_context):
    pts, labels, models = EM.scene(800, seed=12)
    rows = np.zeros((4, 9))
    for i, surface in enumerate((6, 8, 14, 16)):
        rows[i, 0], rows[i, 1:1 + len(models[surface])] = surface, models[surface]
    relabel = np.array([0, 1, -1, 2, 3, -1])[np.where(labels < 6, labels, 0)]
    relabel = np.where((labels >= 0) & (labels < 6), relabel, labels).astype(np.int64)
    relabel[relabel > 3] = 2 ** 40                               # an outlier label that does not fit int32
    a = px.instanceExtents(pts, relabel, rows, 18)
    b = px.instanceExtents(pts, relabel, rows, 18, parent=np.arange(4))
    assert set(a) == {"kind", "surface", "count", "skipped", "origin", "axis", "u", "v", "radii", "lo", "hi", "sectors", "occupancy", "arc", "area"}
    for key in a:
        assert np.array_equal(np.asarray(a[key]), np.asarray(b[key]), equal_nan=True), key
    assert a["kind"].tolist() == [0, 3, 2, 2] and a["surface"].tolist() == [6, 8, 14, 16] and a["skipped"] == 0
    assert np.array_equal(a["count"], np.bincount(relabel[(relabel >= 0) & (relabel < 4)], minlength=4))
    assert a["kind"].dtype == np.int32 and a["count"].dtype == np.int64 and a["sectors"].dtype == a["occupancy"].dtype == np.uint64
    assert a["arc"].shape == (4, 2, 2) and a["area"].shape == (4,) and a["lo"].shape == a["hi"].shape == a["radii"].shape == (4, 2)
    # instances in another order and one model twice
    parent = np.array([3, 0, 0], dtype=np.int32)
    swapped = np.full(len(relabel), -1)
    swapped[relabel == 3], swapped[relabel == 0] = 0, 1
    c = px.instanceExtents(pts, swapped, rows, 20, parent=parent)
    assert c["kind"].tolist() == [2, 0, 0] and c["count"].tolist() == [a["count"][3], a["count"][0], 0]
    assert np.array_equal(c["lo"][:2], a["lo"][[3, 0]]) and np.array_equal(c["occupancy"][:2], a["occupancy"][[3, 0]])
    assert c["area"][2] == 0.0 and np.isnan(c["arc"][2]).all() and c["area"][0] == a["area"][3]
    # the rectangle holds its points; the half shell is a half
    e = pts[relabel == 0] - a["origin"][0]
    assert (e @ a["u"][0] >= a["lo"][0, 0]).all() and (e @ a["v"][0] <= a["hi"][0, 1]).all()
    assert 32 * TWO_PI / 64 <= a["arc"][2, 1, 1] <= 34 * TWO_PI / 64
    empty = px.instanceExtents(np.zeros((0, 3)), np.zeros(0, np.int32), rows, 18)
    assert empty["count"].tolist() == [0] * 4 and empty["skipped"] == 0 and (empty["area"] == 0).all()
    none = px.instanceExtents(pts, relabel, np.zeros((0, 9)), 18)
    assert none["count"].shape == (0,) and none["arc"].shape == (0, 2, 2) and none["skipped"] == 0


def test_the_library_exports_the_entry_point():
    assert "pgx_instance_extents" in _lib.ABI_SYMBOLS
    assert len(_lib.ABI_SYMBOLS) == len(set(_lib.ABI_SYMBOLS))
    header = open(HEADER).read()
    assert ("int pgx_instance_extents(pgx_ctx *ctx, const double *points, int64_t n,\n"
            "                         const int32_t *labels, const double *frames, int32_t K,\n"
            "                         int64_t *count_out, double *lo_out, double *hi_out,\n"
            "                         uint64_t *sectors_out, uint64_t *occupancy_out, int64_t *skipped);") in header
    assert hasattr(C.CDLL(_lib.LIB_PATH), "pgx_instance_extents")
    assert hasattr(_lib.Context, "instance_extents")
    for name, value in (("FRAME", _lib.EXTENTS_FRAME), ("LDS_INSTANCES", _lib.EXTENTS_LDS_INSTANCES), ("MAX_INSTANCES", _lib.EXTENTS_MAX_INSTANCES)):
        assert int(re.search(rf"#define PGX_EXTENTS_{name} (\d+)", header).group(1)) == value
    assert _lib.EXTENTS_FRAME == _extents.FRAME == EM.FRAME and _lib.EXTENTS_LDS_INSTANCES == EM.LDS_INSTANCES
    point_header = open(os.path.join(os.path.dirname(HERE), "progressive-x_amd", "csrc", "extents_point.h")).read()
    for t in EM.TAN:
        assert repr(float(t)) in point_header
