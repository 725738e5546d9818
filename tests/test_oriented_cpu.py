"""findOrientedPrimitives without a GPU: the ABI entries of PGX_ORIENTED_PRIMITIVE3D = 20, the numpy restatement of its compatibility
test (tests/oriented_model.py) - its invariances and its geometry on every class - OrientedPrimitiveEstimator's solver against
PrimitiveEstimator's, and the public call's signature and input checks."""
import ctypes
import inspect

import numpy as np
import pytest

import pyprogressivex as px
from oriented_model import compatible, kappa_of, prefix_compatible, sq_oriented, surface_normal
from primitive_model import CONE, CYLINDER, PLANE, PREFIX, SPHERE, class_of, sq_primitive
from pyprogressivex import _estimators, _lib, datasets


def test_model_dims_and_registries_of_the_oriented_type():
    lib = _lib.load()
    d, p = ctypes.c_int(), ctypes.c_int()
    assert lib.pgx_model_dims(20, ctypes.byref(d), ctypes.byref(p)) == 0
    assert (d.value, p.value) == (3, 9) == _lib.MODEL_TABLE[20][:2]
    assert _lib.ORIENTED_PRIMITIVE3D == 20 and _lib.MODEL_TABLE[20] == (3, 9, 4, 4) == _lib.MODEL_TABLE[18]
    assert _lib.POINT_DIM[20] == 3 and _lib.PARAM_DIM[20] == 9
    for unassigned in (19, 21, -1):
        assert lib.pgx_model_dims(unassigned, None, None) != 0 and unassigned not in _lib.MODEL_TABLE
    est = _estimators.OrientedPrimitiveEstimator
    assert issubclass(est, _estimators.PrimitiveEstimator)
    assert (est.model_type, est.sample_size, est.device_slots, est.cols, est.device_minimal) == (20, 4, 4, 9, True)
    assert _estimators.ESTIMATORS["oriented_primitive"] is est and datasets.MODEL_TYPES["oriented_primitive"] == 20
    assert _estimators.ESTIMATORS["primitive"] is _estimators.PrimitiveEstimator and _estimators.PrimitiveEstimator.model_type == 18
    assert hasattr(lib, "pgx_set_normal_tolerance") and "pgx_set_normal_tolerance" in _lib.ABI_SYMBOLS
    assert hasattr(_lib.Context, "set_normal_tolerance")


def test_the_estimator_adds_one_call_to_the_context_setup():
    calls = []

    class Ctx:
        def set_radius_range(self, lo, hi):
            calls.append(("radius", lo, hi))

        def set_normals(self, nrm):
            calls.append(("normals", nrm))

        def set_primitive_classes(self, mask, lo, hi):
            calls.append(("classes", mask, lo, hi))

        def set_normal_tolerance(self, cos2):
            calls.append(("tolerance", cos2))
    est = _estimators.OrientedPrimitiveEstimator(("plane", "cone"), 30.0)
    est.normals = np.ones((5, 3))
    est.context_setup(Ctx())
    assert sorted(c[0] for c in calls) == ["classes", "normals", "radius", "tolerance"]
    assert dict((c[0], c[1:]) for c in calls)["tolerance"] == (kappa_of(30.0),) and est.kappa == kappa_of(30.0)
    assert abs(est.kappa - 0.75) < 1e-15 and est.class_mask == 9 and est.normal_tolerance == 30.0
    assert _estimators.OrientedPrimitiveEstimator().normal_tolerance == 20.0
    assert _estimators.OrientedPrimitiveEstimator(normal_tolerance=90.0).kappa == 0.0
    for bad in (0.0, -1.0, 91.0, np.nan, np.inf):
        with pytest.raises(ValueError, match="normal_tolerance"):
            _estimators.OrientedPrimitiveEstimator(normal_tolerance=bad)


# ---- the public call ----------------------------------------------------------------------------------------------------------------------
def test_find_oriented_primitives_has_find_primitives_signature_plus_the_tolerance():
    assert "findOrientedPrimitives" in px.__all__ and callable(px.findOrientedPrimitives)
    sig, base = inspect.signature(px.findOrientedPrimitives).parameters, inspect.signature(px.findPrimitives).parameters
    assert [k for k in sig if k != "normal_tolerance"] == list(base)                # findPrimitives' parameters in findPrimitives' order
    for k, v in base.items():
        assert sig[k].kind == v.kind and (sig[k].default is v.default or sig[k].default == v.default), k
    tol = sig["normal_tolerance"]
    assert tol.kind is inspect.Parameter.KEYWORD_ONLY and tol.default == 20.0
    doc = px.findOrientedPrimitives.__doc__
    assert "Schnabel" in doc and "default" in doc and "tuned" in doc and "4.14" in doc and "degrees" in doc


@pytest.mark.parametrize("bad", [0.0, 0, -1.0, 91.0, np.nan])
def test_find_oriented_primitives_rejects_a_bad_tolerance(bad):
    with pytest.raises(ValueError, match="normal_tolerance"):
        px.findOrientedPrimitives(np.zeros((10, 3)), np.zeros((10, 3)), normal_tolerance=bad)


@pytest.mark.parametrize("normals", [np.zeros((10, 2)), np.zeros((9, 3)), np.zeros(30), np.zeros((10, 3, 1)), None])
def test_find_oriented_primitives_rejects_bad_normals(normals):
    with pytest.raises(ValueError, match=r"normals should be an array with dims \[n,3\]"):
        px.findOrientedPrimitives(np.zeros((10, 3)), normals)


def test_find_oriented_primitives_rejects_bad_classes_points_and_ranges():
    p, nrm = np.zeros((10, 3)), np.zeros((10, 3))
    for bad in ((), ("plane", "plane"), ("torus",), "sphere", None, ("plane", 8)):
        with pytest.raises(ValueError, match="classes"):
            px.findOrientedPrimitives(p, nrm, classes=bad)
    with pytest.raises(ValueError, match=r"points should be an array with dims \[n,3\], n>=4"):
        px.findOrientedPrimitives(np.zeros((3, 3)), np.zeros((3, 3)))
    with pytest.raises(ValueError, match="angle_range"):
        px.findOrientedPrimitives(p, nrm, angle_range=(0.0, 10.0))
    with pytest.raises(ValueError, match="radius_range"):
        px.findOrientedPrimitives(p, nrm, radius_range=(2.0, 1.0))


# ---- the restatement: invariances ---------------------------------------------------------------------------------------------------------
def _generic():
    """a scene's points with its (noisy, unit) normals, and rows of all four classes: the ground truth, perturbed copies, random ones"""
    pts, nrm, _, _, gt = datasets.make_primitives(n_per=120, n_outliers=300, seed=3)
    rng = np.random.default_rng(5)
    rows = [g.copy() for g in gt]
    for g in gt:
        r = g.copy()
        r[1:4] += rng.normal(0, 0.05, 3)
        rows.append(r)
    rows.append(np.concatenate([[PLANE], rng.normal(size=3), [-3.0], np.zeros(4)]))
    rows.append(np.concatenate([[CYLINDER], rng.uniform(0, 10, 3), rng.normal(size=3), [1.5, 0.0]]))
    rows.append(np.concatenate([[CONE], rng.uniform(0, 10, 3), rng.normal(size=3), [np.cos(0.5), np.sin(0.5)]]))
    return pts, nrm, np.array(rows)


def test_at_kappa_zero_the_residual_is_type_18s_bit_for_bit():
    pts, nrm, rows = _generic()
    for m in rows:
        assert np.array_equal(sq_oriented(pts, nrm, m, 0.0), sq_primitive(pts, m))
        assert np.array_equal(sq_oriented(pts, nrm * 7.5, m, kappa_of(90.0)), sq_primitive(pts, m))


@pytest.mark.parametrize("tol", [10.0, 20.0, 45.0])
def test_sign_and_power_of_two_scale_of_the_normals_change_nothing(tol):
    pts, nrm, rows = _generic()
    rng = np.random.default_rng(int(tol))
    flip = np.where(rng.random(len(pts)) < 0.5, -1.0, 1.0)[:, None]
    scale = (2.0 ** rng.integers(-40, 41, len(pts)))[:, None]
    kappa = kappa_of(tol)
    some = 0
    for m in rows:
        want = sq_oriented(pts, nrm, m, kappa)
        assert np.array_equal(sq_oriented(pts, nrm * flip, m, kappa), want)
        assert np.array_equal(sq_oriented(pts, nrm * scale, m, kappa), want)
        assert np.array_equal(sq_oriented(pts, nrm * flip * scale, m, kappa), want)
        assert set(np.unique(want[np.isinf(want)])) <= {np.inf} and not np.isnan(want).any()
        some += int(np.isinf(want).sum() > 0) + int(np.isfinite(want).sum() > 0)
        assert np.array_equal(want[np.isfinite(want)], sq_primitive(pts, m)[np.isfinite(want)])
    assert some == 2 * len(rows)                                                  # every row has compatible and incompatible points


def test_nan_and_zero_normals_are_incompatible_and_an_unknown_class_gives_nan():
    pts, nrm, rows = _generic()
    bad = nrm.copy()
    bad[0::3] = 0.0
    bad[1::3, 1] = np.nan
    for kappa in (0.0, kappa_of(20.0), 1.0):
        for m in rows:
            sq = sq_oriented(pts, bad, m, kappa)
            assert np.isposinf(sq[0::3]).all() and np.isposinf(sq[1::3]).all()
            assert np.array_equal(sq[2::3], sq_oriented(pts, nrm, m, kappa)[2::3])
        for cls in (7.0, 0.0, 6.5, 18.0, 20.0, np.nan, np.inf):
            m = rows[0].copy()
            m[0] = cls
            assert class_of(m) is None and np.isnan(sq_oriented(pts, nrm, m, kappa)).all()
            assert surface_normal(pts, m) is None and not compatible(pts, nrm, m, kappa).any()
    # a point at the sphere's centre, on the cylinder's axis and at the cone's apex: g = 0, incompatible even at kappa = 0
    # (models with exactly representable entries, so that g is an exact zero)
    exact = np.array([[SPHERE, 1.0, 2.0, 3.0, 0.5, 0.0, 0.0, 0.0, 0.0], [CYLINDER, 1.0, 2.0, 3.0, 0.0, 0.0, 1.0, 0.5, 0.0],
                      [CONE, 1.0, 2.0, 3.0, 0.0, 0.0, 1.0, 0.8, 0.6], [CONE, 1.0, 2.0, 3.0, 0.0, 0.0, 1.0, 1.0, 0.0]])
    at = np.array([[1.0, 2.0, 3.0], [1.0, 2.0, 7.0], [1.0, 2.0, 3.0], [1.0, 2.0, 7.0]])   # (the last: the axis of a cone of angle 0)
    for p, m in zip(at, exact):
        assert not compatible(p[None], np.array([[0.0, 0.0, 1.0]]), m, 0.0).any()
        assert np.isposinf(sq_oriented(p[None], np.array([[0.0, 0.0, 1.0]]), m, 0.0)).all()
    assert np.isnan(sq_oriented(pts, nrm, np.full(9, np.nan), 0.0)).all()


# ---- the restatement: geometry ------------------------------------------------------------------------------------------------------------
def _frame(rng):
    d = rng.normal(size=3)
    d /= np.linalg.norm(d)
    u = np.cross(d, rng.normal(size=3))
    u /= np.linalg.norm(u)
    return d, u, np.cross(d, u)


def _surface_cases():
    """(name, model row, points on the surface, their true unit normals) for every class at several scales"""
    rng = np.random.default_rng(11)
    out = []
    for k, off in ((1.0, 0.0), (1e-3, 2.5), (1e3, -40.0)):                        # plane: (a, b, c, d) times k, several offsets
        d, u, v = _frame(rng)
        pts = off * d + rng.uniform(-5, 5, (40, 1)) * u + rng.uniform(-5, 5, (40, 1)) * v
        out.append((f"plane k={k}", np.concatenate([[PLANE], k * d, [-k * off], np.zeros(4)]), pts, np.tile(d, (40, 1))))
    for r in (1e-3, 1.0, 1e3):                                                    # sphere: radii over six orders
        c = rng.uniform(-5, 5, 3)
        nrm = rng.normal(size=(40, 3))
        nrm /= np.linalg.norm(nrm, axis=1)[:, None]
        out.append((f"sphere r={r}", np.concatenate([[SPHERE], c, [r], np.zeros(4)]), c + r * nrm, nrm))
    for r, sign in ((1e-2, 1.0), (1.0, -1.0), (1e2, 1.0)):                        # cylinder: radii, either direction of the axis
        d, u, v = _frame(rng)
        p = rng.uniform(-5, 5, 3)
        phi, t = rng.uniform(0, 2 * np.pi, (40, 1)), rng.uniform(-10, 10, (40, 1))
        nrm = np.cos(phi) * u + np.sin(phi) * v
        out.append((f"cylinder r={r}", np.concatenate([[CYLINDER], p, sign * d, [r, 0.0]]), p + t * d + r * nrm, nrm))
    for theta, hs in ((5.0, 1.0), (30.0, 1e-2), (80.0, 1e2)):                     # cone: half-angles, heights over four orders
        d, u, v = _frame(rng)
        a = rng.uniform(-5, 5, 3)
        th = np.deg2rad(theta)
        phi, h = rng.uniform(0, 2 * np.pi, (40, 1)), hs * rng.uniform(0.5, 5, (40, 1))
        radial = np.cos(phi) * u + np.sin(phi) * v
        out.append((f"cone theta={theta}", np.concatenate([[CONE], a, d, [np.cos(th), np.sin(th)]]), a + h * d + h * np.tan(th) * radial,
                    np.cos(th) * radial - np.sin(th) * d))
    return out


def _tilted(nrm, beta_deg, rng):
    """the unit normals rotated by beta about a random tangent direction"""
    t = np.cross(nrm, rng.normal(size=nrm.shape))
    t /= np.linalg.norm(t, axis=1)[:, None]
    b = np.deg2rad(beta_deg)
    return nrm * np.cos(b) + np.cross(t, nrm) * np.sin(b)


@pytest.mark.parametrize("tol", [10.0, 20.0, 45.0, 89.0])
def test_the_tolerance_is_an_angle_to_the_true_surface_normal(tol):
    """half a degree either side of the tolerance: d cos^2 / d beta = sin(2 beta) >= 0.034 per radian at these angles, so the two sides
    differ by 3e-4 (w) or more - ten and more orders above the rounding of three dot products (a few 1e-16 w)"""
    rng = np.random.default_rng(int(tol))
    kappa = kappa_of(tol)
    for name, m, pts, nrm in _surface_cases():
        assert np.sqrt(sq_primitive(pts, m)).max() <= 1e-9 * max(1.0, np.abs(pts).max(), np.abs(m[1:5]).max()), name
        g = np.stack(surface_normal(pts, m), axis=1)
        cosang = np.abs((g * nrm).sum(axis=1)) / np.linalg.norm(g, axis=1)
        assert cosang.min() > 1.0 - 1e-9, name                                    # g is the true normal's direction
        inside, outside = _tilted(nrm, tol - 0.5, rng), _tilted(nrm, tol + 0.5, rng)
        assert compatible(pts, inside, m, kappa).all(), name
        assert not compatible(pts, outside, m, kappa).any(), name
        assert compatible(pts, -3.0 * inside, m, kappa).all() and not compatible(pts, -0.25 * outside, m, kappa).any(), name
        assert np.array_equal(sq_oriented(pts, inside, m, kappa), sq_primitive(pts, m)), name
        assert np.isposinf(sq_oriented(pts, outside, m, kappa)).all(), name


# ---- the solver ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tol,names", [(20.0, ("plane", "sphere", "cylinder", "cone")), (5.0, ("plane", "cone")), (90.0, ("plane", "sphere", "cylinder", "cone"))])
def test_minimal_keeps_type_18s_slots_that_agree_with_their_own_prefix(tol, names):
    pts, nrm, _, inst, _ = datasets.make_primitives(n_per=120, n_outliers=300, seed=7)
    nrm = nrm.copy()
    n = len(pts)
    rng = np.random.default_rng(1)
    samples = rng.integers(20, n, (200, 4)).astype(np.int32)
    for k in range(4):                                                            # samples inside one instance: models that fit their normals
        samples[20 * k:20 * k + 20] = rng.choice(np.flatnonzero(inst == k + 1), (20, 4))
    nrm[6] = 0.0
    nrm[8, 1] = np.nan
    samples[100] = [6, 15, 16, 17]
    samples[101] = [8, 15, 16, 17]
    samples[102] = [15, 16, 17, 6]                                                # the zero normal behind the plane's, the cylinder's and the cone's prefix
    base = _estimators.PrimitiveEstimator(names)
    est = _estimators.OrientedPrimitiveEstimator(names, tol)
    base.normals = est.normals = nrm
    with np.errstate(all="ignore"):
        rows18, src18 = base.minimal(pts, samples)
        rows, src = est.minimal(pts, samples)
    kappa = kappa_of(tol)
    keep = np.array([prefix_compatible(pts, nrm, samples[s], r, kappa) for r, s in zip(rows18, src18)])
    assert np.array_equal(rows, rows18[keep]) and np.array_equal(src, src18[keep])
    assert keep.sum() >= 20 and (~keep).sum() >= 2
    if tol < 90.0:
        assert (~keep).sum() > keep.sum() // 4                                    # random samples mostly disagree with their normals
    else:                                                                         # 90 degrees: only undefined normals remove a slot
        gone = [(int(s), r) for r, s in zip(rows18[~keep], src18[~keep])]
        assert {100, 101, 102} <= {s for s, _ in gone}
        for s, r in gone:                                                         # ... or g . g overflows (a model far away) or is 0 (a centre in the sample)
            idx = samples[s, :PREFIX[class_of(r)]]
            with np.errstate(all="ignore"):
                gg = sum(g * g for g in surface_normal(pts[idx], r))
            assert {6, 8} & set(idx.tolist()) or not np.isfinite(gg).all() or (gg == 0.0).any(), (s, r)
    got = {(int(s), class_of(r)) for r, s in zip(rows, src)}
    assert not any(s in (100, 101) for s, _ in got)                               # the undefined normal is in every prefix
    assert not any(c == SPHERE for s, c in got if s == 102)                       # only the sphere reads the fourth point
