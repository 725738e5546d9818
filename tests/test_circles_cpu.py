"""findCircles without a GPU: the ABI entries of the circle type, the public call's signature and input checks, the 3-point
solver and the algebraic refit of CircleEstimator against hand-made data, and the make_circles generator."""
import ctypes
import inspect

import numpy as np
import pytest

import pyprogressivex as px
from primitive_helpers import numpy_refit
from pyprogressivex import _estimators, _lib, datasets


def test_model_dims_of_the_circle_type():
    lib = _lib.load()
    d, p = ctypes.c_int(), ctypes.c_int()
    assert lib.pgx_model_dims(10, ctypes.byref(d), ctypes.byref(p)) == 0
    assert (d.value, p.value) == (2, 3)
    assert _lib.CIRCLE2D == 10 and _lib.MODEL_TABLE[10] == (2, 3, 3, 1)
    assert _lib.POINT_DIM[10] == 2 and _lib.PARAM_DIM[10] == 3
    assert _lib.GRAM_CIRCLE == 6 and _lib.GRAM_Q[_lib.GRAM_CIRCLE] == 4
    for unassigned in (7, 9, 11, -1):
        assert lib.pgx_model_dims(unassigned, None, None) != 0 and unassigned not in _lib.MODEL_TABLE
    # the types around the gaps are still what they were
    assert lib.pgx_model_dims(8, ctypes.byref(d), ctypes.byref(p)) == 0 and (d.value, p.value) == (3, 4)
    assert lib.pgx_model_dims(0, ctypes.byref(d), ctypes.byref(p)) == 0 and (d.value, p.value) == (2, 3)


def test_find_circles_is_exported_with_its_signature():
    assert "findCircles" in px.__all__ and callable(px.findCircles)
    sig = inspect.signature(px.findCircles)
    spheres = inspect.signature(px.findSpheres).parameters
    positional = [k for k, v in sig.parameters.items() if v.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD]
    assert positional == [k for k, v in spheres.items() if v.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD]
    kw = {k: v.default for k, v in sig.parameters.items() if v.kind is inspect.Parameter.KEYWORD_ONLY}
    assert kw == {k: v.default for k, v in spheres.items() if v.kind is inspect.Parameter.KEYWORD_ONLY}
    assert kw["radius_range"] is None
    # the defaults are findLines' pixel-scale values
    lines = inspect.signature(px.findLines).parameters
    defaults = {k: v.default for k, v in sig.parameters.items()}
    for k in positional:
        if k not in ("points", "weights"):
            assert defaults[k] == lines[k].default, k
    assert defaults["threshold"] == 2.0 and defaults["neighborhood_ball_radius"] == 200.0 and defaults["sampler_id"] == 3
    assert defaults["weights"] is None


@pytest.mark.parametrize("points", [np.zeros((10, 3)), np.zeros((10, 1)), np.zeros(30), np.zeros((2, 2)), np.zeros((0, 2)),
                                    np.zeros((4, 2, 1))])
def test_find_circles_rejects_bad_points(points):
    with pytest.raises(ValueError, match=r"points should be an array with dims \[n,2\], n>=3"):
        px.findCircles(points)


def test_point_cloud_calls_keep_their_messages():
    with pytest.raises(ValueError, match=r"points should be an array with dims \[n,3\], n>=4"):
        px.findSpheres(np.zeros((10, 2)))
    with pytest.raises(ValueError, match=r"points should be an array with dims \[n,3\], n>=3"):
        px.findPlanes(np.zeros((10, 2)))


def test_find_circles_rejects_weights_of_the_wrong_length():
    with pytest.raises(ValueError, match="weights"):
        px.findCircles(np.zeros((10, 2)), np.ones(9))


@pytest.mark.parametrize("rr", [(np.nan, 1.0), (0.0, np.nan), (-0.1, 1.0), (2.0, 1.0), (1.0,), (1.0, 2.0, 3.0), "ab", 3.0])
def test_find_circles_rejects_bad_radius_ranges(rr):
    with pytest.raises(ValueError, match="radius_range"):
        px.findCircles(np.zeros((10, 2)), radius_range=rr)


def test_find_circles_unknown_sampler_prints_and_returns_no_model(capsys):
    pts, _, _ = datasets.make_circles(n_per_circle=50, n_circles=2, n_outliers=20, seed=1)
    circles, labels = px.findCircles(pts, sampler_id=7, radius_range=(1.0, 500.0))
    assert circles.shape == (0, 3) and circles.dtype == np.float64
    assert labels.shape == (pts.shape[0],) and labels.dtype == np.int32 and not labels.any()
    assert "Unknown sampler identifier: 7" in capsys.readouterr().err


def _circle_scalar(p):
    """the solver's operation order on Python floats (IEEE doubles, no contraction)"""
    a10, a11 = p[1][0] - p[0][0], p[1][1] - p[0][1]
    a20, a21 = p[2][0] - p[0][0], p[2][1] - p[0][1]
    h1 = 0.5 * (a10 * a10 + a11 * a11)
    h2 = 0.5 * (a20 * a20 + a21 * a21)
    det = a10 * a21 - a11 * a20
    e0 = (h1 * a21 - h2 * a11) / det
    e1 = (a10 * h2 - a20 * h1) / det
    r = (e0 * e0 + e1 * e1) ** 0.5
    return [p[0][0] + e0, p[0][1] + e1, r]


def test_circle_minimal_solver_on_hand_made_samples():
    pts = np.array([[3.0, 2.0], [1.0, 4.0], [-1.0, 2.0], [1.0, 0.0],         # circle (1, 2), r = 2
                    [0.0, 0.0], [1.0, 1.0], [2.0, 2.0],                      # collinear
                    [0.3, -1.7], [1.1, 0.4], [-2.2, 0.8]])
    est = _estimators.CircleEstimator()
    assert (est.sample_size, est.nonminimal_sample_size, est.device_minimal, est.model_type, est.cols) == (3, 3, True, _lib.CIRCLE2D, 3)
    assert est.device_slots == 1 and est.radius_range == (0.0, np.inf)
    samples = np.array([[0, 1, 2], [4, 5, 6], [0, 0, 1], [7, 8, 9], [3, 2, 1], [1, 1, 1], [2, 3, 0]])
    models, src = est.minimal(pts, samples)
    assert list(src) == [0, 3, 4, 6]              # collinear (1) and duplicate (2, 5) samples give no model
    for k in (0, 2, 3):
        assert np.array_equal(models[k], [1.0, 2.0, 2.0]), k
    assert models[1].tolist() == _circle_scalar(pts[7:10])                  # bitwise the stated operation order
    r = np.linalg.norm(pts[7:10] - models[1][:2], axis=1) - models[1][2]
    assert np.abs(r).max() < 1e-13
    # the radius range drops the models outside it (bounds inclusive)
    est.radius_range = (2.0, 2.0)
    assert list(est.minimal(pts, samples)[1]) == [0, 4, 6]
    r1 = models[1][2]
    assert abs(r1 - 2.0) > 0.1
    est.radius_range = (min(r1, 2.0) + 0.01, np.inf)
    assert list(est.minimal(pts, samples)[1]) == ([3] if r1 > 2.0 else [0, 4, 6])
    est.radius_range = (0.0, max(r1, 2.0) - 0.01)
    assert list(est.minimal(pts, samples)[1]) == ([0, 4, 6] if r1 > 2.0 else [3])
    est.radius_range = (r1, r1)
    assert list(est.minimal(pts, samples)[1]) == [3]


def _drive_fit(est, pts, w=None):
    """runs the refit on numpy Gram matrices (the device's rows, summed in float64)"""
    models, requests = numpy_refit(est, pts, w)
    for kind, prm, use_w, wpow in requests:
        assert use_w is True and wpow == 1
        assert kind == _lib.GRAM_AFFINE or (kind == _lib.GRAM_CIRCLE and prm.shape == (1, 3))
    return models, [r[0] for r in requests]


@pytest.mark.parametrize("coverage", [1.0, 0.5])
def test_circle_refit_recovers_a_known_circle(coverage):
    pts, labels, gt = datasets.make_circles(n_per_circle=400, n_circles=1, n_outliers=0, sigma=0.0, coverage=coverage, seed=4)
    est = _estimators.CircleEstimator()
    scale = np.abs(gt[0]).max()
    for w in (None, np.random.default_rng(2).uniform(0.5, 2.0, len(pts))):
        for est.refit_solver in ("lapack", "jacobi"):      # (no context: "jacobi" falls back to LAPACK here)
            (m,), kinds = _drive_fit(est, pts, w)
            assert kinds == [_lib.GRAM_AFFINE, _lib.GRAM_CIRCLE]
            assert np.abs(m - gt[0]).max() < 1e-12 * scale, (m, gt[0])
    # far from the origin: the normalisation keeps the refit exact to 1e-12 of the coordinates
    off = np.array([1e6, -2e6])
    for w in (None, np.random.default_rng(3).uniform(0.5, 2.0, len(pts))):
        (m,), _ = _drive_fit(est, pts + off, w)
        assert np.abs(m - np.append(gt[0, :2] + off, gt[0, 2])).max() < 1e-12 * 2e6
    est.radius_range = (0.0, 0.5 * gt[0, 2])
    assert _drive_fit(est, pts)[0] == []          # refit outside the radius range: no model
    est.radius_range = (0.0, np.inf)
    assert _drive_fit(est, pts[:2])[0] == []      # fewer than three points: no model
    assert _drive_fit(est, np.tile(pts[:1], (5, 1)))[0] == []                # zero scatter: no model
    assert _drive_fit(est, pts, np.zeros(len(pts)))[0] == []                 # no weight: no model


def test_make_circles_is_seeded_and_its_inliers_lie_on_their_circles():
    kw = dict(n_per_circle=500, n_circles=4, n_outliers=300, sigma=0.4)
    a = datasets.make_circles(seed=3, **kw)
    b = datasets.make_circles(seed=3, **kw)
    c = datasets.make_circles(seed=4, **kw)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    assert not np.array_equal(a[0], c[0])
    pts, labels, gt = a
    assert pts.shape == (2300, 2) and pts.dtype == np.float64 and labels.shape == (2300,) and labels.dtype == np.int32
    assert gt.shape == (4, 3)
    assert np.bincount(labels).tolist() == [300, 500, 500, 500, 500]
    assert ((gt[:, 2] >= 40.0) & (gt[:, 2] <= 150.0)).all()
    for j in range(4):
        for k in range(j):
            assert np.linalg.norm(gt[j, :2] - gt[k, :2]) > gt[j, 2] + gt[k, 2]        # no two circles overlap
        r = np.linalg.norm(pts[labels == j + 1] - gt[j, :2], axis=1) - gt[j, 2]
        assert np.abs(r).max() < 5 * 0.4 and abs(r.std() - 0.4) < 0.08
        assert ((gt[j, :2] - gt[j, 2] >= 0) & (gt[j, :2] + gt[j, 2] <= 1000.0)).all()  # wholly inside the box
    out = pts[labels == 0]
    assert ((out >= 0) & (out <= 1000.0)).all()
    # coverage: the mean unit direction of a uniform arc of the fraction f of the circumference has length sin(pi f) / (pi f)
    for f in (1.0, 0.5, 0.25):
        pts, labels, gt = datasets.make_circles(n_per_circle=20000, n_circles=2, n_outliers=0, sigma=0.0, coverage=f, seed=5)
        for j in range(2):
            d = (pts[labels == j + 1] - gt[j, :2]) / gt[j, 2]
            assert np.abs(np.linalg.norm(d, axis=1) - 1.0).max() < 1e-12
            assert abs(np.linalg.norm(d.mean(axis=0)) - np.sin(np.pi * f) / (np.pi * f)) < 0.02, f
    with pytest.raises(ValueError, match="coverage"):
        datasets.make_circles(coverage=0.0)
