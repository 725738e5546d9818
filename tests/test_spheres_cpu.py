"""findSpheres without a GPU: the ABI entries of the sphere type, the public call's signature and input checks, the 4-point
solver and the algebraic refit of SphereEstimator against hand-made data, and the make_spheres generator."""
import ctypes
import inspect

import numpy as np
import pytest

import pyprogressivex as px
from primitive_helpers import numpy_refit
from pyprogressivex import _estimators, _lib, datasets


def test_model_dims_of_the_sphere_type():
    lib = _lib.load()
    d, p = ctypes.c_int(), ctypes.c_int()
    assert lib.pgx_model_dims(8, ctypes.byref(d), ctypes.byref(p)) == 0
    assert (d.value, p.value) == (3, 4)
    assert _lib.SPHERE3D == 8 and _lib.POINT_DIM[8] == 3 and _lib.PARAM_DIM[8] == 4
    assert _lib.GRAM_SPHERE == 5 and _lib.GRAM_Q[_lib.GRAM_SPHERE] == 5
    assert lib.pgx_model_dims(7, None, None) != 0 and 7 not in _lib.POINT_DIM      # unassigned
    assert lib.pgx_model_dims(9, None, None) != 0
    assert "pgx_set_radius_range" in _lib.ABI_SYMBOLS and hasattr(lib, "pgx_set_radius_range")


def test_find_spheres_is_exported_with_its_defaults():
    assert "findSpheres" in px.__all__ and callable(px.findSpheres)
    sig = inspect.signature(px.findSpheres)
    planes = inspect.signature(px.findPlanes).parameters
    positional = [k for k, v in sig.parameters.items() if v.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD]
    assert positional == [k for k, v in planes.items() if v.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD]
    defaults = {k: v.default for k, v in sig.parameters.items()}
    for k in positional:
        if k != "sampler_id":
            assert defaults[k] == planes[k].default, k
    assert defaults["sampler_id"] == 3 and defaults["threshold"] == 0.05 and defaults["weights"] is None
    kw = {k: v.default for k, v in sig.parameters.items() if v.kind is inspect.Parameter.KEYWORD_ONLY}
    assert kw.pop("radius_range") is None
    assert kw == {k: v.default for k, v in planes.items() if v.kind is inspect.Parameter.KEYWORD_ONLY}


@pytest.mark.parametrize("points", [np.zeros((10, 2)), np.zeros((10, 4)), np.zeros(30), np.zeros((3, 3)), np.zeros((0, 3)),
                                    np.zeros((4, 3, 1))])
def test_find_spheres_rejects_bad_points(points):
    with pytest.raises(ValueError, match=r"points should be an array with dims \[n,3\], n>=4"):
        px.findSpheres(points)


def test_find_spheres_rejects_weights_of_the_wrong_length():
    with pytest.raises(ValueError, match="weights"):
        px.findSpheres(np.zeros((10, 3)), np.ones(9))


@pytest.mark.parametrize("rr", [(np.nan, 1.0), (0.0, np.nan), (-0.1, 1.0), (2.0, 1.0), (1.0,), "ab", 3.0])
def test_find_spheres_rejects_bad_radius_ranges(rr):
    with pytest.raises(ValueError, match="radius_range"):
        px.findSpheres(np.zeros((10, 3)), radius_range=rr)


def test_find_spheres_unknown_sampler_prints_and_returns_no_model(capsys):
    pts, _, _ = datasets.make_spheres(n_per_sphere=50, n_spheres=2, n_outliers=20, seed=1)
    spheres, labels = px.findSpheres(pts, sampler_id=7, radius_range=(0.1, 5.0))
    assert spheres.shape == (0, 4) and spheres.dtype == np.float64
    assert labels.shape == (pts.shape[0],) and labels.dtype == np.int32 and not labels.any()
    assert "Unknown sampler identifier: 7" in capsys.readouterr().err


def _sphere_scalar(p):
    """the solver's operation order on Python floats (IEEE doubles, no contraction)"""
    a = [[p[i][k] - p[0][k] for k in range(3)] for i in (1, 2, 3)]
    h = [0.5 * ((ai[0] * ai[0] + ai[1] * ai[1]) + ai[2] * ai[2]) for ai in a]

    def cross(u, v):
        return [u[1] * v[2] - u[2] * v[1], -(u[0] * v[2] - u[2] * v[0]), u[0] * v[1] - u[1] * v[0]]
    n1, n2, n3 = cross(a[1], a[2]), cross(a[2], a[0]), cross(a[0], a[1])
    det = (a[0][0] * n1[0] + a[0][1] * n1[1]) + a[0][2] * n1[2]
    e = [((h[0] * n1[k] + h[1] * n2[k]) + h[2] * n3[k]) / det for k in range(3)]
    r = ((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]) ** 0.5
    return [p[0][0] + e[0], p[0][1] + e[1], p[0][2] + e[2], r]


def test_sphere_minimal_solver_on_hand_made_samples():
    pts = np.array([[3.0, 2.0, 1.0], [1.0, 4.0, 1.0], [1.0, 2.0, 3.0], [-1.0, 2.0, 1.0],     # sphere (1, 2, 1), r = 2
                    [0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [1.0, 1.0, 0.0],      # coplanar (z = 0)
                    [0.3, -1.7, 2.9], [1.1, 0.4, -0.6], [-2.2, 0.8, 1.3], [0.7, 0.9, -1.9]])
    est = _estimators.SphereEstimator()
    assert (est.sample_size, est.nonminimal_sample_size, est.device_minimal, est.model_type, est.cols) == (4, 4, True, _lib.SPHERE3D, 4)
    samples = np.array([[0, 1, 2, 3], [4, 5, 6, 7], [0, 0, 1, 2], [8, 9, 10, 11], [3, 2, 1, 0], [1, 1, 1, 1]])
    models, src = est.minimal(pts, samples)
    assert list(src) == [0, 3, 4]                 # coplanar (1) and duplicate (2, 5) samples give no model
    assert np.array_equal(models[0], [1.0, 2.0, 1.0, 2.0]) and np.array_equal(models[2], [1.0, 2.0, 1.0, 2.0])
    assert models[1].tolist() == _sphere_scalar(pts[8:12])                # bitwise the stated operation order
    r = np.linalg.norm(pts[8:12] - models[1][:3], axis=1) - models[1][3]
    assert np.abs(r).max() < 1e-13
    # the radius range drops the models outside it (bounds inclusive)
    est.radius_range = (2.0, 2.0)
    assert list(est.minimal(pts, samples)[1]) == [0, 4]
    r1 = models[1][3]
    assert abs(r1 - 2.0) > 0.1
    est.radius_range = (min(r1, 2.0) + 0.01, np.inf)
    assert list(est.minimal(pts, samples)[1]) == ([3] if r1 > 2.0 else [0, 4])
    est.radius_range = (0.0, max(r1, 2.0) - 0.01)
    assert list(est.minimal(pts, samples)[1]) == ([0, 4] if r1 > 2.0 else [3])


def _drive_fit(est, pts, w=None):
    """runs the refit on numpy Gram matrices (the device's rows, summed in float64)"""
    models, requests = numpy_refit(est, pts, w)
    for kind, prm, use_w, wpow in requests:
        assert use_w is True and wpow == 1
        assert kind == _lib.GRAM_AFFINE or (kind == _lib.GRAM_SPHERE and prm.shape == (1, 4))
    return models, [r[0] for r in requests]


@pytest.mark.parametrize("coverage", [1.0, 0.5])
def test_sphere_refit_recovers_a_known_sphere(coverage):
    pts, labels, gt = datasets.make_spheres(n_per_sphere=400, n_spheres=1, n_outliers=0, sigma=0.0, coverage=coverage, seed=4)
    est = _estimators.SphereEstimator()
    for w in (None, np.random.default_rng(2).uniform(0.5, 2.0, len(pts))):
        for est.refit_solver in ("lapack", "jacobi"):      # (no context: "jacobi" falls back to LAPACK here)
            (m,), kinds = _drive_fit(est, pts, w)
            assert kinds == [_lib.GRAM_AFFINE, _lib.GRAM_SPHERE]
            assert np.abs(m - gt[0]).max() < 1e-9, (m, gt[0])
    # far from the origin: the normalisation keeps the refit exact
    off = np.array([1e4, -2e4, 5e3])
    (m,), _ = _drive_fit(est, pts + off)
    assert np.abs(m - np.append(gt[0, :3] + off, gt[0, 3])).max() < 1e-7
    est.radius_range = (0.0, 0.5 * gt[0, 3])
    assert _drive_fit(est, pts)[0] == []          # refit outside the radius range: no model
    est.radius_range = (0.0, np.inf)
    assert _drive_fit(est, pts[:3])[0] == []      # fewer than four points: no model


def test_make_spheres_is_seeded_and_its_inliers_lie_on_their_spheres():
    a = datasets.make_spheres(n_per_sphere=500, n_spheres=4, n_outliers=300, sigma=0.02, seed=3)
    b = datasets.make_spheres(n_per_sphere=500, n_spheres=4, n_outliers=300, sigma=0.02, seed=3)
    c = datasets.make_spheres(n_per_sphere=500, n_spheres=4, n_outliers=300, sigma=0.02, seed=4)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    assert not np.array_equal(a[0], c[0])
    pts, labels, gt = a
    assert pts.shape == (2300, 3) and labels.shape == (2300,) and gt.shape == (4, 4)
    assert np.bincount(labels).tolist() == [300, 500, 500, 500, 500]
    assert ((gt[:, 3] >= 0.3) & (gt[:, 3] <= 1.5)).all()
    for j in range(4):
        for k in range(j):
            assert np.linalg.norm(gt[j, :3] - gt[k, :3]) > gt[j, 3] + gt[k, 3]        # no two spheres overlap
        r = np.linalg.norm(pts[labels == j + 1] - gt[j, :3], axis=1) - gt[j, 3]
        assert np.abs(r).max() < 6 * 0.02 and abs(r.std() - 0.02) < 0.004
    assert ((pts >= 0) & (pts <= 10.0)).all()
    # coverage: the mean unit direction of a uniform cap of that area fraction f has length 1 - f (0 for the whole sphere)
    for f in (1.0, 0.5, 0.25):
        pts, labels, gt = datasets.make_spheres(n_per_sphere=20000, n_spheres=2, n_outliers=0, sigma=0.0, coverage=f, seed=5)
        for j in range(2):
            d = (pts[labels == j + 1] - gt[j, :3]) / gt[j, 3]
            assert np.abs(np.linalg.norm(d, axis=1) - 1.0).max() < 1e-12
            assert abs(np.linalg.norm(d.mean(axis=0)) - (1.0 - f)) < 0.02, f
