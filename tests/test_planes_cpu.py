"""findPlanes without a GPU: the ABI entry of the plane type, the public call's signature and input checks, the 3-point
solver and the refit of PlaneEstimator against hand-made data, and the make_planes generator."""
import ctypes
import inspect

import numpy as np
import pytest

import pyprogressivex as px
from primitive_helpers import numpy_refit
from pyprogressivex import _estimators, _lib, datasets


def test_model_dims_of_the_plane_type():
    lib = _lib.load()
    d, p = ctypes.c_int(), ctypes.c_int()
    assert lib.pgx_model_dims(6, ctypes.byref(d), ctypes.byref(p)) == 0
    assert (d.value, p.value) == (3, 4)
    assert _lib.PLANE3D == 6 and _lib.POINT_DIM[6] == 3 and _lib.PARAM_DIM[6] == 4
    assert lib.pgx_model_dims(7, None, None) != 0


def test_find_planes_is_exported_with_its_defaults():
    assert "findPlanes" in px.__all__ and callable(px.findPlanes)
    sig = inspect.signature(px.findPlanes)
    positional = [k for k, v in sig.parameters.items() if v.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD]
    assert positional == ["points", "weights", "threshold", "conf", "spatial_coherence_weight", "neighborhood_ball_radius",
                          "maximum_tanimoto_similarity", "max_iters", "minimum_point_number", "maximum_model_number",
                          "sampler_id", "scoring_exponent", "do_logging"]
    defaults = {k: v.default for k, v in sig.parameters.items()}
    assert defaults["weights"] is None and defaults["threshold"] == 0.05 and defaults["conf"] == 0.5
    assert defaults["spatial_coherence_weight"] == 0.0 and defaults["neighborhood_ball_radius"] == 0.5
    assert defaults["maximum_tanimoto_similarity"] == 0.4 and defaults["max_iters"] == 1000
    assert defaults["minimum_point_number"] == 10 and defaults["maximum_model_number"] == -1
    assert defaults["sampler_id"] == 2 and defaults["scoring_exponent"] == 2 and defaults["do_logging"] is False
    # the keyword-only extensions of findLines, with the same defaults
    lines = inspect.signature(px.findLines).parameters
    kw = {k: v.default for k, v in sig.parameters.items() if v.kind is inspect.Parameter.KEYWORD_ONLY}
    assert kw == {k: v.default for k, v in lines.items() if v.kind is inspect.Parameter.KEYWORD_ONLY}


@pytest.mark.parametrize("points", [np.zeros((10, 2)), np.zeros((10, 4)), np.zeros(30), np.zeros((2, 3)), np.zeros((0, 3)),
                                    np.zeros((4, 3, 1))])
def test_find_planes_rejects_bad_points(points):
    with pytest.raises(ValueError, match=r"points should be an array with dims \[n,3\], n>=3"):
        px.findPlanes(points)


def test_find_planes_rejects_weights_of_the_wrong_length():
    with pytest.raises(ValueError, match="weights"):
        px.findPlanes(np.zeros((10, 3)), np.ones(9))


def test_find_planes_unknown_sampler_prints_and_returns_no_model(capsys):
    pts, _, _ = datasets.make_planes(n_per_plane=50, n_planes=2, n_outliers=20, seed=1)
    planes, labels = px.findPlanes(pts, sampler_id=7)
    assert planes.shape == (0, 4) and planes.dtype == np.float64
    assert labels.shape == (pts.shape[0],) and labels.dtype == np.int32 and not labels.any()
    assert "Unknown sampler identifier: 7" in capsys.readouterr().err


def _plane_scalar(p0, p1, p2):
    """the solver's operation order on Python floats (IEEE doubles, no contraction)"""
    u = [p1[k] - p0[k] for k in range(3)]
    v = [p2[k] - p0[k] for k in range(3)]
    n = [u[1] * v[2] - u[2] * v[1], -(u[0] * v[2] - u[2] * v[0]), u[0] * v[1] - u[1] * v[0]]
    ln = ((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]) ** 0.5
    a, b, c = n[0] / ln, n[1] / ln, n[2] / ln
    return [a, b, c, -((a * p0[0] + b * p0[1]) + c * p0[2])]


def test_plane_minimal_solver_on_hand_made_samples():
    pts = np.array([[0.0, 0.0, 1.0], [1.0, 0.0, 1.0], [0.0, 1.0, 1.0],       # z = 1
                    [2.0, 2.0, 1.0], [3.0, 3.0, 1.0],                          # collinear with point 0 in x = y
                    [0.3, -1.7, 2.9], [1.1, 0.4, -0.6], [-2.2, 0.8, 1.3]])
    est = _estimators.PlaneEstimator()
    assert (est.sample_size, est.nonminimal_sample_size, est.device_minimal, est.model_type) == (3, 3, True, _lib.PLANE3D)
    samples = np.array([[0, 1, 2], [0, 3, 4], [0, 0, 1], [1, 1, 1], [5, 6, 7], [2, 1, 0]])
    models, src = est.minimal(pts, samples)
    assert list(src) == [0, 4, 5]                 # collinear (1), duplicate (2, 3) samples give no model
    assert np.array_equal(models[0], [0.0, 0.0, 1.0, -1.0])
    assert np.array_equal(models[2], [0.0, 0.0, -1.0, 1.0])
    assert models[1].tolist() == _plane_scalar(pts[5], pts[6], pts[7])   # bitwise the stated operation order
    r = ((models[1][0] * pts[5:, 0] + models[1][1] * pts[5:, 1]) + models[1][2] * pts[5:, 2]) + models[1][3]
    assert np.abs(r).max() < 1e-14 and abs(np.linalg.norm(models[1][:3]) - 1.0) < 1e-15


def _drive_fit(est, pts, w=None):
    models, requests = numpy_refit(est, pts, w)
    assert len(requests) == 1, "the refit asked for a second Gram matrix"
    assert requests[0][0] == _lib.GRAM_AFFINE and requests[0][2] is True
    w = np.ones(len(pts)) if w is None else w
    A = np.column_stack([np.ones(len(pts)), pts])
    return models, (A * w[:, None]).T @ A


def test_plane_refit_recovers_a_known_plane():
    rng = np.random.default_rng(4)
    nrm = np.array([0.36, -0.48, 0.8])
    e1 = np.cross(nrm, [1.0, 0.0, 0.0]); e1 /= np.linalg.norm(e1)
    e2 = np.cross(nrm, e1)
    st = rng.uniform(-3, 3, (200, 2))
    pts = np.array([1.0, 2.0, -0.5]) + st[:, :1] * e1 + st[:, 1:] * e2
    d = -nrm @ np.array([1.0, 2.0, -0.5])
    est = _estimators.PlaneEstimator()
    for w in (None, rng.uniform(0.5, 2.0, 200)):
        (m,), G = _drive_fit(est, pts, w)
        m = m * np.sign(m[2])
        assert np.abs(m - np.append(nrm, d)).max() < 1e-12
        many = est._fit_many(lambda kind, prm, use_w, wpow, rows: (np.repeat(G[None], len(rows), 0), np.full(len(rows), 200), None),
                             2, [None, None])
        assert all(np.array_equal(o[0], m * np.sign(m[2]) * np.sign(o[0][2])) for o in many)
    assert _drive_fit(est, pts[:2])[0] == []      # fewer than three points: no model


def test_make_planes_is_seeded_and_its_inliers_lie_on_their_planes():
    a = datasets.make_planes(n_per_plane=500, n_planes=4, n_outliers=300, sigma=0.02, seed=3)
    b = datasets.make_planes(n_per_plane=500, n_planes=4, n_outliers=300, sigma=0.02, seed=3)
    c = datasets.make_planes(n_per_plane=500, n_planes=4, n_outliers=300, sigma=0.02, seed=4)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    assert not np.array_equal(a[0], c[0])
    pts, labels, gt = a
    assert pts.shape == (2300, 3) and labels.shape == (2300,) and gt.shape == (4, 4)
    assert np.bincount(labels).tolist() == [300, 500, 500, 500, 500]
    assert np.allclose(np.linalg.norm(gt[:, :3], axis=1), 1.0, atol=1e-15)
    for k in range(4):
        r = pts[labels == k + 1] @ gt[k, :3] + gt[k, 3]
        assert np.abs(r).max() < 6 * 0.02 and abs(r.std() - 0.02) < 0.004
    assert ((pts[labels == 0] >= 0) & (pts[labels == 0] <= 10.0)).all()
