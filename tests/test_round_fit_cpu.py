"""RoundEstimator._fit_many, which SphereEstimator and CircleEstimator share, with one item (B = 1) against the two single-item refit
bodies it replaced, restated here as they were (generators that yield Gram requests): bitwise the same models on the inputs of test_spheres_cpu.py / test_circles_cpu.py (known spheres and circles, weights,
offsets, radius ranges, too few points, coincident points, no weight), and no RuntimeWarning where the old sphere body gave one."""
import warnings

import numpy as np
import pytest

from primitive_helpers import numpy_refit
from pyprogressivex import _estimators, _lib, datasets


def _old_sphere_fit(est, init):
    G, cnt, _ = yield (_lib.GRAM_AFFINE, None, True, 1)
    W = G[0, 0]
    if cnt < 4 or not W > 0:
        return []
    o = G[0, 1:] / W
    scatter = G[1:, 1:] - W * np.outer(o, o)
    s = np.sqrt(np.trace(scatter) / W)
    if not (np.isfinite(o).all() and s > 0 and np.isfinite(s)):
        return []
    G, _, _ = yield (_lib.GRAM_SPHERE, np.array([o[0], o[1], o[2], s]), True, 1)
    if not np.isfinite(G).all():
        return []
    th = est._smallest(G[None])[0]
    A = th[4]
    if A == 0:
        return []
    b = th[1:4] / (2.0 * A)
    rad = b @ b - th[0] / A
    if not rad > 0:
        return []
    r = s * np.sqrt(rad)
    c = o - s * b
    if not (np.isfinite(c).all() and np.isfinite(r) and est._in_range(r)):
        return []
    return [np.array([c[0], c[1], c[2], r])]


def _old_circle_fit(est, init):
    G, cnt, _ = yield (_lib.GRAM_AFFINE, None, True, 1)
    W = G[0, 0]
    if cnt < 3 or not W > 0:
        return []
    o = G[0, 1:] / W
    scatter = G[1:, 1:] - W * np.outer(o, o)
    with np.errstate(invalid="ignore"):
        s = np.sqrt(np.trace(scatter) / W)
    if not (np.isfinite(o).all() and s > 0 and np.isfinite(s)):
        return []
    G, _, _ = yield (_lib.GRAM_CIRCLE, np.array([o[0], o[1], s]), True, 1)
    if not np.isfinite(G).all():
        return []
    th = est._smallest(G[None])[0]
    A = th[3]
    if A == 0:
        return []
    b = th[1:3] / (2.0 * A)
    rad = b @ b - th[0] / A
    if not rad > 0:
        return []
    r = s * np.sqrt(rad)
    c = o - s * b
    if not (np.isfinite(c).all() and np.isfinite(r) and est._in_range(r)):
        return []
    return [np.array([c[0], c[1], r])]


def _drive(gen, pts, w):
    """runs an old refit body on numpy Gram matrices: the affine rows, then the rows (1, q, |q|^2) summed left to right (what
    primitive_helpers.numpy_refit feeds the shared refit)"""
    req = next(gen)
    try:
        while True:
            kind, prm, _, _ = req
            if kind == _lib.GRAM_AFFINE:
                A = np.column_stack([np.ones(len(pts)), pts])
            else:
                q = (pts - prm[:-1]) / prm[-1]
                sq = q[:, 0] * q[:, 0]
                for k in range(1, q.shape[1]):
                    sq = sq + q[:, k] * q[:, k]
                A = np.column_stack([np.ones(len(pts)), q, sq])
            req = gen.send(((A * w[:, None]).T @ A, len(pts), 0))
    except StopIteration as done:
        return done.value


def _cases(pts, radius, far):
    n, rng = len(pts), np.random.default_rng(2)
    none = (0.0, np.inf)
    yield "plain", pts, np.ones(n), none
    yield "weighted", pts, rng.uniform(0.5, 2.0, n), none
    yield "far from the origin", pts + far, np.ones(n), none
    yield "outside the radius range", pts, np.ones(n), (0.0, 0.5 * radius)
    yield "inside the radius range", pts, np.ones(n), (0.5 * radius, 2.0 * radius)
    yield "too few points", pts[:pts.shape[1]], np.ones(pts.shape[1]), none
    yield "coincident points", np.tile(pts[:1], (5, 1)), np.ones(5), none
    yield "coincident points far away", np.tile(pts[:1] + far, (7, 1)), rng.uniform(0.5, 2.0, 7), none
    yield "no weight", pts, np.zeros(n), none
    yield "a NaN coordinate", np.vstack([pts[:50], np.full((1, pts.shape[1]), np.nan)]), np.ones(51), none


@pytest.mark.parametrize("coverage", [1.0, 0.5])
@pytest.mark.parametrize("kind", ["sphere", "circle"])
def test_shared_round_refit_is_bitwise_the_two_old_bodies(kind, coverage):
    if kind == "sphere":
        pts, _, gt = datasets.make_spheres(n_per_sphere=400, n_spheres=1, n_outliers=0, sigma=0.0, coverage=coverage, seed=4)
        cls, old, far = _estimators.SphereEstimator, _old_sphere_fit, np.array([1e4, -2e4, 5e3])
    else:
        pts, _, gt = datasets.make_circles(n_per_circle=400, n_circles=1, n_outliers=0, sigma=0.0, coverage=coverage, seed=4)
        cls, old, far = _estimators.CircleEstimator, _old_circle_fit, np.array([1e6, -2e6])
    found = set()
    for name, p, w, rr in _cases(pts, gt[0, -1], far):
        est = cls()
        est.radius_range = rr
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")                  # (the old sphere body warns on a negative variance)
            want = _drive(old(est, None), p, w)
        with warnings.catch_warnings():
            warnings.simplefilter("error")                   # the shared one must not
            got, _ = numpy_refit(est, p, w)
        assert len(got) == len(want), name
        for a, b in zip(got, want):
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (name, a, b)
        if got:
            found.add(name)
    assert found >= {"plain", "weighted", "far from the origin", "inside the radius range"}
    assert not found & {"outside the radius range", "too few points", "coincident points", "no weight", "a NaN coordinate"}
