"""findCones without a GPU: the ABI entries of the cone type, the public call's signature and input checks, the residual's restatement
against the oracle's 2-D line, plane and symmetric-homography steps, the 3-point solver of ConeEstimator against a scalar restatement on
hand-made samples, the Gauss-Newton rows against central differences and the refit against Gauss-Newton at 50 digits, the f32 filter's
error budget on a restatement of Filter32<kCone3D> (tests/cone_model.py), the make_cones generator and the end-to-end scene's sample
statistics."""
import ctypes
import inspect

import numpy as np
import pytest

import pyprogressivex as px
from cone_model import (E2E, EPS, MODEL_LITERALS, OPERATION_LINES, REFIT_CASES, chart, e_rows, f_value, gn_reference, gn_rows, group_reject,
                        group_row, header_block, header_literals, morton_order, near_threshold_cases, near_threshold_points, numpy_gram,
                        on_cone, point_row, prep, random_cone, refit_fixture, refit_ratios, reject, rho_h, rho_h_rows, signed_cone,
                        solve_scalar, sq_cone, sq_line3d, sweep_is_crossed)
from line3d_filter_model import SYM_MODEL, sym_points
from pyprogressivex import _estimators, _lib, datasets


def test_model_dims_of_the_cone_type():
    lib = _lib.load()
    d, p = ctypes.c_int(), ctypes.c_int()
    assert lib.pgx_model_dims(16, ctypes.byref(d), ctypes.byref(p)) == 0
    assert (d.value, p.value) == (3, 8) == _lib.MODEL_TABLE[16][:2]
    assert _lib.CONE3D == 16 and _lib.MODEL_TABLE[16] == (3, 8, 3, 1)
    assert _lib.POINT_DIM[16] == 3 and _lib.PARAM_DIM[16] == 8
    for unassigned in (7, 9, 11, 13, 15, 17, -1):
        assert lib.pgx_model_dims(unassigned, None, None) != 0 and unassigned not in _lib.MODEL_TABLE
    assert lib.pgx_model_dims(14, ctypes.byref(d), ctypes.byref(p)) == 0 and (d.value, p.value) == (3, 7)
    assert _lib.GRAM_CONE_GN == 8 and _lib.GRAM_Q[_lib.GRAM_CONE_GN] == 7
    assert _estimators.ESTIMATORS["cone"] is _estimators.ConeEstimator and datasets.MODEL_TYPES["cone"] == 16


def test_find_cones_is_exported_with_its_signature():
    assert "findCones" in px.__all__ and callable(px.findCones)
    sig = inspect.signature(px.findCones)
    cyl = inspect.signature(px.findCylinders).parameters
    positional = [k for k, v in sig.parameters.items() if v.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD]
    assert positional == [k for k, v in cyl.items() if v.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD]
    assert sig.parameters["normals"].default is inspect.Parameter.empty
    assert [sig.parameters[k].default for k in positional[2:]] == [cyl[k].default for k in positional[2:]]
    kw = {k: v.default for k, v in sig.parameters.items() if v.kind is inspect.Parameter.KEYWORD_ONLY}
    want = {("angle_range" if k == "radius_range" else k): ((1.0, 89.0) if k == "radius_range" else v.default)
            for k, v in cyl.items() if v.kind is inspect.Parameter.KEYWORD_ONLY}
    assert kw == want and list(kw) == list(want)
    doc = px.findCones.__doc__
    assert "threshold" in doc and "angle_range" in doc and "unsigned" in doc and "unit length" in doc and "apex" in doc


@pytest.mark.parametrize("points", [np.zeros((10, 2)), np.zeros((10, 4)), np.zeros(30), np.zeros((2, 3)), np.zeros((0, 3))])
def test_find_cones_rejects_bad_points(points):
    normals = np.zeros((points.shape[0], 3))
    with pytest.raises(ValueError, match=r"points should be an array with dims \[n,3\], n>=3"):
        px.findCones(points, normals)


@pytest.mark.parametrize("normals", [np.zeros((10, 2)), np.zeros((9, 3)), np.zeros(30), np.zeros((10, 3, 1)), None])
def test_find_cones_rejects_bad_normals(normals):
    with pytest.raises(ValueError, match=r"normals should be an array with dims \[n,3\]"):
        px.findCones(np.zeros((10, 3)), normals)


def test_find_cones_rejects_bad_weights_and_angle_ranges():
    with pytest.raises(ValueError, match="weights"):
        px.findCones(np.zeros((10, 3)), np.zeros((10, 3)), np.ones(9))
    for bad in ((0.0, 10.0), (-1.0, 10.0), (20.0, 10.0), (np.nan, 10.0), (10.0, 90.0), (10.0, np.nan), 3.0, (1.0, 2.0, 3.0)):
        with pytest.raises(ValueError, match="angle_range"):
            px.findCones(np.zeros((10, 3)), np.zeros((10, 3)), angle_range=bad)


def test_find_cones_unknown_sampler_prints_and_returns_no_model(capsys):
    pts, nrm, _, _ = datasets.make_cones(n_per_cone=50, n_cones=2, n_outliers=20, seed=1)
    cones, labels = px.findCones(pts, nrm, sampler_id=7)
    assert cones.shape == (0, 8) and cones.dtype == np.float64
    assert labels.shape == (pts.shape[0],) and labels.dtype == np.int32 and not labels.any()
    assert "Unknown sampler identifier: 7" in capsys.readouterr().err


def test_the_cone_estimator_puts_its_sine_range_and_normals_on_the_context():
    calls = []

    class Ctx:
        def set_radius_range(self, lo, hi):
            calls.append(("range", lo, hi))

        def set_normals(self, nrm):
            calls.append(("normals", nrm))
    est = _estimators.ConeEstimator()
    assert est.takes_radius_range and est.radius_range == (0.0, 1.0)
    from pyprogressivex import _api
    est.radius_range, est.normals = _api._angle_range((10.0, 30.0)), np.ones((4, 3))
    est.context_setup(Ctx())
    assert calls[0] == ("range", float(np.sin(np.deg2rad(10.0))), float(np.sin(np.deg2rad(30.0))))
    assert calls[1][0] == "normals" and calls[1][1] is est.normals
    assert abs(calls[0][2] - 0.5) < 1e-15


# ---- the residual -------------------------------------------------------------------------------------------------------------------
def test_the_oracle_holds_the_cone_residual_by_transformation(oracle):
    """sq_cone (numpy, written next to the kernel) against three types the oracle has, bit for bit: its 2-D line (type 0) with the model
    (c, -s, 0) on the rows (rho, h) gives the last step |c rho - s h| and its square; its plane (type 6) with the model (d, 0) on the
    rows e = x - a gives h (as h^2 and through residual() as |h|); its symmetric homography (type 5) on the 3-D line's witness rows gives
    q = rho^2.  Scene scales 1, 1e3, 1e6, offsets 0 and 1e6, direction scales 2^-40 .. 2^40, (c, s) scales 2^-8 .. 2^8."""
    rng = np.random.default_rng(23)
    for k in range(36):
        coord, off, e, f = (1.0, 1e3, 1e6)[k % 3], (0.0, 1e6)[k % 2], (-40, 0, 3, 40)[k % 4], (0, -8, 8)[k % 3]
        base, _, _, gt = datasets.make_cones(n_per_cone=1500, n_cones=3, n_outliers=3000, seed=k)
        pts = base * coord + off
        if k % 5:
            t = np.deg2rad(rng.uniform(2, 88))
            m = np.concatenate([rng.uniform(0, 10, 3) * coord + off, rng.normal(size=3) * 2.0 ** e, np.array([np.cos(t), np.sin(t)]) * 2.0 ** f])
        else:
            m = np.concatenate([gt[0, :3] * coord + off, gt[0, 3:6] * 2.0 ** e, gt[0, 6:8] * 2.0 ** f])
        if k % 7 == 3:
            m[6 + k % 2] = -m[6 + k % 2]
        got = sq_cone(pts, m)
        rows = rho_h_rows(pts, m)
        assert np.array_equal(oracle.squared_residuals(0, rows, np.array([m[6], -m[7], 0.0])), got)
        rho, h = rho_h(pts, m)
        plane = np.array([m[3], m[4], m[5], 0.0])
        assert np.array_equal(oracle.squared_residuals(oracle.PLANE3D, e_rows(pts, m), plane), h * h)
        for j in range(0, len(pts), 997):
            assert oracle.residual(oracle.PLANE3D, e_rows(pts, m)[j], plane) == abs(h[j])
            assert oracle.residual(0, rows[j], np.array([m[6], -m[7], 0.0])) == abs(signed_cone(pts[j:j + 1], m)[0])
        assert np.array_equal(oracle.squared_residuals(5, sym_points(pts, m), SYM_MODEL), sq_line3d(pts, m))
        assert np.array_equal(np.sqrt(sq_line3d(pts, m)), rho)
    zero = np.concatenate([m[:3], np.zeros(3), m[6:8]])
    assert (sq_cone(pts, zero) == 0.0).all()                 # d = 0: every residual is 0
    for j in range(8):                                       # a NaN anywhere: every residual is NaN
        bad = m.copy()
        bad[j] = np.nan
        assert np.isnan(sq_cone(pts[:50], bad)).all(), j
    # homogeneous of degree 1 in d and in (c, s): powers of two scale it bit for bit
    unit = np.concatenate([gt[0, :3] * coord + off, gt[0, 3:]])
    for kd, kc in ((2.0 ** 7, 1.0), (1.0, 2.0 ** -5), (2.0 ** -30, 2.0 ** 6)):
        scaled = unit.copy()
        scaled[3:6] *= kd
        scaled[6:8] *= kc
        assert np.array_equal(sq_cone(pts, scaled), sq_cone(pts, unit) * (kd * kc) ** 2)


def test_what_the_cone_residual_measures():
    """on the nappe's side of the apex the residual is the distance to the surface; behind the apex (h c + rho s < 0) it is smaller
    than the distance to the apex, the nearest point of the surface"""
    rng = np.random.default_rng(2)
    cone = random_cone(rng, 1.0, 0.0, 25.0)
    a, d, c, s = cone[:3], cone[3:6], cone[6], cone[7]
    surf, nrm = on_cone(rng, cone, 400, 0.5, 4.0)
    t = rng.uniform(-0.2, 0.2, 400)
    assert np.abs(np.sqrt(sq_cone(surf + t[:, None] * nrm, cone)) - np.abs(t)).max() < 1e-14
    assert np.abs(np.linalg.norm(nrm, axis=1) - 1.0).max() < 1e-15
    behind = a - rng.uniform(0.1, 2.0, 100)[:, None] * d + rng.normal(0, 0.01, (100, 3))
    rho, h = rho_h(behind, cone)
    assert (h * c + rho * s < 0).all()
    assert (np.sqrt(sq_cone(behind, cone)) < np.linalg.norm(behind - a, axis=1)).all()


# ---- the 3-point solver -------------------------------------------------------------------------------------------------------------
def _hand_made():
    """the cone about z with its apex at the origin and half-angle 45 degrees: points (cos t, sin t, 1) h, normals (cos t, sin t, -1)"""
    r2 = np.sqrt(0.5)
    pts = np.array([[1.0, 0.0, 1.0], [0.0, 2.0, 2.0], [-3.0, 0.0, 3.0],     # 0, 1, 2: on the cone
                    [2.0, 0.0, 2.0],                                         # 3: on 0's generatrix (the same tangent plane)
                    [0.0, 0.0, 0.0],                                         # 4: the apex itself, with a normal of its own
                    [0.5, 0.5, 0.5],                                         # 5: a zero normal
                    [np.nan, 0.0, 1.0], [0.0, np.inf, 1.0],                  # 6, 7
                    [0.0, -1.0, 1.0],                                        # 8: on the cone
                    [1.0, 0.0, -1.0], [0.0, 2.0, -2.0], [-3.0, 0.0, -3.0],   # 9, 10, 11: the other nappe (d comes out as -z)
                    [1e150, 0.0, 1e150], [0.0, 1e150, 1e150], [-1e150, 0.0, 1e150]])  # 12 .. 14: 1e150 coordinates, unit normals
    nrm = np.array([[1.0, 0.0, -1.0], [0.0, 1.0, -1.0], [-1.0, 0.0, -1.0], [1.0, 0.0, -1.0], [0.0, 1.0, 0.0], [0.0, 0.0, 0.0],
                    [1.0, 0.0, -1.0], [0.0, 1.0, -1.0], [0.0, -1.0, -1.0],
                    [1.0, 0.0, 1.0], [0.0, 1.0, 1.0], [-1.0, 0.0, 1.0],
                    [r2, 0.0, -r2], [0.0, r2, -r2], [-r2, 0.0, -r2]])
    return pts, nrm


def test_cone_minimal_solver_on_hand_made_samples():
    rng = np.random.default_rng(5)
    hand, hn = _hand_made()
    cone = np.concatenate([[2.0, -1.0, 0.5, 0.6, 0.0, 0.8], [np.cos(0.5), np.sin(0.5)]])
    on, outward = on_cone(rng, cone, 60)
    pts, nrm = np.vstack([hand, on]), np.vstack([hn, outward])
    est = _estimators.ConeEstimator()
    est.normals = nrm
    assert (est.sample_size, est.device_minimal, est.model_type, est.cols, est.device_slots) == (3, True, _lib.CONE3D, 8, 1)
    assert est.nonminimal_sample_size == 6
    special = [[0, 1, 2], [0, 3, 1], [0, 1, 4], [0, 5, 1], [5, 0, 1], [0, 0, 1], [6, 1, 2], [0, 7, 2], [0, 1, 6], [1, 2, 8], [9, 10, 11],
               [2, 0, 1], [12, 13, 14], [0, 2, 8]]
    samples = np.vstack([special, rng.integers(len(hand), len(pts), (200, 3))])
    models, src = est.minimal(pts, samples)
    want = [solve_scalar(pts[s], nrm[s]) for s in samples]
    assert list(src) == [k for k, m in enumerate(want) if m is not None]
    # two samples on one generatrix (one tangent plane: det = 0), a sample at the apex, a zero normal (either place), the same index
    # twice, NaN (either place), Inf
    assert not {1, 2, 3, 4, 5, 6, 7, 8} & set(src.tolist())
    assert {0, 9, 10, 11, 12, 13} <= set(src.tolist())
    for m, k in zip(models, src):
        assert np.array_equal(m, want[k]), k                 # bitwise the stated operation order
    r2 = np.sqrt(0.5)
    for k in (0, 9, 11, 13):
        m = models[list(src).index(k)]
        assert m[:3].tolist() == [0.0, 0.0, 0.0] and np.abs(m[3:6] - [0.0, 0.0, 1.0]).max() <= EPS and np.abs(m[6:8] - r2).max() <= EPS, (k, m)
    m10 = models[list(src).index(10)]                        # the other nappe: the axis points the other way, the angle is the same
    assert m10[:3].tolist() == [0.0, 0.0, 0.0] and np.abs(m10[3:6] - [0.0, 0.0, -1.0]).max() <= EPS and abs(m10[6] - r2) <= EPS
    m12 = models[list(src).index(12)]                        # 1e150 coordinates with unit normals: nothing overflows
    assert np.abs(m12[:3]).max() <= 1e150 * 8 * EPS and np.abs(m12[3:6] - [0.0, 0.0, 1.0]).max() <= 2 * EPS and abs(m12[7] - r2) <= 2 * EPS
    gen = src >= len(special)
    assert gen.sum() > 150
    assert np.abs(np.linalg.norm(models[:, 3:6], axis=1) - 1.0).max() <= 4 * EPS
    assert np.abs(np.linalg.norm(models[:, 6:8], axis=1) - 1.0).max() <= 4 * EPS and (models[:, 6] > 0).all() and (models[:, 7] >= 0).all()
    # the sine range (the context's radius range)
    s45 = float(models[0][7])
    est.radius_range = (0.6, 0.8)
    models_r, src_r = est.minimal(pts, samples)
    assert 0 in src_r and not (src_r >= len(special)).any() and (models_r[:, 7] >= 0.6).all() and (models_r[:, 7] <= 0.8).all()
    assert solve_scalar(pts[[0, 1, 2]], nrm[[0, 1, 2]], s45, s45) is not None          # inclusive at both ends
    assert solve_scalar(pts[[0, 1, 2]], nrm[[0, 1, 2]], np.nextafter(s45, 1.0), 1.0) is None
    assert solve_scalar(pts[[0, 1, 2]], nrm[[0, 1, 2]], 0.0, np.nextafter(s45, 0.0)) is None


def test_cone_minimal_solver_refuses_a_half_angle_of_ninety_degrees_or_more():
    """three points of a plane with the plane's normal tilted a little at each: the tangent planes meet, but the 'cone' is flat or
    opens backwards (c <= 0 is refused; c > 0 always holds after the flip unless the three g_i are orthogonal to d)"""
    p = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [-1.0, -1.0, 0.0]])
    n = np.array([[0.0, 0.0, 1.0], [0.0, 0.0, 1.0], [0.0, 0.0, 1.0]])
    assert solve_scalar(p, n) is None                        # parallel planes: det = 0
    # the apex in the points' plane: every g_i is orthogonal to d = z, c = 0 exactly
    n2 = np.array([[0.0, 1.0, 0.0], [1.0, 0.0, 0.0], [1.0, -1.0, 1.0]])
    assert solve_scalar(p, n2) is None
    # ... and it is the test c > 0 alone that refuses it, in the estimator as in the restatement: everything before it goes through
    # (det = -1, the apex at the origin, |D| > 0, every entry finite, s = 1 inside the range), and a point lifted off the plane gives a
    # cone of just under 90 degrees that is accepted
    est = _estimators.ConeEstimator()
    est.normals = np.vstack([n2, [[1.0, -1.0, 1.0]]])
    est.radius_range = (0.0, np.inf)
    pts = np.vstack([p, [[-1.0, -1.0, 2.0 ** -20]]])         # lies in the plane x - y + z = 2^-20: the apex moves to (0, 0, 2^-20)
    orders = np.array([[0, 1, 2], [2, 0, 1], [1, 2, 0], [0, 1, 3]])
    models, src = est.minimal(pts, orders)
    assert src.tolist() == [3] and 0 < models[0][6] < 1e-5 and abs(models[0][7] - 1.0) < 1e-10
    steep = solve_scalar(pts[[0, 1, 3]], est.normals[[0, 1, 3]])
    assert np.array_equal(models[0], steep)


def test_cone_minimal_solver_recovers_the_planted_cone_and_ignores_the_normals_sign_and_length():
    rng = np.random.default_rng(9)
    for angle in (5.0, 20.0, 45.0, 70.0):
        cone = random_cone(rng, 1.0, 0.0, angle)
        pts, outward = on_cone(rng, cone, 80)
        samples = rng.integers(0, 80, (100, 3))
        est = _estimators.ConeEstimator()
        est.normals = outward
        base, src = est.minimal(pts, samples)
        est.normals = outward * (rng.choice([-1.0, 1.0], 80) * 10.0 ** rng.uniform(-3, 3, 80))[:, None]
        other, src2 = est.minimal(pts, samples)
        assert np.array_equal(src, src2) and len(src) > 80
        n = outward[samples[src]]
        g = pts[samples[src]] - cone[:3]
        g /= np.linalg.norm(g, axis=2)[:, :, None]
        # Cramer's rule loses a factor |b| / |det| on the apex (unit normals: |b| <= |p|), the axis another 1 / |D|: the tolerance is
        # 64 eps max |p| / (|det| |D|) per sample, and samples whose tolerance exceeds 1e-6 are not looked at
        det = np.abs(np.linalg.det(n))
        D = np.linalg.norm(np.cross(g[:, 1] - g[:, 0], g[:, 2] - g[:, 0]), axis=1)
        with np.errstate(divide="ignore"):
            tol = 64 * EPS * np.abs(pts).max() / (det * D)
        well = tol < 1e-6
        assert well.sum() > 20, (angle, well.sum())
        for got in (base, other):                            # the planted cone, its axis pointing into the nappe
            assert (np.abs(got[well] - cone).max(axis=1) <= tol[well]).all(), (angle, (np.abs(got[well] - cone).max(axis=1) / tol[well]).max())


# ---- the Gauss-Newton rows and the refit ----------------------------------------------------------------------------------------------
def test_cone_gn_rows_are_the_jacobian_and_the_residual():
    for trial in range(6):
        pts, w, gt, start = refit_fixture(64, (0.0, 1e3)[trial % 2], False, seed=trial)
        u, v = chart(start)
        rows, bad = gn_rows(pts, np.concatenate([start, u]))
        assert not bad.any()
        assert np.array_equal(rows[:, 6], signed_cone(pts, start))           # the last entry is the residual before its fabs, bit for bit
        assert np.array_equal(rows[:, 6] * rows[:, 6], sq_cone(pts, start))
        h = 1e-6
        for k in range(6):
            x = np.zeros(6)
            x[k] = h
            fd = (f_value(pts, start, u, v, x) - f_value(pts, start, u, v, -x)) / (2 * h)
            assert np.abs(fd - rows[:, k]).max() < 2e-6 * max(1.0, np.abs(rows[:, k]).max()), (trial, k)
            assert np.abs(rows[:, k]).max() > 1e-3                       # (a column of zeros would pass any sign)
    on_axis = np.vstack([pts, start[:3], [np.nan, 0.0, 0.0]])    # e = 0 exactly: rho == 0
    assert gn_rows(on_axis, np.concatenate([start, u]))[1].tolist() == [False] * 64 + [True, True]


def _refit(pts, w, start, **kw):
    est = _estimators.ConeEstimator()
    log = []
    (models,) = est._fit_many(numpy_gram(pts, w, log=log, **kw), 1, [start])
    return models, log


def test_cone_refit_requests_and_failures():
    pts, w, gt, start = refit_fixture(64, 0.0, True, seed=3)
    models, log = _refit(pts, w, start)
    assert len(models) == 1 and models[0].shape == (8,)
    assert 2 <= len(log) <= 10 and all(r[0] == _lib.GRAM_CONE_GN and r[2] is True and r[3] == 1 and r[1].shape == (1, 11) for r in log)
    for r in log:                                            # the chart handed over: d unit, (c, s) unit, u unit and orthogonal to d
        d, cs, u = r[1][0, 3:6], r[1][0, 6:8], r[1][0, 8:11]
        assert abs(np.linalg.norm(d) - 1) < 4 * EPS and abs(np.linalg.norm(u) - 1) < 4 * EPS and abs(d @ u) < 4 * EPS
        assert abs(np.linalg.norm(cs) - 1) < 4 * EPS
    m = models[0]
    assert abs(np.linalg.norm(m[3:6]) - 1.0) <= 4 * EPS and abs(np.linalg.norm(m[6:8]) - 1.0) <= 4 * EPS and m[6] > 0 and m[7] > 0
    assert ((pts - m[:3]) @ m[3:6] > 0).all()                # d points into the nappe
    assert np.abs(m - gt).max() < 0.05
    # a start on the other sheet of the parametrisation comes back canonical: (-d, -c, s) and (d, -c, -s) describe the same residuals
    for flip in ([3, 4, 5, 6], [6, 7]):
        other = start.copy()
        other[flip] = -other[flip]
        (mo,), _ = _refit(pts, w, other)
        assert np.abs(mo - m).max() < 1e-9, flip
    canon = _estimators.ConeEstimator.canonical(np.array([[1, 2, 3, 0, 0, 1, -0.6, 0.8], [1, 2, 3, 0, 0, 1, 0.6, -0.8], [1, 2, 3, 0, 0, 1, -0.6, -0.8]], float))
    assert canon.tolist() == [[1, 2, 3, 0, 0, -1, 0.6, 0.8], [1, 2, 3, 0, 0, -1, 0.6, 0.8], [1, 2, 3, 0, 0, 1, 0.6, 0.8]]
    est = _estimators.ConeEstimator()
    assert est._fit_many(numpy_gram(pts, w), 1, [None]) == [[]]                          # no init
    assert est._fit_many(numpy_gram(pts[:5], w[:5]), 1, [start]) == [[]]                 # fewer than 6 points
    on_axis = np.vstack([pts, start[:3]])                                                # the apex: rho == 0 exactly
    assert est._fit_many(numpy_gram(on_axis), 1, [start]) == [[]]                        # a bad point
    with np.errstate(all="ignore"):
        assert est._fit_many(numpy_gram(np.vstack([pts, [1e200, 0, 0]])), 1, [start]) == [[]]    # non-finite sums
        assert est._fit_many(numpy_gram(pts), 1, [np.full(8, np.nan)]) == [[]]
    est.radius_range = (0.9, 1.0)
    assert est._fit_many(numpy_gram(pts, w), 1, [start]) == [[]]                         # sine outside the range
    # two items equal two single fits, and a failing neighbour does not matter
    pts2, w2, _, start2 = refit_fixture(1000, 1e3, False, seed=4)
    sets = [(pts, w, start), (pts2, w2, start2)]

    def gram(kind, prm, use_w, wpow, rows):
        out = [numpy_gram(sets[r][0], sets[r][1])(kind, None if prm is None else prm[k:k + 1], use_w, wpow, [0]) for k, r in enumerate(rows)]
        return np.concatenate([o[0] for o in out]), np.concatenate([o[1] for o in out]), np.concatenate([o[2] for o in out])
    est = _estimators.ConeEstimator()
    both = est._fit_many(gram, 2, [start, start2])
    assert np.array_equal(both[0][0], m) and np.array_equal(both[1][0], _refit(pts2, w2, start2)[0][0])
    mixed = est._fit_many(gram, 2, [None, start2])
    assert mixed[0] == [] and np.array_equal(mixed[1][0], both[1][0])


@pytest.fixture(scope="module")
def refit_references():
    """the 50-digit answers, computed once for the refit tests of this module"""
    pytest.importorskip("mpmath")
    out = {}
    for n, offset, weighted in REFIT_CASES:
        pts, w, gt, start = refit_fixture(n, offset, weighted, seed=n + int(offset) + weighted)
        out[(n, offset, weighted)] = (pts, w, gt, start, gn_reference(pts, w, start))
    return out


def test_cone_refit_against_gauss_newton_at_50_digits(refit_references):
    """_fit_many on numpy Gram matrices converges to the model plain Gauss-Newton at 50 digits reaches from the same start, within
    32 eps x the condition number of the reference's own 6x6 normal matrix at its solution x the parameter's scale (DESIGN.md 4.5a's
    rule; the scales: cone_model.refit_ratios).  The reference converges on every fixture, none is skipped.  Worst ratios measured
    (apex, direction, angle): printed, and in docs/lab-notebook.md."""
    worst = np.zeros(3)
    for key, (pts, w, gt, start, ref) in refit_references.items():
        assert ref[4], key                                   # the reference alone converged
        assert np.linalg.norm(ref[2] - gt[6:8]) < 0.05 and np.linalg.norm(ref[1] - gt[3:6]) < 0.05, key       # ... to the cone
        models, _ = _refit(pts, w, start)
        assert len(models) == 1, key
        ratios = np.array(refit_ratios(models[0], ref, pts))
        worst = np.maximum(worst, ratios)
        print(key, "cond %.3g" % ref[3], "ratios", ratios.tolist())
        assert (ratios <= 1.0).all(), (key, ratios, ref[3])
    print("worst ratios (apex, direction, angle):", worst.tolist())


def test_cone_refit_with_a_sign_error_in_a_jacobian_column_is_refused(refit_references):
    """the same check with the sign of one column of the rows reversed, each of the six columns in turn (all six are geometric: there is
    no constant column): the iteration no longer reaches the reference (a failed or dropped fit counts as refused)"""
    for col in range(6):
        refused = 0
        for key, (pts, w, gt, start, ref) in refit_references.items():
            if key[0] == 6:
                continue
            models, _ = _refit(pts, w, start, plant_sign=col)
            refused += not models or not (np.array(refit_ratios(models[0], ref, pts)) <= 1.0).all()
        assert refused >= 6, (col, refused)


# ---- the f32 filter's budget: the restatement runs with the literals READ FROM score_filters.hip.h --------------------------------------
def test_cone_filter_model_and_header_state_the_same_filter():
    assert header_literals() == MODEL_LITERALS
    block = " ".join(header_block().split())
    for line in OPERATION_LINES:
        assert " ".join(line.split()) in block, line
    assert "static constexpr int kRowVals = 6, kGroupVals = 5;" in block and "static constexpr int kStagedVals = 12;" in block
    assert "struct Lane { float p[3]; float d[3]; float c, s, e1, e0, e2, tpp, nrm, nanh; };" in block


def _scaled(gt, T, e, f):
    hyp = gt.copy()
    hyp[3:6] *= 2.0 ** e                                     # the residual scales with |d| and with |(c, s)|, and so does the threshold
    hyp[6:8] *= 2.0 ** f
    return hyp, (T * 2.0 ** e * 2.0 ** f) ** 2


def _near_threshold_pairs(plant_zero_budget=False, per_case=70):
    """(pairs in the band, FP64 inliers among them, FP64 inliers the point test rejected) over all 81 cases"""
    lit = header_literals()
    band = inl = wrong = 0
    seen = set()
    for rng, gt, T, e, f, coord in near_threshold_cases():
        seen.add((e, f, int(round(np.degrees(np.arctan2(gt[7], gt[6]))))))
        pts = near_threshold_points(rng, gt, T, per_case, 5.0 * coord)
        base = gt.copy()
        if rng.random() < 0.5:
            base[:3] += rng.normal(0, 1e-6 * T, 3)
        hyp, T2 = _scaled(base, T, e, f)
        sq = sq_cone(pts, hyp)
        ln = prep(hyp, max(1.0, np.abs(pts).max()), T2, plant_zero_budget, lit=lit)
        assert ln["e0"] < np.inf or plant_zero_budget
        for x, s in zip(pts, sq):
            if not abs(s / T2 - 1.0) < 1e-4:
                continue
            band += 1
            if s < T2:
                inl += 1
                wrong += reject(point_row(x), ln)
    assert len(seen) >= 54 and sweep_is_crossed(seen)         # every d scale met every angle and every scale of (c, s)
    return band, inl, wrong


def test_cone_filter_rejects_no_inlier_near_the_threshold():
    pytest.importorskip("mpmath")
    band, inl, wrong = _near_threshold_pairs()
    assert band >= 3000 and inl >= 1200, (band, inl)
    assert wrong == 0


def test_cone_filter_without_its_budget_is_caught():
    """E planted as 0: scenes far from the origin put the f32 rounding of the coordinates above the 2^-6 margin of the threshold, and
    the check above sees inliers rejected"""
    pytest.importorskip("mpmath")
    band, inl, wrong = _near_threshold_pairs(plant_zero_budget=True, per_case=20)
    assert inl > 0 and wrong > 0


def test_cone_group_bound_rejects_no_group_with_a_near_threshold_inlier():
    """the group test on every one of the 81 near-threshold sets themselves, in Morton order: a rejected group holds no exact inlier"""
    pytest.importorskip("mpmath")
    lit = header_literals()
    groups = 0
    rejected = {-40: 0, 0: 0, 40: 0}                         # per scale of d
    seen = set()
    for k, (rng, gt, T, e, f, coord) in enumerate(near_threshold_cases()):
        seen.add((e, f, int(round(np.degrees(np.arctan2(gt[7], gt[6]))))))
        pts = near_threshold_points(rng, gt, T, 128, 5.0 * coord)
        far = pts[64] + (pts[64] - gt[:3]) / np.linalg.norm(pts[64] - gt[:3]) * 30 * max(T, coord)
        pts[64:] = far + rng.uniform(-1, 1, (64, 3)) * T                         # and a compact half well off the surface
        pts = np.ascontiguousarray(pts[morton_order(pts)])
        hyp, T2 = _scaled(gt, T, e, f)
        ln = prep(hyp, max(1.0, np.abs(pts).max()), T2, lit=lit)
        sq = sq_cone(pts, hyp)
        for g0 in range(0, len(pts), 16):
            groups += 1
            if group_reject(group_row(pts[g0:g0 + 16]), ln):
                rejected[e] += 1
                assert not (sq[g0:g0 + 16] < T2).any(), (k, g0)
    assert groups >= 600 and min(rejected.values()) > 0, (groups, rejected)
    assert len(seen) >= 54 and sweep_is_crossed(seen)         # every d scale met every angle and every scale of (c, s)


def test_cone_filter_rejects_generic_pairs_and_switches_off():
    pytest.importorskip("mpmath")
    rng = np.random.default_rng(4)
    pts = rng.uniform(0, 10, (1500, 3))
    T = 1.5 * 0.05
    lit = header_literals()
    rej = tot = 0
    for k in range(3):
        gt = random_cone(rng, 1.0, 0.0, (20.0, 3.0, 80.0)[k])
        hyp, T2 = _scaled(gt, T, (0, -40, 3)[k], (0, 5, -9)[k])
        ln = prep(hyp, 10.0, T2, lit=lit)
        assert ln["e0"] < np.inf
        sq = sq_cone(pts, hyp)
        for x, s in zip(pts[500 * k:500 * (k + 1)], sq[500 * k:500 * (k + 1)]):
            r = reject(point_row(x), ln)
            assert not (r and s < T2)
            rej += r
            tot += 1
    assert rej > 0.8 * tot
    # never rejected: a zero direction (every residual is 0), Inf entries ((c, s) among them), a direction outside the normaliser's band,
    # thresholds outside the f32 range, apexes and coordinates beyond 1e17, |c| + |s| outside [2^-10, 2^10] (zero included)
    gt = random_cone(rng, 1.0, 0.0, 30.0)
    a, d, cs = gt[:3], gt[3:6], gt[6:8]
    for hyp, T2, pscale in ((np.concatenate([a, np.zeros(3), cs]), T * T, 10.0), (np.concatenate([a, [np.inf, 0.0, 0.0], cs]), T * T, 10.0),
                            (np.concatenate([[np.inf, 0.0, 0.0], d, cs]), T * T, 10.0), (np.concatenate([a, d * 1e-80, cs]), T * T, 10.0),
                            (gt, 1e-70, 10.0), (gt, 1e70, 10.0), (np.concatenate([a * 1e18, d, cs]), T * T, 10.0), (gt, T * T, 1e18),
                            (np.concatenate([a, d, [np.inf, cs[1]]]), T * T, 10.0), (np.concatenate([a, d, [cs[0], -np.inf]]), T * T, 10.0),
                            (np.concatenate([a, d, cs * 2.0 ** 11]), T * T, 10.0), (np.concatenate([a, d, cs * 2.0 ** -12]), T * T, 10.0),
                            (np.concatenate([a, d, [0.0, 0.0]]), T * T, 10.0), (np.concatenate([a, d, [1e300, 1e300]]), T * T, 10.0)):
        ln = prep(hyp, pscale, T2, lit=lit)
        assert ln["e0"] == np.inf and ln["nanh"] == 0.0
        assert not any(reject(point_row(x), ln) for x in pts[:20])
        assert not group_reject(group_row(pts[:64]), ln)
    # just inside the band the filter is on
    for f in (-10, 9):
        assert prep(np.concatenate([a, d, cs * 2.0 ** f]), 10.0, T * T, lit=lit)["e0"] < np.inf
    for k in range(8):                                       # a NaN entry: no pair is rejected (the exact path gives NaN), the group is culled
        nan = gt.copy()
        nan[k] = np.nan
        ln = prep(nan, 10.0, T * T, lit=lit)
        assert ln["nanh"] == 1.0 and group_reject(group_row(pts[:64]), ln)
        assert not any(reject(point_row(x), ln) for x in pts[:20])
        assert np.isnan(sq_cone(pts[:20], nan)).all()


# ---- the generator ------------------------------------------------------------------------------------------------------------------
def test_make_cones_is_seeded_and_its_inliers_lie_on_their_cones():
    kw = dict(n_per_cone=2000, n_cones=4, n_outliers=300, sigma=0.02, normal_noise_deg=5.0)
    a = datasets.make_cones(seed=3, **kw)
    b = datasets.make_cones(seed=3, **kw)
    c = datasets.make_cones(seed=4, **kw)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    assert not np.array_equal(a[0], c[0])
    pts, nrm, labels, gt = a
    assert pts.shape == nrm.shape == (8300, 3) and pts.dtype == nrm.dtype == np.float64
    assert labels.shape == (8300,) and labels.dtype == np.int32 and gt.shape == (4, 8) and gt.dtype == np.float64
    assert np.bincount(labels).tolist() == [300, 2000, 2000, 2000, 2000]
    assert np.abs(np.linalg.norm(gt[:, 3:6], axis=1) - 1.0).max() < 1e-15 and np.abs(np.linalg.norm(nrm, axis=1) - 1.0).max() < 1e-14
    assert np.abs(np.linalg.norm(gt[:, 6:8], axis=1) - 1.0).max() < 1e-15
    ang = np.degrees(np.arctan2(gt[:, 7], gt[:, 6]))
    assert ((ang >= 15.0) & (ang <= 40.0)).all()
    for j in range(4):
        on, nn = pts[labels == j + 1], nrm[labels == j + 1]
        f = signed_cone(on, gt[j])
        assert abs(f.std() - 0.02) < 0.1 * 0.02 and abs(f.mean()) < 0.1 * 0.02          # Gaussian along the surface normal
        rho, h = rho_h(on, gt[j])
        t = h * gt[j, 6] + rho * gt[j, 7]                                                # the position along the generatrix
        hh = t * gt[j, 6]
        assert 1.0 - 0.05 <= hh.min() and hh.max() <= 4.0 + 0.05 and hh.min() < 1.2 and hh.max() > 3.9
        assert abs(np.mean(hh ** 2) - 0.5 * (1.0 + 16.0)) < 0.4                          # uniform on the surface: h^2 is uniform
        e = on - gt[j, :3]
        radial = e - h[:, None] * gt[j, 3:6]
        outward = gt[j, 6] * radial / rho[:, None] - gt[j, 7] * gt[j, 3:6]
        cosang = np.abs((nn * outward).sum(axis=1))                                      # the sign is random
        tilt = np.degrees(np.arccos(np.minimum(cosang, 1.0)))
        assert tilt.max() <= 5.0 + 0.5 and tilt.mean() > 1.0                             # (the noise along the normal moves rhohat a little)
        signs = np.sign((nn * outward).sum(axis=1))
        assert 0.4 < (signs > 0).mean() < 0.6
    out = pts[labels == 0]
    assert ((out >= 0) & (out <= 10.0)).all() and ((pts >= -0.1) & (pts <= 10.1)).all()
    exact = datasets.make_cones(n_per_cone=100, n_cones=1, n_outliers=0, sigma=0.0, normal_noise_deg=0.0, seed=1)
    assert np.abs(signed_cone(exact[0], exact[3][0])).max() < 1e-13
    got = solve_scalar(exact[0][[3, 40, 77]], exact[1][[3, 40, 77]])
    assert np.abs(got - exact[3][0]).max() < 1e-9            # exact points with exact normals give the cone back
    d = datasets.make_cones()
    assert d[0].shape == (96000, 3) and d[3].shape == (6, 8) and np.bincount(d[2]).tolist() == [48000] + [8000] * 6
    with pytest.raises(ValueError, match="half_angle_deg"):
        datasets.make_cones(half_angle_deg=(0.0, 40.0))
    with pytest.raises(ValueError, match="fit the box"):
        datasets.make_cones(extent=(1.0, 9.0))
    with pytest.raises(ValueError, match="normals"):
        datasets.make_cones(normals="other")


# ---- the end-to-end scene, fixed here before the device runs it ------------------------------------------------------------------------
def test_the_end_to_end_scene_gives_the_solver_enough_good_samples():
    """test_gpu_cones.py's scene (three cones of 800 points, 800 outliers, half-angles 15 .. 40 degrees, h in [1, 4], sigma 0.01, tilt
    5 degrees, T = 0.05): of the all-inlier samples, the share whose hypothesis collects at least half of its cone's points within T.
    The prototype measured 46 %; at least 30 % are required on every seed, so that the scene is not what fails on the device.  The
    figures measured here: docs/lab-notebook.md."""
    T = 0.05
    for seed in (0, 1, 2):
        pts, nrm, labels, gt = datasets.make_cones(seed=seed, **E2E)
        rng = np.random.default_rng(100 + seed)
        est = _estimators.ConeEstimator()
        est.normals = nrm
        est.radius_range = (float(np.sin(np.deg2rad(1.0))), float(np.sin(np.deg2rad(89.0))))
        good = total = 0
        for j in range(3):
            idx = np.nonzero(labels == j + 1)[0]
            samples = rng.choice(idx, (200, 3))
            samples = samples[(samples[:, 0] != samples[:, 1]) & (samples[:, 1] != samples[:, 2]) & (samples[:, 0] != samples[:, 2])]
            models, src = est.minimal(pts, samples)
            total += len(samples)
            for m in models:
                good += (sq_cone(pts[idx], m) < T * T).sum() >= 0.5 * len(idx)
        share = good / total
        print("seed", seed, "all-inlier samples collecting half of their cone:", round(share, 3))
        assert share >= 0.30, (seed, share)
