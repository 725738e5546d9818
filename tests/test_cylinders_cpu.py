"""findCylinders without a GPU: the ABI entries of the cylinder type, the public call's signature and input checks, the residual's
restatement against the oracle's sphere step, the 2-point solver of CylinderEstimator against a scalar restatement on hand-made
samples, the Gauss-Newton rows against central differences and the refit against Gauss-Newton at 50 digits, the f32 filter's error
budget on a restatement of Filter32<kCylinder3D> (tests/cylinder_model.py), and the make_cylinders generator."""
import ctypes
import inspect

import numpy as np
import pytest

import pyprogressivex as px
from cylinder_model import (EPS, MODEL_LITERALS, OPERATION_LINES, REFIT_CASES, chart, cross_rows, f_value, gn_reference, gn_rows,
                            group_reject, group_row, header_block, header_literals, morton_order, near_threshold_cases,
                            near_threshold_points, numpy_gram, point_row, prep, random_cylinder, refit_fixture, refit_ratios, reject,
                            solve_scalar, sq_cylinder, sq_line3d)
from pyprogressivex import _estimators, _lib, datasets


def test_model_dims_of_the_cylinder_type():
    lib = _lib.load()
    d, p = ctypes.c_int(), ctypes.c_int()
    assert lib.pgx_model_dims(14, ctypes.byref(d), ctypes.byref(p)) == 0
    assert (d.value, p.value) == (3, 7) == _lib.MODEL_TABLE[14][:2]
    assert _lib.CYLINDER3D == 14 and _lib.MODEL_TABLE[14] == (3, 7, 2, 1)
    assert _lib.POINT_DIM[14] == 3 and _lib.PARAM_DIM[14] == 7
    for unassigned in (7, 9, 11, 13, 15, -1):
        assert lib.pgx_model_dims(unassigned, None, None) != 0 and unassigned not in _lib.MODEL_TABLE
    assert lib.pgx_model_dims(12, ctypes.byref(d), ctypes.byref(p)) == 0 and (d.value, p.value) == (3, 6)
    assert hasattr(lib, "pgx_set_normals") and "pgx_set_normals" in _lib.ABI_SYMBOLS
    assert _lib.GRAM_CYL_GN == 7 and _lib.GRAM_Q[_lib.GRAM_CYL_GN] == 6


def test_find_cylinders_is_exported_with_its_signature():
    assert "findCylinders" in px.__all__ and callable(px.findCylinders)
    sig = inspect.signature(px.findCylinders)
    spheres = inspect.signature(px.findSpheres).parameters
    positional = [k for k, v in sig.parameters.items() if v.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD]
    assert positional == ["points", "normals"] + [k for k, v in spheres.items() if v.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD][1:]
    assert sig.parameters["normals"].default is inspect.Parameter.empty
    assert [sig.parameters[k].default for k in positional[2:]] == [spheres[k].default for k in positional[2:]]
    kw = {k: v.default for k, v in sig.parameters.items() if v.kind is inspect.Parameter.KEYWORD_ONLY}
    assert kw == {k: v.default for k, v in spheres.items() if v.kind is inspect.Parameter.KEYWORD_ONLY} and "radius_range" in kw
    assert list(kw) == [k for k, v in spheres.items() if v.kind is inspect.Parameter.KEYWORD_ONLY]
    doc = px.findCylinders.__doc__
    assert "threshold" in doc and "minimum_point_number" in doc and "unsigned" in doc and "unit length" in doc


@pytest.mark.parametrize("points", [np.zeros((10, 2)), np.zeros((10, 4)), np.zeros(30), np.zeros((1, 3)), np.zeros((0, 3))])
def test_find_cylinders_rejects_bad_points(points):
    normals = np.zeros((points.shape[0], 3))
    with pytest.raises(ValueError, match=r"points should be an array with dims \[n,3\], n>=2"):
        px.findCylinders(points, normals)


@pytest.mark.parametrize("normals", [np.zeros((10, 2)), np.zeros((9, 3)), np.zeros(30), np.zeros((10, 3, 1)), None])
def test_find_cylinders_rejects_bad_normals(normals):
    with pytest.raises(ValueError, match=r"normals should be an array with dims \[n,3\]"):
        px.findCylinders(np.zeros((10, 3)), normals)


def test_find_cylinders_rejects_bad_weights_and_radius_ranges():
    with pytest.raises(ValueError, match="weights"):
        px.findCylinders(np.zeros((10, 3)), np.zeros((10, 3)), np.ones(9))
    for bad in ((-1.0, 1.0), (2.0, 1.0), (np.nan, 1.0), 3.0):
        with pytest.raises(ValueError, match="radius_range"):
            px.findCylinders(np.zeros((10, 3)), np.zeros((10, 3)), radius_range=bad)


def test_find_cylinders_unknown_sampler_prints_and_returns_no_model(capsys):
    pts, nrm, _, _ = datasets.make_cylinders(n_per_cylinder=50, n_cylinders=2, n_outliers=20, seed=1)
    cyl, labels = px.findCylinders(pts, nrm, sampler_id=7)
    assert cyl.shape == (0, 7) and cyl.dtype == np.float64
    assert labels.shape == (pts.shape[0],) and labels.dtype == np.int32 and not labels.any()
    assert "Unknown sampler identifier: 7" in capsys.readouterr().err


def test_the_setup_hook_is_the_estimators():
    """what _find_primitive puts on the context comes from the estimator: the round family its radius range, the cylinder that and its
    normals, the others nothing"""
    calls = []

    class Ctx:
        def set_radius_range(self, lo, hi):
            calls.append(("range", lo, hi))

        def set_normals(self, nrm):
            calls.append(("normals", nrm))
    est = _estimators.CylinderEstimator()
    est.radius_range, est.normals = (0.25, 2.0), np.ones((4, 3))
    est.context_setup(Ctx())
    assert calls[0] == ("range", 0.25, 2.0) and calls[1][0] == "normals" and calls[1][1] is est.normals
    calls.clear()
    sph = _estimators.SphereEstimator()
    sph.radius_range = (1.0, 3.0)
    sph.context_setup(Ctx())
    _estimators.PlaneEstimator().context_setup(Ctx())
    assert calls == [("range", 1.0, 3.0)]
    assert [e.takes_radius_range for e in (est, sph, _estimators.CircleEstimator(), _estimators.PlaneEstimator(),
                                           _estimators.Line3DEstimator())] == [True, True, True, False, False]


# ---- the residual -------------------------------------------------------------------------------------------------------------------
def test_the_oracle_holds_the_cylinder_residuals_last_step(oracle):
    """sq_cylinder (numpy, written next to the kernel) equals the oracle's sphere residual with the model (0, 0, 0, r) on the rows
    C = e x d, bit for bit: scene scales 1, 1e3, 1e6, offsets 0 and 1e6, direction scales 2^-40 .. 2^40 (the first step, C and its sum
    of squares, is sq_line3d's, which test_lines3d_cpu.py holds to the oracle)"""
    rng = np.random.default_rng(19)
    for k in range(36):
        coord, off, e = (1.0, 1e3, 1e6)[k % 3], (0.0, 1e6)[k % 2], (-40, 0, 3, 40)[k % 4]
        base, _, _, gt = datasets.make_cylinders(n_per_cylinder=1500, n_cylinders=3, n_outliers=3000, seed=k)
        pts = base * coord + off
        if k % 5:
            m = np.concatenate([rng.uniform(0, 10, 3) * coord + off, rng.normal(size=3) * 2.0 ** e, [rng.uniform(0.1, 2.0) * coord * 2.0 ** e]])
        else:
            m = np.concatenate([gt[0, :3] * coord + off, gt[0, 3:6] * 2.0 ** e, [gt[0, 6] * coord * 2.0 ** e]])
        if k % 7 == 3:
            m[6] = (0.0, -m[6])[k % 2]
        sphere = np.array([0.0, 0.0, 0.0, m[6]])
        got = sq_cylinder(pts, m)
        assert np.array_equal(oracle.squared_residuals(oracle.SPHERE3D, cross_rows(pts, m), sphere), got)
    zero = np.concatenate([m[:3], np.zeros(3), [0.7]])
    assert (sq_cylinder(pts, zero) == 0.7 * 0.7).all()       # d = 0: every residual is |r|
    for j in range(7):                                       # a NaN anywhere: every residual is NaN
        bad = m.copy()
        bad[j] = np.nan
        assert np.isnan(sq_cylinder(pts[:50], bad)).all(), j


# ---- the 2-point solver -------------------------------------------------------------------------------------------------------------
def _on_cylinder(rng, cyl, n):
    """n exact points of the cylinder (p, d, r) and their outward unit normals"""
    p, d, r = cyl[:3], cyl[3:6], cyl[6]
    a = np.cross(d, [1.0, 0.0, 0.0] if abs(d[0]) < 0.9 else [0.0, 1.0, 0.0])
    a /= np.linalg.norm(a)
    b = np.cross(d, a)
    phi, t = rng.uniform(0, 2 * np.pi, n), rng.uniform(-3, 3, n)
    rad = np.cos(phi)[:, None] * a + np.sin(phi)[:, None] * b
    return p + t[:, None] * d + r * rad, rad


def test_cylinder_minimal_solver_on_hand_made_samples():
    rng = np.random.default_rng(5)
    hand = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 5.0],           # 0, 1: on the unit cylinder about z
                     [1.0, 0.0, 2.0],                            # 2: normal parallel to 0's
                     [0.5, 0.5, 0.5],                            # 3: a zero normal
                     [1.0, 0.0, 0.0],                            # 4: coincides with 0, another normal
                     [np.nan, 0.0, 0.0], [0.0, np.inf, 0.0],     # 5, 6
                     [1e200, 0.0, 0.0], [0.0, 1e200, 1e200],     # 7, 8: 1e200 coordinates, unit normals
                     [3.0, 0.0, 0.0], [0.0, 3.0, 1.0],           # 9, 10: on the cylinder of radius 3 about z
                     [1.0, 0.0, 0.0], [0.0, 1.0, 5.0]])          # 11, 12: 0 and 1 with normals of length 1e200 (|na x nb|^2 overflows)
    hn = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [-2.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0],
                   [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [1e200, 0.0, 0.0], [0.0, 1e200, 0.0]])
    cyl = np.array([2.0, -1.0, 0.5, 0.6, 0.0, 0.8, 0.75])
    on, rad = _on_cylinder(rng, cyl, 60)
    pts, nrm = np.vstack([hand, on]), np.vstack([hn, rad])
    est = _estimators.CylinderEstimator()
    est.normals = nrm
    assert (est.sample_size, est.device_minimal, est.model_type, est.cols, est.device_slots) == (2, True, _lib.CYLINDER3D, 7, 1)
    assert est.nonminimal_sample_size >= 5 and _estimators.ESTIMATORS["cylinder"] is _estimators.CylinderEstimator
    special = [[0, 1], [0, 2], [0, 3], [3, 1], [0, 4], [1, 1], [5, 1], [0, 5], [6, 1], [11, 12], [9, 10], [1, 0], [7, 8]]
    samples = np.vstack([special, rng.integers(len(hand), len(pts), (200, 2))])
    models, src = est.minimal(pts, samples)
    want = [solve_scalar(pts[i], pts[j], nrm[i], nrm[j]) for i, j in samples]
    assert list(src) == [k for k, m in enumerate(want) if m is not None]
    # parallel normals, a zero normal (either end), the same index twice, NaN (either end), Inf, normals whose cross product overflows
    assert not {1, 2, 3, 5, 6, 7, 8, 9} & set(src.tolist())
    assert {0, 4, 10, 11, 12} <= set(src.tolist())
    # 1e200 coordinates with unit normals: nothing overflows, the cylinder about z of radius 1e200
    assert models[list(src).index(12)].tolist() == [0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 1e200]
    for m, k in zip(models, src):
        assert np.array_equal(m, want[k]), k                 # bitwise the stated operation order
    assert models[0].tolist() == [0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 1.0]
    m4 = models[list(src).index(4)]
    assert m4[6] == 0.0 and m4[:3].tolist() == [1.0, 0.0, 0.0]           # coincident points, different normals: radius 0 at the point
    m10 = models[list(src).index(10)]
    assert m10.tolist() == [0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 3.0]
    assert models[list(src).index(11)].tolist() == [0.0, 0.0, 5.0, 0.0, 0.0, -1.0, 1.0]
    gen = src >= len(special)
    assert gen.sum() > 150
    assert np.abs(np.linalg.norm(models[:, 3:6], axis=1) - 1.0).max() <= 2 * EPS
    for m, k in zip(models[gen], src[gen]):                  # exact normals: both sample points lie on the surface, the model is the cylinder
        two = pts[samples[k]]
        scale = max(np.abs(two).max(), 1.0) / max(np.linalg.norm(np.cross(nrm[samples[k, 0]], nrm[samples[k, 1]])), 1e-300)
        assert (np.sqrt(sq_cylinder(two, m)) <= 64 * EPS * scale).all(), k
    # the radius range
    est.radius_range = (2.0, 4.0)
    models_r, src_r = est.minimal(pts, samples)
    assert 10 in src_r and 0 not in src_r and (models_r[:, 6] >= 2.0).all() and (models_r[:, 6] <= 4.0).all()
    assert solve_scalar(pts[9], pts[10], nrm[9], nrm[10], 3.0, 3.0) is not None      # inclusive at both ends
    assert solve_scalar(pts[9], pts[10], nrm[9], nrm[10], np.nextafter(3.0, 4.0), 4.0) is None


def test_cylinder_minimal_solver_ignores_the_normals_sign_and_length():
    rng = np.random.default_rng(9)
    cyl = np.array([1.0, 2.0, 3.0, 0.0, 0.6, 0.8, 1.25])
    pts, rad = _on_cylinder(rng, cyl, 80)
    samples = rng.integers(0, 80, (100, 2))
    est = _estimators.CylinderEstimator()
    est.normals = rad
    base, src = est.minimal(pts, samples)
    est.normals = rad * (rng.choice([-1.0, 1.0], 80) * 10.0 ** rng.uniform(-3, 3, 80))[:, None]
    other, src2 = est.minimal(pts, samples)
    assert np.array_equal(src, src2) and len(src) > 80
    well = np.linalg.norm(np.cross(rad[samples[src, 0]], rad[samples[src, 1]]), axis=1) > 0.1
    flip = np.sign((base[:, 3:6] * other[:, 3:6]).sum(axis=1))
    assert np.abs(base[well, 3:6] - flip[well, None] * other[well, 3:6]).max() < 1e-12
    assert np.abs(base[well, 6] - other[well, 6]).max() < 1e-11 and np.abs(base[well, 6] - 1.25).max() < 1e-11
    off = other[well, :3] - cyl[:3]
    assert np.abs(off - (off @ cyl[3:6])[:, None] * cyl[3:6]).max() < 1e-11             # the axis point lies on the true axis


# ---- the Gauss-Newton rows and the refit ----------------------------------------------------------------------------------------------
def test_cylinder_gn_rows_are_the_jacobian_and_the_residual():
    for trial in range(6):
        pts, w, gt, start = refit_fixture(64, (0.0, 1e3)[trial % 2], False, seed=trial)
        u, v = chart(start)
        rows, bad = gn_rows(pts, np.concatenate([start, u]))
        assert not bad.any()
        # |a[5]| is Residual::plain bit for bit
        assert np.array_equal(np.abs(rows[:, 5]), np.abs(np.sqrt(sq_line3d(pts, start)) - start[6]))
        assert np.array_equal(rows[:, 5] * rows[:, 5], sq_cylinder(pts, start))
        assert (rows[:, 4] == -1.0).all()
        h = 1e-6
        for k in range(5):
            x = np.zeros(5)
            x[k] = h
            fd = (f_value(pts, start, u, v, x) - f_value(pts, start, u, v, -x)) / (2 * h)
            assert np.abs(fd - rows[:, k]).max() < 1e-6 * max(1.0, np.abs(rows[:, k]).max()), (trial, k)
            assert np.abs(rows[:, k]).max() > 1e-3                       # (a column of zeros would pass any sign)
    on_axis = np.vstack([pts, start[:3], [np.nan, 0.0, 0.0]])    # e = 0 exactly: s == 0
    assert gn_rows(on_axis, np.concatenate([start, u]))[1].tolist() == [False] * 64 + [True, True]


def _refit(pts, w, start, **kw):
    est = _estimators.CylinderEstimator()
    log = []
    (models,) = est._fit_many(numpy_gram(pts, w, log=log, **kw), 1, [start])
    return models, log


def test_cylinder_refit_requests_and_failures():
    pts, w, gt, start = refit_fixture(64, 0.0, True, seed=3)
    models, log = _refit(pts, w, start)
    assert len(models) == 1 and models[0].shape == (7,)
    gn = [r for r in log if r[0] == _lib.GRAM_CYL_GN]
    assert 2 <= len(gn) <= 10 and all(r[2] is True and r[3] == 1 and r[1].shape == (1, 10) for r in gn)
    assert [r[0] for r in log] == [_lib.GRAM_CYL_GN] * len(gn) + [_lib.GRAM_AFFINE] and log[-1][1:] == (None, True, 1)
    for r in gn:                                             # the chart handed over: d unit, u unit and orthogonal to d
        d, u = r[1][0, 3:6], r[1][0, 7:10]
        assert abs(np.linalg.norm(d) - 1) < 4 * EPS and abs(np.linalg.norm(u) - 1) < 4 * EPS and abs(d @ u) < 4 * EPS
    m = models[0]
    assert abs(np.linalg.norm(m[3:6]) - 1.0) <= 4 * EPS and m[3 + int(np.argmax(np.abs(m[3:6])))] > 0
    mean = (pts * w[:, None]).sum(axis=0) / w.sum()
    assert abs((mean - m[:3]) @ m[3:6]) < 1e-12              # p is the foot of the weighted mean
    est = _estimators.CylinderEstimator()
    assert est._fit_many(numpy_gram(pts, w), 1, [None]) == [[]]                          # no init
    assert est._fit_many(numpy_gram(pts[:4], w[:4]), 1, [start]) == [[]]                 # fewer than 5 points
    on_axis = np.vstack([pts, start[:3]])
    assert est._fit_many(numpy_gram(on_axis), 1, [start]) == [[]]                        # a bad point
    with np.errstate(all="ignore"):
        assert est._fit_many(numpy_gram(np.vstack([pts, [1e200, 0, 0]])), 1, [start]) == [[]]    # non-finite sums
        assert est._fit_many(numpy_gram(pts), 1, [np.full(7, np.nan)]) == [[]]
    est.radius_range = (5.0, 6.0)
    assert est._fit_many(numpy_gram(pts, w), 1, [start]) == [[]]                         # radius outside the range
    # two items equal two single fits, and a failing neighbour does not matter
    pts2, w2, _, start2 = refit_fixture(1000, 1e3, False, seed=4)
    sets = [(pts, w, start), (pts2, w2, start2)]

    def gram(kind, prm, use_w, wpow, rows):
        out = [numpy_gram(sets[r][0], sets[r][1])(kind, None if prm is None else prm[k:k + 1], use_w, wpow, [0]) for k, r in enumerate(rows)]
        return np.concatenate([o[0] for o in out]), np.concatenate([o[1] for o in out]), np.concatenate([o[2] for o in out])
    est = _estimators.CylinderEstimator()
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


def test_cylinder_refit_against_gauss_newton_at_50_digits(refit_references):
    """_fit_many on numpy Gram matrices converges to the model plain Gauss-Newton at 50 digits reaches from the same start, within
    32 eps x the condition number of the reference's own 5x5 normal matrix at its solution x the parameter's scale (DESIGN.md 4.5a's
    rule; the scales: cylinder_model.refit_ratios).  The reference converges on every fixture, none is skipped.  Worst ratios measured
    (axis offset, direction, radius): printed, and in docs/lab-notebook.md."""
    worst = np.zeros(3)
    for key, (pts, w, gt, start, ref) in refit_references.items():
        assert ref[4], key                                   # the reference alone converged
        assert abs(ref[2] - gt[6]) < 0.05 * gt[6] and abs(abs(ref[1] @ gt[3:6]) - 1.0) < 1e-2, key       # ... to the cylinder
        models, _ = _refit(pts, w, start)
        assert len(models) == 1, key
        ratios = np.array(refit_ratios(models[0], ref, pts))
        worst = np.maximum(worst, ratios)
        assert (ratios <= 1.0).all(), (key, ratios, ref[3])
    print("worst ratios (axis offset, direction, radius):", worst.tolist())


def test_cylinder_refit_with_a_sign_error_in_a_jacobian_column_is_refused(refit_references):
    """the same check with the sign of one column of the rows reversed, each of the four geometric columns in turn: the iteration no
    longer reaches the reference (a failed or dropped fit counts as refused)"""
    for col in range(4):
        refused = 0
        for key, (pts, w, gt, start, ref) in refit_references.items():
            if key[0] == 5:
                continue
            models, _ = _refit(pts, w, start, plant_sign=col)
            refused += not models or not (np.array(refit_ratios(models[0], ref, pts)) <= 1.0).all()
        assert refused >= 6, (col, refused)


# ---- the f32 filter's budget: the restatement runs with the literals READ FROM score_filters.hip.h --------------------------------------
def test_cylinder_filter_model_and_header_state_the_same_filter():
    assert header_literals() == MODEL_LITERALS
    block = " ".join(header_block().split())
    for line in OPERATION_LINES:
        assert " ".join(line.split()) in block, line
    assert "static constexpr int kRowVals = 6, kGroupVals = 5;" in block and "static constexpr int kStagedVals = 11;" in block
    assert "struct Lane { float p[3]; float d[3]; float r, e1, e0, e2, tpp, nrm, nanh; };" in block


def _near_threshold_pairs(plant_zero_budget=False, per_case=70):
    """(pairs in the band, FP64 inliers among them, FP64 inliers the point test rejected)"""
    lit = header_literals()
    band = inl = wrong = 0
    for rng, gt, T, e, coord in near_threshold_cases():
        pts = near_threshold_points(rng, gt, T, per_case, 5.0 * coord)
        hyp = gt.copy()
        if rng.random() < 0.5:
            hyp[:3] += rng.normal(0, 1e-6 * T, 3)
        hyp[3:] *= 2.0 ** e                                   # direction and radius: the residual scales with |d|, and so does the threshold
        T2 = (T * 2.0 ** e) ** 2
        sq = sq_cylinder(pts, hyp)
        ln = prep(hyp, max(1.0, np.abs(pts).max()), T2, plant_zero_budget, lit=lit)
        for x, s in zip(pts, sq):
            if not abs(s / T2 - 1.0) < 1e-4:
                continue
            band += 1
            if s < T2:
                inl += 1
                wrong += reject(point_row(x), ln)
    return band, inl, wrong


def test_cylinder_filter_rejects_no_inlier_near_the_threshold():
    pytest.importorskip("mpmath")
    band, inl, wrong = _near_threshold_pairs()
    assert band >= 3000 and inl >= 1200, (band, inl)
    assert wrong == 0


def test_cylinder_filter_without_its_budget_is_caught():
    """E planted as 0: scenes far from the origin put the f32 rounding of the coordinates above the 2^-6 margin of the threshold, and
    the check above sees inliers rejected"""
    pytest.importorskip("mpmath")
    band, inl, wrong = _near_threshold_pairs(plant_zero_budget=True, per_case=20)
    assert inl > 0 and wrong > 0


def test_cylinder_group_bound_rejects_no_group_with_a_near_threshold_inlier():
    """the group test on the near-threshold sets themselves, in Morton order: a rejected group holds no exact inlier"""
    pytest.importorskip("mpmath")
    lit = header_literals()
    groups = rejected = 0
    for k, (rng, gt, T, e, coord) in enumerate(near_threshold_cases()):
        if k % 3:
            continue
        pts = near_threshold_points(rng, gt, T, 128, 5.0 * coord)
        far = pts[64] + (pts[64] - gt[:3]) / np.linalg.norm(pts[64] - gt[:3]) * 30 * max(T, abs(gt[6]))
        pts[64:] = far + rng.uniform(-1, 1, (64, 3)) * T                         # and a compact half well off the shell
        pts = np.ascontiguousarray(pts[morton_order(pts)])
        hyp = gt.copy()
        hyp[3:] *= 2.0 ** e
        T2 = (T * 2.0 ** e) ** 2
        ln = prep(hyp, max(1.0, np.abs(pts).max()), T2, lit=lit)
        sq = sq_cylinder(pts, hyp)
        for g0 in range(0, len(pts), 16):
            groups += 1
            if group_reject(group_row(pts[g0:g0 + 16]), ln):
                rejected += 1
                assert not (sq[g0:g0 + 16] < T2).any(), (k, g0)
    assert groups >= 200 and rejected > 0, (groups, rejected)


def test_cylinder_filter_rejects_generic_pairs_and_switches_off():
    pytest.importorskip("mpmath")
    rng = np.random.default_rng(4)
    pts = rng.uniform(0, 10, (1500, 3))
    T = 1.5 * 0.05
    lit = header_literals()
    rej = tot = 0
    for k in range(3):
        hyp = random_cylinder(rng, 1.0, 0.0, (0.5, 0.0, -0.3)[k])
        hyp[3:] *= (1.0, 2.0 ** -40, 7.0)[k]
        T2 = (T * np.linalg.norm(hyp[3:6])) ** 2
        ln = prep(hyp, 10.0, T2, lit=lit)
        sq = sq_cylinder(pts, hyp)
        for x, s in zip(pts[500 * k:500 * (k + 1)], sq[500 * k:500 * (k + 1)]):
            r = reject(point_row(x), ln)
            assert not (r and s < T2)
            rej += r
            tot += 1
    assert rej > 0.9 * tot
    # never rejected: a zero direction (every residual is |r|), Inf entries (the radius among them), a direction outside the normaliser's
    # band, thresholds outside the f32 range, points, coordinates and radii beyond 1e17
    gt = random_cylinder(rng, 1.0, 0.0, 0.5)
    p, d, r = gt[:3], gt[3:6], gt[6:]
    for hyp, T2, pscale in ((np.concatenate([p, np.zeros(3), r]), T * T, 10.0), (np.concatenate([p, [np.inf, 0.0, 0.0], r]), T * T, 10.0),
                            (np.concatenate([[np.inf, 0.0, 0.0], d, r]), T * T, 10.0), (np.concatenate([p, d * 1e-80, r]), T * T, 10.0),
                            (gt, 1e-70, 10.0), (gt, 1e70, 10.0), (np.concatenate([p * 1e18, d, r]), T * T, 10.0), (gt, T * T, 1e18),
                            (np.concatenate([p, d, [np.inf]]), T * T, 10.0), (np.concatenate([p, d, [-np.inf]]), T * T, 10.0),
                            (np.concatenate([p, d, [1e18]]), T * T, 10.0), (np.concatenate([p, d, [-1e18]]), T * T, 10.0)):
        ln = prep(hyp, pscale, T2, lit=lit)
        assert ln["e0"] == np.inf and ln["nanh"] == 0.0
        assert not any(reject(point_row(x), ln) for x in pts[:20])
        assert not group_reject(group_row(pts[:64]), ln)
    for k in range(7):                                       # a NaN entry: no pair is rejected (the exact path gives NaN), the group is culled
        nan = gt.copy()
        nan[k] = np.nan
        ln = prep(nan, 10.0, T * T, lit=lit)
        assert ln["nanh"] == 1.0 and group_reject(group_row(pts[:64]), ln)
        assert not any(reject(point_row(x), ln) for x in pts[:20])
        assert np.isnan(sq_cylinder(pts[:20], nan)).all()


# ---- the generator ------------------------------------------------------------------------------------------------------------------
def test_make_cylinders_is_seeded_and_its_inliers_lie_on_their_cylinders():
    kw = dict(n_per_cylinder=2000, n_cylinders=4, n_outliers=300, sigma=0.02, normal_noise_deg=5.0)
    a = datasets.make_cylinders(seed=3, **kw)
    b = datasets.make_cylinders(seed=3, **kw)
    c = datasets.make_cylinders(seed=4, **kw)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    assert not np.array_equal(a[0], c[0])
    pts, nrm, labels, gt = a
    assert pts.shape == nrm.shape == (8300, 3) and pts.dtype == nrm.dtype == np.float64
    assert labels.shape == (8300,) and labels.dtype == np.int32 and gt.shape == (4, 7) and gt.dtype == np.float64
    assert np.bincount(labels).tolist() == [300, 2000, 2000, 2000, 2000]
    assert np.abs(np.linalg.norm(gt[:, 3:6], axis=1) - 1.0).max() < 1e-15 and np.abs(np.linalg.norm(nrm, axis=1) - 1.0).max() < 1e-14
    assert ((gt[:, 6] >= 0.3) & (gt[:, 6] <= 1.0)).all()
    for j in range(4):
        on, nn = pts[labels == j + 1], nrm[labels == j + 1]
        e = on - gt[j, :3]
        t = e @ gt[j, 3:6]
        radial = e - t[:, None] * gt[j, 3:6]
        s = np.linalg.norm(radial, axis=1)
        assert abs((s - gt[j, 6]).std() - 0.02) < 0.1 * 0.02 and abs((s - gt[j, 6]).mean()) < 0.1 * 0.02   # Gaussian along the radius
        assert np.array_equal((s - gt[j, 6]) ** 2 > 0, sq_cylinder(on, gt[j]) > 0)
        half = 0.5 * (t.max() - t.min())
        assert 1.5 - 0.05 <= half <= 3.0 + 0.05 and abs(t.mean()) < 0.1 * half                  # length in (3, 6), about the midpoint
        ends = gt[j, :3] + np.array([[-1.0], [1.0]]) * (half - 0.05) * gt[j, 3:6]
        assert ((ends >= 0) & (ends <= 10.0)).all()                                              # the axis segment lies inside the box
        cosang = np.abs((nn * (radial / s[:, None])).sum(axis=1))                            # the sign is random
        ang = np.degrees(np.arccos(np.minimum(cosang, 1.0)))
        assert ang.max() <= 5.0 + 1e-6 and ang.mean() > 1.0
        signs = np.sign((nn * radial).sum(axis=1))
        assert 0.4 < (signs > 0).mean() < 0.6
    out = pts[labels == 0]
    assert ((out >= 0) & (out <= 10.0)).all() and ((pts >= -0.1) & (pts <= 10.1)).all()
    exact = datasets.make_cylinders(n_per_cylinder=100, n_cylinders=1, n_outliers=0, sigma=0.0, normal_noise_deg=0.0, coverage=0.25, seed=1)
    e = exact[0] - exact[3][0, :3]
    radial = e - (e @ exact[3][0, 3:6])[:, None] * exact[3][0, 3:6]
    assert np.abs(np.abs((exact[1] * radial).sum(axis=1)) - exact[3][0, 6]).max() < 1e-12      # exact radial normals
    phi_spread = np.linalg.norm(radial / exact[3][0, 6] - (radial / exact[3][0, 6]).mean(axis=0), axis=1).max()
    assert phi_spread < 1.0                                  # a quarter of the circumference: all within 45 degrees of the arc's middle
    d = datasets.make_cylinders()
    assert d[0].shape == (96000, 3) and d[3].shape == (6, 7) and np.bincount(d[2]).tolist() == [48000] + [8000] * 6
    with pytest.raises(ValueError, match="coverage"):
        datasets.make_cylinders(coverage=0.0)
    with pytest.raises(ValueError, match="length"):
        datasets.make_cylinders(length=(4.0, 20.0))
