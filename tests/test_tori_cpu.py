"""findTori without a GPU: the ABI entries of the torus type, the public call's signature and input checks, the residual's restatement
against the oracle's 2-D circle, plane and symmetric-homography steps, the 4-point two-slot solver of TorusEstimator on exact data, on
degenerate samples and against another route at 50 digits, the Gauss-Newton rows against differences at 50 digits and the refit
against Gauss-Newton at 50 digits, the f32 filter's error budget on a restatement of Filter32<kTorus3D> (tests/torus_model.py), the
make_tori generator and the end-to-end scene's sample statistics."""
import ctypes
import inspect

import numpy as np
import pytest

import pyprogressivex as px
import torus_model as TM
from line3d_filter_model import SYM_MODEL, sym_points
from pyprogressivex import _estimators, _lib, datasets
from torus_model import (E2E, E2E_SEEDS, E2E_T, MODEL_LITERALS, OPERATION_LINES, REFIT_CASES, chart, e_rows, gn_rows,
                         group_reject, group_row, header_block, header_literals, morton_order, near_threshold_cases,
                         near_threshold_points, numpy_gram, on_torus, point_row, prep, random_torus, refit_fixture, refit_ratios, reject,
                         rho_h, rho_h_rows, same_torus, scaled_model, signed_torus, solve_scalar, sq_line3d, sq_torus, sweep_is_crossed)


def test_model_dims_of_the_torus_type():
    lib = _lib.load()
    d, p = ctypes.c_int(), ctypes.c_int()
    assert lib.pgx_model_dims(22, ctypes.byref(d), ctypes.byref(p)) == 0
    assert (d.value, p.value) == (3, 8) == _lib.MODEL_TABLE[22][:2]
    assert _lib.TORUS3D == 22 and _lib.MODEL_TABLE[22] == (3, 8, 4, 2)
    assert _lib.POINT_DIM[22] == 3 and _lib.PARAM_DIM[22] == 8
    for unassigned in (21, 23, -1):
        assert lib.pgx_model_dims(unassigned, None, None) != 0 and unassigned not in _lib.MODEL_TABLE
    assert _lib.GRAM_TORUS_GN == 9 and _lib.GRAM_Q[_lib.GRAM_TORUS_GN] == 8
    est = _estimators.TorusEstimator
    assert _estimators.ESTIMATORS["torus"] is est and datasets.MODEL_TYPES["torus"] == 22
    assert (est.model_type, est.sample_size, est.device_slots, est.cols, est.device_minimal) == (22, 4, 2, 8, True)
    assert "pgx_set_major_radius_range" in _lib.ABI_SYMBOLS and hasattr(lib, "pgx_set_major_radius_range")
    assert callable(_lib.Context.set_major_radius_range)


def test_find_tori_is_exported_with_its_signature():
    assert "findTori" in px.__all__ and callable(px.findTori)
    sig = inspect.signature(px.findTori)
    cyl = inspect.signature(px.findCylinders).parameters
    positional = [k for k, v in sig.parameters.items() if v.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD]
    assert positional == [k for k, v in cyl.items() if v.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD]
    assert sig.parameters["normals"].default is inspect.Parameter.empty
    assert [sig.parameters[k].default for k in positional[2:]] == [cyl[k].default for k in positional[2:]]
    kw = {k: v.default for k, v in sig.parameters.items() if v.kind is inspect.Parameter.KEYWORD_ONLY}
    assert kw.pop("radius_range") == (0.0, np.inf) and kw.pop("major_radius_range") == (0.0, np.inf)
    assert kw == {k: v.default for k, v in cyl.items() if v.kind is inspect.Parameter.KEYWORD_ONLY and k != "radius_range"}
    doc = px.findTori.__doc__
    assert "threshold" in doc and "major_radius_range" in doc and "unsigned" in doc and "unit length" in doc and "RING torus" in doc


def test_find_tori_rejects_bad_input():
    for points in (np.zeros((10, 2)), np.zeros((10, 4)), np.zeros(30), np.zeros((3, 3)), np.zeros((0, 3))):
        with pytest.raises(ValueError, match=r"points should be an array with dims \[n,3\], n>=4"):
            px.findTori(points, np.zeros((points.shape[0], 3)))
    for normals in (np.zeros((10, 2)), np.zeros((9, 3)), np.zeros(30), None):
        with pytest.raises(ValueError, match=r"normals should be an array with dims \[n,3\]"):
            px.findTori(np.zeros((10, 3)), normals)
    with pytest.raises(ValueError, match="weights"):
        px.findTori(np.zeros((10, 3)), np.zeros((10, 3)), np.ones(9))
    for bad in ((-1.0, 10.0), (20.0, 10.0), (np.nan, 10.0), (10.0, np.nan), 3.0, (1.0, 2.0, 3.0)):
        with pytest.raises(ValueError, match=r"^radius_range"):
            px.findTori(np.zeros((10, 3)), np.zeros((10, 3)), radius_range=bad)
        with pytest.raises(ValueError, match=r"^major_radius_range"):
            px.findTori(np.zeros((10, 3)), np.zeros((10, 3)), major_radius_range=bad)


def test_find_tori_unknown_sampler_prints_and_returns_no_model(capsys):
    pts, nrm, _, _ = datasets.make_tori(n_per_torus=50, n_tori=2, n_outliers=20, seed=1)
    tori, labels = px.findTori(pts, nrm, sampler_id=7)
    assert tori.shape == (0, 8) and tori.dtype == np.float64
    assert labels.shape == (pts.shape[0],) and labels.dtype == np.int32 and not labels.any()
    assert "Unknown sampler identifier: 7" in capsys.readouterr().err


def test_the_torus_estimator_puts_both_ranges_and_the_normals_on_the_context():
    calls = []

    class Ctx:
        def set_radius_range(self, lo, hi):
            calls.append(("minor", lo, hi))

        def set_major_radius_range(self, lo, hi):
            calls.append(("major", lo, hi))

        def set_normals(self, nrm):
            calls.append(("normals", nrm))
    est = _estimators.TorusEstimator()
    assert est.takes_radius_range and est.radius_range == (0.0, np.inf) and est.major_radius_range == (0.0, np.inf)
    est.radius_range, est.major_radius_range, est.normals = (0.1, 0.6), (0.7, 2.5), np.ones((4, 3))
    est.context_setup(Ctx())
    assert sorted(c[:3] for c in calls if c[0] != "normals") == [("major", 0.7, 2.5), ("minor", 0.1, 0.6)]
    assert [c[1] is est.normals for c in calls if c[0] == "normals"] == [True]


# ---- the residual -------------------------------------------------------------------------------------------------------------------
def test_the_oracle_holds_the_torus_residual_by_transformation(oracle):
    """sq_torus (numpy, written next to the kernel) against three types the oracle has, bit for bit: its 2-D circle (type 10) with the
    model (R, 0, r) on the rows (rho, h) gives the last step |sqrt((rho - R)^2 + (h - 0)^2) - r| and its square; its plane (type 6) with
    the model (d, 0) on the rows e = x - c gives h; its symmetric homography (type 5) on the 3-D line's witness rows gives q = rho^2.
    Scene scales 1, 1e3, 1e6, offsets 0 and 1e6, direction scales 2^-40 .. 2^40."""
    rng = np.random.default_rng(23)
    for k in range(36):
        coord, off, e = (1.0, 1e3, 1e6)[k % 3], (0.0, 1e6)[k % 2], (-40, 0, 3, 40)[k % 4]
        base, _, _, gt = datasets.make_tori(n_per_torus=1500, n_tori=3, n_outliers=3000, seed=k)
        pts = base * coord + off
        if k % 5:
            m = np.concatenate([rng.uniform(0, 10, 3) * coord + off, rng.normal(size=3) * 2.0 ** e,
                                np.array([rng.uniform(0.5, 3.0), rng.uniform(0.1, 0.5)]) * coord * 2.0 ** e])
        else:
            m = np.concatenate([gt[0, :3] * coord + off, gt[0, 3:6] * 2.0 ** e, gt[0, 6:8] * coord * 2.0 ** e])
        if k % 7 == 3:
            m[6 + k % 2] = -m[6 + k % 2]
        got = sq_torus(pts, m)
        rows = rho_h_rows(pts, m)
        circle = np.array([m[6], 0.0, m[7]])
        assert np.array_equal(oracle.squared_residuals(10, rows, circle), got)
        rho, h = rho_h(pts, m)
        plane = np.array([m[3], m[4], m[5], 0.0])
        assert np.array_equal(oracle.squared_residuals(oracle.PLANE3D, e_rows(pts, m), plane), h * h)
        for j in range(0, len(pts), 997):
            assert oracle.residual(oracle.PLANE3D, e_rows(pts, m)[j], plane) == abs(h[j])
            assert oracle.residual(10, rows[j], circle) == abs(signed_torus(pts[j:j + 1], m)[0])
        assert np.array_equal(oracle.squared_residuals(5, sym_points(pts, m), SYM_MODEL), sq_line3d(pts, m))
        assert np.array_equal(np.sqrt(sq_line3d(pts, m)), rho)
    zero = np.concatenate([m[:3], np.zeros(3), m[6:8]])
    assert (sq_torus(pts, zero) == (abs(m[6]) - m[7]) ** 2).all()        # d = 0: every residual is ||R| - r|
    for j in range(8):                                       # a NaN anywhere: every residual is NaN
        bad = m.copy()
        bad[j] = np.nan
        assert np.isnan(sq_torus(pts[:50], bad)).all(), j
    # (d, R, r) times a power of two scales the residual bit for bit
    unit = np.concatenate([gt[0, :3] * coord + off, gt[0, 3:6], gt[0, 6:8] * coord])
    for kd in (2.0 ** 7, 2.0 ** -30):
        scaled = unit.copy()
        scaled[3:8] *= kd
        assert np.array_equal(sq_torus(pts, scaled), sq_torus(pts, unit) * kd ** 2)


def test_what_the_torus_residual_measures():
    """for a ring torus the residual is the distance to the surface: points moved off it along the normal, inwards by less than r and
    outwards by less than R - r (farther out on the hole's side the normal line crosses the axis), and points on the axis"""
    rng = np.random.default_rng(2)
    torus = random_torus(rng)
    surf, nrm = on_torus(rng, torus, 400)
    t = rng.uniform(-0.9 * torus[7], 0.9 * (torus[6] - torus[7]), 400)
    assert np.abs(np.sqrt(sq_torus(surf + t[:, None] * nrm, torus)) - np.abs(t)).max() < 1e-14
    axis = torus[:3] + rng.uniform(-1, 1, 50)[:, None] * torus[3:6]
    rho, h = rho_h(axis, torus)
    assert np.abs(np.sqrt(sq_torus(axis, torus)) - np.abs(np.sqrt(torus[6] ** 2 + h * h) - torus[7])).max() < 1e-14


# ---- the 4-point solver -------------------------------------------------------------------------------------------------------------
def _exact_scene(seed, n=300, **kw):
    rng = np.random.default_rng(seed)
    gt = random_torus(rng, **kw)
    pts, nrm = on_torus(rng, gt, n)
    return rng, gt, pts, nrm * (rng.choice([-1.0, 1.0], n) * rng.uniform(0.5, 2.0, n))[:, None]


def test_torus_minimal_solver_returns_the_planted_torus_on_exact_data():
    """noise-free tori at the origin, 1e3 away, at a scale of 1e3 and with R / r of 1.2 and 20, normals of random sign and length:
    every sample with four different points returns the planted torus in one of its two slots within 1e-9 (same_torus: the centre
    relative to the largest coordinate, the direction absolute, both radii relative to R), bitwise the scalar restatement, and
    minimal() is the rows that hold a model"""
    total = 0
    for seed, kw in enumerate((dict(), dict(offset=1e3), dict(coord=1e3), dict(ratio=1.2), dict(ratio=20.0))):
        rng, gt, pts, nrm = _exact_scene(seed, **kw)
        est = _estimators.TorusEstimator()
        est.normals = nrm
        samples = np.array([rng.choice(len(pts), 4, replace=False) for _ in range(120)])
        rows = est.minimal_rows(pts, samples)
        assert rows.shape == (240, 8)
        rel = 1e-9                                            # (measured: 3e-12, 2e-11, 2e-11, 2e-10 and 3e-13 on the five scenes)
        for s in range(len(samples)):
            assert any(not np.isnan(rows[2 * s + j, 0]) and same_torus(rows[2 * s + j], gt, rel) for j in range(2)), (seed, s)
            total += 1
        for s in range(0, len(samples), 7):
            for j in range(2):
                m = solve_scalar(pts[samples[s]], nrm[samples[s]], j)
                assert (m is None and np.isnan(rows[2 * s + j]).all()) or np.array_equal(m, rows[2 * s + j])
        models, src = est.minimal(pts, samples)
        ok = ~np.isnan(rows[:, 0])
        assert np.array_equal(models, rows[ok]) and np.array_equal(src, np.nonzero(ok)[0] // 2)
        assert (models[:, 6] > models[:, 7]).all() and np.abs(np.linalg.norm(models[:, 3:6], axis=1) - 1.0).max() < 1e-15
    assert total == 600


def test_torus_minimal_solver_refusals():
    rng, gt, pts, nrm = _exact_scene(11)
    est = _estimators.TorusEstimator()
    s = np.array([[3, 40, 77, 150]])
    est.normals = nrm
    full = est.minimal_rows(pts, s)
    j = [k for k in range(2) if not np.isnan(full[k, 0]) and same_torus(full[k], gt, 1e-9)][0]
    R, r = gt[6], gt[7]
    # either range: just inside keeps the slot, just outside drops it
    for attr, v in (("radius_range", r), ("major_radius_range", R)):
        for rng_, keep in (((0.0, v * 1.001), True), ((v * 0.999, np.inf), True), ((0.0, v * 0.999), False), ((v * 1.001, np.inf), False)):
            e2 = _estimators.TorusEstimator()
            e2.normals = nrm
            setattr(e2, attr, rng_)
            assert (not np.isnan(e2.minimal_rows(pts, s)[j, 0])) == keep, (attr, rng_)
            kw = dict(zip(("rmin", "rmax") if attr == "radius_range" else ("Rmin", "Rmax"), rng_))
            assert (solve_scalar(pts[s[0]], nrm[s[0]], j, **kw) is not None) == keep
    # parallel normal lines (all coefficients 0) and coplanar ones (four normals of one meridian plane: every line of the plane is a
    # transversal); a repeated point; non-finite input; a zero normal
    par = np.tile(np.array([0.0, 0.0, 1.0]), (4, 1))
    est.normals = np.tile(par[0], (len(pts), 1))
    assert np.isnan(est.minimal_rows(pts, s)).all()
    e1, _ = TM.frame_of(gt[3:6])
    th = np.array([0.3, 1.4, 2.9, 4.0])
    mer_n = np.cos(th)[:, None] * e1 + np.sin(th)[:, None] * gt[3:6]
    mer_p = gt[:3] + R * e1 + r * mer_n
    # coplanar: the z = 0 plane holds all four lines, in whole numbers, so that every coefficient is 0 exactly and qa == 0
    flat_p = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [1.0, 1.0, 0.0]])
    flat_n = np.array([[1.0, 2.0, 0.0], [-1.0, 1.0, 0.0], [2.0, 1.0, 0.0], [1.0, -3.0, 0.0]])
    for slot in range(2):
        assert solve_scalar(flat_p, par, slot) is None and solve_scalar(flat_p, flat_n, slot) is None
    est.normals = flat_n
    assert np.isnan(est.minimal_rows(flat_p, np.array([[0, 1, 2, 3]]))).all()
    # four normals of one meridian plane of the torus are coplanar only up to rounding: whatever comes out is not the planted torus
    # to more digits than the data has, and no claim is made on it beyond the gates
    est.normals = mer_n
    got = est.minimal_rows(mer_p, np.array([[0, 1, 2, 3]]))
    assert all(np.isnan(row[0]) or (row[6] > row[7] and np.isfinite(row).all()) for row in got)
    est.normals = nrm
    for bad_val in (np.nan, np.inf):
        p2, n2 = pts.copy(), nrm.copy()
        p2[40, 1] = bad_val
        assert np.isnan(est.minimal_rows(p2, s)).all()
        n2[77, 0] = bad_val
        est.normals = n2
        assert np.isnan(est.minimal_rows(pts, s)).all()
        est.normals = nrm
    n2 = nrm.copy()
    n2[3] = 0.0
    est.normals = n2
    assert np.isnan(est.minimal_rows(pts, s)).all()
    # R <= r: the samples of a spindle torus (R < r) give its model to the arithmetic, and the solver refuses it
    spindle = gt.copy()
    spindle[6], spindle[7] = 0.4, 0.9
    sp, sn = on_torus(np.random.default_rng(5), spindle, 40)
    est.normals = sn
    rows = est.minimal_rows(sp, np.array([np.random.default_rng(k).choice(40, 4, replace=False) for k in range(30)]))
    assert not any(not np.isnan(row[0]) and same_torus(row, spindle, 1e-6) for row in rows)
    assert (rows[~np.isnan(rows[:, 0]), 6] > rows[~np.isnan(rows[:, 0]), 7]).all()


@pytest.fixture(scope="module")
def route_cases():
    """40 samples of noisy oriented points (so that BOTH transversals are generic) with the 50-digit answers of both routes"""
    pytest.importorskip("mpmath")
    out = []
    for seed in range(40):
        rng = np.random.default_rng(500 + seed)
        gt = random_torus(rng, offset=(0.0, 1e2)[seed % 2])
        pts, nrm = on_torus(rng, gt, 4)
        pts = pts + rng.normal(0, 0.01, pts.shape)
        nrm = nrm + rng.normal(0, 0.03, nrm.shape)
        out.append((pts, nrm, TM.transversal_reference(pts, nrm)))
    return out


def test_torus_minimal_solver_against_the_pluecker_route_at_50_digits(route_cases):
    """The product's route (bilinear elimination) against the Pluecker null space and the Klein quadric at 50 digits: every reference
    torus that passes the solver's gates (R > r) has a slot of its own, no other slot is filled, and the match is within
    32 eps kappa_route of the product's route (torus_model.route_sensitivity: hooks behind every stage, DESIGN.md 4.5b's manner), for
    cases whose tolerance stays below 1e-6; the restated route with every hook at 0 lands on the reference to 1e-30."""
    held = 0
    worst = np.zeros(3)
    for k, (pts, nrm, (refs, gap)) in enumerate(route_cases):
        slots = [solve_scalar(pts, nrm, j) for j in range(2)]
        want = [m for m in refs if m[6] > m[7]]
        filled = [m for m in slots if m is not None]
        margin = min([abs(m[6] - m[7]) / m[6] for m in refs] + [1.0])
        if margin < 1e-6:
            continue                                          # a reference on the R = r gate: either side may round either way
        assert len(filled) == len(want), (k, slots, refs)
        used = set()
        for m in want:
            j = [i for i, s in enumerate(slots) if s is not None and i not in used and same_torus(s, m, 1e-6)]
            assert j, (k, m, slots)
            used.add(j[0])
            mdl, kappa = TM.route_sensitivity(pts, nrm, j[0])
            assert same_torus(mdl, m, 1e-30 * max(1.0, 1.0 / gap))
            if 32.0 * TM.EPS * max(kappa) > 1e-6:
                continue
            ratios = np.array(TM.route_ratios(slots[j[0]], m, kappa, pts))
            worst = np.maximum(worst, ratios)
            assert (ratios <= 1.0).all(), (k, ratios, kappa)
            held += 1
    print("held", held, "worst ratios (centre, direction, radii):", worst.tolist())
    assert held >= 30


# ---- the Gauss-Newton rows and the refit ------------------------------------------------------------------------------------------------
def test_torus_gn_rows_are_the_jacobian_and_the_residual():
    """the seven derivative columns against central differences of the 50-digit f (step 1e-20: the difference is exact to 1e-30), the
    last column against sq_torus's signed value bit for bit; a point on the axis and a point on the spine have no row"""
    pytest.importorskip("mpmath")
    rng = np.random.default_rng(8)
    gt = random_torus(rng)
    pts, nrm = on_torus(rng, gt, 12)
    pts = pts + nrm * rng.normal(0, 0.05, 12)[:, None]
    m = gt.copy()
    m[:3] += 0.02
    u, v = chart(m)
    rows, bad = gn_rows(pts, np.concatenate([m, u]))
    assert not bad.any() and np.array_equal(rows[:, 7], signed_torus(pts, m)) and (rows[:, 6] == -1.0).all()
    import mpmath
    step = mpmath.mpf(10) ** -20
    for col in range(7):
        x = [0] * 7
        x[col] = step
        hi = TM.f_value_mp(pts, m, u, v, x)
        x[col] = -step
        lo = TM.f_value_mp(pts, m, u, v, x)
        fd = np.array([float((a - b) / (2 * step)) for a, b in zip(hi, lo)])
        assert np.abs(fd - rows[:, col]).max() < 1e-12, (col, fd, rows[:, col])
    # in whole and binary numbers, so that rho and w are 0 exactly: a point on the axis, a point on the spine, an ordinary one
    upright = np.array([1.0, 2.0, 3.0, 0.0, 0.0, 1.0, 1.5, 0.25, 1.0, 0.0, 0.0])
    special = np.array([[1.0, 2.0, 3.5], [2.5, 2.0, 3.0], [2.5, 2.0, 3.5]])
    assert gn_rows(special, upright)[1].tolist() == [True, True, False]


def _refit(pts, w, start, plant_sign=None):
    log = []
    est = _estimators.TorusEstimator()
    out = est._fit_many(numpy_gram(pts, w, plant_sign, log), 1, [start])
    return out[0], log


def test_torus_refit_requests_and_failures():
    pts, w, gt, start = refit_fixture(64, 0.0, True, 3)
    models, log = _refit(pts, w, start)
    assert len(models) == 1 and 1 <= len(log) <= 10
    assert all(k == _lib.GRAM_TORUS_GN and uw is True and wp == 1 and prm.shape == (1, 11) for k, prm, uw, wp in log)
    assert same_torus(models[0], gt, 0.02) and models[0][6] > models[0][7] > 0 and abs(np.linalg.norm(models[0][3:6]) - 1.0) < 1e-15
    est = _estimators.TorusEstimator()
    assert est._fit_many(numpy_gram(pts, w), 1, [None]) == [[]]
    assert est._fit_many(numpy_gram(pts[:6], None), 1, [start]) == [[]]                       # fewer than seven points
    for attr, rng_ in (("radius_range", (0.0, gt[7] * 0.5)), ("major_radius_range", (gt[6] * 1.5, np.inf))):
        e2 = _estimators.TorusEstimator()
        setattr(e2, attr, rng_)
        assert e2._fit_many(numpy_gram(pts, w), 1, [start]) == [[]], attr
    inner = numpy_gram(pts, None)

    def one_bad(*a):
        G, cnt, _ = inner(*a)
        return G, cnt, np.array([1])
    assert est._fit_many(one_bad, 1, [start]) == [[]]                                         # bad: a point without a row


@pytest.fixture(scope="module")
def refit_references():
    """the 50-digit answers, computed once for the refit tests of this module"""
    pytest.importorskip("mpmath")
    return {key: TM.refit_case(*key) for key in REFIT_CASES}


def test_torus_refit_against_gauss_newton_at_50_digits(refit_references):
    """_fit_many on numpy Gram matrices converges to the model plain Gauss-Newton at 50 digits reaches from the same start, within
    32 eps x the condition number of the reference's own 7x7 normal matrix at its solution x the parameter's scale (DESIGN.md 4.5a's
    rule; the scales: torus_model.refit_ratios).  The reference converges on every fixture, none is skipped."""
    worst = np.zeros(3)
    for key, (pts, w, gt, start, ref) in refit_references.items():
        assert ref[4], key                                   # the reference alone converged
        assert np.linalg.norm(ref[2] - gt[6:8]) < 0.05 * gt[6], key
        models, _ = _refit(pts, w, start)
        assert len(models) == 1, key
        ratios = np.array(refit_ratios(models[0], ref, pts))
        worst = np.maximum(worst, ratios)
        print(key, "cond %.3g" % ref[3], "ratios", ratios.tolist())
        assert (ratios <= 1.0).all(), (key, ratios, ref[3])
    print("worst ratios (centre, direction, radii):", worst.tolist())


def test_torus_refit_with_a_sign_error_in_a_jacobian_column_is_refused(refit_references):
    """the same check with the sign of one column of the rows reversed, each of the seven columns in turn: the iteration no longer
    reaches the reference (a failed or dropped fit counts as refused)"""
    for col in range(7):
        refused = 0
        for key, (pts, w, gt, start, ref) in refit_references.items():
            if key[0] == 7:
                continue
            models, _ = _refit(pts, w, start, plant_sign=col)
            refused += not models or not (np.array(refit_ratios(models[0], ref, pts)) <= 1.0).all()
        assert refused >= 6, (col, refused)


# ---- the f32 filter's budget: the restatement runs with the literals READ FROM score_filters.hip.h --------------------------------------
def test_torus_filter_model_and_header_state_the_same_filter():
    assert header_literals() == MODEL_LITERALS
    block = " ".join(header_block().split())
    for line in OPERATION_LINES:
        assert " ".join(line.split()) in block, line
    assert "static constexpr int kRowVals = 6, kGroupVals = 5;" in block and "static constexpr int kStagedVals = 12;" in block
    assert "struct Lane { float p[3]; float d[3]; float R, r, e1, e0, e2, tpp, nrm, nanh; };" in block


def _near_threshold_pairs(plant_zero_budget=False, per_case=70):
    """(pairs in the band, FP64 inliers among them, FP64 inliers the point test rejected) over all 81 cases"""
    lit = header_literals()
    band = inl = wrong = 0
    seen = set()
    for rng, gt, T, e, ratio, coord, oc in near_threshold_cases():
        seen.add((e, ratio, coord, oc))
        pts = near_threshold_points(rng, gt, T, per_case)
        base = gt.copy()
        if rng.random() < 0.5:
            base[:3] += rng.normal(0, 1e-6 * T, 3)
        hyp, Ts = scaled_model(base, T, e)
        T2 = Ts * Ts
        sq = sq_torus(pts, hyp)
        ln = prep(hyp, max(1.0, np.abs(pts).max()), T2, plant_zero_budget, lit=lit)
        assert ln["e0"] < np.inf or plant_zero_budget
        for x, s in zip(pts, sq):
            if not abs(s / T2 - 1.0) < 1e-3:
                continue
            band += 1
            if s < T2:
                inl += 1
                wrong += reject(point_row(x), ln)
    assert len(seen) == 81 and sweep_is_crossed(seen)          # every d scale met every ratio, every coordinate scale every offset
    return band, inl, wrong


def test_torus_filter_rejects_no_inlier_near_the_threshold():
    pytest.importorskip("mpmath")
    band, inl, wrong = _near_threshold_pairs()
    assert band >= 3000 and inl >= 1200, (band, inl)
    assert wrong == 0


def test_torus_filter_without_its_budget_is_caught():
    """E planted as 0: scenes far from the origin put the f32 rounding of the coordinates above the 2^-6 margin of the threshold, and
    the check above sees inliers rejected"""
    pytest.importorskip("mpmath")
    band, inl, wrong = _near_threshold_pairs(plant_zero_budget=True, per_case=20)
    assert inl > 0 and wrong > 0


def test_torus_group_bound_rejects_no_group_with_a_near_threshold_inlier():
    """the group test on every one of the 81 near-threshold sets themselves, in Morton order: a rejected group holds no exact inlier"""
    pytest.importorskip("mpmath")
    lit = header_literals()
    groups = 0
    rejected = {-40: 0, 0: 0, 40: 0}                         # per scale of d
    seen = set()
    for k, (rng, gt, T, e, ratio, coord, oc) in enumerate(near_threshold_cases()):
        seen.add((e, ratio, coord, oc))
        pts = near_threshold_points(rng, gt, T, 128)
        far = gt[:3] + (pts[64] - gt[:3]) / np.linalg.norm(pts[64] - gt[:3]) * 5.0 * (gt[6] + gt[7])
        pts[64:] = far + rng.uniform(-1, 1, (64, 3)) * T     # and a compact half well off the surface
        pts = np.ascontiguousarray(pts[morton_order(pts)])
        hyp, Ts = scaled_model(gt, T, e)
        T2 = Ts * Ts
        ln = prep(hyp, max(1.0, np.abs(pts).max()), T2, lit=lit)
        sq = sq_torus(pts, hyp)
        for g0 in range(0, len(pts), 16):
            groups += 1
            if group_reject(group_row(pts[g0:g0 + 16]), ln):
                rejected[e] += 1
                assert not (sq[g0:g0 + 16] < T2).any(), (k, g0)
    assert groups >= 600 and min(rejected.values()) > 0, (groups, rejected)
    assert len(seen) == 81 and sweep_is_crossed(seen)


def test_torus_filter_rejects_generic_pairs_and_switches_off():
    pytest.importorskip("mpmath")
    rng = np.random.default_rng(4)
    pts = rng.uniform(0, 10, (1500, 3))
    T = 1.5 * 0.05
    lit = header_literals()
    rej = tot = 0
    for k in range(3):
        gt = random_torus(rng, ratio=(None, 1.05, 50.0)[k])
        hyp, Ts = scaled_model(gt, T, (0, -40, 3)[k])
        ln = prep(hyp, 10.0, Ts * Ts, lit=lit)
        assert ln["e0"] < np.inf
        sq = sq_torus(pts, hyp)
        for x, s in zip(pts[500 * k:500 * (k + 1)], sq[500 * k:500 * (k + 1)]):
            r = reject(point_row(x), ln)
            assert not (r and s < Ts * Ts)
            rej += r
            tot += 1
    assert rej > 0.8 * tot
    # never rejected: a zero direction, Inf entries (either radius among them), a direction outside the normaliser's band, thresholds
    # outside the f32 range, centres, coordinates and radii beyond 1e17
    gt = random_torus(rng)
    c, d, Rr = gt[:3], gt[3:6], gt[6:8]
    for hyp, T2, pscale in ((np.concatenate([c, np.zeros(3), Rr]), T * T, 10.0), (np.concatenate([c, [np.inf, 0.0, 0.0], Rr]), T * T, 10.0),
                            (np.concatenate([[np.inf, 0.0, 0.0], d, Rr]), T * T, 10.0), (np.concatenate([c, d * 1e-80, Rr]), T * T, 10.0),
                            (gt, 1e-70, 10.0), (gt, 1e70, 10.0), (np.concatenate([c * 1e18, d, Rr]), T * T, 10.0), (gt, T * T, 1e18),
                            (np.concatenate([c, d, [np.inf, Rr[1]]]), T * T, 10.0), (np.concatenate([c, d, [Rr[0], -np.inf]]), T * T, 10.0),
                            (np.concatenate([c, d, [1e18, Rr[1]]]), T * T, 10.0), (np.concatenate([c, d, [Rr[0], 1e18]]), T * T, 10.0)):
        ln = prep(hyp, pscale, T2, lit=lit)
        assert ln["e0"] == np.inf and ln["nanh"] == 0.0
        assert not any(reject(point_row(x), ln) for x in pts[:20])
        assert not group_reject(group_row(pts[:64]), ln)
    for k in range(8):                                       # a NaN entry: no pair is rejected (the exact path gives NaN), the group is culled
        nan = gt.copy()
        nan[k] = np.nan
        ln = prep(nan, 10.0, T * T, lit=lit)
        assert ln["nanh"] == 1.0 and group_reject(group_row(pts[:64]), ln)
        assert not any(reject(point_row(x), ln) for x in pts[:20])
        assert np.isnan(sq_torus(pts[:20], nan)).all()


# ---- the generator ------------------------------------------------------------------------------------------------------------------
def test_make_tori_is_seeded_and_its_inliers_lie_on_their_tori():
    kw = dict(n_per_torus=2000, n_tori=4, n_outliers=300, sigma=0.02, normal_noise_deg=5.0)
    a = datasets.make_tori(seed=3, **kw)
    b = datasets.make_tori(seed=3, **kw)
    c = datasets.make_tori(seed=4, **kw)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    assert not np.array_equal(a[0], c[0])
    pts, nrm, labels, gt = a
    assert pts.shape == nrm.shape == (8300, 3) and pts.dtype == nrm.dtype == np.float64
    assert labels.shape == (8300,) and labels.dtype == np.int32 and gt.shape == (4, 8) and gt.dtype == np.float64
    assert np.bincount(labels).tolist() == [300, 2000, 2000, 2000, 2000]
    assert np.abs(np.linalg.norm(gt[:, 3:6], axis=1) - 1.0).max() < 1e-15 and np.abs(np.linalg.norm(nrm, axis=1) - 1.0).max() < 1e-14
    assert ((gt[:, 6] >= 0.8) & (gt[:, 6] <= 2.0) & (gt[:, 7] >= 0.2) & (gt[:, 7] <= 0.5)).all()
    for j in range(4):
        on, nn = pts[labels == j + 1], nrm[labels == j + 1]
        R, r = gt[j, 6], gt[j, 7]
        f = signed_torus(on, gt[j])
        assert abs(f.std() - 0.02) < 0.1 * 0.02 and abs(f.mean()) < 0.1 * 0.02          # Gaussian along the surface normal
        rho, h = rho_h(on, gt[j])
        cos_t = (rho - R) / np.sqrt((rho - R) ** 2 + h * h)
        # uniform on the surface: the density of theta is (R + r cos theta) / (2 pi R), so E[cos theta] = r / (2 R)
        assert abs(cos_t.mean() - r / (2.0 * R)) < 0.05
        e = on - gt[j, :3]
        radial = (e - h[:, None] * gt[j, 3:6]) / rho[:, None]
        wv = np.sqrt((rho - R) ** 2 + h * h)
        outward = ((rho - R) / wv)[:, None] * radial + (h / wv)[:, None] * gt[j, 3:6]
        cosang = np.abs((nn * outward).sum(axis=1))                                      # the sign is random
        tilt = np.degrees(np.arccos(np.minimum(cosang, 1.0)))
        assert tilt.max() <= 5.0 + 6.0 and np.percentile(tilt, 90) <= 5.0 + 1.5 and tilt.mean() > 1.0    # (sigma / r moves the exact normal)
        signs = np.sign((nn * outward).sum(axis=1))
        assert 0.4 < (signs > 0).mean() < 0.6
    out = pts[labels == 0]
    assert ((out >= 0) & (out <= 10.0)).all() and ((pts >= -0.1) & (pts <= 10.1)).all()
    exact = datasets.make_tori(n_per_torus=100, n_tori=1, n_outliers=0, sigma=0.0, normal_noise_deg=0.0, seed=1)
    assert np.abs(signed_torus(exact[0], exact[3][0])).max() < 1e-13
    got = [solve_scalar(exact[0][[3, 40, 77, 90]], exact[1][[3, 40, 77, 90]], j) for j in range(2)]
    assert any(m is not None and same_torus(m, exact[3][0], 1e-9) for m in got)      # exact points with exact normals give the torus back
    d = datasets.make_tori()
    assert d[0].shape == (96000, 3) and d[3].shape == (6, 8) and np.bincount(d[2]).tolist() == [48000] + [8000] * 6
    with pytest.raises(ValueError, match="minor_radius"):
        datasets.make_tori(minor_radius=(0.2, 0.9))
    with pytest.raises(ValueError, match="fit the box"):
        datasets.make_tori(major_radius=(4.0, 6.0))
    with pytest.raises(ValueError, match="normals"):
        datasets.make_tori(normals="other")


# ---- the end-to-end scene, fixed here before the device runs it ------------------------------------------------------------------------
def test_the_end_to_end_scene_gives_the_solver_enough_good_samples():
    """test_gpu_tori.py's scenes (two tori of 800 points, 800 outliers, R in (0.8, 2.0), r in (0.2, 0.5), sigma 0.01, tilt 2 degrees,
    T = 0.05): of 2000 all-inlier samples, the share that gives (in either slot) a torus collecting at least half of its torus' points
    within T.  At least 20 % are required on every seed, so that the scene is not what fails on the device.

    Measured here: 27.5 % / 23.8 % / 28.6 % on seeds 0 / 1 / 2; with the tilt at 5 degrees 8.7 % / 4.5 % / 10.4 %."""
    for seed in E2E_SEEDS:
        pts, nrm, labels, gt = datasets.make_tori(seed=seed, **E2E)
        rng = np.random.default_rng(100 + seed)
        est = _estimators.TorusEstimator()
        est.normals = nrm
        est.radius_range, est.major_radius_range = E2E["minor_radius"], E2E["major_radius"]
        good = total = 0
        for j in range(2):
            idx = np.nonzero(labels == j + 1)[0]
            samples = np.array([rng.choice(idx, 4, replace=False) for _ in range(1000)])
            rows = est.minimal_rows(pts, samples)
            total += len(samples)
            ok = np.zeros(len(samples), dtype=bool)
            for k in np.nonzero(~np.isnan(rows[:, 0]))[0]:
                ok[k // 2] |= (sq_torus(pts[idx], rows[k]) < E2E_T * E2E_T).sum() >= 0.5 * len(idx)
            good += int(ok.sum())
        share = good / total
        print("seed", seed, "all-inlier samples collecting half of their torus:", round(share, 3))
        assert total == 2000 and share >= 0.20, (seed, share)
