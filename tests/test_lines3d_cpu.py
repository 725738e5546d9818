"""findLines3D without a GPU: the ABI entries of the 3-D line type, the public call's signature and input checks, the 2-point solver
and the refit of Line3DEstimator against hand-made data and a 50-digit reference, the f32 filter's error budget on a restatement of
Filter32<kLine3D> (tests/line3d_filter_model.py), and the make_lines3d generator."""
import ctypes
import inspect
import math

import numpy as np
import pytest

import pyprogressivex as px
from line3d_filter_model import (EPS, MODEL_LITERALS, OPERATION_LINES, REFIT_N, group_reject, header_block, header_literals,
                                 group_row, known_line, morton_order, near_threshold_points, point_row, prep,
                                 refit_fixture, refit_ratios, refit_reference, reject, sq_line3d, sym_points, SYM_MODEL)
from primitive_helpers import numpy_refit
from pyprogressivex import _estimators, _lib, datasets


def test_model_dims_of_the_line3d_type():
    lib = _lib.load()
    d, p = ctypes.c_int(), ctypes.c_int()
    assert lib.pgx_model_dims(12, ctypes.byref(d), ctypes.byref(p)) == 0
    assert (d.value, p.value) == (3, 6) == _lib.MODEL_TABLE[12][:2]
    assert _lib.LINE3D == 12 and _lib.MODEL_TABLE[12] == (3, 6, 2, 1)
    assert _lib.POINT_DIM[12] == 3 and _lib.PARAM_DIM[12] == 6
    for unassigned in (7, 9, 11, 13, -1):
        assert lib.pgx_model_dims(unassigned, None, None) != 0 and unassigned not in _lib.MODEL_TABLE
    # the types around the gaps are still what they were
    assert lib.pgx_model_dims(10, ctypes.byref(d), ctypes.byref(p)) == 0 and (d.value, p.value) == (2, 3)
    assert lib.pgx_model_dims(6, ctypes.byref(d), ctypes.byref(p)) == 0 and (d.value, p.value) == (3, 4)


def test_find_lines3d_is_exported_with_its_signature():
    assert "findLines3D" in px.__all__ and callable(px.findLines3D)
    sig = inspect.signature(px.findLines3D)
    planes = inspect.signature(px.findPlanes).parameters
    positional = [k for k, v in sig.parameters.items() if v.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD]
    assert positional == ["points", "weights", "threshold", "conf", "spatial_coherence_weight", "neighborhood_ball_radius",
                          "maximum_tanimoto_similarity", "max_iters", "minimum_point_number", "maximum_model_number", "sampler_id",
                          "scoring_exponent", "do_logging"]
    defaults = {k: v.default for k, v in sig.parameters.items()}
    assert [defaults[k] for k in positional[1:]] == [None, 0.05, 0.5, 0.0, 0.5, 0.4, 1000, 10, -1, 3, 2, False]
    kw = {k: v.default for k, v in sig.parameters.items() if v.kind is inspect.Parameter.KEYWORD_ONLY}
    assert kw == {k: v.default for k, v in planes.items() if v.kind is inspect.Parameter.KEYWORD_ONLY}
    assert list(kw) == [k for k, v in planes.items() if v.kind is inspect.Parameter.KEYWORD_ONLY]
    doc = px.findLines3D.__doc__
    assert "threshold" in doc and "minimum_point_number" in doc and "1.5 x threshold" in doc


@pytest.mark.parametrize("points", [np.zeros((10, 2)), np.zeros((10, 4)), np.zeros(30), np.zeros((1, 3)), np.zeros((0, 3)),
                                    np.zeros((4, 3, 1))])
def test_find_lines3d_rejects_bad_points(points):
    with pytest.raises(ValueError, match=r"points should be an array with dims \[n,3\], n>=2"):
        px.findLines3D(points)


def test_find_lines3d_rejects_weights_of_the_wrong_length():
    with pytest.raises(ValueError, match="weights"):
        px.findLines3D(np.zeros((10, 3)), np.ones(9))


def test_find_lines3d_unknown_sampler_prints_and_returns_no_model(capsys):
    pts, _, _ = datasets.make_lines3d(n_per_line=50, n_lines=2, n_outliers=20, seed=1)
    lines, labels = px.findLines3D(pts, sampler_id=7)
    assert lines.shape == (0, 6) and lines.dtype == np.float64
    assert labels.shape == (pts.shape[0],) and labels.dtype == np.int32 and not labels.any()
    assert "Unknown sampler identifier: 7" in capsys.readouterr().err


def test_the_oracle_evaluates_the_line_residual_by_transformation(oracle):
    """sq_line3d (numpy, written next to the kernel) and the oracle's symmetric-transfer residual of the transformed points agree bit
    for bit: 4e5 pairs on make_lines3d scenes over scene scales, offsets and direction scales, ground-truth and random lines"""
    rng = np.random.default_rng(17)
    for k in range(40):
        coord, off, e = (1.0, 1e3, 1e6)[k % 3], (0.0, 1e6)[k % 2], (-40, 0, 3, 40)[k % 4]
        base, _, gt = datasets.make_lines3d(n_per_line=1500, n_lines=4, n_outliers=4000, seed=k)
        pts = base * coord + off
        m = (np.concatenate([rng.uniform(0, 10, 3) * coord + off, rng.normal(size=3) * 2.0 ** e]) if k % 5 else
             np.concatenate([gt[0, :3] * coord + off, gt[0, 3:] * 2.0 ** e]))
        assert np.array_equal(oracle.squared_residuals(oracle.HOMOGRAPHY_SYM, sym_points(pts, m), SYM_MODEL), sq_line3d(pts, m))
    zero = np.concatenate([m[:3], np.zeros(3)])
    assert not oracle.squared_residuals(oracle.HOMOGRAPHY_SYM, sym_points(pts, zero), SYM_MODEL).any() and not sq_line3d(pts, zero).any()


# ---- the 2-point solver -------------------------------------------------------------------------------------------------------------
def _line3d_scalar(a, b):
    """the solver's operation order on Python floats (IEEE doubles, no contraction); None = no model"""
    v0, v1, v2 = b[0] - a[0], b[1] - a[1], b[2] - a[2]
    q = (v0 * v0 + v1 * v1) + v2 * v2
    ln = math.sqrt(q) if q >= 0.0 else float("nan")         # (NaN compares false)
    if not (ln > 0.0) or ln == float("inf"):
        return None
    return [a[0], a[1], a[2], v0 / ln, v1 / ln, v2 / ln]


def test_line3d_minimal_solver_on_hand_made_samples():
    rng = np.random.default_rng(5)
    pts = np.vstack([[[1.0, 2.0, 3.0], [1.0, 2.0, 3.0], [4.0, 6.0, 3.0],          # 0 == 1; 0 -> 2 is (3, 4, 0), length 5
                      [np.nan, 0.0, 0.0], [1e200, 0.0, 0.0], [-1e200, 1.0, 2.0],   # NaN; |4 - 5|^2 overflows
                      [0.0, np.inf, 0.0]],
                     rng.uniform(-10, 10, (40, 3)) * 10.0 ** rng.integers(-3, 4, (40, 1))])
    est = _estimators.Line3DEstimator()
    assert (est.sample_size, est.nonminimal_sample_size, est.device_minimal, est.model_type, est.cols) == (2, 2, True, _lib.LINE3D, 6)
    assert est.device_slots == 1 and _estimators.ESTIMATORS["line3d"] is _estimators.Line3DEstimator
    samples = np.vstack([[[0, 2], [0, 1], [3, 2], [2, 3], [4, 5], [5, 5], [6, 0], [2, 0]],
                         rng.integers(7, len(pts), (200, 2))])
    models, src = est.minimal(pts, samples)
    want = [_line3d_scalar(pts[i].tolist(), pts[j].tolist()) for i, j in samples]
    assert list(src) == [k for k, m in enumerate(want) if m is not None]
    assert not {1, 2, 3, 4, 5, 6} & set(src.tolist())      # coincident, NaN (either end), overflowing, the same point twice, Inf
    assert {0, 7} <= set(src.tolist())
    for m, k in zip(models, src):
        assert m.tolist() == want[k], k                      # bitwise the stated operation order
    assert models[0].tolist() == [1.0, 2.0, 3.0, 0.6, 0.8, 0.0]
    assert np.abs(np.sqrt((models[:, 3:] ** 2).sum(axis=1)) - 1.0).max() <= 2 * EPS
    for m, k in zip(models, src):                            # both sample points lie on the line
        two = pts[samples[k]]
        assert (np.sqrt(sq_line3d(two, m)) <= 4 * EPS * np.linalg.norm(two - m[:3], axis=1)).all(), k


# ---- the refit ----------------------------------------------------------------------------------------------------------------------
def test_line3d_refit_recovers_a_known_line():
    rng = np.random.default_rng(3)
    est = _estimators.Line3DEstimator()
    pts, p, d = known_line(rng, 400)
    for w in (None, rng.uniform(0.5, 2.0, len(pts))):
        for est.refit_solver in ("lapack", "jacobi"):      # (no context: "jacobi" runs _smallest(-scatter) on LAPACK here)
            (m,), requests = numpy_refit(est, pts, w)
            assert [(r[0], r[1], r[2], r[3]) for r in requests] == [(_lib.GRAM_AFFINE, None, True, 1)]     # exactly one request
            assert m.shape == (6,) and np.abs(m[3:] - d).max() < 1e-12
            diff = m[:3] - p
            assert np.linalg.norm(diff - (diff @ d) * d) < 1e-12      # the mean lies on the line
            ww = np.ones(len(pts)) if w is None else w
            assert np.abs(m[:3] - (pts * ww[:, None]).sum(axis=0) / ww.sum()).max() < 1e-13
    est.refit_solver = "lapack"
    assert numpy_refit(est, pts[:1])[0] == []                            # one point: no model
    assert numpy_refit(est, pts, np.zeros(len(pts)))[0] == []            # no weight: no model
    assert len(numpy_refit(est, pts[:2])[0]) == 1                        # two points are enough
    bad = pts.copy()
    for v in (np.nan, np.inf, 1e200):                                    # a non-finite Gram matrix: no model
        bad[7, 1] = v
        with np.errstate(all="ignore"):
            assert numpy_refit(est, bad)[0] == [], v


def test_line3d_refit_sign_rule():
    est = _estimators.Line3DEstimator()
    t = np.linspace(-1, 1, 50)[:, None]
    for d, want in (([-3.0, 1.0, 2.0], [3.0, -1.0, -2.0]), ([1.0, -3.0, 2.0], [-1.0, 3.0, -2.0]), ([1.0, 2.0, -3.0], [-1.0, -2.0, 3.0]),
                    ([3.0, 1.0, -2.0], [3.0, 1.0, -2.0]), ([0.0, 0.0, -1.0], [0.0, 0.0, 1.0])):
        pts = np.array([0.5, -0.25, 2.0]) + t * np.array(d)
        for est.refit_solver in ("lapack", "jacobi"):
            (m,), _ = numpy_refit(est, pts)
            k = int(np.argmax(np.abs(m[3:])))
            assert m[3 + k] > 0, (d, m)
            assert np.abs(m[3:] - np.array(want) / np.linalg.norm(want)).max() < 1e-12, (d, m)
    # ties go to the lowest index: on eigenvectors handed over exactly (a computed one rarely ties to the bit)
    for vec, want in (([-0.6, 0.6, 0.0], [0.6, -0.6, 0.0]), ([0.6, -0.6, 0.0], [0.6, -0.6, 0.0]), ([0.0, -0.5, 0.5], [0.0, 0.5, -0.5]),
                      ([-0.5, -0.5, 0.5], [0.5, 0.5, -0.5])):
        est._direction = lambda scatter, v=vec: np.tile(np.array(v), (len(scatter), 1))
        (m,), _ = numpy_refit(est, pts)
        assert m[3:].tolist() == want


def test_line3d_fit_many_with_two_items_equals_two_single_fits():
    rng = np.random.default_rng(8)
    est = _estimators.Line3DEstimator()
    sets = [known_line(rng, 30)[0] + rng.normal(0, 0.01, (30, 3)), known_line(rng, 45)[0] + rng.normal(0, 0.01, (45, 3))]

    def G(p):
        A = np.column_stack([np.ones(len(p)), p])
        return A.T @ A

    def gram(kind, prm, use_w, wpow, rows):
        assert kind == _lib.GRAM_AFFINE and prm is None
        return np.stack([G(sets[r]) for r in rows]), np.array([len(sets[r]) for r in rows]), np.zeros(len(rows), int)
    both = est._fit_many(gram, 2, [None, None])
    assert [len(b) for b in both] == [1, 1]
    for k in range(2):
        (single,), _ = numpy_refit(est, sets[k])
        assert np.array_equal(both[k][0], single)
    # one bad item does not take its neighbour along
    sets[0] = sets[0][:1]
    mixed = est._fit_many(gram, 2, [None, None])
    assert mixed[0] == [] and np.array_equal(mixed[1][0], both[1][0])


def test_line3d_refit_against_the_50_digit_reference():
    """DESIGN.md 4.5a at the top of the spectrum: |d - d_ref| <= 32 eps lambda_max / (lambda_1 - lambda_2), and the mean's error
    perpendicular to d_ref <= tol |mean| + 4 eps |mean|.  Worst ratios measured: in docs/lab-notebook.md."""
    pytest.importorskip("mpmath")
    est = _estimators.Line3DEstimator()
    worst = [0.0, 0.0]
    for n in REFIT_N:
        for offset in (0.0, 1e3):
            for weights in (None, "mild", "wide"):
                pts, w = refit_fixture(n, offset, weights, seed=n + int(offset) + len(str(weights)))
                ref = refit_reference(pts, w)
                for est.refit_solver in ("lapack", "jacobi"):
                    (m,), _ = numpy_refit(est, pts, w)
                    rd, rm = refit_ratios(m, ref)
                    worst = [max(worst[0], rd), max(worst[1], rm)]
                    assert rd <= 1.0 and rm <= 1.0, (n, offset, weights, est.refit_solver, rd, rm)
                    assert abs(np.linalg.norm(m[3:]) - 1.0) <= 4 * EPS
    print("worst ratios (direction, mean):", worst)


# ---- the f32 filter's budget: the tests below run the restatement with the literals READ FROM score_filters.hip.h ----------------------------------------------------------------------------------------------------------
def test_line3d_filter_model_and_header_state_the_same_filter():
    """The mpmath restatement and Filter32<kLine3D> are held together: every literal of the budget and of the switch-off rules is read
    out of the header's text and equals the model's, and every statement of the f32 operation order the model restates stands in the
    header as written here.  A coefficient or a statement changed on one side only fails this; the budget tests below take their
    literals from the header, so a coefficient changed on both sides is still what they test."""
    assert header_literals() == MODEL_LITERALS
    block = " ".join(header_block().split())
    for line in OPERATION_LINES:
        assert " ".join(line.split()) in block, line
    assert "static constexpr int kRowVals = 6, kGroupVals = 5;" in block and "static constexpr int kStagedVals = 10;" in block


def _random_line(rng, coord, offset):
    d = rng.normal(size=3)
    d /= np.linalg.norm(d)
    return np.concatenate([rng.uniform(3, 7, 3) * coord + offset, d])


def _near_threshold_pairs(plant_zero_budget=False, per_case=70):
    """(pairs in the band, FP64 inliers among them, FP64 inliers rejected): coordinate scales 1, 1e3, 1e6, scenes at the origin, 1e3
    scene scales and 1e6 units from it, thresholds 1e-3 .. 1e3 x nominal, d scaled by 2^-40 .. 2^40 (the threshold along: r scales
    with |d|)"""
    rng = np.random.default_rng(29)
    lit = header_literals()
    band = inl = wrong = 0
    for coord in (1.0, 1e3, 1e6):
        for offset in (0.0, 1e3 * coord, 1e6):
            for tf in (1e-3, 1.0, 1e3):
                for e in (-40, 0, 40):
                    gt = _random_line(rng, coord, offset)
                    T = 1.5 * 0.05 * coord * tf
                    pts = near_threshold_points(rng, gt, T, per_case, 5.0 * coord)
                    hyp = gt.copy()
                    if rng.random() < 0.5:
                        hyp[:3] += rng.normal(0, 1e-6 * T, 3)
                    hyp[3:] *= 2.0 ** e
                    T2 = (T * 2.0 ** e) ** 2
                    sq = sq_line3d(pts, hyp)
                    ln = prep(hyp, max(1.0, np.abs(pts).max()), T2, plant_zero_budget, lit=lit)
                    for x, s in zip(pts, sq):
                        if not abs(s / T2 - 1.0) < 1e-4:
                            continue
                        band += 1
                        if s < T2:
                            inl += 1
                            wrong += reject(point_row(x), ln)
    return band, inl, wrong


def test_line3d_filter_rejects_no_inlier_near_the_threshold():
    pytest.importorskip("mpmath")
    band, inl, wrong = _near_threshold_pairs()
    assert band >= 5000 and inl >= 2000, (band, inl)
    assert wrong == 0


def test_line3d_filter_without_its_budget_is_caught():
    """E planted as 0: scenes far from the origin put the f32 rounding of the coordinates above the 2^-6 margin of the threshold, and
    the check above sees inliers rejected"""
    pytest.importorskip("mpmath")
    band, inl, wrong = _near_threshold_pairs(plant_zero_budget=True, per_case=20)
    assert inl > 0 and wrong > 0


def test_line3d_filter_rejects_generic_pairs():
    pytest.importorskip("mpmath")
    rng = np.random.default_rng(4)
    pts = rng.uniform(0, 10, (1500, 3))
    T = 1.5 * 0.05
    rej = tot = 0
    for k in range(3):
        hyp = _random_line(rng, 1.0, 0.0)
        hyp[3:] *= (1.0, 2.0 ** -40, 7.0)[k]
        T2 = (T * np.linalg.norm(hyp[3:])) ** 2
        ln = prep(hyp, 10.0, T2, lit=header_literals())
        sq = sq_line3d(pts, hyp)
        for x, s in zip(pts[500 * k:500 * (k + 1)], sq[500 * k:500 * (k + 1)]):
            r = reject(point_row(x), ln)
            assert not (r and s < T2)
            rej += r
            tot += 1
    assert rej > 0.99 * tot
    # what must never be rejected: a zero direction (every residual is 0), Inf entries, a direction outside the normaliser's band,
    # thresholds outside the f32 range, points and coordinates beyond 1e17
    gt = _random_line(rng, 1.0, 0.0)
    for hyp, T2, pscale in ((np.concatenate([gt[:3], np.zeros(3)]), T * T, 10.0), (np.concatenate([gt[:3], [np.inf, 0.0, 0.0]]), T * T, 10.0),
                            (np.concatenate([[np.inf, 0.0, 0.0], gt[3:]]), T * T, 10.0), (np.concatenate([gt[:3], gt[3:] * 1e-80]), T * T, 10.0),
                            (gt, 1e-70, 10.0), (gt, 1e70, 10.0), (np.concatenate([gt[:3] * 1e18, gt[3:]]), T * T, 10.0), (gt, T * T, 1e18)):
        ln = prep(hyp, pscale, T2, lit=header_literals())
        assert ln["e0"] == np.inf and ln["nanh"] == 0.0
        assert not any(reject(point_row(x), ln) for x in pts[:20])
        assert not group_reject(group_row(pts[:64]), ln)
    nan = gt.copy()
    for k in range(6):                                       # a NaN entry: no pair is rejected (the exact path gives NaN), the group is culled
        nan[:] = gt
        nan[k] = np.nan
        ln = prep(nan, 10.0, T * T, lit=header_literals())
        assert ln["nanh"] == 1.0 and group_reject(group_row(pts[:64]), ln)
        assert not any(reject(point_row(x), ln) for x in pts[:20])
        assert np.isnan(sq_line3d(pts[:20], nan)).all()


def test_line3d_group_bound_rejects_no_group_with_an_inlier():
    pytest.importorskip("mpmath")
    rng = np.random.default_rng(6)
    groups = rejected = 0
    for coord, offset, tf in ((1.0, 0.0, 1.0), (1e3, 0.0, 1e-3), (1.0, 1e3, 1.0), (1e6, 1e6, 1.0)):
        base, _, gt = datasets.make_lines3d(n_per_line=600, n_lines=3, n_outliers=64 * 55 - 1800, sigma=0.01, seed=int(coord) % 7)
        pts = base * coord + offset
        pts = np.ascontiguousarray(pts[morton_order(pts)])
        T = 1.5 * 0.05 * coord * tf
        hyps = []
        for g in gt[:2]:
            h = np.concatenate([g[:3] * coord + offset, g[3:]])
            hyps += [h, np.concatenate([h[:3], h[3:] * 2.0 ** 40]), h + np.concatenate([rng.normal(0, 0.3 * coord, 3), rng.normal(0, 0.05, 3)])]
        hyps.append(_random_line(rng, coord, offset))
        pscale = max(1.0, np.abs(pts).max())
        for h in hyps:
            T2 = (T * (2.0 ** 40 if np.linalg.norm(h[3:]) > 1e6 else 1.0)) ** 2
            ln = prep(h, pscale, T2, lit=header_literals())
            sq = sq_line3d(pts, h)
            for g0 in range(0, len(pts), 64):
                groups += 1
                if group_reject(group_row(pts[g0:g0 + 64]), ln):
                    rejected += 1
                    assert not (sq[g0:g0 + 64] < T2).any(), (coord, offset, tf, g0)
    assert groups >= 200 * 4 and rejected > 0.5 * groups, (groups, rejected)


# ---- the generator ------------------------------------------------------------------------------------------------------------------
def test_make_lines3d_is_seeded_and_its_inliers_lie_on_their_lines():
    kw = dict(n_per_line=2000, n_lines=4, n_outliers=300, sigma=0.02)
    a = datasets.make_lines3d(seed=3, **kw)
    b = datasets.make_lines3d(seed=3, **kw)
    c = datasets.make_lines3d(seed=4, **kw)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    assert not np.array_equal(a[0], c[0])
    pts, labels, gt = a
    assert pts.shape == (8300, 3) and pts.dtype == np.float64 and labels.shape == (8300,) and labels.dtype == np.int32
    assert gt.shape == (4, 6) and gt.dtype == np.float64
    assert np.bincount(labels).tolist() == [300, 2000, 2000, 2000, 2000]
    assert np.abs(np.linalg.norm(gt[:, 3:], axis=1) - 1.0).max() < 1e-15
    for j in range(4):
        on = pts[labels == j + 1]
        r = np.sqrt(sq_line3d(on, gt[j]))
        assert abs(r.mean() - 0.02 * np.sqrt(np.pi / 2)) < 0.15 * 0.02 * np.sqrt(np.pi / 2)     # Rayleigh: isotropic noise
        t = (on - gt[j, :3]) @ gt[j, 3:]
        half = 0.5 * (t.max() - t.min())
        assert 2.0 - 0.1 <= half <= 5.0 + 0.1 and abs(t.mean()) < 0.1 * half                   # length in (4, 10), about the midpoint
        ends = gt[j, :3] + np.array([[-1.0], [1.0]]) * (half - 0.1) * gt[j, 3:]
        assert ((ends >= 0) & (ends <= 10.0)).all()                                              # the segment lies inside the box
    out = pts[labels == 0]
    assert ((out >= 0) & (out <= 10.0)).all()
    d = datasets.make_lines3d()
    assert d[0].shape == (24000, 3) and d[2].shape == (6, 6) and np.bincount(d[1]).tolist() == [12000] + [2000] * 6
    with pytest.raises(ValueError, match="length"):
        datasets.make_lines3d(length=(4.0, 20.0))
