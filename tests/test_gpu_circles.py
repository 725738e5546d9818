"""findCircles on the MI355X: every layer of the 2-D circle type against a numpy restatement of its arithmetic written next to the
kernels (scoring, the culls and the f32 filter, the pointwise kernels, the 3-point solver, the Gram rows of the refit), and the
public call end to end.

Residual<kCircle2D> (residuals.hip.h) is the contract: dx = x - cx, dy = y - cy, r = |sqrt(dx dx + dy dy) - cr|, r^2 = r * r,
inlier iff r^2 < T2."""
import numpy as np
import pytest

import pyprogressivex as px
from pyprogressivex import _estimators, _lib, _rng, datasets, parallel
from primitive_helpers import _check_recovery, _check_scores, _want, ref_score, shuffled

pytestmark = pytest.mark.gpu

THR = 2.0                       # findCircles' default threshold (pixels)
T2_NOMINAL = 2.25 * THR * THR


def dist(pts, m):
    dx, dy = pts[:, 0] - m[0], pts[:, 1] - m[1]
    return np.sqrt(dx * dx + dy * dy)


def sq_circle(pts, m):
    with np.errstate(invalid="ignore", over="ignore"):
        r = np.abs(dist(pts, m) - m[2])
        return r * r


def make_problem(n, M, seed):
    """points of make_circles (truncated to n) and M hypotheses: ground truth, perturbed (1e-7 .. 1 pixel), random, scene-scaled
    copies and the special ones r = 0, r < 0, r = inf, one NaN entry and an all-NaN model"""
    rng = np.random.default_rng(seed)
    k = max(n // 8, 1)
    pts, _, gt = datasets.make_circles(n_per_circle=k, n_circles=4, n_outliers=max(n - 4 * k, 1), seed=seed)
    pts = np.ascontiguousarray(pts[rng.permutation(pts.shape[0])[:n]])
    models = np.empty((M, 3))
    for j in range(M):
        kind = j % 5
        g = gt[j % len(gt)]
        if kind == 1:
            models[j] = g + rng.normal(0, 10.0 ** rng.uniform(-7, 0), 3)
        elif kind == 2:
            models[j] = np.append(rng.uniform(0, 1000.0, 2), rng.uniform(10.0, 600.0))
        elif kind == 3:
            models[j] = g * rng.choice([1e-3, 2.0 ** -40, 0.5, 7.0, 1e5])     # the scene's circle scaled about the origin
        else:
            models[j] = g
    if M >= 5:
        models[M - 1] = np.nan
        models[M - 2] = np.append(gt[0, :2], 0.0)            # r = 0: the residual is the distance from the centre
        models[M - 3] = np.append(gt[1, :2], -gt[1, 2])      # r < 0: every residual is s + |r|
        models[M - 4] = np.append(gt[2, :2], np.inf)         # r = inf: never an inlier
        models[M - 5, 1] = np.nan
    return pts, models


@pytest.mark.parametrize("n", [1, 63, 64, 65, 5000])
@pytest.mark.parametrize("M", [1, 7, 256])
def test_circle_scoring_bit_exact(gpu_ctx, n, M):
    pts, models = make_problem(n, M, seed=n + M)
    T2 = T2_NOMINAL
    if n >= 5000 and M >= 7:                                # a point exactly on the threshold: r^2 == T2 is not an inlier
        on = int(np.flatnonzero(sq_circle(pts, models[0]) > 0)[0])
        T2 = float(sq_circle(pts[on:on + 1], models[0])[0])
        assert T2 > 0
    comp = np.random.default_rng(n).uniform(0, 1, n)
    gpu_ctx.score_set_global_n(0)
    gpu_ctx.set_points(_lib.CIRCLE2D, pts)
    gpu_ctx.set_compound(comp)
    got = gpu_ctx.score(models, T2, has_compound=True, exponent=2, want_masks=True)
    ref = ref_score(sq_circle, pts, models, T2, comp)
    if n >= 5000 and M >= 7:
        assert not (ref["masks"][0, on >> 6] >> np.uint64(on & 63)) & np.uint64(1)
    _check_scores(got, ref)
    nomask = gpu_ctx.score(models, T2, has_compound=True, exponent=2)
    assert np.array_equal(nomask["counts"], ref["counts"])
    st = gpu_ctx.score_stats(T2, has_compound=True)
    if st["path"] == "cull + group-major":
        acc = gpu_ctx.score_accumulators()
        for k in ("counts", "values_q", "shared_q"):
            assert np.array_equal(acc[k].astype(np.int64), ref[k]), k
        q = parallel.fixed_point_scale(n)
        assert np.array_equal(nomask["values"], ref["values_q"].astype(np.float64) / q)


@pytest.fixture(scope="module")
def cull_problem():
    """one problem and its numpy reference for every switch of test_circle_culls_are_invisible"""
    pts, models = make_problem(30011, 300, seed=11)
    comp = np.random.default_rng(2).uniform(0, 1, pts.shape[0])
    return pts, models, comp, ref_score(sq_circle, pts, models, T2_NOMINAL, comp)


@pytest.mark.parametrize("switch", [None, "PGX_NO_FILTER", "PGX_SCORE_NO_CULL", "PGX_NO_GROUP", "PGX_NO_SORT", "PGX_SETPOINTS_HOST"])
def test_circle_culls_are_invisible(switch, monkeypatch, cull_problem):
    pts, models, comp, ref = cull_problem
    T2 = T2_NOMINAL
    if switch:
        monkeypatch.setenv(switch, "1")
    ctx = _lib.Context(0)
    if switch:
        monkeypatch.delenv(switch)
    try:
        ctx.set_points(_lib.CIRCLE2D, pts)
        ctx.set_compound(comp)
        got = ctx.score(models, T2, has_compound=True, want_masks=True)
        _check_scores(got, ref)
        ctx.score(models, T2, has_compound=True)
        st = ctx.score_stats(T2, has_compound=True)
        if st["path"] == "cull + group-major":
            ctx.score(models, T2, has_compound=True)
            acc = ctx.score_accumulators()
            for k in ("counts", "values_q", "shared_q"):
                assert np.array_equal(acc[k].astype(np.int64), ref[k]), k
        else:
            assert switch is not None
        if switch is None:                                   # the cull and the f32 filter ran, and the launch geometry does not matter
            assert st["filter"] == "f32" and st["surviving_group_steps"] < st["group_pairs"]
            for geo in (dict(split=3), dict(group_xcd=1), dict(nrep=16), dict(dense_min=1), dict(cull_segs=5)):
                ctx.score_debug_geometry(**geo)
                ctx.score(models, T2, has_compound=True)
                acc = ctx.score_accumulators()
                for k in ("counts", "values_q", "shared_q"):
                    assert np.array_equal(acc[k].astype(np.int64), ref[k]), (geo, k)
    finally:
        ctx.close()


def test_circle_filter_proof_near_threshold(monkeypatch):
    """Points moved along the radius until |r^2 / T^2 - 1| < 1e-4, on both faces of the circle, with coordinate offsets up to 1e6,
    thresholds 1e-3 .. 1e3 x nominal, radii 1e-3 .. 1e3 and scene scales 2^-40 .. 2^40: PGX_VERIFY=1 counts every inlier the group
    bound or the f32 filter removed - none may be."""
    monkeypatch.setenv("PGX_VERIFY", "1")
    ctx = _lib.Context(0)
    monkeypatch.delenv("PGX_VERIFY")
    rng = np.random.default_rng(23)
    f32_seen = 0
    try:
        for off in (0.0, 1e3, 1e6):
            for tf in (1e-3, 1.0, 1e3):
                for radius, scale in ((1.0, 1.0), (1e-3, 1.0), (1e3, 1.0), (1.0, 2.0 ** -40), (1.0, 2.0 ** 40)):
                    n = 20000
                    c = (rng.uniform(3, 7, 2) + off) * scale
                    R = radius * scale
                    T = 1.5 * 0.05 * tf * scale
                    phi = rng.uniform(0, 2 * np.pi, n)
                    d = np.column_stack([np.cos(phi), np.sin(phi)])
                    target = T * (1.0 + rng.uniform(-0.99e-4 / 2, 0.99e-4 / 2, n))
                    side = np.where((rng.random(n) < 0.5) & (R - 1.01 * T > 0), -1.0, 1.0)   # inner face where there is one
                    pts = np.ascontiguousarray(c + d * (R + side * target)[:, None])
                    pts[n // 2:] = c + rng.uniform(-3, 3, (n - n // 2, 2)) * max(R, T)       # and some points off the circle
                    gt = np.append(c, R)
                    hyps = np.empty((64, 3))
                    for k in range(64):
                        hyps[k] = gt + (rng.normal(0, 1e-12, 3) * np.abs(gt) if k % 2 else 0.0)
                    hyps[5, 2] = -R
                    hyps[7] = np.append(c + rng.normal(0, R, 2), R * rng.uniform(0.5, 2.0))
                    ctx.set_points(_lib.CIRCLE2D, pts)
                    ctx.score_upload(hyps)
                    st = ctx.score_stats(T * T)
                    assert st["contradictions"] == 0, (off, tf, radius, scale, st)
                    got = ctx.score(hyps, T * T, want_masks=True)
                    ref = ref_score(sq_circle, pts, hyps, T * T)
                    assert np.array_equal(got["counts"], ref["counts"]) and np.array_equal(got["masks"], ref["masks"])
                    assert ref["counts"][0] > 0
                    f32_seen += st["filter"] == "f32"
        assert f32_seen > 0
    finally:
        ctx.close()


def test_circle_pointwise_kernels_bit_exact(gpu_ctx):
    """preference, the PEARL unary table, the labelling energy on it, the label buckets and the residual sums"""
    pts, models = make_problem(20011, 8, seed=3)
    n = pts.shape[0]
    thr, lam = THR, 0.3
    T2 = T2_NOMINAL
    gpu_ctx.set_points(_lib.CIRCLE2D, pts)
    gpu_ctx.set_compound(None)
    for k in (0, 1, 2):
        pref = gpu_ctx.preference(models[k], T2, slot=k, want_pref=True)["pref"]
        assert np.array_equal(pref, np.maximum(0.0, 1.0 - sq_circle(pts, models[k]) / T2))
    assert np.isnan(models[3]).any() and np.isinf(models[4, 2])     # the unary table below holds a NaN model and r = inf
    K = 5
    Dq = gpu_ctx.pearl_unary(models[:K], thr, lam, want_table=True)
    oml = 1.0 - lam
    ref = np.empty((n, K + 1), np.int64)
    for k in range(K):
        sq = sq_circle(pts, models[k])
        with np.errstate(invalid="ignore"):
            c = np.where(sq > T2, 2.0 * oml, oml * sq / T2)
        c = np.where(np.isnan(c), 2.0 * oml, c)
        ref[:, k] = np.rint(c * 4294967296.0).astype(np.int64)
    ref[:, K] = np.int64(np.rint(oml * 4294967296.0))
    assert np.array_equal(Dq, ref)
    # energy of a labelling on that table: data terms + lambda_q per arc (j < i) between different labels + h_q per label in use
    off, idx, mult = gpu_ctx.graph_build(pts, _lib.GRAPH_KNN_IN_BALL, radius=20.0, k=5)
    labels = np.random.default_rng(1).integers(0, K + 1, n).astype(np.int32)
    gpu_ctx.set_labels(labels)
    h = 0.01
    lam_q, h_q = 2 * int(np.rint(lam * 2147483648.0)), int(np.rint(h * 4294967296.0))
    site = np.repeat(np.arange(n), np.diff(off))
    cut = (idx < site) & (labels[idx] != labels[site])
    want = int(ref[np.arange(n), labels].sum()) + lam_q * int(mult[cut].astype(np.int64).sum()) + h_q * len(np.unique(labels))
    eq, e = gpu_ctx.energy(lam, h)
    assert eq == want and e == want / 2.0 ** 32 and cut.sum() > 0
    # buckets (labels >= L - 1 fall into the last one; ascending point index inside a bucket)
    for L in (K + 1, 4):
        clipped = np.minimum(labels, L - 1)
        counts, order = gpu_ctx.bucket(L)
        assert np.array_equal(counts, np.bincount(clipped, minlength=L))
        assert np.array_equal(order, np.argsort(clipped, kind="stable"))
    lab4 = (labels % 4).astype(np.int32)
    gpu_ctx.set_labels(lab4)
    finite = models[[0, 1, 2, 5]]                            # (model 3 holds a NaN, model 4 has r = inf)
    sums = gpu_ctx.residual_sums(finite)
    for k in range(4):
        r = np.sqrt(sq_circle(pts[lab4 == k], finite[k]))
        assert abs(sums[k] - r.sum()) <= 1e-12 * max(abs(r.sum()), 1e-300)
        assert abs(gpu_ctx.residual_sum(finite[k], k) - r.sum()) <= 1e-12 * max(abs(r.sum()), 1e-300)


@pytest.fixture(scope="module")
def solver_points():
    pts, _, _ = datasets.make_circles(n_per_circle=500, n_circles=3, n_outliers=500, seed=2)
    pts = pts.copy()
    pts[5] = pts[4]                                          # duplicate points
    pts[8:11] = [[1.0, 1.0], [2.0, 2.0], [4.0, 4.0]]         # exactly collinear
    return pts


@pytest.mark.parametrize("S", [1, 64, 1000])
def test_circle_minimal_solver_bitwise_the_estimator(gpu_ctx, solver_points, S):
    pts = solver_points
    n = pts.shape[0]
    est = _estimators.CircleEstimator()
    gpu_ctx.set_points(_lib.CIRCLE2D, pts)
    gpu_ctx.set_radius_range()
    samples = np.random.default_rng(S).integers(0, n, (S, 3)).astype(np.int32)
    special = np.array([[4, 5, 6], [1, 1, 2], [8, 9, 10], [-1, 2, 3], [n, 0, 1]], np.int32)[:min(S - 1, 5)]
    samples[:len(special)] = special                         # (S = 1: the one sample is an ordinary one)
    got = gpu_ctx.solve_minimal(samples)
    assert got.shape == (S, 3)
    assert np.array_equal(got, _want(est, pts, samples, S), equal_nan=True)
    assert np.isnan(got[:len(special)]).all() and np.isfinite(got[len(special):]).all(1).mean() > 0.9
    if len(special):
        assert (gpu_ctx.score(got[:len(special)], T2_NOMINAL)["counts"] == 0).all()
    # the radius range (bounds inclusive): set, then reset - the second call gives the fresh result
    finite = got[np.isfinite(got).all(1), 2]
    lo, hi = (np.sort(finite)[[len(finite) // 4, (3 * len(finite)) // 4]] if len(finite) > 4 else (finite[0], finite[0]))
    est.radius_range = (float(lo), float(hi))
    gpu_ctx.set_radius_range(float(lo), float(hi))
    ranged = gpu_ctx.solve_minimal(samples)
    assert np.array_equal(ranged, _want(est, pts, samples, S), equal_nan=True)
    r = ranged[np.isfinite(ranged).all(1), 2]
    assert ((r >= lo) & (r <= hi)).all() and lo in r and hi in r
    if S > 4:
        assert len(r) < len(finite)
    gpu_ctx.set_radius_range()
    assert np.array_equal(gpu_ctx.solve_minimal(samples), got, equal_nan=True)


def test_circle_device_drawn_samples_equal_the_generator(gpu_ctx, solver_points):
    """pgx_solve_minimal_sampled with m = 3: the rows are _rng's for the uniform, NAPSAC and PROSAC samplers, the models the solver's"""
    pts = solver_points
    n = pts.shape[0]
    est = _estimators.CircleEstimator()
    gpu_ctx.set_points(_lib.CIRCLE2D, pts)
    off, idx, _ = gpu_ctx.graph_build(pts, _lib.GRAPH_KNN_IN_BALL, radius=60.0, k=5)
    tops = np.minimum(n, np.arange(3, 3 + 512)).astype(np.int32)
    gpu_ctx.sampler_prosac_set(tops)
    want_rows = dict(uniform=_rng.uniform_samples(12345, 7, 512, n, 3), napsac=_rng.napsac_samples(12345, 7, 512, n, 3, off, idx),
                     prosac=_rng.prosac_samples(12345, 7, 512, n, 3, tops))
    for rr in ((0.0, np.inf), (40.0, 150.0)):
        est.radius_range = rr
        gpu_ctx.set_radius_range(*rr)
        for sampler in ("uniform", "napsac", "prosac"):
            models, smp = gpu_ctx.solve_minimal_sampled(12345, 7, 512, fetch_samples=True, sampler=sampler)
            assert smp.shape == (512, 3) and (smp >= 0).all(1).sum() > 0
            assert np.array_equal(smp, want_rows[sampler].astype(np.int32)), sampler
            assert np.array_equal(models, _want(est, pts, smp, 512), equal_nan=True), (sampler, rr)
    gpu_ctx.set_radius_range()


def test_circle_refit_grams(gpu_ctx):
    pts, labels, gt = datasets.make_circles(n_per_circle=15000, n_circles=3, n_outliers=21000, seed=6)
    n = pts.shape[0]
    assert n == 66000                                        # index lists of 65 536 | 65 537 entries: both sides of the fused upload
    w = np.random.default_rng(1).uniform(0.5, 2.0, n)
    gpu_ctx.set_points(_lib.CIRCLE2D, pts)

    def rows(prm, sel):
        q = (pts[sel] - prm[:2]) / prm[2]
        return np.column_stack([np.ones(len(q)), q, q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]])

    def close(G, Gr):
        return np.abs(G - Gr).max() <= 1e-12 * np.abs(Gr).max()

    prms = np.array([[400.0, 500.0, 150.0], [100.0, -200.0, 300.0], [0.0, 0.0, 1.0], [500.0, 500.0, 25.0]])
    idx = np.stack([np.random.default_rng(s).choice(n, 300, replace=False) for s in range(4)]).astype(np.int32)
    for ww in (w, None):
        Gb, bad = gpu_ctx.gram_batch(_lib.GRAM_CIRCLE, idx, params=prms, weights=ww, wpow=1)
        assert Gb.shape == (4, 4, 4)
        for b in range(4):
            G, cnt, _ = gpu_ctx.gram(_lib.GRAM_CIRCLE, ("index", idx[b]), params=prms[b], weights=ww, wpow=1)
            A = rows(prms[b], idx[b])
            Gr = (A * (1.0 if ww is None else ww[idx[b], None])).T @ A
            assert cnt == 300 and not bad[b] and G.shape == (4, 4)
            assert close(G, Gr) and close(Gb[b], Gr)
    perm = np.random.default_rng(9).permutation(n).astype(np.int32)
    for m in (65536, 65537):
        for ww in (w, None):
            G, cnt, bad = gpu_ctx.gram(_lib.GRAM_CIRCLE, ("index", perm[:m]), params=prms[0], weights=ww, wpow=1)
            A = rows(prms[0], perm[:m])
            Gr = (A * (1.0 if ww is None else ww[perm[:m], None])).T @ A
            assert (cnt, bad) == (m, 0) and close(G, Gr), m
    gpu_ctx.set_labels(labels)
    for ww in (w, None):
        GL, cntL, _ = gpu_ctx.gram_labels(_lib.GRAM_CIRCLE, 4, params=prms, weights=ww, wpow=1)
        for k in range(4):
            G, cnt, _ = gpu_ctx.gram(_lib.GRAM_CIRCLE, ("label", k), params=prms[k], weights=ww, wpow=1)
            sel = labels == k
            A = rows(prms[k], sel)
            Gr = (A * (1.0 if ww is None else ww[sel, None])).T @ A
            assert cnt == cntL[k] == sel.sum() and np.array_equal(G, GL[k])
            assert close(G, Gr)
    # the row kind needs 2-D points and exactly three parameters
    with pytest.raises(_lib.PgxError):
        gpu_ctx.gram(_lib.GRAM_CIRCLE, ("label", 1), params=np.array([1.0, 2.0, 3.0, 4.0]))
    with pytest.raises(_lib.PgxError):
        gpu_ctx.gram(_lib.GRAM_SPHERE, ("label", 1), params=np.array([1.0, 2.0, 3.0, 4.0]))
    # the refits: LAPACK and the device's Jacobi solver agree, and both find the circles
    est = _estimators.CircleEstimator()
    lap = est.nonminimal_labels(gpu_ctx, 4, weights=w)
    est.refit_solver = "jacobi"
    jac = est.nonminimal_labels(gpu_ctx, 4, weights=w)
    for k, (a, b) in enumerate(zip(lap[1:], jac[1:])):
        assert len(a) == len(b) == 1
        assert np.abs(a[0] - b[0]).max() < 1e-10 * 1000.0    # (the sphere test's 1e-10 at its 10 m scene, here on 1000 pixels)
        assert np.abs(a[0] - gt[k]).max() < 0.5
    one = est.nonminimal(gpu_ctx, ("label", 1), weights=w)
    assert np.abs(one[0] - jac[1][0]).max() < 1e-10 * 1000.0
    batch = est.nonminimal_batch(gpu_ctx, idx)               # the batched form runs the same statement of the refit
    assert len(batch) == 4


# minimum_point_number: a spurious circle through the uniform outliers collects those inside its annulus of width 3 x threshold = 6
# pixels; the largest that fits the 1000 x 1000 box (r = 500) covers 2 pi 500 * 6 = 1.9 % of it - about 150 of 8 000 outliers.  The true
# circles have 2 000 inliers each.  It also has to stay below what the run's stop rule predicts as unseen: after three
# of four circles and at most 3 000 iterations that is 6.1 % of the 10 000 uncovered points, 614.
MPN = 300


def test_find_circles_end_to_end():
    """The issue's scene: four circles of 2 000 points, as many uniform outliers as inliers, half a pixel of noise, every default."""
    sigma = 0.5
    pts, gen, gt = datasets.make_circles(n_per_circle=2000, n_circles=4, n_outliers=8000, sigma=sigma, seed=0)
    assert pts.shape == (16000, 2)
    pts, gen = shuffled(pts, gen)
    kw = dict(minimum_point_number=MPN, seed=1)
    circles, labels = px.findCircles(pts, **kw)
    _check_recovery(circles, labels, pts, gen, gt, THR, sigma)
    circles2, labels2 = px.findCircles(pts, **kw)
    assert np.array_equal(circles, circles2) and np.array_equal(labels, labels2)
    # refit_solver="jacobi": the eigenvectors agree with LAPACK's to ~1e-13, which a refit turns into < 1e-8 pixel on these
    # coordinates.  A point whose two best labels tie within that may change sides, and one point entering or leaving the 3-pixel band
    # of a circle with 2 000 inliers moves its fit by up to 3 / 2000 = 1.5e-3 pixel: the two runs agree within a handful of such points.
    cj, lj = px.findCircles(pts, **kw, refit_solver="jacobi")
    assert cj.shape == circles.shape and np.abs(cj - circles).max() < 1e-2
    assert np.mean(lj != labels) < 1e-3
    _check_recovery(cj, lj, pts, gen, gt, THR, sigma)
    # a call with a radius range leaves nothing behind: the next call without one is the fresh result
    px.findCircles(pts, **kw, radius_range=(10.0, 60.0))
    circles3, labels3 = px.findCircles(pts, **kw)
    assert np.array_equal(circles, circles3) and np.array_equal(labels, labels3)


def test_find_circles_on_half_coverage_arcs():
    """Three circles of which half the circumference is seen."""
    sigma = 0.5
    pts, gen, gt = datasets.make_circles(n_per_circle=2000, n_circles=3, n_outliers=6000, sigma=sigma, coverage=0.5, seed=4)
    pts, gen = shuffled(pts, gen)
    circles, labels = px.findCircles(pts, minimum_point_number=MPN, seed=2)
    _check_recovery(circles, labels, pts, gen, gt, THR, sigma)


def test_find_circles_in_a_mixed_scene():
    """make_lines (3 lines) + make_circles (3 circles): with radius_range=(20, 200) exactly the three circles come back.  An arc of
    radius 200 stays inside a line's 6-pixel band over a chord of sqrt(8 * 200 * 6) = 98 pixels; the shortest line (240 pixels, 600
    points) has 245 points on that - under minimum_point_number."""
    sigma = 0.5
    pl, _, _ = datasets.make_lines(n_per_line=600, n_lines=3, n_outliers=0, sigma=sigma, seed=5)
    pc, gc, gt = datasets.make_circles(n_per_circle=2000, n_circles=3, n_outliers=6000, sigma=sigma, seed=6)
    pts = np.ascontiguousarray(np.vstack([pl, pc]))
    gen = np.concatenate([np.zeros(len(pl), np.int32), gc])
    pts, gen = shuffled(pts, gen)
    circles, labels = px.findCircles(pts, minimum_point_number=MPN, radius_range=(20.0, 200.0), seed=3)
    assert circles.shape == (3, 3)
    for g in gt:
        k = int(np.argmin(np.linalg.norm(circles[:, :2] - g[:2], axis=1)))
        assert np.linalg.norm(circles[k, :2] - g[:2]) < 2 * sigma and abs(circles[k, 2] - g[2]) < 2 * sigma
    assert ((circles[:, 2] >= 20.0) & (circles[:, 2] <= 200.0)).all()
    on = labels < 3
    assert (gen[on] > 0).mean() > 0.9                    # the circles' labels are on the circles' points


def test_the_numpy_restatement_and_the_oracle_are_the_same_witness(oracle):
    """sq_circle above (numpy, written next to the kernels) and the C oracle's squared_residuals (pinned against exact arithmetic in
    tests/test_oracle.py) agree bit for bit on every point and hypothesis of make_problem(5000, 256, ...), the special models
    (r = 0, r < 0, r = inf, NaN) included: the two witnesses the circle kernels are held to say the same"""
    pts, models = make_problem(5000, 256, seed=12)
    for m in models:
        assert np.array_equal(sq_circle(pts, m), oracle.squared_residuals(oracle.CIRCLE2D, pts, m), equal_nan=True)
