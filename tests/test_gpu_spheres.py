"""findSpheres on the MI355X: every layer of the 3-D sphere type against a numpy restatement of its arithmetic written next to the
kernels, and against the oracle where the step is model-agnostic (the neighbourhood graph, alpha-expansion on a given table).  The CPU
oracle has its own sphere rows since (oracle/pgx_oracle.c, checked against exact arithmetic in tests/test_oracle.py): the per-type
sweeps of tests/test_gpu_parity.py, the API / replay files and the soaks hold the device to those; this file stays as a second,
numpy-side statement of the same contract.

Residual<kSphere3D> (residuals.hip.h) is the contract: dx = x - cx, dy = y - cy, dz = z - cz,
r = |sqrt((dx dx + dy dy) + dz dz) - cr|, r^2 = r * r, inlier iff r^2 < T2."""
import numpy as np
import pytest

import pyprogressivex as px
from pyprogressivex import _estimators, _lib, _rng, datasets, parallel
from primitive_helpers import _check_recovery, _check_scores, _want, ref_score, shuffled

pytestmark = pytest.mark.gpu


def dist(pts, m):
    dx, dy, dz = pts[:, 0] - m[0], pts[:, 1] - m[1], pts[:, 2] - m[2]
    return np.sqrt((dx * dx + dy * dy) + dz * dz)


def sq_sphere(pts, m):
    with np.errstate(invalid="ignore", over="ignore"):
        r = np.abs(dist(pts, m) - m[3])
        return r * r


def make_problem(n, M, seed, scale=1.0):
    """points of make_spheres (truncated / padded to n) and M hypotheses: ground truth, perturbed, random, scene-scaled copies
    (other spheres of the same scene family) and the special ones r = 0, r < 0, r = inf and NaN"""
    rng = np.random.default_rng(seed)
    k = max(n // 8, 1)
    pts, _, gt = datasets.make_spheres(n_per_sphere=k, n_spheres=4, n_outliers=max(n - 4 * k, 1), seed=seed)
    pts = np.ascontiguousarray(pts[rng.permutation(pts.shape[0])[:n]] * scale)
    gt = gt * scale
    models = np.empty((M, 4))
    for j in range(M):
        kind = j % 5
        g = gt[j % len(gt)]
        if kind == 0:
            models[j] = g
        elif kind == 1:
            models[j] = g + rng.normal(0, 10.0 ** rng.uniform(-9, -2), 4) * scale
        elif kind == 2:
            models[j] = np.append(rng.uniform(0, 10 * scale, 3), rng.uniform(0.1, 6.0) * scale)
        elif kind == 3:
            models[j] = g * rng.choice([1e-3, 2.0 ** -40, 0.5, 7.0, 1e5])     # the scene's sphere scaled about the origin
        else:
            models[j] = g
    if M >= 5:
        models[M - 1] = np.nan
        models[M - 2] = np.append(gt[0, :3], 0.0)            # r = 0
        models[M - 3] = np.append(gt[1, :3], -gt[1, 3])      # r < 0: every residual is s + |r|
        models[M - 4] = np.append(gt[2, :3], np.inf)         # r = inf: never an inlier
        models[M - 5, 1] = np.nan
    return pts, models


@pytest.mark.parametrize("n", [1, 63, 64, 65, 5000, 200000])
@pytest.mark.parametrize("M", [1, 7, 256, 2048])
def test_sphere_scoring_bit_exact(gpu_ctx, n, M):
    pts, models = make_problem(n, M, seed=n + M)
    thr = 0.05
    T2 = 2.25 * thr * thr
    if n >= 5000 and M >= 7:                                # a point exactly on the threshold: r^2 == T2 is not an inlier
        T2 = float(sq_sphere(pts[3:4], models[0])[0])
        assert T2 > 0
    comp = np.random.default_rng(n).uniform(0, 1, n)
    gpu_ctx.score_set_global_n(0)
    gpu_ctx.set_points(_lib.SPHERE3D, pts)
    gpu_ctx.set_compound(comp)
    got = gpu_ctx.score(models, T2, has_compound=True, exponent=2, want_masks=True)
    ref = ref_score(sq_sphere, pts, models, T2, comp)
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
    if n >= 100000:
        assert st["path"] == "cull + group-major" and st["filter"] == "f32"


@pytest.mark.parametrize("switch", [None, "PGX_NO_FILTER", "PGX_SCORE_NO_CULL", "PGX_NO_GROUP", "PGX_NO_SORT", "PGX_SETPOINTS_HOST"])
def test_sphere_culls_are_invisible(switch, monkeypatch):
    pts, models = make_problem(30011, 300, seed=11)
    T2 = 2.25 * 0.05 ** 2
    comp = np.random.default_rng(2).uniform(0, 1, pts.shape[0])
    ref = ref_score(sq_sphere, pts, models, T2, comp)
    if switch:
        monkeypatch.setenv(switch, "1")
    ctx = _lib.Context(0)
    if switch:
        monkeypatch.delenv(switch)
    try:
        ctx.set_points(_lib.SPHERE3D, pts)
        ctx.set_compound(comp)
        got = ctx.score(models, T2, has_compound=True, want_masks=True)
        assert np.array_equal(got["counts"], ref["counts"]) and np.array_equal(got["masks"], ref["masks"])
        assert np.all(np.abs(got["values"] - ref["values"]) <= 1e-9 * np.maximum(np.abs(ref["values"]), 1e-4))
        ctx.score(models, T2, has_compound=True)
        if ctx.score_stats(T2, has_compound=True)["path"] == "cull + group-major":
            ctx.score(models, T2, has_compound=True)
            acc = ctx.score_accumulators()
            for k in ("counts", "values_q", "shared_q"):
                assert np.array_equal(acc[k].astype(np.int64), ref[k]), k
        else:
            assert switch is not None
        if switch is None:                                   # the group-major launch geometry does not matter either
            for geo in (dict(split=3), dict(group_xcd=1), dict(nrep=16), dict(dense_min=1), dict(cull_segs=5)):
                ctx.score_debug_geometry(**geo)
                ctx.score(models, T2, has_compound=True)
                acc = ctx.score_accumulators()
                for k in ("counts", "values_q", "shared_q"):
                    assert np.array_equal(acc[k].astype(np.int64), ref[k]), (geo, k)
    finally:
        ctx.close()


def test_sphere_filter_proof_near_threshold(monkeypatch):
    """Points moved along the radius until |r^2 / T^2 - 1| < 1e-4, on both faces of the shell, with coordinate offsets up to 1e6,
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
                    c = (rng.uniform(3, 7, 3) + off) * scale
                    R = radius * scale
                    T = 1.5 * 0.05 * tf * scale
                    d = rng.normal(size=(n, 3))
                    d /= np.linalg.norm(d, axis=1)[:, None]
                    target = T * (1.0 + rng.uniform(-0.99e-4 / 2, 0.99e-4 / 2, n))
                    side = np.where((rng.random(n) < 0.5) & (R - 1.01 * T > 0), -1.0, 1.0)   # inner face where there is one
                    pts = np.ascontiguousarray(c + d * (R + side * target)[:, None])
                    pts[n // 2:] = c + rng.uniform(-3, 3, (n - n // 2, 3)) * max(R, T)       # and some points off the shell
                    gt = np.append(c, R)
                    hyps = np.empty((64, 4))
                    for k in range(64):
                        hyps[k] = gt + (rng.normal(0, 1e-12, 4) * np.abs(gt) if k % 2 else 0.0)
                    hyps[5, 3] = -R
                    hyps[7] = np.append(c + rng.normal(0, R, 3), R * rng.uniform(0.5, 2.0))
                    ctx.set_points(_lib.SPHERE3D, pts)
                    ctx.score_upload(hyps)
                    st = ctx.score_stats(T * T)
                    assert st["contradictions"] == 0, (off, tf, radius, scale, st)
                    got = ctx.score(hyps, T * T, want_masks=True)
                    ref = ref_score(sq_sphere, pts, hyps, T * T)
                    assert np.array_equal(got["counts"], ref["counts"]) and np.array_equal(got["masks"], ref["masks"])
                    assert ref["counts"][0] > 0
                    f32_seen += st["filter"] == "f32"
        assert f32_seen > 0
    finally:
        ctx.close()


def test_sphere_pointwise_kernels_bit_exact(gpu_ctx):
    pts, models = make_problem(20011, 8, seed=3)
    thr, lam = 0.05, 0.3
    T2 = 2.25 * thr * thr
    gpu_ctx.set_points(_lib.SPHERE3D, pts)
    gpu_ctx.set_compound(None)
    for k in (0, 1, 2):
        pref = gpu_ctx.preference(models[k], T2, slot=k, want_pref=True)["pref"]
        assert np.array_equal(pref, np.maximum(0.0, 1.0 - sq_sphere(pts, models[k]) / T2))
    K = 5
    Dq = gpu_ctx.pearl_unary(models[:K], thr, lam, want_table=True)
    oml = 1.0 - lam
    ref = np.empty((pts.shape[0], K + 1), np.int64)
    for k in range(K):
        sq = sq_sphere(pts, models[k])
        with np.errstate(invalid="ignore"):
            c = np.where(sq > T2, 2.0 * oml, oml * sq / T2)
        c = np.where(np.isnan(c), 2.0 * oml, c)
        ref[:, k] = np.rint(c * 4294967296.0).astype(np.int64)
    ref[:, K] = np.int64(np.rint(oml * 4294967296.0))
    assert np.array_equal(Dq, ref)
    labels = np.random.default_rng(1).integers(0, 4, pts.shape[0]).astype(np.int32)
    gpu_ctx.set_labels(labels)
    finite = models[[0, 1, 2, 5]]                            # (model 3 holds a NaN, model 4 has r = inf)
    sums = gpu_ctx.residual_sums(finite)
    for k in range(4):
        r = np.sqrt(sq_sphere(pts[labels == k], finite[k]))
        assert abs(sums[k] - r.sum()) <= 1e-12 * max(abs(r.sum()), 1e-300)
        assert abs(gpu_ctx.residual_sum(finite[k], k) - r.sum()) <= 1e-12 * max(abs(r.sum()), 1e-300)


def test_sphere_gc_labeling_matches_the_oracle_cut(gpu_ctx, oracle):
    """pgx_gc_labeling / pgx_gc_inliers on spheres, bit for bit.  The oracle's cut depends on the model only through r^2, and the
    2-D line residual |(1 * s + (-r) * 1) + 0| of the point (s, 1) with s = sqrt((dx dx + dy dy) + dz dz) is the sphere residual
    |s - r| exactly (every added operation is exact), so the oracle cuts the sphere problem as a line problem on the same graph."""
    pts, labels, gt = datasets.make_spheres(n_per_sphere=3000, n_spheres=2, n_outliers=3000, seed=8)
    T2 = 2.25 * 0.05 ** 2
    gpu_ctx.set_points(_lib.SPHERE3D, pts)
    graph = gpu_ctx.graph_build(pts, _lib.GRAPH_KNN_IN_BALL, radius=0.5, k=5)
    for m in (gt[0], gt[1], gt[0] + np.array([0.01, -0.02, 0.0, 0.03])):
        line_pts = np.ascontiguousarray(np.column_stack([dist(pts, m), np.ones(len(pts))]))
        line_model = np.array([1.0, -m[3], 0.0])
        assert np.array_equal(oracle.squared_residuals(oracle.LINE2D, line_pts, line_model), sq_sphere(pts, m))
        for lam in (0.1, 0.5):
            flags = gpu_ctx.gc_labeling(m, T2, lam)
            assert np.array_equal(flags, oracle.gc_labeling(oracle.LINE2D, line_pts, line_model, T2, lam, graph)), lam
            assert np.array_equal(np.flatnonzero(flags), gpu_ctx.gc_inliers(m, T2, lam))
    assert flags[labels == 1].mean() > 0.95


@pytest.mark.parametrize("kind", [_lib.GRAPH_BALL, _lib.GRAPH_KNN_IN_BALL])
def test_sphere_graph_and_expansion_match_the_oracle(gpu_ctx, oracle, kind):
    pts, _, gt = datasets.make_spheres(n_per_sphere=1500, n_spheres=3, n_outliers=1500, seed=12)
    gpu_ctx.set_points(_lib.SPHERE3D, pts)
    graph = gpu_ctx.graph_build(pts, kind, radius=0.4, k=5)
    for a, b in zip(graph, oracle.graph_build(pts, kind, radius=0.4, k=5)):
        assert np.array_equal(a, b)
    lam, h = 0.1, 6.0
    Dq = gpu_ctx.pearl_unary(gt, 0.05, lam, want_table=True)
    gpu_ctx.set_labels(np.zeros(pts.shape[0], np.int32))
    eq, e, cyc = gpu_ctx.expansion(lam, h)
    ref_labels, ref_e, ref_cyc = oracle.expansion(Dq, graph, oracle.quantize_lambda(lam), oracle.quantize(h),
                                                  np.zeros(pts.shape[0], np.int32))
    assert np.array_equal(gpu_ctx.get_labels(), ref_labels) and eq == ref_e and cyc == ref_cyc


def test_sphere_minimal_solvers_bitwise_the_estimator(gpu_ctx):
    pts, _, gt = datasets.make_spheres(n_per_sphere=500, n_spheres=3, n_outliers=500, seed=2)
    pts = pts.copy()
    pts[5] = pts[4]                                          # duplicate points
    pts[8:12] = [[1.0, 1.0, 1.0], [2.0, 1.0, 1.0], [1.0, 2.0, 1.0], [3.0, 3.0, 1.0]]   # exactly coplanar
    n = pts.shape[0]
    est = _estimators.SphereEstimator()
    gpu_ctx.set_points(_lib.SPHERE3D, pts)
    gpu_ctx.set_radius_range()
    rng = np.random.default_rng(0)
    samples = rng.integers(0, n, (3000, 4)).astype(np.int32)
    samples[:5] = [[4, 5, 6, 7], [1, 1, 2, 3], [8, 9, 10, 11], [-1, 2, 3, 4], [n, 0, 1, 2]]
    got = gpu_ctx.solve_minimal(samples)
    assert got.shape == (3000, 4)
    assert np.array_equal(got, _want(est, pts, samples, 3000), equal_nan=True)
    assert np.isnan(got[:5]).all() and np.isfinite(got[5:]).all(1).mean() > 0.9
    sc = gpu_ctx.score(got[:5], 2.25 * 0.05 ** 2)
    assert (sc["counts"] == 0).all()
    # the radius range: set, then reset - the second call gives the fresh result
    est.radius_range = (0.4, 1.0)
    gpu_ctx.set_radius_range(0.4, 1.0)
    ranged = gpu_ctx.solve_minimal(samples)
    assert np.array_equal(ranged, _want(est, pts, samples, 3000), equal_nan=True)
    assert np.isfinite(ranged).all(1).sum() < np.isfinite(got).all(1).sum()
    r = ranged[np.isfinite(ranged).all(1), 3]
    assert ((r >= 0.4) & (r <= 1.0)).all()
    gpu_ctx.set_radius_range()
    assert np.array_equal(gpu_ctx.solve_minimal(samples), got, equal_nan=True)
    for bad in ((np.nan, 1.0), (0.0, np.nan), (-1.0, 1.0), (2.0, 1.0)):
        with pytest.raises(_lib.PgxError):
            gpu_ctx.set_radius_range(*bad)
    # device-drawn samples: uniform, NAPSAC on the resident graph, PROSAC; with and without a range
    gpu_ctx.graph_build(pts, _lib.GRAPH_KNN_IN_BALL, radius=0.5, k=5, fetch=False)
    tops = np.minimum(n, np.arange(4, 4 + 512)).astype(np.int32)
    gpu_ctx.sampler_prosac_set(tops)
    for rr in ((0.0, np.inf), (0.4, 1.0)):
        est.radius_range = rr
        gpu_ctx.set_radius_range(*rr)
        for sampler in ("uniform", "napsac", "prosac"):
            models, smp = gpu_ctx.solve_minimal_sampled(12345, 7, 512, fetch_samples=True, sampler=sampler)
            assert smp.shape == (512, 4)
            assert (smp >= 0).all(1).sum() > 0
            assert np.array_equal(models, _want(est, pts, smp, 512), equal_nan=True), (sampler, rr)
            if sampler == "uniform":
                assert np.array_equal(smp, _rng.uniform_samples(12345, 7, 512, n, 4).astype(np.int32))
    gpu_ctx.set_radius_range()


def test_sphere_refit_grams(gpu_ctx):
    pts, labels, gt = datasets.make_spheres(n_per_sphere=4000, n_spheres=3, n_outliers=2000, seed=6)
    n = pts.shape[0]
    w = np.random.default_rng(1).uniform(0.5, 2.0, n)
    gpu_ctx.set_points(_lib.SPHERE3D, pts)

    def rows(prm, sel):
        q = (pts[sel] - prm[:3]) / prm[3]
        return np.column_stack([np.ones(len(q)), q, (q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]])

    prms = np.array([[4.0, 5.0, 6.0, 1.5], [1.0, -2.0, 0.5, 3.0], [0.0, 0.0, 0.0, 1.0], [5.0, 5.0, 5.0, 0.25]])
    idx = np.stack([np.random.default_rng(s).choice(n, 300, replace=False) for s in range(4)]).astype(np.int32)
    Gb, bad = gpu_ctx.gram_batch(_lib.GRAM_SPHERE, idx, params=prms, weights=w, wpow=1)
    for b in range(4):
        G, cnt, _ = gpu_ctx.gram(_lib.GRAM_SPHERE, ("index", idx[b]), params=prms[b], weights=w, wpow=1)
        A = rows(prms[b], idx[b])
        Gr = (A * w[idx[b], None]).T @ A
        assert cnt == 300 and not bad[b]
        assert np.abs(G - Gr).max() <= 1e-12 * np.abs(Gr).max() and np.abs(Gb[b] - Gr).max() <= 1e-12 * np.abs(Gr).max()
    gpu_ctx.set_labels(labels)
    GL, cntL, _ = gpu_ctx.gram_labels(_lib.GRAM_SPHERE, 4, params=prms, weights=w, wpow=1)
    for k in range(4):
        G, cnt, _ = gpu_ctx.gram(_lib.GRAM_SPHERE, ("label", k), params=prms[k], weights=w, wpow=1)
        sel = labels == k
        A = rows(prms[k], sel)
        Gr = (A * w[sel, None]).T @ A
        assert cnt == cntL[k] == sel.sum() and np.array_equal(G, GL[k])
        assert np.abs(G - Gr).max() <= 1e-12 * np.abs(Gr).max()
    # the row kind needs 3-D points and exactly four parameters
    with pytest.raises(_lib.PgxError):
        gpu_ctx.gram(_lib.GRAM_SPHERE, ("label", 1), params=prms[0][:3])
    # the refits: LAPACK and the device's Jacobi solver agree, and both find the spheres
    est = _estimators.SphereEstimator()
    lap = est.nonminimal_labels(gpu_ctx, 4, weights=w)
    est.refit_solver = "jacobi"
    jac = est.nonminimal_labels(gpu_ctx, 4, weights=w)
    for k, (a, b) in enumerate(zip(lap[1:], jac[1:])):
        assert len(a) == len(b) == 1
        assert np.abs(a[0] - b[0]).max() < 1e-10
        assert np.abs(a[0] - gt[k]).max() < 0.01
    # the single-selection refit through pgx_gram is the same fit
    one = est.nonminimal(gpu_ctx, ("label", 1), weights=w)
    assert np.abs(one[0] - jac[1][0]).max() < 1e-10


# minimum_point_number: a spurious sphere through the uniform outliers collects those inside its shell of width 3 x threshold; the
# largest fit the 10 m box with ~47 m^3 of shell (r ~ 5 m) - about 2 400 of the 50 000 outliers at 10^5 points - so a sphere must
# have more support than that.  The true spheres have ~8 300 inliers.
MPN = 4000


def test_find_spheres_end_to_end():
    """The issue's scene: six spheres, 10^5 points, half of them uniform outliers, 1 cm noise, the default sampler (3)."""
    sigma, thr = 0.01, 0.05
    pts, gen, gt = datasets.make_spheres(n_per_sphere=50000 // 6, n_spheres=6, n_outliers=50000, sigma=sigma, seed=0)
    assert pts.shape == (99998, 3)
    pts, gen = shuffled(pts, gen)
    kw = dict(threshold=thr, minimum_point_number=MPN, seed=1)
    spheres, labels = px.findSpheres(pts, **kw)
    _check_recovery(spheres, labels, pts, gen, gt, thr, sigma)
    spheres2, labels2 = px.findSpheres(pts, **kw)
    assert np.array_equal(spheres, spheres2) and np.array_equal(labels, labels2)
    w = np.random.default_rng(1).uniform(0.5, 1.5, len(pts))
    for extra in (dict(sampler_rng="philox"), dict(refit_solver="jacobi"), dict(spatial_coherence_weight=0.1), dict(weights=w)):
        s, lab = px.findSpheres(pts, **kw, **extra)
        _check_recovery(s, lab, pts, gen, gt, thr, sigma)
    # a call with a radius range leaves nothing behind: the next call without one is the fresh result
    px.findSpheres(pts, **kw, radius_range=(0.2, 0.5))
    spheres3, labels3 = px.findSpheres(pts, **kw)
    assert np.array_equal(spheres, spheres3) and np.array_equal(labels, labels3)


def test_find_spheres_on_half_coverage_caps():
    """Three spheres seen from one side each (half of the surface, as one depth scan sees a ball)."""
    sigma, thr = 0.01, 0.05
    pts, gen, gt = datasets.make_spheres(n_per_sphere=10000, n_spheres=3, n_outliers=30000, sigma=sigma, coverage=0.5, seed=4)
    pts, gen = shuffled(pts, gen)
    spheres, labels = px.findSpheres(pts, threshold=thr, minimum_point_number=3000, seed=2)
    _check_recovery(spheres, labels, pts, gen, gt, thr, sigma)


def test_find_spheres_in_a_mixed_scene():
    """make_planes (3 planes) + make_spheres (3 spheres): with radius_range=(0.2, 2.0) exactly the three spheres come back."""
    sigma, thr = 0.01, 0.05
    pp, _, _ = datasets.make_planes(n_per_plane=8000, n_planes=3, n_outliers=0, sigma=sigma, seed=5)
    ps, gs, gt = datasets.make_spheres(n_per_sphere=8000, n_spheres=3, n_outliers=24000, sigma=sigma, seed=6)
    pts = np.ascontiguousarray(np.vstack([pp, ps]))
    gen = np.concatenate([np.zeros(len(pp), np.int32), gs])
    pts, gen = shuffled(pts, gen)
    spheres, labels = px.findSpheres(pts, threshold=thr, minimum_point_number=MPN, radius_range=(0.2, 2.0), seed=3)
    assert spheres.shape == (3, 4)
    for g in gt:
        k = int(np.argmin(np.linalg.norm(spheres[:, :3] - g[:3], axis=1)))
        assert np.linalg.norm(spheres[k, :3] - g[:3]) < 2 * sigma and abs(spheres[k, 3] - g[3]) < 2 * sigma
    assert ((spheres[:, 3] >= 0.2) & (spheres[:, 3] <= 2.0)).all()
    on = labels < 3
    assert (gen[on] > 0).mean() > 0.9                    # the spheres' labels are on the spheres' points
