"""findPlanes on the MI355X: every layer of the 3-D plane type against a numpy restatement of its arithmetic written next to the
kernels, and against the oracle where the step is model-agnostic (the neighbourhood graph, alpha-expansion on a given table).  The CPU
oracle has its own plane rows since (oracle/pgx_oracle.c, checked against exact arithmetic in tests/test_oracle.py): the per-type
sweeps of tests/test_gpu_parity.py, the API / replay files and the soaks hold the device to those; this file stays as a second,
numpy-side statement of the same contract.

Residual<kPlane3D> (residuals.hip.h) is the contract: r = |((a x + b y) + c z) + d|, r^2 = r * r, inlier iff r^2 < T2."""
import numpy as np
import pytest

import pyprogressivex as px
from pyprogressivex import _estimators, _lib, _rng, datasets, parallel
from primitive_helpers import _check_labelling, _check_scores, ref_score

pytestmark = pytest.mark.gpu


def sq_plane(pts, m):
    r = np.abs(((m[0] * pts[:, 0] + m[1] * pts[:, 1]) + m[2] * pts[:, 2]) + m[3])
    return r * r


def make_problem(n, M, seed, scale=1.0):
    """points of make_planes (truncated / padded to n) and M hypotheses: ground truth, perturbed, random, NaN and zero-normal"""
    rng = np.random.default_rng(seed)
    pts, _, gt = datasets.make_planes(n_per_plane=max(n // 8, 1), n_planes=4, n_outliers=max(n - 4 * max(n // 8, 1), 1), seed=seed)
    pts = np.ascontiguousarray(pts[rng.permutation(pts.shape[0])[:n]] * scale)
    gt = gt.copy()
    gt[:, 3] *= scale
    models = np.empty((M, 4))
    for k in range(M):
        kind = k % 5
        g = gt[k % len(gt)]
        if kind == 0:
            models[k] = g
        elif kind == 1:
            models[k] = g + rng.normal(0, 10.0 ** rng.uniform(-9, -2), 4) * np.array([1, 1, 1, scale])
        elif kind == 2:
            nrm = rng.normal(size=3)
            nrm /= np.linalg.norm(nrm)
            models[k] = np.append(nrm, -nrm @ rng.uniform(0, 10 * scale, 3))
        elif kind == 3:
            models[k] = g * rng.choice([1e-3, 2.0 ** -40, 7.0, 1e5])      # scaled copies: the residual scales along
        else:
            models[k] = g
    if M >= 3:
        models[M - 1] = np.nan
        models[M - 2] = [0.0, 0.0, 0.0, 0.5]
        models[M - 3, 1] = np.nan
    return pts, models


@pytest.mark.parametrize("n", [1, 63, 64, 65, 5000, 200000])
@pytest.mark.parametrize("M", [1, 7, 256, 2048])
def test_plane_scoring_bit_exact(gpu_ctx, n, M):
    if n == 200000 and M == 2048:
        M = 1024                                           # (the numpy side is the slow one)
    pts, models = make_problem(n, M, seed=n + M)
    thr = 0.05
    T2 = 2.25 * thr * thr
    if n >= 5000 and M >= 7:                                # a point exactly on the threshold: r^2 == T2 is not an inlier
        T2 = float(sq_plane(pts[3:4], models[0])[0])
        assert T2 > 0
    comp = np.random.default_rng(n).uniform(0, 1, n)
    gpu_ctx.score_set_global_n(0)
    gpu_ctx.set_points(_lib.PLANE3D, pts)
    gpu_ctx.set_compound(comp)
    got = gpu_ctx.score(models, T2, has_compound=True, exponent=2, want_masks=True)
    ref = ref_score(sq_plane, pts, models, T2, comp)
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


def test_plane_scoring_takes_the_group_major_path_at_scale(gpu_ctx):
    pts, models = make_problem(200000, 512, seed=5)
    gpu_ctx.score_set_global_n(0)
    gpu_ctx.set_points(_lib.PLANE3D, pts)
    gpu_ctx.score_upload(models)
    st = gpu_ctx.score_stats(2.25 * 0.05 ** 2)
    assert st["path"] == "cull + group-major" and st["filter"] == "f32"
    assert st["surviving_group_steps"] < 0.5 * st["group_pairs"]          # the slab test culls most (hypothesis, group) pairs


@pytest.mark.parametrize("switch", [None, "PGX_NO_FILTER", "PGX_SCORE_NO_CULL", "PGX_NO_GROUP", "PGX_NO_SORT", "PGX_SETPOINTS_HOST"])
def test_plane_culls_are_invisible(switch, monkeypatch):
    pts, models = make_problem(30011, 300, seed=11)
    T2 = 2.25 * 0.05 ** 2
    comp = np.random.default_rng(2).uniform(0, 1, pts.shape[0])
    ref = ref_score(sq_plane, pts, models, T2, comp)
    if switch:
        monkeypatch.setenv(switch, "1")
    ctx = _lib.Context(0)
    if switch:
        monkeypatch.delenv(switch)
    try:
        ctx.set_points(_lib.PLANE3D, pts)
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


def test_plane_filter_proof_near_threshold(monkeypatch):
    """Points moved along the normal until |r^2 / T^2 - 1| < 1e-4, model scales 2^-200 .. 2^200, thresholds 1e-3 .. 1e3 x nominal,
    coordinates up to 1e6: PGX_VERIFY=1 counts every inlier the group bound or the f32 filter removed - none may be."""
    monkeypatch.setenv("PGX_VERIFY", "1")
    ctx = _lib.Context(0)
    monkeypatch.delenv("PGX_VERIFY")
    rng = np.random.default_rng(23)
    f32_seen = False
    try:
        for coord in (1.0, 1e3, 1e6):
            for tf in (1e-3, 1.0, 1e3):
                base, models = make_problem(20000, 64, seed=int(coord) % 97 + int(tf * 1000) % 89)
                pts = base * coord
                thr = 0.05 * coord * tf
                T = 1.5 * thr
                gt = models[0].copy()
                gt[3] *= coord
                r = ((gt[0] * pts[:, 0] + gt[1] * pts[:, 1]) + gt[2] * pts[:, 2]) + gt[3]
                target = T * (1.0 + rng.uniform(-0.99e-4 / 2, 0.99e-4 / 2, pts.shape[0])) * np.where(rng.random(pts.shape[0]) < 0.5, -1, 1)
                pts = np.ascontiguousarray(pts - (r - target)[:, None] * gt[None, :3])
                hyps = np.empty((64, 4))
                for k in range(64):
                    e = rng.choice(np.arange(-200, 201, 40))
                    hyps[k] = (gt + (rng.normal(0, 1e-12, 4) if k % 2 else 0.0)) * 2.0 ** float(e)
                ctx.set_points(_lib.PLANE3D, pts)
                ctx.score_upload(hyps)
                st = ctx.score_stats(T * T)
                assert st["contradictions"] == 0, (coord, tf, st)
                got = ctx.score(hyps, T * T, want_masks=True)
                ref = ref_score(sq_plane, pts, hyps, T * T)
                assert np.array_equal(got["counts"], ref["counts"]) and np.array_equal(got["masks"], ref["masks"])
                f32_seen |= st["filter"] == "f32"
        assert f32_seen
    finally:
        ctx.close()


def test_plane_pointwise_kernels_bit_exact(gpu_ctx):
    pts, models = make_problem(20011, 8, seed=3)
    thr, lam = 0.05, 0.3
    T2 = 2.25 * thr * thr
    gpu_ctx.set_points(_lib.PLANE3D, pts)
    gpu_ctx.set_compound(None)
    for k in (0, 1, 2):
        pref = gpu_ctx.preference(models[k], T2, slot=k, want_pref=True)["pref"]
        assert np.array_equal(pref, np.maximum(0.0, 1.0 - sq_plane(pts, models[k]) / T2))
    K = 5
    Dq = gpu_ctx.pearl_unary(models[:K], thr, lam, want_table=True)
    oml = 1.0 - lam
    ref = np.empty((pts.shape[0], K + 1), np.int64)
    for k in range(K):
        sq = sq_plane(pts, models[k])
        with np.errstate(invalid="ignore"):
            c = np.where(sq > T2, 2.0 * oml, oml * sq / T2)
        c = np.where(np.isnan(c), 2.0 * oml, c)
        ref[:, k] = np.rint(c * 4294967296.0).astype(np.int64)
    ref[:, K] = np.int64(np.rint(oml * 4294967296.0))
    assert np.array_equal(Dq, ref)
    labels = np.random.default_rng(1).integers(0, 4, pts.shape[0]).astype(np.int32)
    gpu_ctx.set_labels(labels)
    sums = gpu_ctx.residual_sums(models[:4])
    for k in range(4):
        r = np.sqrt(sq_plane(pts[labels == k], models[k]))
        assert abs(sums[k] - r.sum()) <= 1e-12 * max(abs(r.sum()), 1e-300)
        assert abs(gpu_ctx.residual_sum(models[k], k) - r.sum()) <= 1e-12 * max(abs(r.sum()), 1e-300)


def test_plane_gc_labeling_matches_the_oracle_cut(gpu_ctx, oracle):
    """pgx_gc_labeling / pgx_gc_inliers on planes, bit for bit.  The oracle's cut depends on the model only through r^2, and the
    2-D line residual |(1 * s + d * 1) + 0| of the point (s, 1) with s = (a x + b y) + c z is the plane residual |((a x + b y) + c z) + d|
    exactly (every added operation is exact), so the oracle cuts the plane problem as a line problem on the same graph."""
    pts, labels, gt = datasets.make_planes(n_per_plane=3000, n_planes=2, n_outliers=3000, seed=8)
    T2 = 2.25 * 0.05 ** 2
    gpu_ctx.set_points(_lib.PLANE3D, pts)
    graph = gpu_ctx.graph_build(pts, _lib.GRAPH_KNN_IN_BALL, radius=0.5, k=5)
    for m in (gt[0], gt[1], gt[0] + np.array([0.01, -0.02, 0.0, 0.03])):
        s = (m[0] * pts[:, 0] + m[1] * pts[:, 1]) + m[2] * pts[:, 2]
        line_pts = np.ascontiguousarray(np.column_stack([s, np.ones(len(pts))]))
        line_model = np.array([1.0, m[3], 0.0])
        assert np.array_equal(oracle.squared_residuals(oracle.LINE2D, line_pts, line_model), sq_plane(pts, m))
        for lam in (0.1, 0.5):
            flags = gpu_ctx.gc_labeling(m, T2, lam)
            assert np.array_equal(flags, oracle.gc_labeling(oracle.LINE2D, line_pts, line_model, T2, lam, graph)), lam
            assert np.array_equal(np.flatnonzero(flags), gpu_ctx.gc_inliers(m, T2, lam))
    assert flags[labels == 1].mean() > 0.95


def test_plane_minimal_solvers_bitwise_the_estimator(gpu_ctx):
    pts, _, _ = datasets.make_planes(n_per_plane=500, n_planes=3, n_outliers=500, seed=2)
    pts = pts.copy()
    pts[5] = pts[4]                                          # duplicate points
    pts[8:11] = [[1.0, 1.0, 1.0], [2.0, 2.0, 2.0], [3.0, 3.0, 3.0]]   # exactly collinear
    n = pts.shape[0]
    est = _estimators.PlaneEstimator()
    gpu_ctx.set_points(_lib.PLANE3D, pts)
    rng = np.random.default_rng(0)
    samples = rng.integers(0, n, (3000, 3)).astype(np.int32)
    samples[:5] = [[4, 5, 6], [1, 1, 2], [8, 9, 10], [-1, 2, 3], [n, 0, 1]]
    got = gpu_ctx.solve_minimal(samples)
    assert got.shape == (3000, 4)
    valid = (samples >= 0).all(1) & (samples < n).all(1)
    ref, src = est.minimal(pts, samples[valid])
    want = np.full((3000, 4), np.nan)
    want[np.flatnonzero(valid)[src]] = ref
    assert np.array_equal(got, want, equal_nan=True)
    assert np.isnan(got[:5]).all()
    sc = gpu_ctx.score(got[:5], 2.25 * 0.05 ** 2)
    assert (sc["counts"] == 0).all()
    # device-drawn samples: uniform, NAPSAC on the resident graph, PROSAC
    gpu_ctx.graph_build(pts, _lib.GRAPH_KNN_IN_BALL, radius=0.5, k=5, fetch=False)
    tops = np.minimum(n, np.arange(3, 3 + 512)).astype(np.int32)
    gpu_ctx.sampler_prosac_set(tops)
    for sampler in ("uniform", "napsac", "prosac"):
        models, smp = gpu_ctx.solve_minimal_sampled(12345, 7, 512, fetch_samples=True, sampler=sampler)
        assert smp.shape == (512, 3)
        ok = (smp >= 0).all(1)
        assert ok.sum() > 0
        ref, src = est.minimal(pts, smp[ok])
        want = np.full((512, 4), np.nan)
        want[np.flatnonzero(ok)[src]] = ref
        assert np.array_equal(models, want, equal_nan=True), sampler
        if sampler == "uniform":
            assert np.array_equal(smp, _rng.uniform_samples(12345, 7, 512, n, 3).astype(np.int32))


def test_plane_refit_grams(gpu_ctx):
    pts, labels, _ = datasets.make_planes(n_per_plane=4000, n_planes=3, n_outliers=2000, seed=6)
    n = pts.shape[0]
    w = np.random.default_rng(1).uniform(0.5, 2.0, n)
    gpu_ctx.set_points(_lib.PLANE3D, pts)
    A = np.column_stack([np.ones(n), pts])
    idx = np.stack([np.random.default_rng(s).choice(n, 300, replace=False) for s in range(4)]).astype(np.int32)
    Gb, bad = gpu_ctx.gram_batch(_lib.GRAM_AFFINE, idx, weights=w, wpow=1)
    for b in range(4):
        G, cnt, _ = gpu_ctx.gram(_lib.GRAM_AFFINE, ("index", idx[b]), weights=w, wpow=1)
        Gr = (A[idx[b]] * w[idx[b], None]).T @ A[idx[b]]
        assert cnt == 300 and not bad[b]
        # (one wave per selection against the multi-block reduction: the same sums in another order)
        assert np.abs(G - Gr).max() <= 1e-12 * np.abs(Gr).max() and np.abs(Gb[b] - Gr).max() <= 1e-12 * np.abs(Gr).max()
    gpu_ctx.set_labels(labels)
    GL, cntL, _ = gpu_ctx.gram_labels(_lib.GRAM_AFFINE, 4, weights=w, wpow=1)
    for k in range(4):
        G, cnt, _ = gpu_ctx.gram(_lib.GRAM_AFFINE, ("label", k), weights=w, wpow=1)
        sel = labels == k
        Gr = (A[sel] * w[sel, None]).T @ A[sel]
        assert cnt == cntL[k] == sel.sum() and np.array_equal(G, GL[k])
        assert np.abs(G - Gr).max() <= 1e-12 * np.abs(Gr).max()
    # the Jacobi refit on the device agrees with LAPACK
    est = _estimators.PlaneEstimator()
    lap = est.nonminimal_labels(gpu_ctx, 4, weights=w)
    est.refit_solver = "jacobi"
    jac = est.nonminimal_labels(gpu_ctx, 4, weights=w)
    for a, b in zip(lap[1:], jac[1:]):
        assert np.abs(a[0] * np.sign(a[0][2]) - b[0] * np.sign(b[0][2])).max() < 1e-10


@pytest.mark.parametrize("kind", [_lib.GRAPH_BALL, _lib.GRAPH_KNN_IN_BALL])
def test_plane_graph_and_expansion_match_the_oracle(gpu_ctx, oracle, kind):
    pts, _, gt = datasets.make_planes(n_per_plane=1500, n_planes=3, n_outliers=1500, seed=12)
    gpu_ctx.set_points(_lib.PLANE3D, pts)
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


def _check_recovery(planes, labels, pts, gen_labels, gt, thr, sigma):
    K = len(gt)
    assert planes.shape == (K, 4) and labels.dtype == np.int32
    for j, g in enumerate(gt):
        cosang = np.abs(planes[:, :3] @ g[:3])
        k = int(np.argmax(cosang))
        assert np.degrees(np.arccos(min(1.0, cosang[k]))) < 2.0
        # offset where the plane's points are (d itself also carries the normal's error times the distance from the origin)
        on = pts[gen_labels == j + 1]
        assert abs(np.mean(on @ planes[k, :3] + planes[k, 3])) < 2 * sigma
    _check_labelling(np.abs(pts @ gt[:, :3].T + gt[:, 3]), labels, gen_labels, thr)


def test_find_planes_end_to_end():
    """The issue's scene: six planes, 10^5 points, half of them uniform outliers, 1 cm noise.
    scoring_exponent = 1: the compound score value - shared^e squares the support a candidate shares with the accepted planes
    (their slabs cross every patch); that square grows with n^2 against a value that grows with n, and with e = 2 the proposal
    prefers tilted partial planes that avoid the crossings (3-6 of 6 planes at 10^5 and 10^6, profiles/planes_bench.json).
    minimum_point_number: a slab of width 3 thr across the box holds ~10^3 outliers, so planes need more support than that."""
    sigma, thr = 0.01, 0.05
    pts, gen, gt = datasets.make_planes(n_per_plane=50000 // 6, n_planes=6, n_outliers=50000, sigma=sigma, seed=0)
    assert pts.shape == (99998, 3)
    kw = dict(threshold=thr, scoring_exponent=1, minimum_point_number=2500, seed=1)
    planes, labels = px.findPlanes(pts, **kw)
    _check_recovery(planes, labels, pts, gen, gt, thr, sigma)
    planes2, labels2 = px.findPlanes(pts, **kw)
    assert np.array_equal(planes, planes2) and np.array_equal(labels, labels2)
    for extra in (dict(sampler_rng="philox"), dict(refit_solver="jacobi"), dict(spatial_coherence_weight=0.1)):
        p, lab = px.findPlanes(pts, **kw, **extra)
        _check_recovery(p, lab, pts, gen, gt, thr, sigma)


@pytest.mark.parametrize("sampler_id", [0, 1, 3])
def test_find_planes_other_samplers_and_weights(sampler_id):
    sigma, thr = 0.002, 0.05
    pts, gen, gt = datasets.make_planes(n_per_plane=4000, n_planes=3, n_outliers=3000, sigma=sigma, seed=3)
    # PROSAC and Progressive NAPSAC take the points as ordered by quality (their first samples come from the first points):
    # in make_planes' order every proposal would start inside plane 1, so the points go in a random order here
    order = np.random.default_rng(0).permutation(len(pts))
    pts, gen = np.ascontiguousarray(pts[order]), gen[order]
    w = np.random.default_rng(1).uniform(0.5, 1.5, len(pts))
    for weights in (None, w):
        planes, labels = px.findPlanes(pts, weights, threshold=thr, scoring_exponent=1, sampler_id=sampler_id,
                                       minimum_point_number=1000, seed=2)
        _check_recovery(planes, labels, pts, gen, gt, thr, sigma)
