"""findLines3D on the MI355X: every layer of the 3-D line type against the numpy restatement of its arithmetic
(tests/line3d_filter_model.py), against the oracle by transformation - the symmetric-homography residual of the point (c2, 0, c0, c1)
under H = H^-1 = diag(0, 0, 1) is the line residual bit for bit - and against a 50-digit refit; and the public call end to end.

Residual<kLine3D> (residuals.hip.h) is the contract: e = x - p, c = e x d in cross3's component order, r^2 = (c0 c0 + c1 c1) + c2 c2,
inlier iff r^2 < T2."""
import numpy as np
import pytest

import pyprogressivex as px
from line3d_filter_model import (EPS, REFIT_N, SYM_MODEL, near_threshold_points, refit_fixture, refit_ratios, refit_reference,
                                 sq_line3d, sym_points)
from primitive_helpers import _check_labelling, _check_scores, _want, ref_score, shuffled
from pyprogressivex import _estimators, _lib, _rng, datasets, parallel

pytestmark = pytest.mark.gpu

THR = 0.05
T2_NOMINAL = 2.25 * THR * THR


def make_problem(n, M, seed):
    """points of make_lines3d (truncated to n) and M hypotheses: ground truth, perturbed (1e-7 .. 1), random, d scaled by 2^+-40, 1e-3
    and 7, p far outside the scene, and the special ones d = 0, an Inf entry, one NaN entry and an all-NaN model"""
    rng = np.random.default_rng(seed)
    k = max(n // 8, 1)
    pts, _, gt = datasets.make_lines3d(n_per_line=k, n_lines=4, n_outliers=max(n - 4 * k, 1), seed=seed)
    pts = np.ascontiguousarray(pts[rng.permutation(pts.shape[0])[:n]])
    models = np.empty((M, 6))
    for j in range(M):
        kind = j % 5
        g = gt[j % len(gt)].copy()
        if kind == 1:
            g += rng.normal(0, 10.0 ** rng.uniform(-7, 0), 6)
        elif kind == 2:
            g = np.concatenate([rng.uniform(0, 10.0, 3), rng.normal(size=3)])
        elif kind == 3:
            g[3:] *= rng.choice([2.0 ** -40, 2.0 ** 40, 1e-3, 7.0])
        elif kind == 4:
            g[:3] += g[3:] * 1e5 * (1.0 if j % 2 else 1.0 + 1e-7 * rng.normal())      # the same line from far outside the scene
        models[j] = g
    if M >= 7:
        models[M - 1] = np.nan
        models[M - 2, rng.integers(0, 6)] = np.nan
        models[M - 3, rng.integers(0, 6)] = np.inf
        models[M - 4, 3:] = 0.0                              # d = 0: every residual is 0, every point an inlier
        models[M - 5, :3] = gt[1, :3] + np.array([3e6, -2e6, 1e6])                     # p far outside the scene, off the line
    return pts, models


def oracle_score_by_transformation(oracle, pts, models, T2, comp):
    """oracle.score on the symmetric-homography type, once per model with finite entries, on the points transformed in numpy"""
    out = {}
    for k, m in enumerate(models):
        if np.isfinite(m).all():
            out[k] = oracle.score(oracle.HOMOGRAPHY_SYM, sym_points(pts, m), SYM_MODEL, T2, compound=comp, exponent=2, want_masks=True)
    return out


@pytest.mark.parametrize("n", [1, 63, 64, 65, 5000])
@pytest.mark.parametrize("M", [1, 7, 256])
def test_line3d_scoring_bit_exact(gpu_ctx, oracle, n, M):
    pts, models = make_problem(n, M, seed=n + M)
    T2 = T2_NOMINAL
    if n >= 5000 and M >= 7:                                # a point exactly on the threshold: r^2 == T2 is not an inlier
        on = int(np.flatnonzero(sq_line3d(pts, models[0]) > 0)[0])
        T2 = float(sq_line3d(pts[on:on + 1], models[0])[0])
        assert T2 > 0
    comp = np.random.default_rng(n).uniform(0, 1, n)
    gpu_ctx.score_set_global_n(0)
    gpu_ctx.set_points(_lib.LINE3D, pts)
    gpu_ctx.set_compound(comp)
    got = gpu_ctx.score(models, T2, has_compound=True, exponent=2, want_masks=True)
    ref = ref_score(sq_line3d, pts, models, T2, comp)
    if n >= 5000 and M >= 7:
        assert not (ref["masks"][0, on >> 6] >> np.uint64(on & 63)) & np.uint64(1)
    if M >= 7:
        assert ref["counts"][M - 4] == n and ref["counts"][M - 1] == ref["counts"][M - 2] == ref["counts"][M - 3] == 0
    _check_scores(got, ref)
    if M <= 7:                                               # the second witness
        for k, o in oracle_score_by_transformation(oracle, pts, models, T2, comp).items():
            assert got["counts"][k] == o["counts"][0] and np.array_equal(got["masks"][k], o["masks"][0]), k
            assert abs(got["values"][k] - o["values"][0]) <= 1e-9 * max(abs(o["values"][0]), 1e-4)
            assert abs(got["shared"][k] - o["shared"][0]) <= 1e-9 * max(abs(o["shared"][0]), 1e-4)
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
    """one problem and its numpy reference for every switch of test_line3d_culls_are_invisible"""
    pts, models = make_problem(30011, 300, seed=11)
    comp = np.random.default_rng(2).uniform(0, 1, pts.shape[0])
    return pts, models, comp, ref_score(sq_line3d, pts, models, T2_NOMINAL, comp)


@pytest.mark.parametrize("switch", [None, "PGX_NO_FILTER", "PGX_SCORE_NO_CULL", "PGX_NO_GROUP", "PGX_NO_SORT", "PGX_SETPOINTS_HOST"])
def test_line3d_culls_are_invisible(switch, monkeypatch, cull_problem):
    pts, models, comp, ref = cull_problem
    T2 = T2_NOMINAL
    if switch:
        monkeypatch.setenv(switch, "1")
    ctx = _lib.Context(0)
    if switch:
        monkeypatch.delenv(switch)
    try:
        ctx.set_points(_lib.LINE3D, pts)
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


def test_line3d_filter_proof_near_threshold(monkeypatch):
    """Points moved perpendicular to the axis until |r^2 / T^2 - 1| < 1e-4, coordinate scales 1, 1e3, 1e6, scenes up to 1e6 from the
    origin, thresholds 1e-3 .. 1e3 x nominal, d scaled by 2^-200 .. 2^200 (the threshold along, r scales with |d|): PGX_VERIFY=1 counts
    every inlier the group bound or the f32 filter removed - none may be."""
    monkeypatch.setenv("PGX_VERIFY", "1")
    ctx = _lib.Context(0)
    monkeypatch.delenv("PGX_VERIFY")
    rng = np.random.default_rng(23)
    f32_seen = case = 0
    exps = (-200, -40, -12, 0, 12, 40, 200)
    try:
        for coord in (1.0, 1e3, 1e6):
            for tf in (1e-3, 1.0, 1e3):
                for offset in (0.0, 1e6):
                    e = exps[case % len(exps)]
                    case += 1
                    n = 20000
                    d = rng.normal(size=3)
                    d /= np.linalg.norm(d)
                    gt = np.concatenate([rng.uniform(3, 7, 3) * coord + offset, d])
                    T = 1.5 * THR * coord * tf
                    pts = near_threshold_points(rng, gt, T, n, 5.0 * coord)
                    pts[n // 2:] = gt[:3] + rng.uniform(-3, 3, (n - n // 2, 3)) * max(T, coord)     # and some points off the tube
                    hyps = np.empty((64, 6))
                    for k in range(64):
                        hyps[k] = gt
                        if k % 2:
                            hyps[k, :3] += rng.normal(0, 1e-6 * T, 3)
                        hyps[k, 3:] *= 2.0 ** e
                    hyps[5, 3:] = 0.0
                    hyps[7] = np.concatenate([gt[:3] + rng.normal(0, coord, 3), rng.normal(size=3) * 2.0 ** e])
                    hyps[9, 3:] *= 2.0 ** 3                  # other scales next to the batch's own
                    hyps[11, 3:] *= 2.0 ** -3
                    T2 = (T * 2.0 ** e) ** 2
                    ctx.set_points(_lib.LINE3D, pts)
                    ctx.score_upload(hyps)
                    st = ctx.score_stats(T2)
                    assert st["contradictions"] == 0, (coord, tf, offset, e, st)
                    got = ctx.score(hyps, T2, want_masks=True)
                    ref = ref_score(sq_line3d, pts, hyps, T2)
                    assert np.array_equal(got["counts"], ref["counts"]) and np.array_equal(got["masks"], ref["masks"])
                    assert 0 < ref["counts"][0] < n and ref["counts"][5] == n
                    f32_seen += st["filter"] == "f32"
        assert f32_seen > 0
    finally:
        ctx.close()


def test_line3d_pointwise_kernels_bit_exact(gpu_ctx, oracle):
    """preference, the PEARL unary table and the residual sums against numpy; the unary table and the sums also against the oracle by
    transformation"""
    pts, models = make_problem(20011, 8, seed=3)
    n = pts.shape[0]
    thr, lam = THR, 0.3
    T2 = T2_NOMINAL
    gpu_ctx.set_points(_lib.LINE3D, pts)
    gpu_ctx.set_compound(None)
    for k in (0, 1, 2):
        pref = gpu_ctx.preference(models[k], T2, slot=k, want_pref=True)["pref"]
        assert np.array_equal(pref, np.maximum(0.0, 1.0 - sq_line3d(pts, models[k]) / T2))
    K = 8
    assert np.isnan(models[7]).all() and np.isnan(models[6]).any() and np.isinf(models[5]).any() and not models[4, 3:].any()
    Dq = gpu_ctx.pearl_unary(models[:K], thr, lam, want_table=True)
    oml = 1.0 - lam
    ref = np.empty((n, K + 1), np.int64)
    for k in range(K):
        sq = sq_line3d(pts, models[k])
        with np.errstate(invalid="ignore"):
            c = np.where(sq > T2, 2.0 * oml, oml * sq / T2)
        c = np.where(np.isnan(c), 2.0 * oml, c)
        ref[:, k] = np.rint(c * 4294967296.0).astype(np.int64)
    ref[:, K] = np.int64(np.rint(oml * 4294967296.0))
    assert np.array_equal(Dq, ref)
    for k in range(3):                                       # K = 3 under the oracle: one column per transformed point set
        o = oracle.unary_q(oracle.HOMOGRAPHY_SYM, sym_points(pts, models[k]), SYM_MODEL, thr, lam)
        assert np.array_equal(Dq[:, k], o[:, 0]) and np.array_equal(Dq[:, K], o[:, 1]), k
    labels = np.random.default_rng(1).integers(0, 4, n).astype(np.int32)
    gpu_ctx.set_labels(labels)
    finite = models[[0, 1, 2, 3]]
    sums = gpu_ctx.residual_sums(finite)
    for k in range(4):
        r = np.sqrt(sq_line3d(pts[labels == k], finite[k]))
        assert abs(sums[k] - r.sum()) <= 1e-12 * max(abs(r.sum()), 1e-300)
        assert abs(gpu_ctx.residual_sum(finite[k], k) - r.sum()) <= 1e-12 * max(abs(r.sum()), 1e-300)
        o = oracle.residual_sum(oracle.HOMOGRAPHY_SYM, sym_points(pts, finite[k]), SYM_MODEL, labels, k)
        assert abs(sums[k] - o) <= 1e-12 * max(abs(o), 1e-300)


def test_line3d_gc_labeling_matches_the_oracle_cut(gpu_ctx, oracle):
    """pgx_gc_labeling / pgx_gc_inliers on 3-D lines, bit for bit: the oracle's cut depends on the model only through r^2, so it cuts
    the line problem as a symmetric-homography problem on the graph built over the 3-D points"""
    pts, labels, gt = datasets.make_lines3d(n_per_line=3000, n_lines=2, n_outliers=3000, seed=8)
    T2 = T2_NOMINAL
    gpu_ctx.set_points(_lib.LINE3D, pts)
    graph = gpu_ctx.graph_build(pts, _lib.GRAPH_KNN_IN_BALL, radius=0.5, k=5)
    for m in (gt[0], gt[1], gt[0] + np.array([0.01, -0.02, 0.0, 0.003, 0.0, -0.002])):
        sp = sym_points(pts, m)
        assert np.array_equal(oracle.squared_residuals(oracle.HOMOGRAPHY_SYM, sp, SYM_MODEL), sq_line3d(pts, m))
        for lam in (0.1, 0.5):
            flags = gpu_ctx.gc_labeling(m, T2, lam)
            assert np.array_equal(flags, oracle.gc_labeling(oracle.HOMOGRAPHY_SYM, sp, SYM_MODEL, T2, lam, graph)), lam
            assert np.array_equal(np.flatnonzero(flags), gpu_ctx.gc_inliers(m, T2, lam))
    assert gpu_ctx.gc_labeling(gt[0], T2, 0.1)[labels == 1].mean() > 0.95


@pytest.fixture(scope="module")
def solver_points():
    pts, _, _ = datasets.make_lines3d(n_per_line=500, n_lines=3, n_outliers=500, seed=2)
    pts = pts.copy()
    pts[5] = pts[4]                                          # duplicate points
    pts[8] = [1e200, 0.0, 0.0]                               # the squared length of 8 -> 9 overflows
    pts[9] = [-1e200, 1.0, 2.0]
    return pts


@pytest.mark.parametrize("S", [1, 63, 64, 65, 129, 3000])
def test_line3d_minimal_solver_bitwise_the_estimator(gpu_ctx, solver_points, S):
    pts = solver_points
    n = pts.shape[0]
    est = _estimators.Line3DEstimator()
    gpu_ctx.set_points(_lib.LINE3D, pts)
    samples = np.random.default_rng(S).integers(10, n, (S, 2)).astype(np.int32)
    special = np.array([[4, 5], [1, 1], [8, 9], [-1, 2], [n, 0], [9, 8]], np.int32)[:min(S - 1, 6)]
    samples[:len(special)] = special                         # (S = 1: the one sample is an ordinary one)
    got = gpu_ctx.solve_minimal(samples)
    assert got.shape == (S, 6)
    assert np.array_equal(got, _want(est, pts, samples, S), equal_nan=True)
    assert np.isnan(got[:len(special)]).all() and np.isfinite(got[len(special):]).all(1).mean() > 0.9
    fin = got[np.isfinite(got).all(1)]
    assert np.abs(np.sqrt((fin[:, 3:] ** 2).sum(axis=1)) - 1.0).max() <= 2 * EPS
    if len(special):
        assert (gpu_ctx.score(got[:len(special)], T2_NOMINAL)["counts"] == 0).all()


def test_line3d_device_drawn_samples_equal_the_generator(gpu_ctx):
    """pgx_solve_minimal_sampled with m = 2: the rows are _rng's for the uniform, NAPSAC and PROSAC samplers, the models the solver's"""
    pts, _, _ = datasets.make_lines3d(n_per_line=500, n_lines=3, n_outliers=500, seed=2)
    n = pts.shape[0]
    est = _estimators.Line3DEstimator()
    gpu_ctx.set_points(_lib.LINE3D, pts)
    off, idx, _ = gpu_ctx.graph_build(pts, _lib.GRAPH_KNN_IN_BALL, radius=0.5, k=5)
    tops = np.minimum(n, np.arange(2, 2 + 512)).astype(np.int32)
    gpu_ctx.sampler_prosac_set(tops)
    want_rows = dict(uniform=_rng.uniform_samples(12345, 7, 512, n, 2), napsac=_rng.napsac_samples(12345, 7, 512, n, 2, off, idx),
                     prosac=_rng.prosac_samples(12345, 7, 512, n, 2, tops))
    for sampler in ("uniform", "napsac", "prosac"):
        models, smp = gpu_ctx.solve_minimal_sampled(12345, 7, 512, fetch_samples=True, sampler=sampler)
        assert smp.shape == (512, 2) and (smp >= 0).all(1).sum() > 0
        assert np.array_equal(smp, want_rows[sampler].astype(np.int32)), sampler
        assert np.array_equal(models, _want(est, pts, smp, 512), equal_nan=True), sampler


def test_line3d_refit_grams(gpu_ctx):
    pts, labels, gt = datasets.make_lines3d(n_per_line=4000, n_lines=3, n_outliers=2000, seed=6)
    n = pts.shape[0]
    w = np.random.default_rng(1).uniform(0.5, 2.0, n)
    gpu_ctx.set_points(_lib.LINE3D, pts)
    A = np.column_stack([np.ones(n), pts])
    idx = np.stack([np.random.default_rng(s).choice(n, 300, replace=False) for s in range(4)]).astype(np.int32)
    for ww in (w, None):
        Gb, bad = gpu_ctx.gram_batch(_lib.GRAM_AFFINE, idx, weights=ww, wpow=1)
        assert Gb.shape == (4, 4, 4)
        for b in range(4):
            G, cnt, _ = gpu_ctx.gram(_lib.GRAM_AFFINE, ("index", idx[b]), weights=ww, wpow=1)
            Gr = (A[idx[b]] * (1.0 if ww is None else ww[idx[b], None])).T @ A[idx[b]]
            assert cnt == 300 and not bad[b]
            assert np.abs(G - Gr).max() <= 1e-12 * np.abs(Gr).max() and np.abs(Gb[b] - Gr).max() <= 1e-12 * np.abs(Gr).max()
    gpu_ctx.set_labels(labels)
    GL, cntL, _ = gpu_ctx.gram_labels(_lib.GRAM_AFFINE, 4, weights=w, wpow=1)
    for k in range(4):
        G, cnt, _ = gpu_ctx.gram(_lib.GRAM_AFFINE, ("label", k), weights=w, wpow=1)
        sel = labels == k
        Gr = (A[sel] * w[sel, None]).T @ A[sel]
        assert cnt == cntL[k] == sel.sum() and np.array_equal(G, GL[k])
        assert np.abs(G - Gr).max() <= 1e-12 * np.abs(Gr).max()
    # the three entry points of the refit state the same fit; LAPACK and the device's Jacobi solver agree in direction and sign
    est = _estimators.Line3DEstimator()
    lap = est.nonminimal_labels(gpu_ctx, 4, weights=w)
    est.refit_solver = "jacobi"
    jac = est.nonminimal_labels(gpu_ctx, 4, weights=w)
    for k, (a, b) in enumerate(zip(lap[1:], jac[1:])):
        assert len(a) == len(b) == 1
        assert np.abs(a[0] - b[0]).max() < 1e-10 and a[0][3:] @ b[0][3:] > 0.999
        assert abs(abs(a[0][3:] @ gt[k, 3:]) - 1.0) < 1e-4
    one = est.nonminimal(gpu_ctx, ("label", 1), weights=w)
    assert np.abs(one[0] - jac[1][0]).max() < 1e-10
    assert len(est.nonminimal_batch(gpu_ctx, idx)) == 4


def test_line3d_refit_against_the_50_digit_reference_on_the_device(gpu_ctx):
    """the rule of test_lines3d_cpu.py on the device's Gram matrices, under both eigen-solvers: each within the tolerance of the
    reference, and of the same sign"""
    pytest.importorskip("mpmath")
    worst = [0.0, 0.0]
    for n in REFIT_N:
        for offset in (0.0, 1e3):
            for weights in (None, "mild", "wide"):
                pts, w = refit_fixture(n, offset, weights, seed=n + int(offset) + len(str(weights)))
                ref = refit_reference(pts, w)
                gpu_ctx.set_points(_lib.LINE3D, pts)
                fits = {}
                for solver in ("lapack", "jacobi"):
                    est = _estimators.Line3DEstimator()
                    est.refit_solver = solver
                    (m,) = est.nonminimal(gpu_ctx, ("index", np.arange(n, dtype=np.int32)), weights=w)
                    rd, rm = refit_ratios(m, ref)
                    worst = [max(worst[0], rd), max(worst[1], rm)]
                    assert rd <= 1.0 and rm <= 1.0, (n, offset, weights, solver, rd, rm)
                    fits[solver] = m
                assert fits["lapack"][3:] @ fits["jacobi"][3:] > 0
    print("worst ratios on the device (direction, mean):", worst)


@pytest.mark.parametrize("kind", [_lib.GRAPH_BALL, _lib.GRAPH_KNN_IN_BALL])
def test_line3d_graph_and_expansion_match_the_oracle(gpu_ctx, oracle, kind):
    pts, _, gt = datasets.make_lines3d(n_per_line=1500, n_lines=3, n_outliers=1500, seed=12)
    gpu_ctx.set_points(_lib.LINE3D, pts)
    graph = gpu_ctx.graph_build(pts, kind, radius=0.4, k=5)
    for a, b in zip(graph, oracle.graph_build(pts, kind, radius=0.4, k=5)):
        assert np.array_equal(a, b)
    lam, h = 0.1, 6.0
    Dq = gpu_ctx.pearl_unary(gt, THR, lam, want_table=True)
    gpu_ctx.set_labels(np.zeros(pts.shape[0], np.int32))
    eq, e, cyc = gpu_ctx.expansion(lam, h)
    ref_labels, ref_e, ref_cyc = oracle.expansion(Dq, graph, oracle.quantize_lambda(lam), oracle.quantize(h),
                                                  np.zeros(pts.shape[0], np.int32))
    assert np.array_equal(gpu_ctx.get_labels(), ref_labels) and eq == ref_e and cyc == ref_cyc
    assert len(np.unique(ref_labels)) > 1


# ---- end to end -----------------------------------------------------------------------------------------------------------------------
SIGMA = 0.01


def _scene(seed):
    pts, gen, gt = datasets.make_lines3d(n_per_line=500, n_lines=4, n_outliers=500, sigma=SIGMA, seed=seed)
    pts, gen = shuffled(pts, gen)
    ends = []
    for k, g in enumerate(gt):                               # the extreme projections of the line's own points onto the true axis
        t = (pts[gen == k + 1] - g[:3]) @ g[3:]
        ends.append(np.array([g[:3] + t.min() * g[3:], g[:3] + t.max() * g[3:]]))
    return pts, gen, gt, ends


def _found(lines, ends):
    """per ground-truth segment: does a found line pass within 2 sigma of both its ends"""
    return [any((np.sqrt(sq_line3d(e, m)) < 2 * SIGMA).all() for m in lines) for e in ends]


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_find_lines3d_end_to_end(seed):
    """four lines of 500 points, 500 uniform outliers, 1 cm noise; every default except minimum_point_number = 50"""
    pts, gen, gt, ends = _scene(seed)
    lines, labels = px.findLines3D(pts, minimum_point_number=50)
    assert lines.shape == (4, 6) and lines.dtype == np.float64 and labels.dtype == np.int32 and labels.shape == (len(pts),)
    assert all(_found(lines, ends)), (lines, gt)
    assert np.abs(np.linalg.norm(lines[:, 3:], axis=1) - 1.0).max() <= 4 * EPS
    _check_labelling(np.sqrt(np.column_stack([sq_line3d(pts, g) for g in gt])), labels, gen, THR)


@pytest.mark.parametrize("sampler_id", [0, 1, 2])
def test_find_lines3d_other_samplers_and_weights(sampler_id):
    pts, gen, gt, ends = _scene(0)
    w = np.random.default_rng(1).uniform(0.5, 1.5, len(pts))
    lines, labels = px.findLines3D(pts, w, minimum_point_number=50, sampler_id=sampler_id)
    assert lines.ndim == 2 and lines.shape[1] == 6 and lines.dtype == np.float64
    assert labels.shape == (len(pts),) and labels.dtype == np.int32
    assert sum(_found(lines, ends)) >= 2, lines


def test_line3d_handover_between_types_on_one_context(gpu_ctx):
    """planes, then 3-D lines, then spheres on the same n: nothing of one type's rows or lanes survives into the next"""
    n = 20011
    pts, models = make_problem(n, 64, seed=5)
    rng = np.random.default_rng(7)
    planes = np.column_stack([rng.normal(size=(64, 3)), rng.uniform(-10, 0, 64)])
    planes[:, :3] /= np.linalg.norm(planes[:, :3], axis=1)[:, None]
    spheres = np.column_stack([rng.uniform(0, 10, (64, 3)), rng.uniform(0.5, 5.0, 64)])

    def sq_plane(p, m):
        r = np.abs(((m[0] * p[:, 0] + m[1] * p[:, 1]) + m[2] * p[:, 2]) + m[3])
        return r * r

    def sq_sphere(p, m):
        dx, dy, dz = p[:, 0] - m[0], p[:, 1] - m[1], p[:, 2] - m[2]
        r = np.abs(np.sqrt((dx * dx + dy * dy) + dz * dz) - m[3])
        return r * r
    gpu_ctx.set_compound(None)
    for mt, hyps, fn in ((_lib.PLANE3D, planes, sq_plane), (_lib.LINE3D, models, sq_line3d), (_lib.SPHERE3D, spheres, sq_sphere),
                         (_lib.LINE3D, models, sq_line3d)):
        gpu_ctx.set_points(mt, pts)
        if mt == _lib.SPHERE3D:
            gpu_ctx.set_radius_range()
        got = gpu_ctx.score(hyps, T2_NOMINAL, want_masks=True)
        ref = ref_score(fn, pts, hyps, T2_NOMINAL)
        assert np.array_equal(got["counts"], ref["counts"]) and np.array_equal(got["masks"], ref["masks"]), mt
        assert ref["counts"].max() > 0
