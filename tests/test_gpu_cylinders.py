"""findCylinders on the MI355X: every layer of the cylinder type against the numpy restatement of its arithmetic
(tests/cylinder_model.py), against the oracle where it can serve - its sphere residual with the model (0, 0, 0, r) on the rows
C = (x - p) x d is the cylinder residual's last step bit for bit - and against Gauss-Newton at 50 digits; and the public call end to end.

Residual<kCylinder3D> (residuals.hip.h) is the contract: q = Residual<kLine3D>::squared, plain = |sqrt(q) - r|, squared = plain^2,
inlier iff squared < T2."""
import numpy as np
import pytest

import pyprogressivex as px
from cylinder_model import (EPS, REFIT_CASES, cross_rows, gn_reference, gn_rows, near_threshold_cases, near_threshold_points,
                            refit_fixture, refit_ratios, sq_cylinder)
from primitive_helpers import _check_labelling, _check_scores, _want, ref_score
from pyprogressivex import _estimators, _lib, _rng, datasets, parallel

pytestmark = pytest.mark.gpu

THR = 0.05
T2_NOMINAL = 2.25 * THR * THR


def make_problem(n, M, seed):
    """points of make_cylinders (truncated to n) and M hypotheses drawn as test_gpu_lines3d.make_problem draws its lines, with a radius:
    ground truth, perturbed (1e-7 .. 1), random, d scaled by 2^+-40, 1e-3 and 7 (the radius along), p far along the axis; and the
    special ones: d = 0, an Inf entry, one NaN entry, an all-NaN model, p far off the scene, r = 0, r < 0, r = 1e6 and an Inf radius"""
    rng = np.random.default_rng(seed)
    k = max(n // 8, 1)
    pts, nrm, _, gt = datasets.make_cylinders(n_per_cylinder=k, n_cylinders=4, n_outliers=max(n - 4 * k, 1), seed=seed)
    pick = rng.permutation(pts.shape[0])[:n]
    pts, nrm = np.ascontiguousarray(pts[pick]), np.ascontiguousarray(nrm[pick])
    models = np.empty((M, 7))
    for j in range(M):
        kind = j % 5
        g = gt[j % len(gt)].copy()
        if kind == 1:
            g += rng.normal(0, 10.0 ** rng.uniform(-7, 0), 7)
        elif kind == 2:
            g = np.concatenate([rng.uniform(0, 10.0, 3), rng.normal(size=3), [rng.uniform(0.1, 2.0)]])
        elif kind == 3:
            g[3:] *= rng.choice([2.0 ** -40, 2.0 ** 40, 1e-3, 7.0])
        elif kind == 4:
            g[:3] += g[3:6] * 1e5 * (1.0 if j % 2 else 1.0 + 1e-7 * rng.normal())     # the same cylinder from far outside the scene
        models[j] = g
    if M >= 7:
        models[M - 1] = np.nan
        models[M - 2, rng.integers(0, 7)] = np.nan
        models[M - 3, rng.integers(0, 6)] = np.inf
        models[M - 4, 3:6] = 0.0                              # d = 0: every residual is |r|
        models[M - 4, 6] = THR                               # ... here below the threshold: every point an inlier
        models[M - 5, :3] = gt[1, :3] + np.array([3e6, -2e6, 1e6])                    # p far outside the scene, off the axis
    if M >= 256:
        models[M - 6, 6] = 0.0                               # r = 0: the 3-D line
        models[M - 7, 6] = -0.5 * models[M - 7, 6]           # r < 0
        models[M - 8, 6] = 1e6
        models[M - 9, 6] = np.inf
        models[M - 10, 6] = -np.inf
    return pts, nrm, models


@pytest.mark.parametrize("n", [1, 63, 64, 65, 5000])
@pytest.mark.parametrize("M", [1, 7, 256])
def test_cylinder_scoring_bit_exact(gpu_ctx, n, M):
    pts, _, models = make_problem(n, M, seed=n + M)
    T2 = T2_NOMINAL
    if n >= 5000 and M >= 7:                                # a point exactly on the threshold: r^2 == T2 is not an inlier
        on = int(np.flatnonzero(sq_cylinder(pts, models[0]) > 0)[0])
        T2 = float(sq_cylinder(pts[on:on + 1], models[0])[0])
        assert T2 > 0
    comp = np.random.default_rng(n).uniform(0, 1, n)
    gpu_ctx.score_set_global_n(0)
    gpu_ctx.set_points(_lib.CYLINDER3D, pts)
    gpu_ctx.set_compound(comp)
    got = gpu_ctx.score(models, T2, has_compound=True, exponent=2, want_masks=True)
    ref = ref_score(sq_cylinder, pts, models, T2, comp)
    if n >= 5000 and M >= 7:
        assert not (ref["masks"][0, on >> 6] >> np.uint64(on & 63)) & np.uint64(1)
    if M >= 7:
        assert ref["counts"][M - 1] == ref["counts"][M - 2] == ref["counts"][M - 3] == 0
        if T2 > THR * THR:
            assert ref["counts"][M - 4] == n
    if M >= 256:
        assert ref["counts"][M - 9] == ref["counts"][M - 10] == 0
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
    """one problem and its numpy reference for every switch of test_cylinder_culls_are_invisible"""
    pts, _, models = make_problem(30011, 300, seed=11)
    comp = np.random.default_rng(2).uniform(0, 1, pts.shape[0])
    return pts, models, comp, ref_score(sq_cylinder, pts, models, T2_NOMINAL, comp)


@pytest.mark.parametrize("switch", [None, "PGX_NO_FILTER", "PGX_SCORE_NO_CULL", "PGX_NO_GROUP", "PGX_NO_SORT", "PGX_SETPOINTS_HOST"])
def test_cylinder_culls_are_invisible(switch, monkeypatch, cull_problem):
    pts, models, comp, ref = cull_problem
    T2 = T2_NOMINAL
    if switch:
        monkeypatch.setenv(switch, "1")
    ctx = _lib.Context(0)
    if switch:
        monkeypatch.delenv(switch)
    try:
        ctx.set_points(_lib.CYLINDER3D, pts)
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


def test_cylinder_filter_proof_near_threshold(gpu_ctx):
    """the point sets of the CPU budget test (coordinate scales 1 .. 1e6, offsets to 1e6, thresholds 1e-3 .. 1e3 x nominal, radii 1e-3 ..
    1e3 x the scale, d and r scaled by 2^-40 .. 2^40), 2048 points a case, scored on the device with the cull and the f32 filter on:
    the masks are the exact ones"""
    f32_seen = 0
    for k, (rng, gt, T, e, coord) in enumerate(near_threshold_cases()):
        if k % 3 != 1:
            continue
        n = 2048
        pts = near_threshold_points(rng, gt, T, n, 5.0 * coord)
        pts[n // 2:] = gt[:3] + rng.uniform(-3, 3, (n - n // 2, 3)) * max(T, abs(gt[6]), coord)      # and some points off the shell
        hyps = np.tile(gt, (64, 1))
        hyps[1::2, :3] += rng.normal(0, 1e-6 * T, (32, 3))
        hyps[:, 3:] *= 2.0 ** e
        hyps[5, 3:6] = 0.0
        hyps[9, 3:] *= 2.0 ** 3                              # other scales next to the batch's own
        hyps[11, 3:] *= 2.0 ** -3
        T2 = (T * 2.0 ** e) ** 2
        gpu_ctx.set_points(_lib.CYLINDER3D, pts)
        gpu_ctx.set_compound(None)
        got = gpu_ctx.score(hyps, T2, want_masks=True)
        ref = ref_score(sq_cylinder, pts, hyps, T2)
        assert np.array_equal(got["counts"], ref["counts"]) and np.array_equal(got["masks"], ref["masks"]), (k, coord, T, e)
        assert 0 < ref["counts"][0] < n
        f32_seen += gpu_ctx.score_stats(T2)["filter"] == "f32"
    assert f32_seen > 0


def test_cylinder_pointwise_kernels_bit_exact(gpu_ctx, oracle):
    """preference, the PEARL unary table, the residual sums and the inlier/outlier cut: against numpy, and the cut against the oracle's
    on the sphere type's rows C with the model (0, 0, 0, r), whose residuals are the cylinder's bit for bit"""
    pts, _, models = make_problem(20011, 8, seed=3)
    n = pts.shape[0]
    thr, lam = THR, 0.3
    T2 = T2_NOMINAL
    gpu_ctx.set_points(_lib.CYLINDER3D, pts)
    gpu_ctx.set_compound(None)
    for k in (0, 1, 2):
        pref = gpu_ctx.preference(models[k], T2, slot=k, want_pref=True)["pref"]
        assert np.array_equal(pref, np.maximum(0.0, 1.0 - sq_cylinder(pts, models[k]) / T2))
    K = 8
    assert np.isnan(models[7]).all() and np.isnan(models[6]).any() and np.isinf(models[5]).any() and not models[4, 3:6].any()
    Dq = gpu_ctx.pearl_unary(models[:K], thr, lam, want_table=True)
    oml = 1.0 - lam
    ref = np.empty((n, K + 1), np.int64)
    for k in range(K):
        sq = sq_cylinder(pts, models[k])
        with np.errstate(invalid="ignore"):
            c = np.where(sq > T2, 2.0 * oml, oml * sq / T2)
        c = np.where(np.isnan(c), 2.0 * oml, c)
        ref[:, k] = np.rint(c * 4294967296.0).astype(np.int64)
    ref[:, K] = np.int64(np.rint(oml * 4294967296.0))
    assert np.array_equal(Dq, ref)
    labels = np.random.default_rng(1).integers(0, 4, n).astype(np.int32)
    gpu_ctx.set_labels(labels)
    finite = models[[0, 1, 2, 3]]
    sums = gpu_ctx.residual_sums(finite)
    for k in range(4):
        r = np.sqrt(sq_cylinder(pts[labels == k], finite[k]))
        assert abs(sums[k] - r.sum()) <= 1e-12 * max(abs(r.sum()), 1e-300)
        assert abs(gpu_ctx.residual_sum(finite[k], k) - r.sum()) <= 1e-12 * max(abs(r.sum()), 1e-300)
    graph = gpu_ctx.graph_build(pts, _lib.GRAPH_KNN_IN_BALL, radius=0.5, k=5)
    for m in (models[0], models[1]):
        rows, sphere = cross_rows(pts, m), np.array([0.0, 0.0, 0.0, m[6]])
        assert np.array_equal(oracle.squared_residuals(oracle.SPHERE3D, rows, sphere), sq_cylinder(pts, m))
        for lam_gc in (0.1, 0.5):
            flags = gpu_ctx.gc_labeling(m, T2, lam_gc)
            assert np.array_equal(flags, oracle.gc_labeling(oracle.SPHERE3D, rows, sphere, T2, lam_gc, graph)), lam_gc
            assert np.array_equal(np.flatnonzero(flags), gpu_ctx.gc_inliers(m, T2, lam_gc))
    assert gpu_ctx.gc_labeling(models[0], T2, 0.1).sum() > 1000


def test_cylinder_graph_and_expansion_match_the_oracle(gpu_ctx, oracle):
    """the graph against the oracle's; one expansion on an injected unary table computed in numpy against the oracle's expansion"""
    pts, _, _, gt = datasets.make_cylinders(n_per_cylinder=1500, n_cylinders=3, n_outliers=1500, seed=12)
    n = pts.shape[0]
    gpu_ctx.set_points(_lib.CYLINDER3D, pts)
    graph = gpu_ctx.graph_build(pts, _lib.GRAPH_KNN_IN_BALL, radius=0.4, k=5)
    for a, b in zip(graph, oracle.graph_build(pts, _lib.GRAPH_KNN_IN_BALL, radius=0.4, k=5)):
        assert np.array_equal(a, b)
    lam, h = 0.1, 6.0
    oml, T2 = 1.0 - lam, T2_NOMINAL
    Dq = np.empty((n, 4), np.int64)
    for k in range(3):
        sq = sq_cylinder(pts, gt[k])
        Dq[:, k] = np.rint(np.where(sq > T2, 2.0 * oml, oml * sq / T2) * 4294967296.0).astype(np.int64)
    Dq[:, 3] = np.int64(np.rint(oml * 4294967296.0))
    assert np.array_equal(gpu_ctx.pearl_unary(gt, THR, lam, want_table=True), Dq)
    gpu_ctx.set_unary_q(Dq)
    gpu_ctx.set_labels(np.zeros(n, np.int32))
    eq, e, cyc = gpu_ctx.expansion(lam, h)
    ref_labels, ref_e, ref_cyc = oracle.expansion(Dq, graph, oracle.quantize_lambda(lam), oracle.quantize(h), np.zeros(n, np.int32))
    assert np.array_equal(gpu_ctx.get_labels(), ref_labels) and eq == ref_e and cyc == ref_cyc
    assert len(np.unique(ref_labels)) > 1


# ---- the solver ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def solver_scene():
    pts, nrm, _, _ = datasets.make_cylinders(n_per_cylinder=500, n_cylinders=3, n_outliers=500, seed=2)
    pts, nrm = pts.copy(), nrm.copy()
    pts[5], nrm[5] = pts[4], nrm[4]                          # a duplicate point with the same normal
    nrm[6] = 0.0                                             # a zero normal
    nrm[7] = -4.0 * nrm[3]                                   # parallel to 3's (a power of two: the cross product is 0 exactly)
    pts[8] = [1e200, 0.0, 0.0]
    nrm[9] = [1e200, 1e200, 0.0]                             # its cross products overflow
    nrm[2, 1] = np.nan
    nrm[1, 0] = np.inf
    return pts, nrm


@pytest.mark.parametrize("S", [1, 63, 64, 65, 129])
def test_cylinder_minimal_solver_bitwise_the_estimator(gpu_ctx, solver_scene, S):
    pts, nrm = solver_scene
    n = pts.shape[0]
    est = _estimators.CylinderEstimator()
    est.normals = nrm
    gpu_ctx.set_radius_range()
    gpu_ctx.set_points(_lib.CYLINDER3D, pts)
    gpu_ctx.set_normals(nrm)
    samples = np.random.default_rng(S).integers(10, n, (S, 2)).astype(np.int32)
    special = np.array([[4, 5], [11, 11], [6, 12], [3, 7], [9, 13], [2, 14], [1, 15], [-1, 2], [n, 0], [12, 6]], np.int32)[:min(S - 1, 10)]
    samples[:len(special)] = special                         # (S = 1: the one sample is an ordinary one)
    got = gpu_ctx.solve_minimal(samples)
    assert got.shape == (S, 7)
    assert np.array_equal(got, _want(est, pts, samples, S), equal_nan=True)
    assert np.isnan(got[:len(special)]).all() and np.isfinite(got[len(special):]).all(1).mean() > 0.9
    fin = got[np.isfinite(got).all(1)]
    assert np.abs(np.sqrt((fin[:, 3:6] ** 2).sum(axis=1)) - 1.0).max() <= 2 * EPS and (fin[:, 6] >= 0).all()
    if len(special):
        assert (gpu_ctx.score(got[:len(special)], T2_NOMINAL)["counts"] == 0).all()
    if S == 129:                                             # the radius range: inclusive, honoured by device and estimator alike
        lo, hi = np.sort(fin[:, 6])[[len(fin) // 4, 3 * len(fin) // 4]]
        gpu_ctx.set_radius_range(float(lo), float(hi))
        est.radius_range = (float(lo), float(hi))
        ranged = gpu_ctx.solve_minimal(samples)
        gpu_ctx.set_radius_range()
        assert np.array_equal(ranged, _want(est, pts, samples, S), equal_nan=True)
        kept = np.isfinite(ranged).all(1)
        assert 0 < kept.sum() < len(fin) and ranged[kept, 6].min() == lo and ranged[kept, 6].max() == hi


def test_cylinder_device_drawn_samples_equal_the_generator(gpu_ctx, solver_scene):
    """pgx_solve_minimal_sampled with m = 2: the rows are _rng's for the uniform, NAPSAC and PROSAC samplers, the models the solver's"""
    pts, nrm = solver_scene
    pts = np.where(np.isfinite(pts) & (np.abs(pts) < 1e100), pts, 5.0)       # (the graph is built on finite coordinates)
    n = pts.shape[0]
    est = _estimators.CylinderEstimator()
    est.normals = nrm
    gpu_ctx.set_radius_range()
    gpu_ctx.set_points(_lib.CYLINDER3D, pts)
    gpu_ctx.set_normals(nrm)
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
        assert np.isfinite(models).all(1).sum() > 100, sampler


def test_cylinder_solver_needs_resident_normals(gpu_ctx, solver_scene):
    pts, nrm = solver_scene
    n = pts.shape[0]
    samples = np.array([[20, 30], [40, 50]], np.int32)
    gpu_ctx.set_points(_lib.CYLINDER3D, pts)
    with pytest.raises(_lib.PgxError, match="pgx_solve_minimal: the cylinder solver needs the resident points' normals"):
        gpu_ctx.solve_minimal(samples)
    with pytest.raises(_lib.PgxError, match="needs the resident points' normals"):
        gpu_ctx.solve_minimal_sampled(1, 0, 8)
    for bad in (nrm[:-1], np.vstack([nrm, nrm[:1]])):
        with pytest.raises(_lib.PgxError, match=rf"pgx_set_normals: {len(bad)} normals for {n} points"):
            gpu_ctx.set_normals(bad)
    with pytest.raises(_lib.PgxError, match="needs the resident points' normals"):
        gpu_ctx.solve_minimal(samples)                       # (a refused upload uploads nothing)
    gpu_ctx.set_normals(nrm)
    first = gpu_ctx.solve_minimal(samples)
    assert np.isfinite(first).all()
    gpu_ctx.set_normals(None)                                # (NULL, 0) clears
    with pytest.raises(_lib.PgxError, match="needs the resident points' normals"):
        gpu_ctx.solve_minimal(samples)
    gpu_ctx.set_normals(nrm)
    gpu_ctx.set_points(_lib.CYLINDER3D, pts)                 # a second pgx_set_points invalidates them
    with pytest.raises(_lib.PgxError, match="needs the resident points' normals"):
        gpu_ctx.solve_minimal(samples)
    gpu_ctx.set_normals(nrm)                                 # the context stays usable
    assert np.array_equal(gpu_ctx.solve_minimal(samples), first)
    # the other types' solvers take no notice of resident normals
    gpu_ctx.set_points(_lib.LINE3D, pts)
    lines = gpu_ctx.solve_minimal(samples)
    gpu_ctx.set_normals(nrm)
    assert np.array_equal(gpu_ctx.solve_minimal(samples), lines)


# ---- the refit ----------------------------------------------------------------------------------------------------------------------------
def _numpy_G(pts, prm, w=None):
    rows, bad = gn_rows(pts, prm)
    ww = np.ones(len(pts)) if w is None else w
    return (rows[~bad] * ww[~bad, None]).T @ rows[~bad], int(bad.sum())


def test_cylinder_gn_grams(gpu_ctx):
    pts, _, labels, gt = datasets.make_cylinders(n_per_cylinder=4000, n_cylinders=3, n_outliers=2000, seed=6)
    n = pts.shape[0]
    w = np.random.default_rng(1).uniform(0.5, 2.0, n)
    gpu_ctx.set_points(_lib.CYLINDER3D, pts)
    prm = np.column_stack([gt, _estimators._cylinder_frame(gt[:, 3:6])])
    prm[:, :3] += 0.01
    idx = np.stack([np.random.default_rng(s).choice(n, 300, replace=False) for s in range(3)]).astype(np.int32)
    for ww in (w, None):
        Gb, bad = gpu_ctx.gram_batch(_lib.GRAM_CYL_GN, idx, params=prm, weights=ww, wpow=1)
        assert Gb.shape == (3, 6, 6)
        for b in range(3):
            G, cnt, bd = gpu_ctx.gram(_lib.GRAM_CYL_GN, ("index", idx[b]), params=prm[b], weights=ww, wpow=1)
            Gr, _ = _numpy_G(pts[idx[b]], prm[b], None if ww is None else ww[idx[b]])
            assert cnt == 300 and bd == 0 and not bad[b]
            assert np.abs(G - Gr).max() <= 1e-12 * np.abs(Gr).max() and np.abs(Gb[b] - Gr).max() <= 1e-12 * np.abs(Gr).max()
    gpu_ctx.set_labels(labels)
    full = np.vstack([np.concatenate([gt[0], prm[0, 7:]])[None], prm])           # label 0 = the outliers, under the first model
    GL, cntL, badL = gpu_ctx.gram_labels(_lib.GRAM_CYL_GN, 4, params=full, weights=w, wpow=1)
    for k in range(4):
        G, cnt, bd = gpu_ctx.gram(_lib.GRAM_CYL_GN, ("label", k), params=full[k], weights=w, wpow=1)
        sel = labels == k
        Gr, _ = _numpy_G(pts[sel], full[k], w[sel])
        assert cnt == cntL[k] == sel.sum() and bd == badL[k] == 0 and np.array_equal(G, GL[k])     # bitwise the single-label call
        assert np.abs(G - Gr).max() <= 1e-12 * np.abs(Gr).max()
    # a point on the axis has no row and is counted
    on_axis = pts.copy()
    on_axis[idx[0, 7]] = prm[0, :3]
    gpu_ctx.set_points(_lib.CYLINDER3D, on_axis)
    G, cnt, bd = gpu_ctx.gram(_lib.GRAM_CYL_GN, ("index", idx[0]), params=prm[0], wpow=1)
    Gr, nbad = _numpy_G(on_axis[idx[0]], prm[0])
    assert (cnt, bd, nbad) == (300, 1, 1) and np.abs(G - Gr).max() <= 1e-12 * np.abs(Gr).max()
    assert gpu_ctx.gram_batch(_lib.GRAM_CYL_GN, idx, params=prm, wpow=1)[1].astype(bool).tolist() == [bool((row == idx[0, 7]).any()) for row in idx]
    for bad_params in (prm[0, :7], np.zeros(12)):
        with pytest.raises(_lib.PgxError, match="needs 3-D points and 10 parameters"):
            gpu_ctx.gram(_lib.GRAM_CYL_GN, ("index", idx[0]), params=bad_params, wpow=1)
    # the three entry points state the same fit
    gpu_ctx.set_points(_lib.CYLINDER3D, pts)
    gpu_ctx.set_labels(labels)
    est = _estimators.CylinderEstimator()
    inits = [gt[0]] + [g + np.array([0.01, -0.01, 0.01, 0.01, 0.0, -0.01, 0.01]) for g in gt]
    per_label = est.nonminimal_labels(gpu_ctx, 4, weights=w, inits=inits, skip=(0,))
    for k in range(3):
        (m,) = per_label[k + 1]
        assert abs(abs(m[3:6] @ gt[k, 3:6]) - 1.0) < 1e-5 and abs(m[6] - gt[k, 6]) < 1e-3
        (one,) = est.nonminimal(gpu_ctx, ("label", k + 1), weights=w, init=inits[k + 1])
        assert np.abs(one - m).max() < 1e-10
    assert [len(f) for f in est.nonminimal_batch(gpu_ctx, np.flatnonzero(labels == 1)[:600].reshape(3, 200), init=inits[1])] == [1, 1, 1]


def test_cylinder_refit_against_gauss_newton_at_50_digits_on_the_device(gpu_ctx):
    """the rule of test_cylinders_cpu.py on the device's Gram matrices: within 32 eps x the condition number of the reference's own
    normal matrix x the parameter's scale of the 50-digit answer, on the same fixtures"""
    pytest.importorskip("mpmath")
    worst = np.zeros(3)
    for n, offset, weighted in REFIT_CASES:
        pts, w, gt, start = refit_fixture(n, offset, weighted, seed=n + int(offset) + weighted)
        ref = gn_reference(pts, w, start)
        assert ref[4]
        gpu_ctx.set_points(_lib.CYLINDER3D, pts)
        est = _estimators.CylinderEstimator()
        (m,) = est.nonminimal(gpu_ctx, ("index", np.arange(n, dtype=np.int32)), weights=w, init=start)
        ratios = np.array(refit_ratios(m, ref, pts))
        worst = np.maximum(worst, ratios)
        assert (ratios <= 1.0).all(), (n, offset, weighted, ratios)
    print("worst ratios on the device (axis offset, direction, radius):", worst.tolist())


# ---- hand-over ------------------------------------------------------------------------------------------------------------------------------
def test_cylinder_handover_between_types_on_one_context(gpu_ctx):
    """planes, then cylinders, then spheres, then cylinders on the same n: nothing of one type's rows, lanes or normals survives into
    the next, and the radius range - context state by pgx.h, not a point set's - is the one last set, for whichever solver reads it"""
    n = 20011
    pts, nrm, models = make_problem(n, 64, seed=5)
    rng = np.random.default_rng(7)
    planes = np.column_stack([rng.normal(size=(64, 3)), rng.uniform(-10, 0, 64)])
    planes[:, :3] /= np.linalg.norm(planes[:, :3], axis=1)[:, None]
    spheres = np.column_stack([rng.uniform(0, 10, (64, 3)), rng.uniform(0.5, 5.0, 64)])
    samples = rng.integers(0, n, (64, 2)).astype(np.int32)
    four = rng.integers(0, n, (64, 4)).astype(np.int32)
    est = _estimators.CylinderEstimator()
    est.normals = nrm

    def sq_plane(p, m):
        r = np.abs(((m[0] * p[:, 0] + m[1] * p[:, 1]) + m[2] * p[:, 2]) + m[3])
        return r * r

    def sq_sphere(p, m):
        dx, dy, dz = p[:, 0] - m[0], p[:, 1] - m[1], p[:, 2] - m[2]
        r = np.abs(np.sqrt((dx * dx + dy * dy) + dz * dz) - m[3])
        return r * r
    gpu_ctx.set_compound(None)
    gpu_ctx.set_radius_range()
    for step, (mt, hyps, fn) in enumerate(((_lib.PLANE3D, planes, sq_plane), (_lib.CYLINDER3D, models, sq_cylinder),
                                           (_lib.SPHERE3D, spheres, sq_sphere), (_lib.CYLINDER3D, models, sq_cylinder))):
        gpu_ctx.set_points(mt, pts)
        got = gpu_ctx.score(hyps, T2_NOMINAL, want_masks=True)
        ref = ref_score(fn, pts, hyps, T2_NOMINAL)
        assert np.array_equal(got["counts"], ref["counts"]) and np.array_equal(got["masks"], ref["masks"]), mt
        assert ref["counts"].max() > 0
        if mt == _lib.CYLINDER3D:
            with pytest.raises(_lib.PgxError, match="needs the resident points' normals"):
                gpu_ctx.solve_minimal(samples)               # the normals of the earlier cylinder step are gone
            gpu_ctx.set_normals(nrm)
            est.radius_range = (0.0, np.inf) if step == 1 else (0.4, 0.9)      # step 3 runs under the range the sphere step left
            solved = gpu_ctx.solve_minimal(samples)
            assert np.array_equal(solved, _want(est, pts, samples, 64), equal_nan=True)
            assert step == 3 or np.isfinite(solved).all(1).sum() > 20
            fin = np.isfinite(solved).all(1)
            assert step == 1 or ((solved[fin, 6] >= 0.4) & (solved[fin, 6] <= 0.9)).all()
        elif mt == _lib.SPHERE3D:
            gpu_ctx.set_radius_range(0.4, 0.9)
            sph = gpu_ctx.solve_minimal(four)
            fin = np.isfinite(sph).all(1)
            assert ((sph[fin, 3] >= 0.4) & (sph[fin, 3] <= 0.9)).all()
    gpu_ctx.set_radius_range()


# ---- end to end -----------------------------------------------------------------------------------------------------------------------
SIGMA = 0.01
MPN = 100      # minimum_point_number of the end-to-end tests: an eighth of a cylinder's 800 points.  A shell of width 3 x threshold about a
#                cylinder of radius 1 and length 6 holds 2 pi x 1 x 6 x 0.15 = 5.7 of the box's 1000 volume units: 5 of the 800 outliers


def _scene(seed):
    pts, nrm, gen, gt = datasets.make_cylinders(n_per_cylinder=800, n_cylinders=3, n_outliers=800, sigma=SIGMA, normal_noise_deg=5.0,
                                                seed=seed)
    order = np.random.default_rng(0).permutation(len(pts))
    pts, nrm, gen = np.ascontiguousarray(pts[order]), np.ascontiguousarray(nrm[order]), gen[order]
    ends = []
    for k, g in enumerate(gt):                               # the extreme projections of the cylinder's own points onto the true axis
        t = (pts[gen == k + 1] - g[:3]) @ g[3:6]
        ends.append(np.array([g[:3] + t.min() * g[3:6], g[:3] + t.max() * g[3:6]]))
    return pts, nrm, gen, gt, ends


def _matches(m, g, e):
    """the found cylinder m is the ground truth g: radius within 2 sigma, axis within 2 sigma of both ends of the true segment"""
    axis = np.concatenate([m[:6], [0.0]])
    return abs(m[6] - g[6]) < 2 * SIGMA and (np.sqrt(sq_cylinder(e, axis)) < 2 * SIGMA).all()


def _check_call(cyl, labels, pts, gt, ends):
    assert cyl.ndim == 2 and cyl.shape[1] == 7 and cyl.dtype == np.float64
    assert labels.shape == (len(pts),) and labels.dtype == np.int32
    if len(cyl):
        assert np.abs(np.linalg.norm(cyl[:, 3:6], axis=1) - 1.0).max() <= 4 * EPS
    return [any(_matches(m, g, e) for m in cyl) for g, e in zip(gt, ends)]


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_find_cylinders_end_to_end(seed):
    """three cylinders of 800 points, 800 uniform outliers, 1 cm noise along the radius, normals within 5 degrees of radial with random
    sign, points shuffled; every default except minimum_point_number = MPN.  Every returned cylinder is a ground truth one and at least
    two of the three are found.  Measured on an MI355X: three returned and three of three found for each of the seeds 0, 1 and 2 with
    the default sampler, and for samplers 0, 1 and 2 on seed 0 with weights (test_find_cylinders_other_samplers_and_weights prints its
    counts); DESIGN.md 4.9 has them too."""
    pts, nrm, gen, gt, ends = _scene(seed)
    cyl, labels = px.findCylinders(pts, nrm, minimum_point_number=MPN)
    found = _check_call(cyl, labels, pts, gt, ends)
    print(f"seed {seed}: returned {len(cyl)}, found {sum(found)} of 3")
    for m in cyl:                                            # every returned cylinder matches a ground truth
        assert any(_matches(m, g, e) for g, e in zip(gt, ends)), (m, gt)
    assert sum(found) >= 2, (cyl, gt)
    keep = [k for k, f in enumerate(found) if f]
    assert len(cyl) == len(keep)                             # no ground truth is returned twice
    remap = np.zeros(4, dtype=gen.dtype)                     # a cylinder that was not found counts as outliers
    remap[np.array(keep) + 1] = np.arange(1, len(keep) + 1)
    _check_labelling(np.sqrt(np.column_stack([sq_cylinder(pts, gt[k]) for k in keep])), labels, remap[gen], THR)


@pytest.mark.parametrize("sampler_id", [0, 1, 2])
def test_find_cylinders_other_samplers_and_weights(sampler_id):
    pts, nrm, gen, gt, ends = _scene(0)
    w = np.random.default_rng(1).uniform(0.5, 1.5, len(pts))
    cyl, labels = px.findCylinders(pts, nrm, w, minimum_point_number=MPN, sampler_id=sampler_id, radius_range=(0.1, 2.0))
    found = _check_call(cyl, labels, pts, gt, ends)
    print(f"sampler {sampler_id}: returned {len(cyl)}, found {sum(found)} of 3")
    assert ((cyl[:, 6] >= 0.1) & (cyl[:, 6] <= 2.0)).all()


def test_find_cylinders_survives_bad_normals():
    """non-finite and zero normals in rows the samplers use: no crash, well-formed arrays"""
    pts, nrm, gen, gt, ends = _scene(1)
    nrm = nrm.copy()
    nrm[::7] = np.nan
    nrm[1::7] = 0.0
    nrm[2::7, 0] = np.inf
    cyl, labels = px.findCylinders(pts, nrm, minimum_point_number=MPN, max_iters=200)
    _check_call(cyl, labels, pts, gt, ends)
