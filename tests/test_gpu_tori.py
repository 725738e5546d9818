"""findTori on the MI355X: every layer of the torus type against the numpy restatement of its arithmetic (tests/torus_model.py), against
the oracle where it can serve - its 2-D circle with the model (R, 0, r) on the rows (rho, h) is the torus residual's last step bit for
bit - and against Gauss-Newton at 50 digits; and the public call end to end.

Residual<kTorus3D> (residuals.hip.h) is the contract: q = Residual<kLine3D>::squared, rho = sqrt(q), h = (e0 d0 + e1 d1) + e2 d2,
t = rho - R, w = sqrt(t t + h h), plain = |w - r|, squared = plain^2, inlier iff squared < T2."""
import numpy as np
import pytest

import pyprogressivex as px
from cone_model import sq_cone
from cylinder_model import sq_cylinder
from primitive_helpers import _check_labelling, _check_scores, ref_score
from pyprogressivex import _estimators, _lib, _rng, datasets, parallel
from torus_model import (E2E, E2E_SEEDS, E2E_T, EPS, REFIT_CASES, frame_of, gn_rows, near_threshold_cases, near_threshold_points,
                         refit_case, refit_ratios, rho_h_rows, scaled_model, sq_torus, sweep_is_crossed)

pytestmark = pytest.mark.gpu

THR = 0.05
T2_NOMINAL = 2.25 * THR * THR


def make_problem(n, M, seed):
    """points of make_tori (truncated to n) and M hypotheses: ground truth, perturbed (1e-7 .. 1), random, (d, R, r) scaled together by
    2^+-40, d alone by 1e-3 and 7, a radius negated; and the special ones: an all-NaN model, one NaN entry, an Inf entry, d = 0 with
    R = r (every residual is 0), the centre far off the scene, R = 0 (a sphere), r = 0 (the spine's tube), radii beyond the filter's
    range and an Inf radius"""
    rng = np.random.default_rng(seed)
    k = max(n // 8, 1)
    pts, nrm, _, gt = datasets.make_tori(n_per_torus=k, n_tori=4, n_outliers=max(n - 4 * k, 1), seed=seed)
    pick = rng.permutation(pts.shape[0])[:n]
    pts, nrm = np.ascontiguousarray(pts[pick]), np.ascontiguousarray(nrm[pick])
    models = np.empty((M, 8))
    for j in range(M):
        kind = j % 5
        g = gt[j % len(gt)].copy()
        if kind == 1:
            g += rng.normal(0, 10.0 ** rng.uniform(-7, 0), 8)
        elif kind == 2:
            g = np.concatenate([rng.uniform(0, 10.0, 3), rng.normal(size=3), [rng.uniform(0.5, 3.0), rng.uniform(0.05, 0.6)]])
        elif kind == 3:
            g[3:8] *= rng.choice([2.0 ** -40, 2.0 ** 40])
        elif kind == 4:
            f = rng.choice([1e-3, 7.0, -1.0, -2.0])
            if f > 0:
                g[3:6] *= f
            else:
                g[6 + int(f == -2.0)] *= -1.0
        models[j] = g
    if M >= 7:
        models[M - 1] = np.nan
        models[M - 2, rng.integers(0, 8)] = np.nan
        models[M - 3, rng.integers(0, 6)] = np.inf
        models[M - 4, 3:6] = 0.0                              # d = 0: every residual is ||R| - r|,
        models[M - 4, 6:8] = 1.0                              # 0 here: every point an inlier
        models[M - 5, :3] = gt[1, :3] + np.array([3e6, -2e6, 1e6])                    # the centre far outside the scene
    if M >= 64:
        models[M - 6, 6] = 0.0                                # R = 0: the sphere of radius r about the centre
        models[M - 7, 7] = 0.0                                # r = 0: the distance to the spine
        models[M - 8, 6] = 1e18                               # beyond the filter's range: the exact path decides
        models[M - 9, 7] = 1e18
        models[M - 10, 6] = np.inf
        models[M - 11, 7] = -np.inf
    return pts, nrm, models


@pytest.mark.parametrize("n", [63, 64, 65, 129, 2048])
@pytest.mark.parametrize("M", [1, 64, 65])
def test_torus_scoring_bit_exact(gpu_ctx, n, M):
    pts, _, models = make_problem(n, M, seed=n + M)
    T2 = T2_NOMINAL
    if n >= 2048 and M >= 7:                                # a point exactly on the threshold: r^2 == T2 is not an inlier
        on = int(np.flatnonzero(sq_torus(pts, models[0]) > 0)[0])
        T2 = float(sq_torus(pts[on:on + 1], models[0])[0])
        assert T2 > 0
    comp = np.random.default_rng(n).uniform(0, 1, n)
    gpu_ctx.score_set_global_n(0)
    gpu_ctx.set_points(_lib.TORUS3D, pts)
    gpu_ctx.set_compound(comp)
    got = gpu_ctx.score(models, T2, has_compound=True, exponent=2, want_masks=True)
    ref = ref_score(sq_torus, pts, models, T2, comp)
    if n >= 2048 and M >= 7:
        assert not (ref["masks"][0, on >> 6] >> np.uint64(on & 63)) & np.uint64(1)
    if M >= 7:
        assert ref["counts"][M - 1] == ref["counts"][M - 2] == ref["counts"][M - 3] == 0
        assert ref["counts"][M - 4] == n
    if M >= 64:
        assert ref["counts"][M - 10] == ref["counts"][M - 11] == ref["counts"][M - 8] == ref["counts"][M - 9] == 0
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
    """one problem and its numpy reference for every switch of test_torus_culls_are_invisible: large enough that the planner takes the
    cull and the group-major kernel"""
    pts, _, models = make_problem(30011, 300, seed=11)
    comp = np.random.default_rng(2).uniform(0, 1, pts.shape[0])
    return pts, models, comp, ref_score(sq_torus, pts, models, T2_NOMINAL, comp)


@pytest.mark.parametrize("switch", [None, "PGX_NO_FILTER", "PGX_SCORE_NO_CULL", "PGX_NO_GROUP", "PGX_NO_SORT", "PGX_SETPOINTS_HOST"])
def test_torus_culls_are_invisible(switch, monkeypatch, cull_problem):
    pts, models, comp, ref = cull_problem
    T2 = T2_NOMINAL
    if switch:
        monkeypatch.setenv(switch, "1")
    ctx = _lib.Context(0)
    if switch:
        monkeypatch.delenv(switch)
    try:
        ctx.set_points(_lib.TORUS3D, pts)
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


def test_torus_filter_proof_near_threshold(gpu_ctx):
    """every one of the 81 point sets of the CPU budget test (coordinate scales 1 .. 1e6, offsets to 1e6, thresholds from 1e-3 x nominal
    to half the tube radius, R / r from 1.05 to 50, (d, R, r) scaled by 2^-40, 1 and 2^40), 2048 points a case, scored on the device
    with the cull and the f32 filter on: the masks are the exact ones"""
    f32_seen = 0
    seen = set()
    for k, (rng, gt, T, e, ratio, coord, oc) in enumerate(near_threshold_cases()):
        seen.add((e, ratio, coord, oc))
        n = 2048
        pts = near_threshold_points(rng, gt, T, n)
        pts[n // 2:] = gt[:3] + rng.uniform(-3, 3, (n - n // 2, 3)) * max(T, coord)      # and some points off the surface
        hyp, Ts = scaled_model(gt, T, e)
        hyps = np.tile(hyp, (64, 1))
        hyps[1::2, :3] += rng.normal(0, 1e-6 * T, (32, 3))
        hyps[5, 3:6] = 0.0
        hyps[9, 3:8] *= 2.0 ** 3                             # other scales next to the batch's own
        hyps[11, 6:8] *= 1.0 + 2.0 ** -12
        hyps[13, 3:6] *= -1.0
        T2 = Ts * Ts
        gpu_ctx.set_points(_lib.TORUS3D, pts)
        gpu_ctx.set_compound(None)
        got = gpu_ctx.score(hyps, T2, want_masks=True)
        ref = ref_score(sq_torus, pts, hyps, T2)
        assert np.array_equal(got["counts"], ref["counts"]) and np.array_equal(got["masks"], ref["masks"]), (k, coord, T, e, ratio)
        assert 0 < ref["counts"][0] < n
        f32_seen += gpu_ctx.score_stats(T2)["filter"] == "f32"
    assert f32_seen > 0
    assert len(seen) == 81 and sweep_is_crossed(seen)


def _circle2d(m):
    return np.array([m[6], 0.0, m[7]])


def test_torus_pointwise_kernels_bit_exact(gpu_ctx, oracle):
    """preference, the PEARL unary table, the residual sums and the inlier/outlier cut: against numpy, and the cut against the oracle's
    on its 2-D circle type's rows (rho, h) with the model (R, 0, r), whose residuals are the torus' bit for bit"""
    pts, _, models = make_problem(20011, 8, seed=3)
    n = pts.shape[0]
    thr, lam = THR, 0.3
    T2 = T2_NOMINAL
    gpu_ctx.set_points(_lib.TORUS3D, pts)
    gpu_ctx.set_compound(None)
    for k in (0, 1, 2):
        pref = gpu_ctx.preference(models[k], T2, slot=k, want_pref=True)["pref"]
        assert np.array_equal(pref, np.maximum(0.0, 1.0 - sq_torus(pts, models[k]) / T2))
    K = 8
    assert np.isnan(models[7]).all() and np.isnan(models[6]).any() and np.isinf(models[5]).any() and not models[4, 3:6].any()
    Dq = gpu_ctx.pearl_unary(models[:K], thr, lam, want_table=True)
    oml = 1.0 - lam
    ref = np.empty((n, K + 1), np.int64)
    for k in range(K):
        sq = sq_torus(pts, models[k])
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
        r = np.sqrt(sq_torus(pts[labels == k], finite[k]))
        assert abs(sums[k] - r.sum()) <= 1e-12 * max(abs(r.sum()), 1e-300)
        assert abs(gpu_ctx.residual_sum(finite[k], k) - r.sum()) <= 1e-12 * max(abs(r.sum()), 1e-300)
    graph = gpu_ctx.graph_build(pts, _lib.GRAPH_KNN_IN_BALL, radius=0.5, k=5)
    for m in (models[0], models[1]):
        rows = rho_h_rows(pts, m)
        assert np.array_equal(oracle.squared_residuals(10, rows, _circle2d(m)), sq_torus(pts, m))
        for lam_gc in (0.1, 0.5):
            flags = gpu_ctx.gc_labeling(m, T2, lam_gc)
            assert np.array_equal(flags, oracle.gc_labeling(10, rows, _circle2d(m), T2, lam_gc, graph)), lam_gc
            assert np.array_equal(np.flatnonzero(flags), gpu_ctx.gc_inliers(m, T2, lam_gc))
    assert gpu_ctx.gc_labeling(models[0], T2, 0.1).sum() > 1000


def test_torus_graph_and_expansion_match_the_oracle(gpu_ctx, oracle):
    """the graph against the oracle's; one expansion on the type's unary table (computed in numpy, equal to the device's) against the
    oracle's expansion, and its energy"""
    pts, _, _, gt = datasets.make_tori(n_per_torus=1500, n_tori=3, n_outliers=1500, seed=12)
    n = pts.shape[0]
    gpu_ctx.set_points(_lib.TORUS3D, pts)
    graph = gpu_ctx.graph_build(pts, _lib.GRAPH_KNN_IN_BALL, radius=0.4, k=5)
    for a, b in zip(graph, oracle.graph_build(pts, _lib.GRAPH_KNN_IN_BALL, radius=0.4, k=5)):
        assert np.array_equal(a, b)
    lam, h = 0.1, 6.0
    oml, T2 = 1.0 - lam, T2_NOMINAL
    Dq = np.empty((n, 4), np.int64)
    for k in range(3):
        sq = sq_torus(pts, gt[k])
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
def _want_rows(est, pts, samples):
    """the 2 S rows the device solver must give: the estimator's, NaN where a sample has an index outside the points"""
    ok = (samples >= 0).all(1) & (samples < len(pts)).all(1)
    want = np.full((2 * len(samples), 8), np.nan)
    if ok.any():
        rows = est.minimal_rows(pts, samples[ok])
        keep = np.flatnonzero(ok)
        want[2 * keep] = rows[0::2]
        want[2 * keep + 1] = rows[1::2]
    return want


@pytest.fixture(scope="module")
def solver_scene():
    pts, nrm, _, _ = datasets.make_tori(n_per_torus=500, n_tori=3, n_outliers=500, seed=2, normal_noise_deg=1.0)
    pts, nrm = pts.copy(), nrm.copy()
    pts[5], nrm[5] = pts[4], nrm[4]                          # a duplicate point with the same normal
    nrm[6] = 0.0                                             # a zero normal: qa = 0 exactly in whichever place of the sample
    nrm[7] = -4.0 * nrm[3]                                   # parallel to 3's
    pts[8] = [1e200, 0.0, 0.0]
    nrm[9] = [1e200, 1e200, 0.0]                             # a long normal: legal
    nrm[2, 1] = np.nan
    nrm[1, 0] = np.inf
    return pts, nrm


@pytest.mark.parametrize("S", [1, 63, 64, 65, 129])
def test_torus_minimal_solver_bitwise_the_estimator(gpu_ctx, solver_scene, S):
    pts, nrm = solver_scene
    n = pts.shape[0]
    est = _estimators.TorusEstimator()
    est.normals = nrm
    gpu_ctx.set_radius_range()
    gpu_ctx.set_major_radius_range()
    gpu_ctx.set_points(_lib.TORUS3D, pts)
    gpu_ctx.set_normals(nrm)
    # mostly all-inlier samples of one torus (the first 1500 points are the three tori's), some across
    rng = np.random.default_rng(S)
    samples = (rng.integers(0, 3, (S, 1)) * 500 + rng.integers(10, 500, (S, 4))).astype(np.int32)
    samples[::5] = rng.integers(10, n, (len(samples[::5]), 4))
    # no model for certain: a zero normal in each place, a NaN normal, indices outside the points
    special = np.array([[6, 12, 13, 14], [12, 6, 13, 14], [12, 13, 6, 14], [12, 13, 14, 6], [2, 14, 16, 18], [-1, 2, 3, 4], [n, 0, 1, 2],
                        [20, 21, 22, n]], np.int32)[:min(S - 1, 8)]
    samples[:len(special)] = special                         # (S = 1: the one sample is an ordinary one)
    if S > 13:                                               # legal but hard: the same point twice, parallel normals, 1e200, Inf
        samples[8:13] = [[4, 5, 20, 21], [3, 7, 14, 15], [8, 13, 15, 16], [9, 13, 15, 17], [1, 15, 17, 19]]
    got = gpu_ctx.solve_minimal(samples)
    assert got.shape == (2 * S, 8)
    assert np.array_equal(got, _want_rows(est, pts, samples), equal_nan=True)
    assert np.isnan(got[:2 * len(special)]).all()
    fin = got[np.isfinite(got).all(1)]
    assert S == 1 or len(fin) > S // 4
    assert (np.isnan(got).all(1) | np.isfinite(got).all(1)).all()                      # a row is a model or all NaN
    if len(fin):
        assert np.abs(np.sqrt((fin[:, 3:6] ** 2).sum(axis=1)) - 1.0).max() <= 4 * EPS and (fin[:, 6] > fin[:, 7]).all() and (fin[:, 7] >= 0).all()
    if len(special):
        assert (gpu_ctx.score(got[:2 * len(special)], T2_NOMINAL)["counts"] == 0).all()
    if S == 129:                                             # both ranges: inclusive, honoured by device and estimator alike
        assert (~np.isnan(got[0::2, 0])).sum() > 10 and (~np.isnan(got[1::2, 0])).sum() > 10        # both slots are in use
        for col, setter, attr in ((7, gpu_ctx.set_radius_range, "radius_range"), (6, gpu_ctx.set_major_radius_range, "major_radius_range")):
            lo, hi = np.sort(fin[:, col])[[len(fin) // 4, 3 * len(fin) // 4]]
            setter(float(lo), float(hi))
            setattr(est, attr, (float(lo), float(hi)))
            ranged = gpu_ctx.solve_minimal(samples)
            setter()
            assert np.array_equal(ranged, _want_rows(est, pts, samples), equal_nan=True)
            setattr(est, attr, (0.0, np.inf))
            kept = np.isfinite(ranged).all(1)
            assert 0 < kept.sum() < len(fin) and ranged[kept, col].min() == lo and ranged[kept, col].max() == hi


def test_torus_device_drawn_samples_equal_the_generator(gpu_ctx, solver_scene):
    """pgx_solve_minimal_sampled with m = 4 and two slots: the rows are _rng's for the uniform, NAPSAC and PROSAC samplers, the models
    the solver's"""
    pts, nrm = solver_scene
    pts = np.where(np.isfinite(pts) & (np.abs(pts) < 1e100), pts, 5.0)       # (the graph is built on finite coordinates)
    n = pts.shape[0]
    est = _estimators.TorusEstimator()
    est.normals = nrm
    gpu_ctx.set_radius_range()
    gpu_ctx.set_major_radius_range()
    gpu_ctx.set_points(_lib.TORUS3D, pts)
    gpu_ctx.set_normals(nrm)
    off, idx, _ = gpu_ctx.graph_build(pts, _lib.GRAPH_KNN_IN_BALL, radius=0.5, k=5)
    tops = np.minimum(n, np.arange(4, 4 + 512)).astype(np.int32)
    gpu_ctx.sampler_prosac_set(tops)
    want_rows = dict(uniform=_rng.uniform_samples(12345, 7, 512, n, 4), napsac=_rng.napsac_samples(12345, 7, 512, n, 4, off, idx),
                     prosac=_rng.prosac_samples(12345, 7, 512, n, 4, tops))
    for sampler in ("uniform", "napsac", "prosac"):
        models, smp = gpu_ctx.solve_minimal_sampled(12345, 7, 512, fetch_samples=True, sampler=sampler)
        assert smp.shape == (512, 4) and models.shape == (1024, 8)
        assert np.array_equal(smp, want_rows[sampler].astype(np.int32)), sampler
        assert np.array_equal(models, _want_rows(est, pts, smp), equal_nan=True), sampler
        assert np.isfinite(models).all(1).sum() > 20, sampler


def test_torus_solver_needs_resident_normals(gpu_ctx, solver_scene):
    pts, nrm = solver_scene
    samples = np.array([[20, 30, 40, 50], [40, 50, 60, 70]], np.int32)
    gpu_ctx.set_radius_range()
    gpu_ctx.set_major_radius_range()
    gpu_ctx.set_points(_lib.TORUS3D, pts)
    with pytest.raises(_lib.PgxError, match="pgx_solve_minimal: the torus solver needs the resident points' normals"):
        gpu_ctx.solve_minimal(samples)
    with pytest.raises(_lib.PgxError, match="the torus solver needs the resident points' normals"):
        gpu_ctx.solve_minimal_sampled(1, 0, 8)
    gpu_ctx.set_normals(nrm)
    first = gpu_ctx.solve_minimal(samples)
    assert first.shape == (4, 8)
    gpu_ctx.set_normals(None)                                # (NULL, 0) clears
    with pytest.raises(_lib.PgxError, match="needs the resident points' normals"):
        gpu_ctx.solve_minimal(samples)
    gpu_ctx.set_normals(nrm)
    gpu_ctx.set_points(_lib.TORUS3D, pts)                    # a second pgx_set_points invalidates them
    with pytest.raises(_lib.PgxError, match="the torus solver needs the resident points' normals"):
        gpu_ctx.solve_minimal(samples)
    gpu_ctx.set_normals(nrm)                                 # the context stays usable
    assert np.array_equal(gpu_ctx.solve_minimal(samples), first, equal_nan=True)
    # the major radius range is checked like the radius range, and a refused call leaves the state as it was
    for bad in ((-1.0, 2.0), (3.0, 2.0), (np.nan, 2.0), (1.0, np.nan)):
        with pytest.raises(_lib.PgxError, match="pgx_set_major_radius_range: need 0 <= Rmin <= Rmax"):
            gpu_ctx.set_major_radius_range(*bad)
    assert np.array_equal(gpu_ctx.solve_minimal(samples), first, equal_nan=True)
    gpu_ctx.set_major_radius_range(0.0, np.inf)              # +inf is allowed
    gpu_ctx.set_points(_lib.HOMOGRAPHY_SYM, np.zeros((8, 4)))
    with pytest.raises(_lib.PgxError, match=r"no device solver for model type 5 yet \(built: .*4-point torus, "):
        gpu_ctx.solve_minimal(samples)


# ---- the refit ----------------------------------------------------------------------------------------------------------------------------
def _numpy_G(pts, prm, w=None):
    rows, bad = gn_rows(pts, prm)
    ww = np.ones(len(pts)) if w is None else w
    return (rows[~bad] * ww[~bad, None]).T @ rows[~bad], int(bad.sum())


def test_torus_gn_grams(gpu_ctx):
    pts, _, labels, gt = datasets.make_tori(n_per_torus=4000, n_tori=3, n_outliers=2000, seed=6)
    n = pts.shape[0]
    w = np.random.default_rng(1).uniform(0.5, 2.0, n)
    gpu_ctx.set_points(_lib.TORUS3D, pts)
    prm = np.column_stack([gt, _estimators._cylinder_frame(gt[:, 3:6])])
    prm[:, :3] += 0.01
    idx = np.stack([np.random.default_rng(s).choice(n, 300, replace=False) for s in range(3)]).astype(np.int32)
    for ww in (w, None):
        Gb, bad = gpu_ctx.gram_batch(_lib.GRAM_TORUS_GN, idx, params=prm, weights=ww, wpow=1)
        assert Gb.shape == (3, 8, 8)
        for b in range(3):
            G, cnt, bd = gpu_ctx.gram(_lib.GRAM_TORUS_GN, ("index", idx[b]), params=prm[b], weights=ww, wpow=1)
            Gr, _ = _numpy_G(pts[idx[b]], prm[b], None if ww is None else ww[idx[b]])
            assert cnt == 300 and bd == 0 and not bad[b]
            assert np.abs(G - Gr).max() <= 1e-12 * np.abs(Gr).max() and np.abs(Gb[b] - Gr).max() <= 1e-12 * np.abs(Gr).max()
    gpu_ctx.set_labels(labels)
    full = np.vstack([np.concatenate([gt[0], prm[0, 8:]])[None], prm])           # label 0 = the outliers, under the first model
    GL, cntL, badL = gpu_ctx.gram_labels(_lib.GRAM_TORUS_GN, 4, params=full, weights=w, wpow=1)
    for k in range(4):
        G, cnt, bd = gpu_ctx.gram(_lib.GRAM_TORUS_GN, ("label", k), params=full[k], weights=w, wpow=1)
        sel = labels == k
        Gr, _ = _numpy_G(pts[sel], full[k], w[sel])
        assert cnt == cntL[k] == sel.sum() and bd == badL[k] == 0 and np.array_equal(G, GL[k])     # bitwise the single-label call
        assert np.abs(G - Gr).max() <= 1e-12 * np.abs(Gr).max()
    # a point at the centre (on the axis) and a point on the spine have no row and are counted; in binary numbers, so that rho and w
    # are 0 exactly
    upright = np.array([1.0, 2.0, 3.0, 0.0, 0.0, 1.0, 1.5, 0.25, 1.0, 0.0, 0.0])
    special = pts.copy()
    special[idx[0, 7]] = [1.0, 2.0, 3.5]
    special[idx[0, 9]] = [2.5, 2.0, 3.0]
    gpu_ctx.set_points(_lib.TORUS3D, special)
    G, cnt, bd = gpu_ctx.gram(_lib.GRAM_TORUS_GN, ("index", idx[0]), params=upright, wpow=1)
    Gr, nbad = _numpy_G(special[idx[0]], upright)
    assert (cnt, bd, nbad) == (300, 2, 2) and np.abs(G - Gr).max() <= 1e-12 * np.abs(Gr).max()
    for bad_params in (prm[0, :8], np.zeros(12)):
        with pytest.raises(_lib.PgxError, match="needs 3-D points and 11 parameters"):
            gpu_ctx.gram(_lib.GRAM_TORUS_GN, ("index", idx[0]), params=bad_params, wpow=1)
    # the three entry points state the same fit
    gpu_ctx.set_points(_lib.TORUS3D, pts)
    gpu_ctx.set_labels(labels)
    est = _estimators.TorusEstimator()
    bump = np.array([0.01, -0.01, 0.01, 0.01, 0.0, -0.01, 0.01, -0.01])
    inits = [gt[0]] + [g + bump for g in gt]
    per_label = est.nonminimal_labels(gpu_ctx, 4, weights=w, inits=inits, skip=(0,))
    for k in range(3):
        (m,) = per_label[k + 1]
        assert min(np.abs(m[3:6] - gt[k, 3:6]).max(), np.abs(m[3:6] + gt[k, 3:6]).max()) < 2e-3
        assert np.abs(m[6:8] - gt[k, 6:8]).max() < 2e-3 and np.linalg.norm(m[:3] - gt[k, :3]) < 2e-2
        (one,) = est.nonminimal(gpu_ctx, ("label", k + 1), weights=w, init=inits[k + 1])
        assert np.abs(one - m).max() < 1e-9
    assert [len(f) for f in est.nonminimal_batch(gpu_ctx, np.flatnonzero(labels == 1)[:600].reshape(3, 200), init=inits[1])] == [1, 1, 1]


def test_torus_refit_against_gauss_newton_at_50_digits_on_the_device(gpu_ctx):
    """the rule of test_tori_cpu.py on the device's Gram matrices: within 32 eps x the condition number of the reference's own normal
    matrix x the parameter's scale of the 50-digit answer, on the same fixtures"""
    pytest.importorskip("mpmath")
    worst = np.zeros(3)
    for n, offset, weighted in REFIT_CASES:
        pts, w, gt, start, ref = refit_case(n, offset, weighted)
        assert ref[4]
        gpu_ctx.set_points(_lib.TORUS3D, pts)
        est = _estimators.TorusEstimator()
        (m,) = est.nonminimal(gpu_ctx, ("index", np.arange(n, dtype=np.int32)), weights=w, init=start)
        ratios = np.array(refit_ratios(m, ref, pts))
        worst = np.maximum(worst, ratios)
        assert (ratios <= 1.0).all(), (n, offset, weighted, ratios)
    print("worst ratios on the device (centre, direction, radii):", worst.tolist())


# ---- hand-over ------------------------------------------------------------------------------------------------------------------------------
def test_torus_handover_between_types_on_one_context(gpu_ctx):
    """tori, then cylinders, then cones, then the mixed primitives (cylinder rows behind their class), then tori on the same n: nothing
    of one type's rows, lanes or normals survives into the next, and both radius ranges - context state by pgx.h, not a point set's -
    are the ones last set"""
    n = 20011
    pts, nrm, models = make_problem(n, 64, seed=5)
    rng = np.random.default_rng(7)
    cyls = np.column_stack([rng.uniform(0, 10, (64, 3)), rng.normal(size=(64, 3)), rng.uniform(0.3, 3.0, 64)])
    cyls[:, 3:6] /= np.linalg.norm(cyls[:, 3:6], axis=1)[:, None]
    t = np.deg2rad(rng.uniform(5, 60, 64))
    cones = np.column_stack([cyls[:, :6], np.cos(t), np.sin(t)])
    prims = np.column_stack([np.full(64, 14.0), cyls, np.zeros(64)])
    four = rng.integers(0, n, (64, 4)).astype(np.int32)
    four[::2] = (rng.integers(0, 4, (32, 1)) * (n // 8) + rng.integers(0, n // 8, (32, 4))).astype(np.int32)
    two = np.ascontiguousarray(four[:, :2])
    tor_est, cyl_est = _estimators.TorusEstimator(), _estimators.CylinderEstimator()
    # make_problem shuffles: samples within one torus need the generator's order, so the solver runs on samples as drawn
    tor_est.normals = cyl_est.normals = nrm
    gpu_ctx.set_compound(None)
    gpu_ctx.set_radius_range()
    gpu_ctx.set_major_radius_range()
    steps = ((_lib.TORUS3D, models, sq_torus), (_lib.CYLINDER3D, cyls, sq_cylinder), (_lib.CONE3D, cones, sq_cone),
             (_lib.PRIMITIVE3D, prims, lambda p, m: sq_cylinder(p, m[1:8])), (_lib.TORUS3D, models, sq_torus))
    for step, (mt, hyps, fn) in enumerate(steps):
        gpu_ctx.set_points(mt, pts)
        got = gpu_ctx.score(hyps, T2_NOMINAL, want_masks=True)
        ref = ref_score(fn, pts, hyps, T2_NOMINAL)
        assert np.array_equal(got["counts"], ref["counts"]) and np.array_equal(got["masks"], ref["masks"]), mt
        assert ref["counts"].max() > 0
        if mt == _lib.TORUS3D:
            with pytest.raises(_lib.PgxError, match="the torus solver needs the resident points' normals"):
                gpu_ctx.solve_minimal(four)                  # the normals of the earlier step are gone
            gpu_ctx.set_normals(nrm)
            if step == 0:
                gpu_ctx.set_major_radius_range(0.5, 2.5)
                tor_est.major_radius_range = (0.5, 2.5)
            else:                                            # the last step runs under both ranges left behind
                tor_est.radius_range = (0.2, 0.6)
            solved = gpu_ctx.solve_minimal(four)
            assert np.array_equal(solved, _want_rows(tor_est, pts, four), equal_nan=True)
            fin = np.isfinite(solved).all(1)
            assert ((solved[fin, 6] >= 0.5) & (solved[fin, 6] <= 2.5)).all()
            assert step == 0 or ((solved[fin, 7] >= 0.2) & (solved[fin, 7] <= 0.6)).all()
        elif mt == _lib.CYLINDER3D:
            with pytest.raises(_lib.PgxError, match="the cylinder solver needs the resident points' normals"):
                gpu_ctx.solve_minimal(two)
            gpu_ctx.set_normals(nrm)
            gpu_ctx.set_radius_range(0.2, 0.6)
            cyl_est.radius_range = (0.2, 0.6)
            got2 = gpu_ctx.solve_minimal(two)
            ref2, src = cyl_est.minimal(pts, two)
            want = np.full((64, 7), np.nan)
            want[src] = ref2
            assert np.array_equal(got2, want, equal_nan=True)
    gpu_ctx.set_radius_range()
    gpu_ctx.set_major_radius_range()


# ---- end to end -----------------------------------------------------------------------------------------------------------------------
SIGMA = E2E["sigma"]
MPN = 100      # minimum_point_number of the end-to-end tests: an eighth of a torus' 800 points.  A shell of width 3 x threshold about the
#                largest torus (R = 2, r = 0.5: area 4 pi^2 R r = 39.5) holds 5.9 of the box's 1000 volume units: 5 of the 800 outliers


def _scene(seed):
    pts, nrm, gen, gt = datasets.make_tori(seed=seed, **E2E)
    order = np.random.default_rng(0).permutation(len(pts))
    pts, nrm, gen = np.ascontiguousarray(pts[order]), np.ascontiguousarray(nrm[order]), gen[order]
    spines = []
    for g in gt:                                             # sixteen exact points of the true torus' spine (the tube's centre circle)
        e1, e2 = frame_of(g[3:6])
        phi = np.arange(16) * (np.pi / 8)
        spines.append(g[:3] + g[6] * (np.cos(phi)[:, None] * e1 + np.sin(phi)[:, None] * e2))
    return pts, nrm, gen, gt, spines


def _matches(m, g, spine):
    """the found torus m is the ground truth g: the true spine lies within 2 sigma of the found spine (which fixes centre and axis
    together to what the points can resolve: the distance to the found spine is w of the residual, its value with r = 0) and both
    radii are within 3 sigma"""
    on_spine = np.sqrt(sq_torus(spine, np.concatenate([m[:7], [0.0]])))
    return bool((on_spine < 2 * SIGMA).all() and abs(m[6] - g[6]) < 3 * SIGMA and abs(m[7] - g[7]) < 3 * SIGMA)


def _check_call(tori, labels, pts, gt, spines):
    assert tori.ndim == 2 and tori.shape[1] == 8 and tori.dtype == np.float64
    assert labels.shape == (len(pts),) and labels.dtype == np.int32
    if len(tori):
        assert np.abs(np.linalg.norm(tori[:, 3:6], axis=1) - 1.0).max() <= 4 * EPS
        assert (tori[:, 6] > tori[:, 7]).all() and (tori[:, 7] > 0).all()
        assert ((tori[:, 7] >= E2E["minor_radius"][0]) & (tori[:, 7] <= E2E["minor_radius"][1])).all()
        assert ((tori[:, 6] >= E2E["major_radius"][0]) & (tori[:, 6] <= E2E["major_radius"][1])).all()
    return [sum(_matches(m, g, s) for m in tori) for g, s in zip(gt, spines)]


def _find(pts, nrm, w=None, **kw):
    return px.findTori(pts, nrm, w, threshold=E2E_T, minimum_point_number=MPN, radius_range=E2E["minor_radius"],
                       major_radius_range=E2E["major_radius"], **kw)


@pytest.mark.parametrize("seed", E2E_SEEDS)
def test_find_tori_end_to_end(seed):
    """two tori of 800 points (R in (0.8, 2), r in (0.2, 0.5)), 800 uniform outliers, 1 cm noise along the surface normal, normals
    within 2 degrees of the surface's with random sign, points shuffled; every default except minimum_point_number = MPN and both
    radius ranges, the generator's; the run's seed = the scene's, so that the call is a pure function of the scene.

    Asserted on every seed: at least one planted torus is found - its spine within 2 sigma of the found one, both radii within 3
    sigma - and none is found twice.  Found / returned per seed as measured: DESIGN.md 4.15."""
    pts, nrm, gen, gt, spines = _scene(seed)
    tori, labels = _find(pts, nrm, seed=seed)
    found = _check_call(tori, labels, pts, gt, spines)
    unmatched = sum(not any(_matches(m, g, s) for g, s in zip(gt, spines)) for m in tori)
    print(f"seed {seed}: returned {len(tori)}, found {sum(f > 0 for f in found)} of 2, unmatched {unmatched}")
    assert sum(f > 0 for f in found) >= 1, (tori, gt)
    assert max(found) <= 1, (found, tori)                    # no ground truth is returned twice
    keep = [k for k, f in enumerate(found) if f]
    if unmatched == 0:
        remap = np.zeros(3, dtype=gen.dtype)                 # a torus that was not found counts as outliers
        remap[np.array(keep) + 1] = np.arange(1, len(keep) + 1)
        _check_labelling(np.sqrt(np.column_stack([sq_torus(pts, gt[k]) for k in keep])), labels, remap[gen], THR)


@pytest.mark.parametrize("sampler_id", [0, 1, 2])
def test_find_tori_other_samplers_and_weights(sampler_id):
    pts, nrm, gen, gt, spines = _scene(0)
    w = np.random.default_rng(1).uniform(0.5, 1.5, len(pts))
    tori, labels = _find(pts, nrm, w, sampler_id=sampler_id, seed=0)
    found = _check_call(tori, labels, pts, gt, spines)
    print(f"sampler {sampler_id}: returned {len(tori)}, found {sum(f > 0 for f in found)} of 2")


def test_find_tori_survives_bad_normals():
    """non-finite and zero normals in rows the samplers use: no crash, well-formed arrays"""
    pts, nrm, gen, gt, spines = _scene(1)
    nrm = nrm.copy()
    nrm[::7] = np.nan
    nrm[1::7] = 0.0
    nrm[2::7, 0] = np.inf
    tori, labels = _find(pts, nrm, max_iters=200)
    _check_call(tori, labels, pts, gt, spines)
