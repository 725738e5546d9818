"""findOrientedPrimitives on the MI355X.  Model type PGX_ORIENTED_PRIMITIVE3D = 20 is type 18 with one addition, the test of the point's
normal, so every check is bit for bit against the numpy restatement (tests/oriented_model.py, which takes its distances from
tests/primitive_model.py) or against type 18 on the device: scoring on both paths, the pointwise kernels, the solver, then the public
call end to end.  The shapes are those of tests/test_gpu_primitives.py."""
import os

import numpy as np
import pytest

import pyprogressivex as px
from oriented_model import compatible, kappa_of, prefix_compatible, sq_fn, sq_oriented
from primitive_helpers import _check_scores, ref_score
from primitive_model import CLASSES, PLANE, class_of, sq_primitive
from pyprogressivex import _estimators, _lib, datasets
from test_gpu_primitives import ANGLE_RANGE, COMBOS, E2E, MPN, RADII, RADIUS_RANGE, SINES, _matched, _samples, _shuffled, mixed_batch

pytestmark = pytest.mark.gpu

THR = 0.05
T2 = 2.25 * THR * THR
TOL = 20.0
KAPPA = kappa_of(TOL)
NEEDS = "the oriented residual needs the resident points' normals"


@pytest.fixture(scope="module")
def small():
    """513 points: 100 on each of a plane, a sphere, a cylinder and a cone and 113 outliers, shuffled; the tests take the first n"""
    return _shuffled(datasets.make_primitives(n_per=100, n_outliers=113, seed=4))


@pytest.fixture(scope="module")
def medium():
    """two instances of each class, 500 points each, and 1000 outliers"""
    return _shuffled(datasets.make_primitives(n_per=500, n_outliers=1000, n_each=2, seed=6))


def _switched_ctx(name):
    old = os.environ.get(name)
    os.environ[name] = "1"
    try:
        return _lib.Context(0)
    finally:
        if old is None:
            del os.environ[name]
        else:
            os.environ[name] = old


@pytest.fixture(scope="module")
def lane_ctx():
    """a context whose scoring takes the hypothesis-per-lane kernel (no cull, no group-major kernel): the switch is read at creation"""
    ctx = _switched_ctx("PGX_NO_GROUP")
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def verify_ctx():
    """a context whose pgx_score_stats re-decides every pair with the exact residual (PGX_VERIFY: read at creation)"""
    ctx = _switched_ctx("PGX_VERIFY")
    yield ctx
    ctx.close()


def spoiled(nrm, seed=0):
    """the scene's normals (within 5 degrees of the true ones) with a fifth rotated by 40 degrees - past every tolerance used here - about
    a tangent direction, and some rows NaN, zero, negated and scaled"""
    rng = np.random.default_rng(seed)
    out = nrm.copy()
    idx = np.arange(len(out))
    turn = idx % 5 == 1
    t = np.cross(out[turn], rng.normal(size=(int(turn.sum()), 3)))
    t /= np.linalg.norm(t, axis=1)[:, None]
    out[turn] = out[turn] * np.cos(np.deg2rad(40.0)) + np.cross(t, out[turn]) * np.sin(np.deg2rad(40.0))
    out[idx % 7 == 2] *= -1.0
    out[idx % 9 == 4] *= 0.125
    out[idx % 11 == 3, 1] = np.nan
    out[idx % 13 == 5] = 0.0
    return out


def clean(nrm):
    """finite non-zero normals"""
    out = nrm.copy()
    bad = ~np.isfinite(out).all(axis=1) | ~out.any(axis=1)
    out[bad] = [0.0, 0.6, 0.8]
    return out


# ---- scoring ------------------------------------------------------------------------------------------------------------------------------
def _scoring_case(ctx, scene, n, M, path):
    pts, nrm, _, _, gt = scene
    pts, nrm = np.ascontiguousarray(pts[:n]), spoiled(nrm[:n], seed=n)
    rows, bad7, badnan = mixed_batch(M, gt, seed=n + M)
    comp = np.random.default_rng(n).uniform(0, 1, n)
    ctx.score_set_global_n(0)
    ctx.set_normal_tolerance(KAPPA)
    ctx.set_points(_lib.ORIENTED_PRIMITIVE3D, pts)
    with pytest.raises(_lib.PgxError, match=NEEDS):                               # a fresh set_points: the normals are gone
        ctx.score(rows, T2)
    ctx.set_normals(nrm)
    ctx.set_compound(comp)
    ref = ref_score(sq_fn(nrm, KAPPA), pts, rows, T2, comp)
    plain = ref_score(sq_primitive, pts, rows, T2, comp)
    assert (ref["counts"] <= plain["counts"]).all() and (M == 4 or n < 64 or ref["counts"].sum() < plain["counts"].sum())
    for combo in COMBOS:
        got = ctx.score(rows, T2, has_compound=combo[0], exponent=combo[1], want_masks=True)
        r = ref if combo[0] else ref_score(sq_fn(nrm, KAPPA), pts, rows, T2)
        _check_scores(got, r)                                                     # counts and masks exactly, the sums to 1e-9
        for bad in (bad7, badnan):
            assert got["counts"][bad] == 0 and not got["masks"][bad].any() and got["values"][bad] == 0 and got["shared"][bad] == 0
    ctx.score(rows, T2, has_compound=True)
    assert ctx.score_stats(T2, has_compound=True)["path"] == path
    if path == "cull + group-major":                                              # the integers behind the sums
        ctx.score(rows, T2, has_compound=True)
        acc = ctx.score_accumulators()
        for k in ("counts", "values_q", "shared_q"):
            assert np.array_equal(acc[k].astype(np.int64), ref[k]), k
    assert M == 4 or n < 513 or ref["counts"].max() > 40
    # other normals on the same points: the results follow them.  Finite and non-zero, at kappa = 0: type 18's triples from the device
    ctx.set_normals(clean(nrm))
    ctx.set_normal_tolerance(0.0)
    mine = {combo: ctx.score(rows, T2, has_compound=combo[0], exponent=combo[1], want_masks=True) for combo in COMBOS}
    ctx.set_normal_tolerance(KAPPA)
    again = ctx.score(rows, T2, has_compound=True, want_masks=True)
    _check_scores(again, ref_score(sq_fn(clean(nrm), KAPPA), pts, rows, T2, comp))
    ctx.set_points(_lib.PRIMITIVE3D, pts)
    ctx.set_compound(comp)
    for combo in COMBOS:
        base = ctx.score(rows, T2, has_compound=combo[0], exponent=combo[1], want_masks=True)
        for key in ("counts", "values", "shared", "scores", "masks"):
            assert np.array_equal(mine[combo][key], base[key]), (combo, key)
    assert np.array_equal(mine[COMBOS[2]]["counts"], plain["counts"])


@pytest.mark.parametrize("n", [1, 64, 65, 513])
@pytest.mark.parametrize("M", [4, 64, 68, 260])
def test_oriented_scoring_is_the_restatement_group_major(gpu_ctx, small, n, M):
    _scoring_case(gpu_ctx, small, n, M, "cull + group-major")


@pytest.mark.parametrize("n", [1, 64, 65, 513])
@pytest.mark.parametrize("M", [4, 64, 68, 260])
def test_oriented_scoring_is_the_restatement_hypothesis_per_lane(lane_ctx, small, n, M):
    _scoring_case(lane_ctx, small, n, M, "every pair")


def test_every_call_that_evaluates_the_residual_needs_the_normals(gpu_ctx, small):
    pts, nrm, _, _, gt = small
    gpu_ctx.set_points(_lib.ORIENTED_PRIMITIVE3D, pts)
    gpu_ctx.graph_build(pts, _lib.GRAPH_KNN_IN_BALL, radius=0.5, k=5)
    gpu_ctx.set_normal_tolerance(KAPPA)
    calls = [lambda: gpu_ctx.score(gt, T2), lambda: gpu_ctx.score(gt, T2, want_masks=True), lambda: gpu_ctx.preference(gt[0], T2, slot=0),
             lambda: gpu_ctx.pearl_unary(gt, THR, 0.3), lambda: gpu_ctx.gc_labeling(gt[0], T2, 0.2), lambda: gpu_ctx.gc_inliers(gt[0], T2, 0.2),
             lambda: gpu_ctx.solve_minimal(np.arange(8, dtype=np.int32).reshape(2, 4))]
    for call in calls:
        with pytest.raises(_lib.PgxError, match="needs the resident points' normals"):
            call()
    gpu_ctx.set_normals(nrm)
    for call in calls:
        call()
    gpu_ctx.set_normals(None)                                                     # cleared: refused again
    with pytest.raises(_lib.PgxError, match=NEEDS):
        gpu_ctx.score(gt, T2)
    gpu_ctx.set_normals(nrm)
    gpu_ctx.set_points(_lib.ORIENTED_PRIMITIVE3D, pts)                            # a fresh point set: refused again
    with pytest.raises(_lib.PgxError, match=NEEDS):
        gpu_ctx.preference(gt[0], T2, slot=0)
    # the tolerance is context state: a refused value leaves it as it was
    gpu_ctx.set_normals(nrm)
    before = gpu_ctx.score(gt, T2)["counts"]
    for bad in (-0.1, 1.5, np.nan, np.inf):
        with pytest.raises(_lib.PgxError, match="pgx_set_normal_tolerance"):
            gpu_ctx.set_normal_tolerance(bad)
        assert np.array_equal(gpu_ctx.score(gt, T2)["counts"], before)
    gpu_ctx.set_normal_tolerance(1.0)
    assert gpu_ctx.score(gt, T2)["counts"].sum() < before.sum()
    # type 18 asks for no normals when it scores
    gpu_ctx.set_points(_lib.PRIMITIVE3D, pts)
    assert gpu_ctx.score(gt, T2)["counts"].sum() >= before.sum()
    gpu_ctx.set_normal_tolerance(0.0)


def test_cull_and_filter_remove_no_oriented_inlier(verify_ctx, medium):
    """PGX_VERIFY: every pair of the batch re-decided with the exact oriented residual; none that the group bound or the f32 filter
    discarded is an inlier, and the exhaustive count is the scoring path's"""
    pts, nrm, _, _, gt = medium
    nrm = spoiled(nrm, seed=1)
    rows, _, _ = mixed_batch(512, gt, seed=20)
    counts = {}
    for mt in (_lib.ORIENTED_PRIMITIVE3D, _lib.PRIMITIVE3D):
        verify_ctx.set_points(mt, pts)
        verify_ctx.set_compound(None)
        if mt == _lib.ORIENTED_PRIMITIVE3D:
            verify_ctx.set_normals(nrm)
            verify_ctx.set_normal_tolerance(KAPPA)
        got = verify_ctx.score(rows, T2)
        st = verify_ctx.score_stats(T2)
        print(f"type {mt}: {st}")
        assert st["path"] == "cull + group-major" and st["filter"] == "f32" and st["contradictions"] == 0
        assert 0 < st["surviving_group_steps"] < st["group_pairs"] and st["inlier_pairs"] == got["counts"].sum() > 0
        counts[mt] = got["counts"]
    ref = ref_score(sq_fn(nrm, KAPPA), pts, rows, T2)
    assert np.array_equal(counts[_lib.ORIENTED_PRIMITIVE3D], ref["counts"])
    assert (counts[_lib.ORIENTED_PRIMITIVE3D] <= counts[_lib.PRIMITIVE3D]).all()
    assert counts[_lib.ORIENTED_PRIMITIVE3D].sum() < counts[_lib.PRIMITIVE3D].sum()


# ---- the pointwise kernels -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [63, 64, 65, 129])
def test_oriented_pointwise_kernels_are_the_restatement(gpu_ctx, oracle, small, n):
    pts, nrm, _, _, gt = small
    pts, nrm = np.ascontiguousarray(pts[:n]), spoiled(nrm[:n], seed=n)
    rng = np.random.default_rng(n)
    models = np.vstack([gt, gt])
    models[4:, 1:4] += rng.normal(0, 1e-3, (4, 3))
    bad = gt[0].copy()
    bad[0] = 7.0
    models = np.vstack([models, bad])
    K = len(models)
    lam, lam_gc, h = 0.3, 0.2, 1.5
    oml = 1.0 - lam
    gpu_ctx.set_points(_lib.ORIENTED_PRIMITIVE3D, pts)
    gpu_ctx.set_normals(nrm)
    gpu_ctx.set_normal_tolerance(KAPPA)
    gpu_ctx.set_compound(None)
    graph = gpu_ctx.graph_build(pts, _lib.GRAPH_KNN_IN_BALL, radius=1.0, k=5)
    sq = [sq_oriented(pts, nrm, m, KAPPA) for m in models]
    assert sum(int(np.isinf(s).sum()) for s in sq) > n and sum(int((s < T2).sum()) for s in sq) > 8
    with np.errstate(invalid="ignore"):
        for k, m in enumerate(models):
            pref = gpu_ctx.preference(m, T2, slot=k, want_pref=True)
            want = np.where(sq[k] == sq[k], np.maximum(0.0, 1.0 - sq[k] / T2), 0.0)  # (MAX(0, NaN) is 0 in the kernel's order)
            assert np.array_equal(pref["pref"], want), k
            assert pref["pref_sqnorm"] == pytest.approx(float((want * want).sum()), rel=1e-12)
        Dq = gpu_ctx.pearl_unary(models, THR, lam, want_table=True)
        for k in range(K):
            c = np.where(sq[k] > T2, 2.0 * oml, oml * sq[k] / T2)
            c = np.where(c == c, c, 2.0 * oml)
            assert np.array_equal(Dq[:, k], np.rint(c * 4294967296.0).astype(np.int64)), k
    assert (Dq[:, K] == np.int64(np.rint(oml * 4294967296.0))).all()
    # what runs on the table: energy, greedy labelling, bucket
    labels = rng.integers(0, K + 1, n).astype(np.int32)
    gpu_ctx.set_labels(labels)
    sums = gpu_ctx.residual_sums(models)
    assert gpu_ctx.energy(0.0, h)[0] == oracle.energy(Dq, None, 0, oracle.quantize(h), labels)
    assert gpu_ctx.energy(lam, h)[0] == oracle.energy(Dq, graph, oracle.quantize_lambda(lam), oracle.quantize(h), labels)
    eq, _, opened = gpu_ctx.greedy_labeling(h)
    ref_labels, ref_e, ref_opened = oracle.greedy_labeling(Dq, oracle.quantize(h))
    got_labels = gpu_ctx.get_labels()
    assert np.array_equal(got_labels, ref_labels) and (eq, opened) == (ref_e, ref_opened)
    for k in range(K):                                                            # a labelled point is a compatible inlier of its model
        mine = got_labels == k
        assert (sq[k][mine] <= T2).all() and compatible(pts[mine], nrm[mine], models[k], KAPPA).all()
    counts, order = gpu_ctx.bucket(K + 1)
    rc, ro = oracle.bucket(got_labels, K + 1)
    assert np.array_equal(counts, rc) and np.array_equal(order, ro)
    # the inlier / outlier cut: its terms see the oriented residual.  The same cut under type 18 on the same graph, with every point that
    # is incompatible moved out of reach of the model (both give e = 1 there), has the same terms: the same flags (the pairwise term may
    # still pull such a point to the inlier side, under either type)
    cuts = []
    for k, m in enumerate(models[:4]):
        cuts.append((gpu_ctx.gc_labeling(m, T2, lam_gc), gpu_ctx.gc_inliers(m, T2, lam_gc)))
    gpu_ctx.set_points(_lib.PRIMITIVE3D, pts)
    gpu_ctx.set_labels(labels)
    assert np.array_equal(gpu_ctx.residual_sums(models), sums, equal_nan=True)     # plain ignores the normals: type 18's sums
    for k in range(K):
        assert gpu_ctx.residual_sum(models[k], k) == sums[k] or (sums[k] != sums[k])
    for k, m in enumerate(models[:4]):
        moved = pts.copy()
        moved[np.isinf(sq[k])] = 1e6
        assert (sq_primitive(moved[np.isinf(sq[k])], m) > T2).all()
        gpu_ctx.set_points(_lib.PRIMITIVE3D, moved)
        gpu_ctx.graph_build(pts, _lib.GRAPH_KNN_IN_BALL, radius=1.0, k=5, fetch=False)   # (the graph of the points where they were)
        flags = gpu_ctx.gc_labeling(m, T2, lam_gc)
        assert np.array_equal(cuts[k][0], flags) and np.array_equal(cuts[k][1], np.flatnonzero(flags)), k
    assert sum(int(c[0].sum()) for c in cuts) > 8


# ---- the solver ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def solver_scene(small):
    pts, nrm, _, inst, _ = small
    pts, nrm = pts.copy(), nrm.copy()
    pts[5], nrm[5] = pts[4], nrm[4]                           # a duplicate point with its normal
    nrm[6] = 0.0
    nrm[7] = -3.0 * nrm[3]                                    # parallel normals
    nrm[8, 1] = np.nan
    return pts, nrm, inst


def _both(ctx, pts, nrm, kappa, run, mask=15):
    out = {}
    for mt in (_lib.PRIMITIVE3D, _lib.ORIENTED_PRIMITIVE3D):
        ctx.set_points(mt, pts)
        ctx.set_normals(nrm)
        ctx.set_radius_range(*RADII)
        ctx.set_primitive_classes(mask, *SINES)
        ctx.set_normal_tolerance(kappa)
        out[mt] = run(ctx)
    return out[_lib.PRIMITIVE3D], out[_lib.ORIENTED_PRIMITIVE3D]


def _expected(pts, nrm, samples, rows18, kappa):
    want = rows18.copy()
    for t, row in enumerate(rows18):
        if not prefix_compatible(pts, nrm, samples[t // 4], row, kappa):
            want[t] = np.nan
    return want


@pytest.mark.parametrize("S", [1, 63, 64, 65, 129])
def test_oriented_solver_keeps_the_slots_that_agree_with_their_prefix(gpu_ctx, solver_scene, S):
    pts, nrm, inst = solver_scene
    samples = _samples(S, len(pts), inst)
    try:
        base, got = _both(gpu_ctx, pts, nrm, KAPPA, lambda c: c.solve_minimal(samples))
        assert got.shape == (4 * S, 9)
        want = _expected(pts, nrm, samples, base, KAPPA)
        assert np.array_equal(got, want, equal_nan=True)
        have = ~np.isnan(got[:, 0])
        assert np.array_equal(np.isnan(got).all(axis=1), ~have)
        if S >= 63:
            assert have.sum() >= 8 and (have < ~np.isnan(base[:, 0])).sum() >= 8    # some kept, some removed by the test of the normals
        # the host route follows
        est = _estimators.OrientedPrimitiveEstimator(normal_tolerance=TOL)
        est.normals, est.radius_range, est.sine_range = nrm, RADII, SINES
        inb = ((samples >= 0) & (samples < len(pts))).all(axis=1)
        with np.errstate(all="ignore"):
            rows, src = est.minimal(pts, samples[inb])
        mine = have & np.repeat(inb, 4)
        assert np.array_equal(rows, got[mine], equal_nan=True) and np.array_equal(np.flatnonzero(inb)[src], np.flatnonzero(mine) // 4)
        # the tolerance and the class mask are honoured
        _, wide = _both(gpu_ctx, pts, nrm, 0.0, lambda c: c.solve_minimal(samples))
        _, tight = _both(gpu_ctx, pts, nrm, kappa_of(2.0), lambda c: c.solve_minimal(samples))
        assert np.array_equal(wide, _expected(pts, nrm, samples, base, 0.0), equal_nan=True)
        assert np.array_equal(tight, _expected(pts, nrm, samples, base, kappa_of(2.0)), equal_nan=True)
        nw, ng, nt = ((~np.isnan(x[:, 0])).sum() for x in (wide, got, tight))
        assert nw >= ng >= nt and (S < 63 or nw > ng > nt)
        _, masked = _both(gpu_ctx, pts, nrm, KAPPA, lambda c: c.solve_minimal(samples), mask=5)
        assert np.isnan(masked[1::4]).all() and np.isnan(masked[3::4]).all()
        assert np.array_equal(masked[0::4], got[0::4], equal_nan=True) and np.array_equal(masked[2::4], got[2::4], equal_nan=True)
        # the solved batch is resident: scoring it is scoring the rows
        gpu_ctx.set_primitive_classes(15, *SINES)
        gpu_ctx.solve_minimal(samples, fetch=False)
        gpu_ctx.set_compound(None)
        gpu_ctx.score_launch(T2)
        assert np.array_equal(gpu_ctx.score_fetch()["counts"], ref_score(sq_fn(nrm, KAPPA), pts, got, T2)["counts"])
    finally:
        gpu_ctx.set_primitive_classes()
        gpu_ctx.set_radius_range()
        gpu_ctx.set_normal_tolerance(0.0)


def test_oriented_device_drawn_samples_follow_the_same_rule(gpu_ctx, solver_scene):
    pts, nrm, _ = solver_scene
    try:
        def run(c):
            models, smp = c.solve_minimal_sampled(12345, 7, 256, fetch_samples=True)
            return models, smp
        (base, smp18), (got, smp) = _both(gpu_ctx, pts, nrm, KAPPA, run)
        assert np.array_equal(smp, smp18) and got.shape == (1024, 9)
        assert np.array_equal(got, _expected(pts, nrm, smp, base, KAPPA), equal_nan=True)
        assert np.array_equal(got, gpu_ctx.solve_minimal(smp), equal_nan=True)
        assert (~np.isnan(base[:, 0])).sum() > (~np.isnan(got[:, 0])).sum() > 0
    finally:
        gpu_ctx.set_primitive_classes()
        gpu_ctx.set_radius_range()
        gpu_ctx.set_normal_tolerance(0.0)


# ---- end to end ---------------------------------------------------------------------------------------------------------------------------
def _decoy(normal):
    rng = np.random.default_rng(12)
    plane = np.column_stack([rng.uniform(-1, 1, (400, 2)), rng.normal(0, 0.005, 400)])
    out = rng.uniform(-1, 1, (200, 3))
    nout = rng.normal(size=(200, 3))
    nout /= np.linalg.norm(nout, axis=1)[:, None]
    pts, nrm = np.vstack([plane, out]), np.vstack([np.tile(normal, (400, 1)), nout])
    order = rng.permutation(600)
    return np.ascontiguousarray(pts[order]), np.ascontiguousarray(nrm[order])


def test_a_plane_whose_normals_disagree_is_not_found():
    """400 points on z = 0 (sigma 0.005) that all carry the normal (0, sin 45, cos 45), and 200 uniform outliers with random normals.
    findPrimitives reads no normal when it scores and returns the plane; at 20 degrees the oriented call has nothing to return - the
    slab of a plane through outliers holds about six of them, far below minimum_point_number = 50; with the normals (0, 0, 1) it
    returns the plane."""
    s = float(np.sin(np.deg2rad(45.0)))
    kw = dict(classes=("plane",), threshold=0.02, minimum_point_number=50, seed=3)
    pts, tilted = _decoy([0.0, s, s])

    def is_the_plane(models):
        return len(models) == 1 and models[0, 0] == PLANE and abs(models[0, 3]) > 0.999 and abs(models[0, 4]) < 0.01
    models, labels = px.findPrimitives(pts, tilted, **kw)
    assert is_the_plane(models) and 350 <= (labels == 0).sum() <= 420, models
    models, labels = px.findOrientedPrimitives(pts, tilted, normal_tolerance=20.0, **kw)
    assert models.shape == (0, 9) and labels.shape == (600,) and not labels.any()
    pts, upright = _decoy([0.0, 0.0, 1.0])
    models, labels = px.findOrientedPrimitives(pts, upright, normal_tolerance=20.0, **kw)
    assert is_the_plane(models) and 350 <= (labels == 0).sum() <= 420, models


_runs = {}


def _run(seed, **kw):
    pts, nrm, cls, inst, gt = _shuffled(datasets.make_primitives(seed=seed, **E2E), seed=1)
    models, labels = px.findOrientedPrimitives(pts, nrm, minimum_point_number=MPN, radius_range=RADIUS_RANGE, angle_range=ANGLE_RANGE, seed=seed,
                                               spatial_coherence_weight=0.0, normal_tolerance=TOL, **kw)
    return pts, nrm, inst, gt, models, labels


def _check_labelling(pts, nrm, models, labels, enabled):
    assert models.ndim == 2 and models.shape[1] == 9 and labels.shape == (len(pts),) and labels.min() >= 0 and labels.max() <= len(models)
    for k, m in enumerate(models):
        assert class_of(m) in enabled and np.isfinite(m).all(), m
        mine = labels == k
        sq = sq_oriented(pts[mine], nrm[mine], m, KAPPA)
        assert compatible(pts[mine], nrm[mine], m, KAPPA).all(), (k, m)
        assert (sq < T2).all(), (k, float(sq.max()) / T2)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_find_oriented_primitives_end_to_end(seed):
    """the scene of test_find_primitives_end_to_end with the generator's normals (5 degrees of noise), spatial_coherence_weight = 0.
    Asserted: every point labelled to an instance is compatible with it at the tolerance and within the truncated threshold by the
    restatement; the class selection is honoured; two runs from one seed are identical.  How many of the four planted instances are
    found is printed next to findPrimitives on the same scene (DESIGN.md 4.14 has the table), not asserted."""
    pts, nrm, inst, gt, models, labels = _run(seed)
    _check_labelling(pts, nrm, models, labels, CLASSES)
    again = _run(seed)
    assert np.array_equal(again[4], models) and np.array_equal(again[5], labels)
    _, _, _, _, planes, plabels = _run(seed, classes=("plane",))
    _check_labelling(pts, nrm, planes, plabels, (PLANE,))
    base, _ = px.findPrimitives(pts, nrm, minimum_point_number=MPN, radius_range=RADIUS_RANGE, angle_range=ANGLE_RANGE, seed=seed)

    def found(ms):
        return [m[1] if m else None for m in _matched(pts, inst, gt, ms)]
    print(f"seed {seed}: findOrientedPrimitives returned {len(models)} {[int(m[0]) for m in models]}, planted instances matched {found(models)}; "
          f"findPrimitives returned {len(base)} {[int(m[0]) for m in base]}, matched {found(base)}; planes only: {len(planes)}")
