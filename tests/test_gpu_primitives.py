"""findPrimitives on the MI355X.  The union type PGX_PRIMITIVE3D = 18 adds no arithmetic of its own, so every check is bit for bit
against code that exists without it: a model row (class, q) scored, labelled, solved or refitted under type 18 gives what q gives under
its own type (6 plane, 8 sphere, 14 cylinder, 16 cone) on the same points, and the dense counts are those of the numpy restatement
(tests/primitive_model.py).  Then the public call end to end."""
import os

import numpy as np
import pytest

import pyprogressivex as px
from primitive_helpers import ref_score
from primitive_model import CLASSES, CONE, CYLINDER, PARAMS, PLANE, PREFIX, SPHERE, class_of, interleave, sq_primitive, union_rows
from pyprogressivex import _estimators, _lib, _rng, datasets

pytestmark = pytest.mark.gpu

THR = 0.05
T2 = 2.25 * THR * THR
PART = {PLANE: _estimators.PlaneEstimator, SPHERE: _estimators.SphereEstimator, CYLINDER: _estimators.CylinderEstimator,
        CONE: _estimators.ConeEstimator}


def _shuffled(scene, seed=0):
    pts, nrm, cls, inst, gt = scene
    order = np.random.default_rng(seed).permutation(len(pts))
    return np.ascontiguousarray(pts[order]), np.ascontiguousarray(nrm[order]), cls[order], inst[order], gt


@pytest.fixture(scope="module")
def small():
    """513 points: 100 on each of a plane, a sphere, a cylinder and a cone and 113 outliers, shuffled; the tests take the first n"""
    return _shuffled(datasets.make_primitives(n_per=100, n_outliers=113, seed=4))


@pytest.fixture(scope="module")
def medium():
    """two instances of each class, 500 points each, and 1000 outliers"""
    return _shuffled(datasets.make_primitives(n_per=500, n_outliers=1000, n_each=2, seed=6))


@pytest.fixture(scope="module")
def lane_ctx():
    """a context whose scoring takes the hypothesis-per-lane kernel (no cull, no group-major kernel): the switch is read at creation"""
    old = os.environ.get("PGX_NO_GROUP")
    os.environ["PGX_NO_GROUP"] = "1"
    try:
        ctx = _lib.Context(0)
    finally:
        if old is None:
            del os.environ["PGX_NO_GROUP"]
        else:
            os.environ["PGX_NO_GROUP"] = old
    yield ctx
    ctx.close()


def _q(rows, c):
    """the constituent's model rows of union rows of class c"""
    return np.ascontiguousarray(rows[:, 1:1 + PARAMS[c]])


def mixed_batch(M, gt, seed):
    """M union rows with the classes interleaved as the solver emits them (row j has class CLASSES[j % 4]): ground truth, perturbed by
    1e-6 .. 1e-1, or random; then the special rows - all NaN, class 7 on a good plane, a NaN class on a good sphere"""
    rng = np.random.default_rng(seed)
    rows = np.zeros((M, 9))
    for j in range(M):
        c = CLASSES[j % 4]
        g = gt[gt[:, 0] == c][(j // 4) % int((gt[:, 0] == c).sum())].copy()
        kind = (j // 4) % 3
        if kind == 1:
            g[1:1 + PARAMS[c]] += rng.normal(0, 10.0 ** rng.uniform(-6, -1), PARAMS[c])
        elif kind == 2:
            q = {PLANE: np.concatenate([rng.normal(size=3), [rng.uniform(-10, 0)]]),
                 SPHERE: np.concatenate([rng.uniform(0, 10, 3), [rng.uniform(0.2, 3.0)]]),
                 CYLINDER: np.concatenate([rng.uniform(0, 10, 3), rng.normal(size=3), [rng.uniform(0.2, 3.0)]]),
                 CONE: np.concatenate([rng.uniform(0, 10, 3), rng.normal(size=3), [np.cos(0.5), np.sin(0.5)]])}[c]
            g[1:1 + PARAMS[c]] = q
        rows[j] = g
    bad7, badnan = 2, 3
    if M >= 64:
        rows[M - 1] = np.nan
        rows[M - 6] = np.nan
        bad7, badnan = M - 2, M - 3
    else:                                                     # four rows: a cone, an all-NaN row, and the two bad classes
        rows[0] = gt[gt[:, 0] == CONE][0]
        rows[1] = np.nan
    rows[bad7] = gt[gt[:, 0] == PLANE][0]
    rows[bad7, 0] = 7.0
    rows[badnan] = gt[gt[:, 0] == SPHERE][0]
    rows[badnan, 0] = np.nan
    return rows, bad7, badnan


COMBOS = [(False, 1), (False, 2), (True, 1), (True, 2)]      # (compound vector, scoring exponent)


def _score_all(ctx, mt, pts, comp, models):
    ctx.set_points(mt, pts)
    ctx.set_compound(comp)
    return {combo: ctx.score(models, T2, has_compound=combo[0], exponent=combo[1], want_masks=True) for combo in COMBOS}


def _scoring_case(ctx, scene, n, M, path):
    pts, _, _, _, gt = scene
    pts = np.ascontiguousarray(pts[:n])
    rows, bad7, badnan = mixed_batch(M, gt, seed=n + M)
    comp = np.random.default_rng(n).uniform(0, 1, n)
    ctx.score_set_global_n(0)
    union = _score_all(ctx, _lib.PRIMITIVE3D, pts, comp, rows)
    ctx.score(rows, T2, has_compound=True)
    assert ctx.score_stats(T2, has_compound=True)["path"] == path
    ref = ref_score(sq_primitive, pts, rows, T2, comp)        # the dense exact count of the restatement
    classes = np.array([class_of(r) or 0 for r in rows])
    assert {int(c) for c in classes} >= ({0, CONE} if M == 4 else {0, *CLASSES})
    for combo in COMBOS:
        got = union[combo]
        assert np.array_equal(got["counts"], ref["counts"]) and np.array_equal(got["masks"], ref["masks"]), combo
        for bad in (bad7, badnan):                            # the two bad classes have no inlier, whatever their parameters
            assert got["counts"][bad] == 0 and not got["masks"][bad].any() and got["values"][bad] == 0 and got["shared"][bad] == 0
    assert M == 4 or n < 513 or ref["counts"].max() > 50
    for c in CLASSES:
        sel = classes == c
        if not sel.any():
            continue
        alone = np.full((M, PARAMS[c]), np.nan)               # the same batch size and positions: the rows of other classes are NaN rows
        alone[sel] = _q(rows[sel], c)
        own = _score_all(ctx, c, pts, comp, alone)
        for combo in COMBOS:
            for key in ("counts", "values", "shared", "scores", "masks"):
                assert np.array_equal(union[combo][key][sel], own[combo][key][sel]), (c, combo, key)
            assert not own[combo]["counts"][~sel].any()


@pytest.mark.parametrize("n", [1, 64, 65, 513])
@pytest.mark.parametrize("M", [4, 64, 68, 260])
def test_union_scoring_equals_the_constituents_group_major(gpu_ctx, small, n, M):
    _scoring_case(gpu_ctx, small, n, M, "cull + group-major")


@pytest.mark.parametrize("n", [1, 64, 65, 513])
@pytest.mark.parametrize("M", [4, 64, 68, 260])
def test_union_scoring_equals_the_constituents_hypothesis_per_lane(lane_ctx, small, n, M):
    _scoring_case(lane_ctx, small, n, M, "every pair")


@pytest.mark.parametrize("c", CLASSES)
def test_union_filter_and_bound_are_the_constituents(gpu_ctx, medium, c):
    """a batch of one class: the cull keeps the same (hypothesis, group) pairs, the f32 filter passes the same pairs on to the exact path
    and the exact path finds the same inliers as under the class's own type"""
    pts, _, _, _, gt = medium
    rows, _, _ = mixed_batch(512, gt, seed=c)
    rows = rows[[class_of(r) == c for r in rows]]
    assert 126 <= len(rows) <= 128                            # (the special rows of the 512 are not of a class)
    stats = {}
    for mt, models in ((_lib.PRIMITIVE3D, rows), (c, _q(rows, c))):
        gpu_ctx.set_points(mt, pts)
        gpu_ctx.set_compound(None)
        got = gpu_ctx.score(models, T2)
        stats[mt] = (gpu_ctx.score_stats(T2), got["counts"])
    a, b = stats[_lib.PRIMITIVE3D], stats[c]
    assert a[0] == b[0] and np.array_equal(a[1], b[1]), (a[0], b[0])
    assert a[0]["path"] == "cull + group-major" and a[0]["filter"] == "f32"
    assert 0 < a[0]["surviving_group_steps"] < a[0]["group_pairs"] and a[0]["inlier_pairs"] == a[1].sum() > 0


# ---- the pointwise kernels -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [4, 9])
def test_union_pointwise_kernels_equal_the_constituents(gpu_ctx, medium, K):
    pts, _, _, _, gt = medium
    n = len(pts)
    rng = np.random.default_rng(K)
    models = np.array([gt[gt[:, 0] == CLASSES[k % 4]][(k // 4) % 2] for k in range(K)])
    models[:, 1:4] += rng.normal(0, 1e-3, (K, 3))
    classes = [class_of(m) for m in models]
    labels = rng.integers(0, K + 1, n).astype(np.int32)       # K = the outlier label
    lam, lam_gc = 0.3, 0.2

    def run(mt, rows, lab):
        gpu_ctx.set_points(mt, pts)
        gpu_ctx.set_compound(None)
        gpu_ctx.graph_build(pts, _lib.GRAPH_KNN_IN_BALL, radius=0.5, k=5)
        out = dict(pref=[], gc=[], inl=[])
        for k, m in enumerate(rows):
            out["pref"].append(gpu_ctx.preference(m, T2, slot=k, want_pref=True))
            out["gc"].append(gpu_ctx.gc_labeling(m, T2, lam_gc))
            out["inl"].append(gpu_ctx.gc_inliers(m, T2, lam_gc))
        out["unary"] = gpu_ctx.pearl_unary(rows, THR, lam, want_table=True)
        gpu_ctx.set_labels(lab)
        out["sums"] = gpu_ctx.residual_sums(rows)
        return out
    union = run(_lib.PRIMITIVE3D, models, labels)
    assert union["unary"].shape == (n, K + 1)
    for k, m in enumerate(models):
        assert np.array_equal(union["pref"][k]["pref"], np.maximum(0.0, 1.0 - sq_primitive(pts, m) / T2))
    assert sum(int(g.sum()) for g in union["gc"]) > 500
    for c in CLASSES:
        mine = [k for k in range(K) if classes[k] == c]
        remap = np.full(K + 1, len(mine), dtype=np.int32)     # the other classes' points are outliers of this type's label set
        remap[mine] = np.arange(len(mine))
        own = run(c, _q(models[mine], c), remap[labels])
        for j, k in enumerate(mine):
            for key in ("pref", "dot", "pref_sqnorm", "comp_sqnorm"):
                assert np.array_equal(union["pref"][k][key], own["pref"][j][key]), (c, k, key)
            assert np.array_equal(union["gc"][k], own["gc"][j]) and np.array_equal(union["inl"][k], own["inl"][j]), (c, k)
            assert np.array_equal(union["inl"][k], np.flatnonzero(union["gc"][k]))
            assert np.array_equal(union["unary"][:, k], own["unary"][:, j]), (c, k)
            assert union["sums"][k] == own["sums"][j], (c, k)
        assert np.array_equal(union["unary"][:, K], own["unary"][:, len(mine)])          # the outlier column


def test_union_expansion_matches_the_oracle(gpu_ctx, oracle, medium):
    """pgx_expansion on the mixed unary table against the oracle's expansion on that table (the route of the types the oracle does not have)"""
    pts, _, _, _, gt = medium
    n = len(pts)
    lam, h = 0.1, 6.0
    gpu_ctx.set_points(_lib.PRIMITIVE3D, pts)
    graph = gpu_ctx.graph_build(pts, _lib.GRAPH_KNN_IN_BALL, radius=0.4, k=5)
    Dq = gpu_ctx.pearl_unary(gt, THR, lam, want_table=True)
    oml = 1.0 - lam
    for k, m in enumerate(gt):                                # the table is the restatement's
        sq = sq_primitive(pts, m)
        assert np.array_equal(Dq[:, k], np.rint(np.where(sq > T2, 2.0 * oml, oml * sq / T2) * 4294967296.0).astype(np.int64))
    gpu_ctx.set_unary_q(Dq)
    gpu_ctx.set_labels(np.zeros(n, np.int32))
    eq, e, cyc = gpu_ctx.expansion(lam, h)
    ref_labels, ref_e, ref_cyc = oracle.expansion(Dq, graph, oracle.quantize_lambda(lam), oracle.quantize(h), np.zeros(n, np.int32))
    assert np.array_equal(gpu_ctx.get_labels(), ref_labels) and eq == ref_e and cyc == ref_cyc
    assert len(np.unique(ref_labels)) > 4


# ---- the solver ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def solver_scene(small):
    pts, nrm, _, inst, _ = small
    pts, nrm = pts.copy(), nrm.copy()
    pts[5], nrm[5] = pts[4], nrm[4]                           # a duplicate point with its normal
    nrm[6] = 0.0
    nrm[7] = -3.0 * nrm[3]                                    # parallel normals
    nrm[8, 1] = np.nan
    pts[9] = pts[10] + [1e-9, 0.0, 0.0]                       # two points a rounding apart
    return pts, nrm, inst


RADII = (0.2, 3.0)
SINES = (float(np.sin(np.deg2rad(10.0))), float(np.sin(np.deg2rad(50.0))))


def _samples(S, n, inst):
    rng = np.random.default_rng(S)
    samples = rng.integers(10, n, (S, 4)).astype(np.int32)
    for s in range(0, S, 2):                                  # every other sample inside one instance: models inside the ranges
        samples[s] = rng.choice(np.flatnonzero(inst == 1 + (s // 2) % 4), 4, replace=False)
    special = np.array([[4, 5, 30, 31], [11, 11, 11, 11], [6, 15, 16, 17], [3, 7, 18, 19], [8, 15, 16, 17], [9, 10, 22, 23], [-1, 2, 3, 4],
                        [20, 21, 22, n], [30, 31, 32, 30]], np.int32)[:max(0, min(S - 1, 9))]
    samples[1:1 + len(special)] = special
    return samples


def _constituent_slots(ctx, pts, nrm, samples, mask=15):
    """{class: [S, 9] union rows} from the four constituent solvers under their own types, on the sample prefixes"""
    out = {}
    for j, c in enumerate(CLASSES):
        if not (mask >> j) & 1:
            out[c] = np.full((len(samples), 9), np.nan)
            continue
        ctx.set_points(c, pts)
        ctx.set_normals(nrm)
        ctx.set_radius_range(*(SINES if c == CONE else RADII))
        out[c] = union_rows(c, ctx.solve_minimal(np.ascontiguousarray(samples[:, :PREFIX[c]])))
    ctx.set_radius_range()
    return out


@pytest.mark.parametrize("S", [1, 63, 64, 65, 129])
def test_union_solver_slots_equal_the_constituent_solvers(gpu_ctx, solver_scene, S):
    pts, nrm, inst = solver_scene
    samples = _samples(S, len(pts), inst)
    want = interleave(_constituent_slots(gpu_ctx, pts, nrm, samples))
    gpu_ctx.set_points(_lib.PRIMITIVE3D, pts)
    gpu_ctx.set_normals(nrm)
    gpu_ctx.set_radius_range(*RADII)
    gpu_ctx.set_primitive_classes(15, *SINES)
    try:
        got = gpu_ctx.solve_minimal(samples)
        assert got.shape == (4 * S, 9)
        assert np.array_equal(got, want, equal_nan=True)
        have = ~np.isnan(got[:, 0])
        assert np.array_equal(np.isnan(got).all(axis=1), ~have)                   # a slot without a model is all NaN, class included
        assert (got[have, 0] == np.tile(CLASSES, S)[have]).all()
        if S >= 63:
            assert all(have[j::4].sum() >= 1 for j in range(4)), [have[j::4].sum() for j in range(4)]
            assert all(not have[j::4].all() for j in range(4))                    # and every class lost some: degenerate or out of range
            r = np.concatenate([got[1::4][have[1::4], 4], got[2::4][have[2::4], 7]])
            assert r.min() >= RADII[0] and r.max() <= RADII[1]
            s_ = got[3::4][have[3::4], 8]
            assert s_.min() >= SINES[0] and s_.max() <= SINES[1]
        # the estimator restates the kernel: the same rows, without the empty slots
        est = _estimators.PrimitiveEstimator()
        est.normals, est.radius_range, est.sine_range = nrm, RADII, SINES
        inb = ((samples >= 0) & (samples < len(pts))).all(axis=1)                # (an index outside the points concerns the slots that read it)
        with np.errstate(all="ignore"):
            rows, src = est.minimal(pts, samples[inb])
        mine = have & np.repeat(inb, 4)
        assert np.array_equal(rows, got[mine], equal_nan=True) and np.array_equal(np.flatnonzero(inb)[src], np.flatnonzero(mine) // 4)
        last = np.flatnonzero((samples[:, 3] == len(pts)) & ((samples[:, :3] >= 0) & (samples[:, :3] < len(pts))).all(axis=1))
        assert S < 9 or (len(last) and np.isnan(got[4 * last + 1]).all() and not np.isnan(got[4 * last]).any())   # the plane does not read it
        # a masked class leaves its slot NaN and the others as they were
        gpu_ctx.set_primitive_classes(5, *SINES)
        masked = gpu_ctx.solve_minimal(samples)
        assert np.isnan(masked[1::4]).all() and np.isnan(masked[3::4]).all()
        assert np.array_equal(masked[0::4], got[0::4], equal_nan=True) and np.array_equal(masked[2::4], got[2::4], equal_nan=True)
        # the solved batch is resident: scoring it is scoring the rows
        gpu_ctx.set_primitive_classes(15, *SINES)
        gpu_ctx.solve_minimal(samples, fetch=False)
        gpu_ctx.set_compound(None)
        gpu_ctx.score_launch(T2)
        assert np.array_equal(gpu_ctx.score_fetch()["counts"], ref_score(sq_primitive, pts, got, T2)["counts"])
    finally:
        gpu_ctx.set_primitive_classes()
        gpu_ctx.set_radius_range()


def test_union_solver_needs_normals_and_a_valid_class_selection(gpu_ctx, solver_scene):
    pts, nrm, inst = solver_scene
    samples = _samples(65, len(pts), inst)
    gpu_ctx.set_points(_lib.PRIMITIVE3D, pts)
    with pytest.raises(_lib.PgxError, match="pgx_solve_minimal: the primitive solver needs the resident points' normals"):
        gpu_ctx.solve_minimal(samples)
    with pytest.raises(_lib.PgxError, match="the primitive solver needs the resident points' normals"):
        gpu_ctx.solve_minimal_sampled(1, 0, 8)
    gpu_ctx.set_normals(nrm)
    gpu_ctx.set_radius_range(*RADII)
    try:
        gpu_ctx.set_primitive_classes(13, 0.2, 0.7)
        first = gpu_ctx.solve_minimal(samples)
        assert np.isnan(first[1::4]).all() and not np.isnan(first[0::4]).all() and not np.isnan(first[3::4]).all()
        for mask, lo, hi in ((0, 0.2, 0.7), (16, 0.2, 0.7), (31, 0.2, 0.7), (-1, 0.2, 0.7), (15, -0.1, 0.5), (15, 0.6, 0.5), (15, 0.0, 1.1),
                             (15, np.nan, 1.0), (15, 0.0, np.nan), (15, np.inf, np.inf)):
            with pytest.raises(_lib.PgxError, match="pgx_set_primitive_classes"):
                gpu_ctx.set_primitive_classes(mask, lo, hi)
            assert np.array_equal(gpu_ctx.solve_minimal(samples), first, equal_nan=True), (mask, lo, hi)   # the state is unchanged
        gpu_ctx.set_primitive_classes(15, 0.0, 1.0)                                # the creation state: wider in both respects
        wide = gpu_ctx.solve_minimal(samples)
        assert (~np.isnan(wide[:, 0])).sum() > (~np.isnan(first[:, 0])).sum() and not np.isnan(wide[1::4]).all()
        # the radius range is the spheres' and cylinders' alone, the sine range the cones' alone
        gpu_ctx.set_radius_range(5.0, 6.0)
        far = gpu_ctx.solve_minimal(samples)
        r = np.concatenate([far[1::4, 4], far[2::4, 7]])
        r = r[~np.isnan(r)]
        assert (r >= 5.0).all() and (r <= 6.0).all() and len(r) < (~np.isnan(wide[1::4, 0])).sum() + (~np.isnan(wide[2::4, 0])).sum()
        assert np.array_equal(far[0::4], wide[0::4], equal_nan=True) and np.array_equal(far[3::4], wide[3::4], equal_nan=True)
    finally:
        gpu_ctx.set_primitive_classes()
        gpu_ctx.set_radius_range()


def test_union_device_drawn_samples_equal_the_generator(gpu_ctx, solver_scene):
    """pgx_solve_minimal_sampled with m = 4: the rows are _rng's for the uniform, NAPSAC and PROSAC samplers, the models pgx_solve_minimal's"""
    pts, nrm, _ = solver_scene
    pts = np.where(np.isfinite(pts) & (np.abs(pts) < 1e100), pts, 5.0)            # (the graph is built on finite coordinates)
    n = len(pts)
    gpu_ctx.set_points(_lib.PRIMITIVE3D, pts)
    gpu_ctx.set_normals(nrm)
    gpu_ctx.set_radius_range()
    gpu_ctx.set_primitive_classes()
    off, idx, _ = gpu_ctx.graph_build(pts, _lib.GRAPH_KNN_IN_BALL, radius=2.0, k=5)
    tops = np.minimum(n, np.arange(4, 4 + 256)).astype(np.int32)
    gpu_ctx.sampler_prosac_set(tops)
    want_rows = dict(uniform=_rng.uniform_samples(12345, 7, 256, n, 4), napsac=_rng.napsac_samples(12345, 7, 256, n, 4, off, idx),
                     prosac=_rng.prosac_samples(12345, 7, 256, n, 4, tops))
    for sampler in ("uniform", "napsac", "prosac"):
        models, smp = gpu_ctx.solve_minimal_sampled(12345, 7, 256, fetch_samples=True, sampler=sampler)
        assert smp.shape == (256, 4) and models.shape == (1024, 9) and (smp >= 0).all(1).sum() > 0
        assert np.array_equal(smp, want_rows[sampler].astype(np.int32)), sampler
        assert np.array_equal(models, gpu_ctx.solve_minimal(smp), equal_nan=True), sampler
        assert (~np.isnan(models[:, 0])).sum() > 100, sampler


# ---- the refit -----------------------------------------------------------------------------------------------------------------------------
def test_union_refit_equals_the_constituent_estimators(gpu_ctx, medium):
    """nonminimal_labels on a mixed labelling of eight instances against the four constituent estimators, each on its own two labels
    under its own resident type"""
    pts, nrm, _, inst, gt = medium
    n, K = len(pts), len(gt)
    w = np.random.default_rng(3).uniform(0.5, 2.0, n)
    labels = np.where(inst > 0, inst - 1, K).astype(np.int32)
    inits = gt.copy()
    inits[:, 1:4] += 0.01
    est = _estimators.PrimitiveEstimator()
    gpu_ctx.set_points(_lib.PRIMITIVE3D, pts)
    gpu_ctx.set_labels(labels)
    got = est.nonminimal_labels(gpu_ctx, K, weights=w, inits=inits, skip=(3,))
    assert got[3] == [] and sum(len(g) for g in got) >= 6 and all(len(g) <= 1 for g in got)
    for c in CLASSES:
        mine = [k for k in range(K) if gt[k, 0] == c]
        remap = np.full(K + 1, len(mine), dtype=np.int32)
        remap[mine] = np.arange(len(mine))
        gpu_ctx.set_points(c, pts)
        gpu_ctx.set_labels(remap[labels])
        own = PART[c]().nonminimal_labels(gpu_ctx, len(mine), weights=w, inits=_q(inits[mine], c), skip=tuple(j for j, k in enumerate(mine) if k == 3))
        for j, k in enumerate(mine):
            assert len(own[j]) == len(got[k])
            if own[j]:
                assert np.array_equal(got[k][0], union_rows(c, own[j][0])[0]), (c, k)
                assert np.sqrt(sq_primitive(pts[inst == k + 1], got[k][0])).max() < 0.06


# ---- end to end ---------------------------------------------------------------------------------------------------------------------------
E2E = dict(n_per=600, n_outliers=2400, sigma=0.01)
MPN = 100             # minimum_point_number: a sixth of an instance's 600 points.  A slab of width 3 x threshold across the box (the
#                       largest shell any class has here: 10 x 10 x 0.15 of 1000 volume units) holds 36 of the 2400 outliers
RADIUS_RANGE = (0.2, 3.0)
ANGLE_RANGE = (5.0, 60.0)
NORMALS_RADIUS = 0.3  # estimateNormals' ball: 30 sigma, chosen against the noise
_runs = {}


def _e2e_scene(seed, normals):
    pts, nrm, cls, inst, gt = _shuffled(datasets.make_primitives(seed=seed, **E2E), seed=1)
    if normals == "estimated":
        nrm = px.estimateNormals(pts, radius=NORMALS_RADIUS)
    return pts, nrm, cls, inst, gt


def _run(seed, normals, **kw):
    pts, nrm, cls, inst, gt = _e2e_scene(seed, normals)
    models, labels = px.findPrimitives(pts, nrm, minimum_point_number=MPN, radius_range=RADIUS_RANGE, angle_range=ANGLE_RANGE, seed=seed, **kw)
    return pts, inst, gt, models, labels


def _check_call(pts, models, labels, enabled):
    K = len(models)
    assert models.ndim == 2 and models.shape[1] == 9 and models.dtype == np.float64
    assert labels.shape == (len(pts),) and labels.dtype == np.int32 and labels.min() >= 0 and labels.max() <= K
    worst = 0.0
    for k, m in enumerate(models):
        c = class_of(m)
        assert c in enabled, m
        assert not m[1 + PARAMS[c]:].any() and np.isfinite(m).all()
        if c in (SPHERE, CYLINDER):
            r = m[4] if c == SPHERE else m[7]
            assert RADIUS_RANGE[0] <= r <= RADIUS_RANGE[1], m
        if c == CONE:
            assert np.sin(np.deg2rad(ANGLE_RANGE[0])) <= m[8] <= np.sin(np.deg2rad(ANGLE_RANGE[1])) and m[7] > 0, m
        mine = labels == k
        if mine.any():
            worst = max(worst, float(sq_primitive(pts[mine], m).max()) / T2)
    return worst


def _matched(pts, inst, gt, models):
    """per ground-truth instance: the returned model that explains it - the one with the most of its points within the threshold, if
    these are more than half - as (index, class) or None"""
    out = []
    for k in range(len(gt)):
        sel = pts[inst == k + 1]
        hits = [int((sq_primitive(sel, m) < THR * THR).sum()) for m in models]
        j = int(np.argmax(hits)) if hits else -1
        out.append((j, class_of(models[j])) if j >= 0 and hits[j] > len(sel) // 2 else None)
    return out


@pytest.mark.parametrize("normals", ["true", "estimated"])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_find_primitives_end_to_end(seed, normals):
    """one plane, sphere, cylinder and cone of 600 points each and 2400 uniform outliers (1 cm noise, points shuffled), with the
    generator's tilted normals and with estimateNormals' over a 30 cm ball; every default except minimum_point_number, the two ranges and
    the run's seed = the scene's.  Asserted outright: shapes, every class number among the enabled ones, zeros behind a class's
    parameters, radii and sines inside their ranges, labels in 0 .. K, every labelled point within the truncated threshold 1.5 x
    threshold of its model (r^2 <= T2, the data term's rule).  How many of the four are found, and as which class, is measured and
    printed (DESIGN.md 4.13 has the table); asserted of it is only what held on all three seeds with either normals."""
    pts, inst, gt, models, labels = _run(seed, normals)
    _runs[(seed, normals)] = (models, labels)
    worst = _check_call(pts, models, labels, CLASSES)
    got = _matched(pts, inst, gt, models)
    print(f"seed {seed} normals {normals}: returned {len(models)} {[int(m[0]) for m in models]}, matched (true class -> class of the model) "
          f"{[(int(g[0]), m[1] if m else None) for g, m in zip(gt, got)]}, worst r^2 / T2 of a labelled point {worst:.4f}")
    assert worst <= 1.0
    # what held on all three seeds with either normals: the plane, the sphere and the cylinder are found, each as its own class; the
    # cone was matched by a cone on three of the six runs and by nothing on the others
    assert [m[1] if m else None for m in got[:3]] == [PLANE, SPHERE, CYLINDER]
    assert got[3] is None or got[3][1] == CONE


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_find_primitives_is_reproducible_and_honours_classes(seed):
    if (seed, "true") not in _runs:
        _runs[(seed, "true")] = _run(seed, "true")[3:]
    pts, inst, gt, models, labels = _run(seed, "true")
    first = _runs[(seed, "true")]
    assert np.array_equal(models, first[0]) and np.array_equal(labels, first[1])  # bit for bit from its seed
    pts, inst, gt, planes, plabels = _run(seed, "true", classes=("plane",))
    _check_call(pts, planes, plabels, (PLANE,))
    assert (planes[:, 0] == PLANE).all()
    print(f"seed {seed}: classes=('plane',) returned {len(planes)}, matched {_matched(pts, inst, gt, planes)}")
    assert _matched(pts, inst, gt, planes)[0] is not None
    # the yardstick beside it: what the four single-class calls find on the same scene (printed; DESIGN.md 4.13 has the table)
    nrm = _e2e_scene(seed, "true")[1]
    kw = dict(minimum_point_number=MPN, seed=seed)
    alone = {PLANE: px.findPlanes(pts, **kw)[0], SPHERE: px.findSpheres(pts, radius_range=RADIUS_RANGE, **kw)[0],
             CYLINDER: px.findCylinders(pts, nrm, radius_range=RADIUS_RANGE, **kw)[0], CONE: px.findCones(pts, nrm, angle_range=ANGLE_RANGE, **kw)[0]}
    for k, c in enumerate(CLASSES):
        rows = union_rows(c, alone[c]) if len(alone[c]) else np.zeros((0, 9))
        hit = _matched(pts, inst, gt, rows)
        print(f"seed {seed}: the {c} call alone returned {len(rows)}, its own instance {'found' if hit[k] else 'not found'}, "
              f"holds other classes' instances: {[int(g[0]) for g, h in zip(gt, hit) if h and g[0] != c]}")
