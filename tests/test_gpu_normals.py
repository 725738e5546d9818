"""estimateNormals on the MI355X: pgx_estimate_normals bit for bit against the numpy restatement of its definition
(tests/normals_model.py) on every graph kind and both lane mappings, its edge cases, refusals and absence of side effects, the
50-digit fixture held to the tolerance of DESIGN.md 4.10 on the device, and findCylinders fed with estimated normals."""
import ctypes as C
import os

import numpy as np
import pytest

import normals_model as NM
import pyprogressivex as px
from cylinder_model import sq_cylinder
from pyprogressivex import _lib, datasets

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kat_normals_v1.npz")
KINDS = (_lib.GRAPH_KNN, _lib.GRAPH_KNN_IN_BALL, _lib.GRAPH_BALL)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a[~na].view(np.int64), b[~nb].view(np.int64))


def check_against_model(ctx, pts, graph, viewpoint=None):
    """the device on the resident graph (whatever lane mapping it has) against the restatement on the CSR `graph`; returns the model"""
    ref = NM.estimate(pts, graph[0], graph[1], viewpoint=viewpoint)
    nrm, curv, undefined = ctx.estimate_normals(pts, viewpoint=viewpoint, want_curvature=True)
    assert same_bits(nrm, ref["normals"]) and same_bits(curv, ref["curvature"]) and undefined == ref["undefined"]
    only, none, undefined2 = ctx.estimate_normals(pts, viewpoint=viewpoint)          # curvature_out = NULL
    assert none is None and same_bits(only, nrm) and undefined2 == undefined
    return ref


def both_mappings(ctx, pts, kind, radius, k, viewpoint=None):
    graph = ctx.graph_build(pts, kind, radius=radius, k=k)                          # leaves the Morton order of the sites resident
    ref = check_against_model(ctx, pts, graph, viewpoint)
    ctx.set_graph(*graph)                                                           # the same CSR without an order: lane t serves site t
    check_against_model(ctx, pts, graph, viewpoint)
    sel = np.flatnonzero(ref["defined"])
    if len(sel):                                                                    # the same matrices through pgx_eigh_smallest_batch
        vec, val = ctx.eigh_smallest_batch(ref["cov"][sel])
        turned = np.array([NM.orient(v, pts[i], viewpoint) for v, i in zip(vec, sel)])
        assert same_bits(turned, ref["normals"][sel])
        trace = (ref["cov"][sel, 0, 0] + ref["cov"][sel, 1, 1]) + ref["cov"][sel, 2, 2]
        with np.errstate(all="ignore"):
            assert same_bits(val / trace, ref["curvature"][sel])
    return ref


@pytest.mark.parametrize("n", [3, 4, 63, 64, 65, 129])
def test_normals_bit_exact_small_clouds(gpu_ctx, oracle, n):
    pts = np.random.default_rng(100 + n).normal(size=(n, 3))
    for k in (2, 5, 16):
        for kind in KINDS:
            if kind == _lib.GRAPH_BALL and k != 2:
                continue                                                            # (k is ignored: once)
            both_mappings(gpu_ctx, pts, kind, 1.0, k)
    both_mappings(gpu_ctx, pts, _lib.GRAPH_KNN, 0.0, 5, viewpoint=[0.3, -4.0, 2.5])


@pytest.fixture(scope="module")
def scene():
    pts, _, labels, gt = datasets.make_cylinders(n_per_cylinder=500, n_cylinders=3, n_outliers=500, seed=4)
    return pts, labels, gt


@pytest.mark.parametrize("kind, k", [(_lib.GRAPH_KNN, 2), (_lib.GRAPH_KNN, 5), (_lib.GRAPH_KNN, 16), (_lib.GRAPH_KNN_IN_BALL, 16),
                                     (_lib.GRAPH_BALL, 1)])
def test_normals_bit_exact_scene(gpu_ctx, oracle, scene, kind, k):
    pts = scene[0]
    ref = both_mappings(gpu_ctx, pts, kind, 0.35, k, viewpoint=None if k == 5 else [5.0, 5.0, 20.0])
    if kind == _lib.GRAPH_KNN:
        assert ref["undefined"] == 0
    if kind == _lib.GRAPH_KNN and k == 16:                                          # a hub row: longer than k
        off = gpu_ctx.graph_fetch()[0]
        assert np.diff(off).max() > 16


def test_public_call_is_the_restatement(oracle, scene):
    pts = scene[0]
    ctx = px._api._context()
    nrm, curv = px.estimateNormals(pts, k=5, viewpoint=(0.0, 0.0, 0.0), return_curvature=True)
    ref = NM.estimate(pts, *ctx.graph_fetch()[:2], viewpoint=(0.0, 0.0, 0.0))
    assert same_bits(nrm, ref["normals"]) and same_bits(curv, ref["curvature"])
    assert same_bits(px.estimateNormals(pts), NM.estimate(pts, *ctx.graph_fetch()[:2])["normals"])
    ball = px.estimateNormals(pts, k=None, radius=0.3)
    assert same_bits(ball, NM.estimate(pts, *ctx.graph_fetch()[:2])["normals"])
    inball = px.estimateNormals(pts, k=8, radius=0.3)
    off, idx, _ = ctx.graph_fetch()
    assert same_bits(inball, NM.estimate(pts, off, idx)["normals"])
    assert np.isnan(inball).any() and not np.isnan(px.estimateNormals(pts, k=8)).any()      # outliers alone in their ball
    with pytest.raises(_lib.PgxError, match="pgx_graph_build: k = 17 outside 1..16"):
        px.estimateNormals(pts, k=17)


# ---- edges ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2])
def test_normals_of_one_and_two_points_are_undefined(gpu_ctx, n):
    pts = np.arange(3.0 * n).reshape(n, 3)
    if n == 1:
        gpu_ctx.set_graph(np.array([0, 0], np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32))
    else:
        gpu_ctx.set_graph(np.array([0, 1, 2], np.int32), np.array([1, 0], np.int32), np.ones(2, np.int32))
    nrm, curv, undefined = gpu_ctx.estimate_normals(pts, want_curvature=True)
    assert np.isnan(nrm).all() and np.isnan(curv).all() and undefined == n


def test_normals_empty_rows_of_a_tiny_ball(gpu_ctx, oracle):
    pts = np.random.default_rng(5).uniform(0, 10, (200, 3))
    pts[:6] = pts[0] + 1e-4 * np.random.default_rng(6).normal(size=(6, 3))            # one cluster inside the ball, everyone else alone
    graph = gpu_ctx.graph_build(pts, _lib.GRAPH_BALL, radius=1e-2)
    assert (np.diff(graph[0]) == 0).sum() >= 190
    ref = check_against_model(gpu_ctx, pts, graph)
    assert ref["defined"][:6].all() and ref["undefined"] == 194


def test_normals_duplicate_points(gpu_ctx, oracle):
    rng = np.random.default_rng(7)
    pts = rng.normal(size=(40, 3))
    pts[10:20] = pts[:10]                                                           # pairs of duplicates
    pts[20:40] = pts[20]                                                            # a neighbourhood of one repeated point: the zero matrix
    ref = both_mappings(gpu_ctx, pts, _lib.GRAPH_KNN, 0.0, 5)
    zero = np.flatnonzero((ref["cov"].reshape(40, 9) == 0).all(1))
    assert len(zero) >= 10 and np.isnan(ref["curvature"][zero]).all()                # 0 / 0; the normal is Jacobi's of the zero matrix
    assert (ref["normals"][zero] == [1.0, 0.0, 0.0]).all() and ref["undefined"] == 0


def test_normals_of_a_coplanar_grid(gpu_ctx, oracle):
    g = np.array([[0.25 * i, 0.25 * j, 0.5] for i in range(5) for j in range(5)])
    ref = both_mappings(gpu_ctx, g, _lib.GRAPH_KNN, 0.0, 5)
    nrm, curv, undefined = gpu_ctx.estimate_normals(g, want_curvature=True)
    assert undefined == 0 and (curv == 0.0).all()
    # exactly coplanar: lambda_0 = 0 and the gap is lambda_1; the tolerance of DESIGN.md 4.10 from the matrices' own eigenvalues
    m = 1 + np.diff(gpu_ctx.graph_fetch()[0])
    for i in range(25):
        w = np.linalg.eigvalsh(ref["cov"][i])
        assert abs(nrm[i, 2]) == np.abs(nrm[i]).max() and nrm[i, 2] > 0
        assert np.hypot(nrm[i, 0], nrm[i, 1]) <= NM.tolerance_factor(int(m[i])) * NM.EPS * w[2] / (w[1] - w[0])


def test_normals_of_three_collinear_points(gpu_ctx, oracle):
    pts = np.array([[0.0, 0.0, 0.0], [1.0, 2.0, 3.0], [2.0, 4.0, 6.0]])
    ref = both_mappings(gpu_ctx, pts, _lib.GRAPH_KNN, 0.0, 2)
    assert ref["undefined"] == 0 and np.isfinite(ref["normals"]).all()


def test_normals_of_the_fixture_on_the_device(gpu_ctx, oracle):
    """the 50-digit fixture (a quarter of it moved by 1e6: the offsets from the point itself keep the tolerance) as disjoint stars"""
    z = np.load(GOLDEN)
    off, idx, centres = NM.star_graph(z["sizes"])
    gpu_ctx.set_graph(off, idx, np.ones(len(idx), np.int32))
    nrm, _, undefined = gpu_ctx.estimate_normals(z["points"])
    assert undefined == len(z["points"]) - len(centres)
    assert same_bits(nrm, NM.estimate(z["points"], off, idx)["normals"])
    tol = np.array([NM.tolerance_factor(int(m)) for m in z["sizes"]]) * NM.EPS * z["eig"][:, 2] / (z["eig"][:, 1] - z["eig"][:, 0])
    ratio = np.array([NM.angle_to(nrm[c], z["normal_hi"][f], z["normal_lo"][f]) for f, c in enumerate(centres)]) / tol
    moved = z["groups"][z["group"], 1] != 0
    print(f"worst angle / tolerance on the device {ratio.max():.4f}; moved by 1e6: {ratio[moved].max():.4f}")
    assert moved.sum() == 60 and ratio.max() <= 1.0


def test_normals_one_nan_row(gpu_ctx, oracle, scene):
    pts = scene[0][:300]
    off, idx, mult = gpu_ctx.graph_build(pts, _lib.GRAPH_KNN, k=5)
    clean, _, _ = gpu_ctx.estimate_normals(pts)
    bad = pts.copy()
    bad[17, 1] = np.nan
    ref = check_against_model(gpu_ctx, bad, (off, idx))
    hit = np.zeros(300, dtype=bool)
    hit[17] = True
    hit[idx[off[17]:off[18]]] = True                                                # symmetric: the rows that hold 17 are 17's row
    assert np.array_equal(np.isnan(ref["normals"]).any(1), hit) and ref["undefined"] == hit.sum()
    nrm, _, _ = gpu_ctx.estimate_normals(bad)
    assert same_bits(nrm[~hit], clean[~hit])
    bad[17, 1] = np.inf
    check_against_model(gpu_ctx, bad, (off, idx))


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def raw_call(ctx, points, n, viewpoint, normals, curvature=None):
    undefined = C.c_int64(-7)
    r = ctx._lib.pgx_estimate_normals(ctx._h, _lib._ptr(points, C.c_double), C.c_int64(n), _lib._ptr(viewpoint, C.c_double),
                                      _lib._ptr(normals, C.c_double), _lib._ptr(curvature, C.c_double), C.byref(undefined))
    return r, ctx._lib.pgx_last_error(ctx._h).decode(), undefined.value


def test_normals_refusals(oracle):
    pts = np.random.default_rng(9).normal(size=(50, 3))
    out = np.zeros((50, 3))
    with _lib.Context(0) as ctx:
        r, msg, _ = raw_call(ctx, pts, 50, None, out)
        assert r == -1 and "pgx_estimate_normals: needs a neighbourhood graph of the points" in msg                # no graph
        assert raw_call(ctx, None, 0, None, None) == (0, msg, 0)                                                  # n == 0 is fine, graph or not
        graph = ctx.graph_build(pts, _lib.GRAPH_KNN, k=5)
        r, msg, _ = raw_call(ctx, pts, 49, None, out)
        assert r == -1 and "pgx_estimate_normals: 49 points for a graph of 50 sites" in msg
        with pytest.raises(_lib.PgxError, match="51 points for a graph of 50 sites"):
            ctx.estimate_normals(np.vstack([pts, pts[:1]]))
        for p, o in ((None, out), (pts, None)):
            r, msg, _ = raw_call(ctx, p, 50, None, o)
            assert r == -1 and "pgx_estimate_normals: NULL argument" in msg
        for v in ([np.nan, 0.0, 0.0], [0.0, np.inf, 0.0], [0.0, 0.0, -np.inf]):
            with pytest.raises(_lib.PgxError, match="pgx_estimate_normals: non-finite viewpoint"):
                ctx.estimate_normals(pts, viewpoint=v)
        assert (out == 0).all()                                                     # a refused call writes nothing
        check_against_model(ctx, pts, graph)                                        # the context is still usable
        r, _, undefined = raw_call(ctx, pts, 50, None, out)                         # NULL curvature_out
        assert r == 0 and undefined == 0 and same_bits(out, NM.estimate(pts, graph[0], graph[1])["normals"])
        assert ctx._lib.pgx_estimate_normals(ctx._h, _lib._ptr(pts, C.c_double), C.c_int64(50), None, _lib._ptr(out, C.c_double), None,
                                             None) == 0                             # NULL undefined


# ---- side effects ---------------------------------------------------------------------------------------------------------------------
def test_normals_leave_the_resident_problem_alone(gpu_ctx, oracle):
    pts, nrm, _, gt = datasets.make_cylinders(n_per_cylinder=300, n_cylinders=2, n_outliers=200, seed=8)
    other = np.random.default_rng(3).normal(size=(120, 3))                          # the cloud whose normals are estimated: another size
    samples = np.random.default_rng(4).integers(0, len(pts), (64, 2)).astype(np.int32)
    T2 = 2.25 * 0.05 * 0.05
    gpu_ctx.set_points(_lib.CYLINDER3D, pts)
    gpu_ctx.set_normals(nrm)
    gpu_ctx.set_radius_range(0.1, 2.0)
    try:
        before = gpu_ctx.solve_minimal(samples)                                     # reads the resident points and normals
        pref = gpu_ctx.preference(gt[0], T2, slot=0, want_pref=True)["pref"]       # reads the resident points
        score = gpu_ctx.score(gt, T2)
        graph = gpu_ctx.graph_build(other, _lib.GRAPH_KNN, k=5)
        check_against_model(gpu_ctx, other, graph)
        assert np.array_equal(gpu_ctx.preference(gt[0], T2, slot=0, want_pref=True)["pref"], pref)
        after = gpu_ctx.score(gt, T2)
        assert all(np.array_equal(score[key], after[key]) for key in ("counts", "values", "shared"))
        assert same_bits(gpu_ctx.solve_minimal(samples), before)
        assert np.isfinite(before).all(1).sum() > 10
    finally:
        gpu_ctx.set_radius_range()


# ---- end to end -----------------------------------------------------------------------------------------------------------------------
SIGMA = 0.01
MPN = 100          # test_gpu_cylinders.py's: an eighth of a cylinder's 800 points


def _scene(seed):
    pts, _, gen, gt = datasets.make_cylinders(n_per_cylinder=800, n_cylinders=3, n_outliers=800, sigma=SIGMA, normal_noise_deg=5.0,
                                              seed=seed)
    order = np.random.default_rng(0).permutation(len(pts))
    pts, gen = np.ascontiguousarray(pts[order]), gen[order]
    ends = []
    for k, g in enumerate(gt):                               # the extreme projections of the cylinder's own points onto the true axis
        t = (pts[gen == k + 1] - g[:3]) @ g[3:6]
        ends.append(np.array([g[:3] + t.min() * g[3:6], g[:3] + t.max() * g[3:6]]))
    return pts, gen, gt, ends


def _matches(m, g, e):
    """test_gpu_cylinders.py's criterion: radius within 2 sigma, axis within 2 sigma of both ends of the true segment"""
    axis = np.concatenate([m[:6], [0.0]])
    return abs(m[6] - g[6]) < 2 * SIGMA and (np.sqrt(sq_cylinder(e, axis)) < 2 * SIGMA).all()


@pytest.mark.parametrize("k", [16, 6])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_find_cylinders_on_estimated_normals(seed, k):
    """test_gpu_cylinders.py's 3-cylinder scene (800 points each, 800 outliers, shuffled) with estimateNormals(pts, k) in place of the
    synthetic normals: every returned cylinder is a ground truth one.  How many are found is printed, not asserted.  The scene is
    sparse for a covariance normal - 800 points on some 20 square units of surface, neighbours 0.15 apart on cylinders of radius 0.3
    to 1 - and the restatement's normals, checked on the CPU first, are NOT within the order of the synthetic 5 degree tilt at k = 16:
    their error against the radial direction has a median of 11.5, 19.9 and 7.9 degrees on the seeds 0, 1, 2 and a 95th percentile of
    85 (neighbourhoods that reach round the cylinder or into the outliers).  No k brings the tail down; the median is of that order for
    k = 5 .. 8 (k = 6: 6.6, 5.6, 5.8 degrees, 65 to 72 % of the inliers within 10), so k = 6 is run next to the k = 16 the public default
    gives.  Measured on an MI355X: three returned and three of three found for every seed, at either k."""
    pts, gen, gt, ends = _scene(seed)
    nrm = px.estimateNormals(pts, k=k)
    assert nrm.shape == pts.shape and not np.isnan(nrm).any()
    inl = gen > 0
    radial = pts[inl] - gt[gen[inl] - 1, :3]
    axis = gt[gen[inl] - 1, 3:6]
    radial -= (radial * axis).sum(1)[:, None] * axis
    radial /= np.linalg.norm(radial, axis=1)[:, None]
    err = np.degrees(np.arccos(np.clip(np.abs((radial * nrm[inl]).sum(1)), 0.0, 1.0)))
    cyl, labels = px.findCylinders(pts, nrm, minimum_point_number=MPN)
    found = [any(_matches(m, g, e) for m in cyl) for g, e in zip(gt, ends)]
    print(f"seed {seed}, k = {k}: normals' error on the inliers median {np.median(err):.2f} deg, 95th percentile {np.percentile(err, 95):.2f} deg; "
          f"returned {len(cyl)}, found {sum(found)} of 3")
    assert cyl.ndim == 2 and cyl.shape[1] == 7 and labels.shape == (len(pts),)
    for m in cyl:
        assert any(_matches(m, g, e) for g, e in zip(gt, ends)), (m, gt)
