"""Shared input builders for the tests (seeded, small)."""
import numpy as np

from pyprogressivex import datasets

MODEL_CASES = {"line": 0, "homography": 1, "fundamental": 2, "pnp": 3, "vanishing_point": 4, "homography_sym": 5}
# The 3-D point-cloud types live in a table of their own: tests index per-name dictionaries with MODEL_CASES and the soaks pick the
# type by trial % len(MODEL_CASES), so growing that table would silently change what the committed seeds test.
MODEL_CASES_3D = {"plane": 6, "sphere": 8}
# ... and so does the 2-D circle (findCircles, type 10), for the same reason: MODEL_CASES and MODEL_CASES_3D keep their contents and order
MODEL_CASES_2D = {"circle": 10}
ALL_MODEL_CASES = {**MODEL_CASES, **MODEL_CASES_3D, **MODEL_CASES_2D}


def _fit_n(rng, arr, n):
    idx = rng.permutation(arr.shape[0])
    if arr.shape[0] >= n:
        return np.ascontiguousarray(arr[idx[:n]])
    extra = rng.integers(0, arr.shape[0], n - arr.shape[0])
    return np.ascontiguousarray(np.vstack([arr, arr[extra]])[rng.permutation(n)])


def make_case(name, n, M, seed=0):
    """(model_type, points[n,d], models[M,p], threshold): a few ground-truth structures with inliers, outliers, and
    hypotheses that are ground truth, perturbed ground truth or random (so counts span 0 .. many)."""
    rng = np.random.default_rng(seed)
    mt = ALL_MODEL_CASES[name]
    per = max(2, n // 5)
    if name == "line":
        pts, _, gt = datasets.make_lines(n_per_line=per, n_lines=3, n_outliers=per, seed=seed)
        thr = 2.0
    elif name in ("homography", "homography_sym"):
        pts, _, gt = datasets.make_homographies(n_per_plane=per, n_planes=3, n_outliers=per, seed=seed)
        thr = 3.0
        if name == "homography_sym":
            gt = np.array([np.concatenate([h, np.linalg.inv(h.reshape(3, 3)).reshape(-1)]) for h in gt])
    elif name == "fundamental":
        pts, _, gt = datasets.make_two_view_motions(n_per_motion=per, n_motions=3, n_outliers=per, seed=seed)
        thr = 0.75
    elif name == "pnp":
        x1, x2, K, _, gt = datasets.make_poses(n_per_object=per, n_objects=3, n_outliers=per, seed=seed)
        pts, f = datasets.normalize_pnp(x1, x2, K)
        thr = 4.0 / f
    elif name == "vanishing_point":
        pts, _, gt = datasets.make_vanishing_points(n_inliers=3 * per, n_vps=3, n_outliers=per, seed=seed)
        thr = 1.5
    elif name == "plane":
        pts, _, gt = datasets.make_planes(n_per_plane=per, n_planes=3, n_outliers=per, seed=seed)
        thr = 0.05
    elif name == "sphere":
        pts, _, gt = datasets.make_spheres(n_per_sphere=per, n_spheres=3, n_outliers=per, seed=seed)
        thr = 0.05
    elif name == "circle":            # pixel units (box 1000, radii 40 .. 150, noise 0.5); findCircles' default threshold
        pts, _, gt = datasets.make_circles(n_per_circle=per, n_circles=3, n_outliers=per, seed=seed)
        thr = 2.0
    else:
        raise KeyError(name)
    pts = _fit_n(rng, pts, n)
    models = []
    for m in range(M):
        g = gt[m % len(gt)]
        kind = m % 4 if m >= len(gt) else 0
        if kind == 0:
            models.append(g.copy())
        elif kind == 1:
            models.append(g * (1.0 + rng.normal(0, 1e-4, g.shape)))
        elif kind == 2:
            models.append(g * (1.0 + rng.normal(0, 1e-2, g.shape)))
        else:
            models.append(rng.normal(0, 1, g.shape) * np.abs(g).max())
    return mt, pts, np.ascontiguousarray(np.array(models)), thr


def random_sym_graph(rng, n, p):
    """Symmetric CSR (off, idx, mult) with random multiplicities 1..2 per undirected pair."""
    if p <= 0 or n < 2:
        return np.zeros(n + 1, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32)
    iu, ju = np.triu_indices(n, 1)
    keep = rng.random(iu.shape[0]) < p
    iu, ju = iu[keep], ju[keep]
    mult = rng.integers(1, 3, iu.shape[0])
    return csr_from_pairs(n, iu, ju, mult)


def csr_from_pairs(n, iu, ju, mult):
    a = np.concatenate([iu, ju])
    b = np.concatenate([ju, iu])
    m = np.concatenate([mult, mult])
    o = np.lexsort((b, a))
    a, b, m = a[o], b[o], m[o]
    off = np.zeros(n + 1, dtype=np.int64)
    np.add.at(off, a + 1, 1)
    return np.cumsum(off).astype(np.int32), b.astype(np.int32), m.astype(np.int32)


def realistic_labeling_problem(n, L, lam, seed=0):
    """Points in the unit square with a radius graph; clusters of points prefer one of L-1 model labels, the last
    label is the outlier label with constant cost (1 - lambda), as PEARL's data term prices it."""
    from scipy.spatial import cKDTree
    rng = np.random.default_rng(seed)
    pts = rng.random((n, 2))
    pairs = cKDTree(pts).query_pairs(r=2.0 / np.sqrt(n), output_type="ndarray")
    graph = csr_from_pairs(n, pairs[:, 0], pairs[:, 1], np.full(pairs.shape[0], 2))
    D = rng.random((n, L)) * 2 * (1 - lam)
    D[:, L - 1] = 1 - lam
    cl = (pts[:, 0] * 5).astype(int) % (L - 1)
    D[np.arange(n), cl] *= 0.1
    Dq = np.rint(D * 2.0 ** 32).astype(np.int64)
    return Dq, graph


def fixed_point_accumulators(O, mt, pts, models, T2, comp=None, n_total=None):
    """The integer accumulators the group-major score path builds (score.hip: count, and value / shared support as sums of
    round-to-nearest-even(term * 2^q) per inlier), restated from the ORACLE's residuals: getScore's terms
    (scoring_function_with_compound_model.h:85-97, 115-117) in the fixed point of a job of n_total points."""
    from pyprogressivex import parallel
    pts = np.ascontiguousarray(pts, dtype=np.float64)
    models = np.ascontiguousarray(models, dtype=np.float64)
    q = parallel.fixed_point_scale(pts.shape[0] if n_total is None else n_total)
    M = models.shape[0]
    counts = np.zeros(M, np.int64)
    values_q = np.zeros(M, np.int64)
    shared_q = np.zeros(M, np.int64)
    for m in range(M):
        sq = O.squared_residuals(mt, pts, models[m])
        with np.errstate(invalid="ignore"):
            inl = sq < T2
        sc = np.maximum(0.0, 1.0 - sq[inl] / T2)
        counts[m] = int(inl.sum())
        values_q[m] = int(np.rint(sc * q).astype(np.int64).sum())
        if comp is not None:
            shared_q[m] = int(np.rint(np.minimum(np.asarray(comp)[inl], sc) * q).astype(np.int64).sum())
    return dict(counts=counts, values_q=values_q, shared_q=shared_q)


# ---- point-cloud scenes shared by the CPU and GPU files of findPlanes / findSpheres / findCircles ---------------------------------
def scene_3d(kind, per=800, structures=3, outliers=800, seed=0):
    """(points [n, 3] in random order, labels, ground truth [K, 4]) of datasets.make_planes / make_spheres; for kind "circle"
    (points [n, 2], labels, ground truth [K, 3]) of datasets.make_circles.  Shuffled: PROSAC and Progressive NAPSAC read the order
    as quality, and the generators emit structure by structure."""
    mk = {"plane": datasets.make_planes, "sphere": datasets.make_spheres, "circle": datasets.make_circles}[kind]
    pts, gt, models = mk(per, structures, outliers, seed=seed)
    order = np.random.default_rng(seed + 100).permutation(len(pts))
    return np.ascontiguousarray(pts[order]), gt[order], models


def match_3d(kind, found, truth):
    """for every ground-truth structure the distance to the nearest found model: planes max(|n x n'| sign-free normal difference,
    |d - d'|), spheres and circles max(|c - c'|, |r - r'|)"""
    out = []
    for g in truth:
        best = np.inf
        for m in found:
            if kind == "plane":
                s = 1.0 if float(m[:3] @ g[:3]) >= 0 else -1.0
                best = min(best, float(np.abs(s * m - g).max()))
            else:
                best = min(best, float(np.abs(m - g).max()))
        out.append(best)
    return np.array(out)


def edge_clouds_3d(kind):
    """name -> (points, zero_models): the degenerate and hostile clouds every findPlanes / findSpheres path has to get through.
    zero_models: no structure of this kind can be generated from the cloud, so no model may come back.  The degenerate clouds have
    dyadic coordinates of a few bits, so that every difference and product of the minimal solvers is exact and the degeneracy is
    exact too (ln == 0, det == 0: NaN rows); with rounded coordinates a plane through a line, or a huge sphere hugging a plane, is a
    legitimate model.  Non-finite values sit in the third column: pgx_graph_build refuses them in the first two ("refused_*")."""
    rng = np.random.default_rng(17)
    m = 3 if kind == "plane" else 4
    t = rng.integers(-24, 25, 60) / 8.0
    uv = rng.integers(-32, 33, (120, 2)) / 16.0
    base, _, _ = scene_3d(kind, per=150, structures=2, outliers=100, seed=4)
    nan_row, inf_row, refused_nan, refused_inf = base.copy(), base.copy(), base.copy(), base.copy()
    nan_row[5, 2] = np.nan
    inf_row[7, 2] = np.inf
    refused_nan[5, 0] = np.nan
    refused_inf[7, 1] = -np.inf
    return {
        "n_equals_sample_size": (rng.uniform(0.0, 10.0, (m, 3)), False),
        "coincident": (np.tile(np.array([[1.5, -2.0, 3.25]]), (60, 1)), True),
        "collinear": (np.array([1.0, 2.0, 3.0]) + t[:, None] * np.array([0.5, 0.0, 0.75]), True),
        "coplanar": (np.column_stack([uv[:, 0], uv[:, 1], 0.25 * uv[:, 0] - 0.5 * uv[:, 1] + 1.0]), kind == "sphere"),
        "outliers_only": (rng.uniform(0.0, 10.0, (300, 3)), False),
        "offset_1e6": (base + np.array([1e6, -1e6, 5e5]), False),
        "nan_row": (nan_row, False),
        "inf_row": (inf_row, False),
        "refused_nan": (refused_nan, False),
        "refused_inf": (refused_inf, False),
    }


def edge_clouds_2d():
    """edge_clouds_3d for findCircles (pixel units): name -> (points [n, 2], zero_models).  The degenerate clouds have dyadic
    coordinates of a few bits, so every difference and product of the 3-point solver is exact and det == 0 exactly (NaN rows); with
    rounded coordinates a huge circle hugging a line is a legitimate model.  Both columns of a 2-D point are grid coordinates of
    pgx_graph_build, so every non-finite row is refused there: "nan_row" / "inf_row" are the refused rows of the 2-D table, in the
    second column, and "refused_nan" / "refused_inf" the same in the first."""
    rng = np.random.default_rng(23)
    t = rng.integers(-24, 25, 60) / 8.0
    base, _, _ = scene_3d("circle", per=150, structures=2, outliers=100, seed=4)
    nan_row, inf_row, refused_nan, refused_inf = base.copy(), base.copy(), base.copy(), base.copy()
    nan_row[5, 1] = np.nan
    inf_row[7, 1] = np.inf
    refused_nan[5, 0] = np.nan
    refused_inf[7, 0] = -np.inf
    return {
        "n_equals_sample_size": (rng.uniform(0.0, 1000.0, (3, 2)), False),
        "coincident": (np.tile(np.array([[150.5, -20.25]]), (60, 1)), True),
        "collinear": (np.array([100.0, 200.0]) + 16.0 * t[:, None] * np.array([0.5, 0.75]), True),
        "outliers_only": (rng.uniform(0.0, 1000.0, (300, 2)), False),
        "offset_1e6": (base + np.array([1e6, -1e6]), False),
        "nan_row": (nan_row, False),
        "inf_row": (inf_row, False),
        "refused_nan": (refused_nan, False),
        "refused_inf": (refused_inf, False),
    }
