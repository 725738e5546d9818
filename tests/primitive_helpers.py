"""What the GPU tests of the geometric primitives (test_gpu_planes.py, test_gpu_spheres.py, test_gpu_circles.py) share: the numpy
reference of a scoring call, its comparison, the expected output of the device's minimal solvers, and the recovery criterion of the
end-to-end calls; and what their CPU tests share: one refit on numpy Gram matrices.  The per-type arithmetic (sq_*, dist,
make_problem) stays with each test file."""
import numpy as np

from pyprogressivex import _lib, datasets, parallel


def ref_score(sq_fn, pts, models, T2, comp=None):
    """counts, values, shared, their fixed-point sums and the inlier masks of scoring `models`; sq_fn(pts, model) = the type's squared
    residuals in the kernels' operation order"""
    n = pts.shape[0]
    q = parallel.fixed_point_scale(n)
    words = (n + 63) // 64
    out = dict(counts=[], values=[], shared=[], values_q=[], shared_q=[], masks=np.zeros((len(models), words), np.uint64))
    for k, m in enumerate(models):
        sq = sq_fn(pts, m)
        with np.errstate(invalid="ignore"):
            inl = sq < T2
        sc = np.maximum(0.0, 1.0 - sq[inl] / T2)
        out["counts"].append(int(inl.sum()))
        out["values"].append(sc.sum())
        out["values_q"].append(int(np.rint(sc * q).astype(np.int64).sum()))
        sh = np.minimum(comp[inl], sc) if comp is not None else np.zeros(0)
        out["shared"].append(sh.sum())
        out["shared_q"].append(int(np.rint(sh * q).astype(np.int64).sum()))
        bits = np.zeros(words * 64, dtype=bool)
        bits[:n] = inl
        out["masks"][k] = np.packbits(bits, bitorder="little").view("<u8")
    for key in ("counts", "values_q", "shared_q"):
        out[key] = np.array(out[key], dtype=np.int64)
    out["values"] = np.array(out["values"])
    out["shared"] = np.array(out["shared"])
    return out


def _check_scores(got, ref):
    assert np.array_equal(got["counts"], ref["counts"])
    assert np.array_equal(got["masks"], ref["masks"])
    assert np.all(np.abs(got["values"] - ref["values"]) <= 1e-9 * np.maximum(np.abs(ref["values"]), 1e-4))
    assert np.all(np.abs(got["shared"] - ref["shared"]) <= 1e-9 * np.maximum(np.abs(ref["shared"]), 1e-4))


def _want(est, pts, samples, S):
    """the S models the device solver must give: the estimator's, NaN where a sample has an index outside the points or no model"""
    ok = (samples >= 0).all(1) & (samples < len(pts)).all(1)
    ref, src = est.minimal(pts, samples[ok])
    want = np.full((S, est.cols), np.nan)
    want[np.flatnonzero(ok)[src]] = ref
    return want


def _check_labelling(res, labels, gen_labels, thr):
    """res [n, K] = the distances to the K ground-truth models: a labelling no worse than two points in a hundred above that of the
    ground truth with the band the labelling uses"""
    K = res.shape[1]
    band = 1.5 * thr
    near = np.argmin(res, axis=1)
    floor_labels = np.where(res[np.arange(len(res)), near] < band, near + 1, 0)
    floor = float(np.mean(floor_labels != gen_labels))
    me = datasets.misclassification(np.where(labels == K, 0, labels + 1), gen_labels)
    assert me <= floor + 0.02, (me, floor)


def _check_recovery(found, labels, pts, gen_labels, gt, thr, sigma):
    """spheres and circles (c[D], r): every ground-truth model found within 2 sigma in centre and radius, and _check_labelling"""
    K, D = len(gt), pts.shape[1]
    assert found.shape == (K, D + 1) and found.dtype == np.float64 and labels.dtype == np.int32
    for g in gt:
        k = int(np.argmin(np.linalg.norm(found[:, :D] - g[:D], axis=1)))
        assert np.linalg.norm(found[k, :D] - g[:D]) < 2 * sigma, (found[k], g)
        assert abs(found[k, D] - g[D]) < 2 * sigma, (found[k], g)
    _check_labelling(np.abs(np.linalg.norm(pts[:, None, :] - gt[None, :, :D], axis=2) - gt[None, :, D]), labels, gen_labels, thr)


def shuffled(pts, gen, seed=0):
    """Progressive NAPSAC (the default sampler) and PROSAC take the points as ordered by quality: their first samples come from the
    first points, and every proposal restarts the sampler.  In the generators' order (model by model) every proposal would start
    inside the first model, so the end-to-end tests put the points in a random order."""
    order = np.random.default_rng(seed).permutation(len(pts))
    return np.ascontiguousarray(pts[order]), gen[order]


def numpy_refit(est, pts, w=None):
    """est._fit_many with one item (B = 1) through a numpy Gram provider (the device's rows, summed in float64): the affine rows
    (1, p), then for the round family the rows (1, q, |q|^2), q = (p - o) / s, the last entry summed left to right.  Returns
    (models, requests), requests = the (kind, params [1, p] | None, use_weights, wpow) the refit asked for, in order."""
    w = np.ones(len(pts)) if w is None else w
    requests = []

    def gram(kind, prm, use_w, wpow, rows):
        assert list(rows) == [0] and (prm is None or prm.shape[0] == 1)
        requests.append((kind, prm, use_w, wpow))
        if kind == _lib.GRAM_AFFINE:
            A = np.column_stack([np.ones(len(pts)), pts])
        else:
            q = (pts - prm[0, :-1]) / prm[0, -1]
            sq = q[:, 0] * q[:, 0]
            for k in range(1, q.shape[1]):
                sq = sq + q[:, k] * q[:, k]
            A = np.column_stack([np.ones(len(pts)), q, sq])
        return ((A * w[:, None]).T @ A)[None], np.array([len(pts)]), np.array([0])
    (models,) = est._fit_many(gram, 1, [None])
    return models, requests
