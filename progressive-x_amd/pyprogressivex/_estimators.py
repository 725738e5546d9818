"""Estimators: batched minimal solvers (hypothesis generation) and non-minimal refits, host side (numpy).

Replaces the Estimator concept of the reference (`sampleSize()`, `nonMinimalSampleSize()`, `estimateModel`,
`estimateModelNonminimal`; exemplar in-tree: vanishing_point_estimator.h:34-226 and
solver_vanishing_point_two_lines.h:128-237, paths relative to /root/reference/src/pyprogressivex/include/).
Only the vanishing-point solver exists in the snapshot; the line / homography / fundamental / PnP solvers live in the
absent graph-cut-ransac submodule and are restated from the literature [UPSTREAM-MEMORY] — SURVEY.md §8f ranks them
"next" (GPU versions), so round 1 keeps them on the host: they produce the hypothesis batches that the HIP scorer
consumes and the refits PEARL asks for.  Residuals are NOT computed here — that is libpgx's job.

Every refit is stated once, as `_fit_many(gram, B, inits)` on [B, ...] stacks; `Estimator.nonminimal` (one selection),
`nonminimal_labels` (all labels) and `nonminimal_batch` (B index selections) hand it a Gram provider over pgx_gram,
pgx_gram_labels and pgx_gram_batch.  PnP alone keeps a second, single-item statement (see `PnPEstimator.nonminimal`).
"""
import numpy as np

from . import _lib


class Estimator:
    model_type = None
    sample_size = 0
    nonminimal_sample_size = 0
    device_minimal = False     # True: ctx.solve_minimal(samples) replaces minimal() in the proposal engine
    device_slots = 1           # hypotheses the device solver emits per sample (NaN = none)
    rows_per_model = 1       # rows of the returned model array per instance (3 for 3x3 / 3x4 matrices)
    cols = 3

    # The small dense solve of the refits: "lapack" (default) = numpy.linalg.eigh on the host; "jacobi" (round 6, keyword
    # refit_solver= of the drop-in calls) = the context's batched cyclic-Jacobi solver (pgx_eigh_smallest_batch: on the device,
    # bitwise the CPU restatement the tests hold; agrees with LAPACK to ~1e-13 on the eigenvector) - the eigen-solves behind the
    # C ABI, the first step towards one C call per local-optimisation round.
    refit_solver = "lapack"
    _eig_ctx = None            # the context of the refit being run (set by nonminimal / nonminimal_labels / nonminimal_batch)

    def _smallest(self, A):
        """eigenvectors of the smallest eigenvalue of the symmetric matrices A [B, q, q] -> [B, q]"""
        ctx = self._eig_ctx
        if self.refit_solver == "jacobi" and ctx is not None and hasattr(ctx, "eigh_smallest_batch"):
            return ctx.eigh_smallest_batch(A)[0]
        return np.linalg.eigh(A)[1][:, :, 0]

    takes_radius_range = False   # True: the estimator has a `radius_range` that the radius_range= keyword of its entry point sets

    def context_setup(self, ctx):
        """Per-call context state this estimator's device solver reads besides the points (the radius range, the cylinder's normals);
        the run calls it once the points are resident, since some of that state belongs to a point set.  Default: none."""

    def minimal(self, pts, samples):
        """samples [S, m] -> (models [H, P], sample_of_model [H]); several or zero solutions per sample allowed."""
        raise NotImplementedError

    # -- model validity (gcransac Estimator::isValidModel, both overloads) [U-14] -------------------------------------------
    validity = "off"

    def valid_samples(self, pts, samples, models, src):
        """Quick test of hypotheses against their own minimal samples, before they are scored (isValidModel(model, data,
        sample, threshold)).  models [H, P], src [H] = row of `samples` each came from -> bool [H].  Default: all valid."""
        return np.ones(len(models), dtype=bool)

    def valid_best(self, ctx, pts, model, sample, threshold, rescore):
        """Test of a model that is about to become the so-far-best (isValidModel(model, data, inliers, sample, threshold,
        model_updated)).  Returns (valid, model): the model may come back replaced.  `rescore(models) -> scores` evaluates
        candidates with the proposal's scoring function.  Default: valid, unchanged."""
        return True, model

    def _fit_many(self, gram, B, inits):
        """The least-squares refit of B items at once, stated once per estimator: the data passes go to the Gram provider,
        gram(kind, params [len(rows), p] | None, use_weights, wpow, rows) -> (G [len(rows), q, q], count [len(rows)],
        bad [len(rows)]), one request for all the items that still need it (rows = their numbers); the small dense solves run
        here on stacks.  inits = B start models or None.  Returns a list of B model lists.  The three entry points below
        differ in the provider alone."""
        raise NotImplementedError

    def nonminimal(self, ctx, sel, weights=None, init=None):
        """Least-squares fit to the selected resident points -> list of models (the reference accepts the refit only
        if exactly 1).  sel = ("index", indices) or ("label", k); the data pass runs on the device (ctx.gram =
        pgx_gram: weighted Gram matrix of the design rows), the small dense solve here: `_fit_many` with one item."""
        self._eig_ctx = ctx

        def gram(kind, prm, use_w, wpow, rows):
            G, cnt, bad = ctx.gram(kind, sel, params=None if prm is None else prm[0], weights=weights if use_w else None, wpow=wpow)
            return G[None], np.array([cnt]), np.array([bad])
        return self._fit_many(gram, 1, [init])[0]

    def nonminimal_labels(self, ctx, K, weights=None, inits=None, skip=()):
        """`nonminimal(ctx, ("label", k), weights, init=inits[k])` for k = 0..K-1 at once: every Gram request is ONE
        pgx_gram_labels launch for all labels (PEARL refits every instance per iteration; one host round trip per instance
        and request made that loop latency-bound).  Labels in `skip` are not fitted.  The Gram matrices are bit-identical to
        the single-label calls, so the results are those of K separate `nonminimal` calls."""
        self._eig_ctx = ctx
        live = [k for k in range(K) if k not in skip]
        out = [[] for _ in range(K)]
        if not live:
            return out

        def gram(kind, prm, use_w, wpow, rows):
            sel = [live[r] for r in rows]
            full = None
            if prm is not None:                   # labels not asked about get a zero-filled params row
                full = np.zeros((K, prm.shape[1]))
                full[sel] = prm
            G, cnt, bad = ctx.gram_labels(kind, K, params=full, weights=weights if use_w else None, wpow=wpow)
            return G[sel], cnt[sel], bad[sel]
        res = self._fit_many(gram, len(live), [None if inits is None else inits[k] for k in live])
        for r, k in enumerate(live):
            out[k] = res[r]
        return out

    def nonminimal_batch(self, ctx, index, weights=None, init=None):
        """`nonminimal` for B index selections of equal size (index [B, m]) sharing `init`: every Gram request is ONE
        pgx_gram_batch launch.  Returns a list of B model lists."""
        index = np.asarray(index)
        B, m = index.shape
        self._eig_ctx = ctx

        def gram(kind, prm, use_w, wpow, rows):
            G, bad = ctx.gram_batch(kind, index[rows], params=prm, weights=weights if use_w else None, wpow=wpow)
            return G, np.full(len(rows), m, dtype=np.int64), bad
        return self._fit_many(gram, B, [init] * B)

    def descriptor(self, model):
        return np.asarray(model, dtype=np.float64)

    def output(self, model):
        return np.asarray(model, dtype=np.float64).reshape(self.rows_per_model, self.cols)


# ---------------------------------------------------------------------------------------------------------------------
# 2D line  (Default2DLineEstimator, progressivex_python.cpp:489)  [U-4]
# ---------------------------------------------------------------------------------------------------------------------
class LineEstimator(Estimator):
    model_type = _lib.LINE2D
    sample_size = 2
    nonminimal_sample_size = 2
    device_minimal = True      # pgx_solve_minimal generates the hypotheses on the GPU (same formulas as minimal())

    def minimal(self, pts, samples):
        a, b = pts[samples[:, 0]], pts[samples[:, 1]]
        with np.errstate(all="ignore"):
            d = b - a
            ln = np.linalg.norm(d, axis=1)
            ok = (ln > 0) & np.isfinite(ln)        # (a length that is not finite: (-dy, dx) / inf would be a zero normal)
            nrm = np.column_stack([-d[:, 1], d[:, 0]]) / np.where(ok, ln, 1.0)[:, None]
            c = -(nrm * a).sum(axis=1)
        models = np.column_stack([nrm, c])
        return models[ok], np.nonzero(ok)[0]

    def _fit_many(self, gram, B, inits):
        """Total least squares: the normal is the smallest eigenvector of the weighted scatter about the mean.  One Gram request
        (sum w [1,x,y][1,x,y]^T), stacked 2x2 eigh (LAPACK per matrix, so an item's model does not depend on its neighbours; a
        Python-level fit per item was half of a findLines call at C1 - 5 800 fits of ~7 us each)."""
        out = [[] for _ in range(B)]
        G, cnt, _ = gram(_lib.GRAM_AFFINE, None, True, 1, np.arange(B))
        W = G[:, 0, 0]
        idx = np.nonzero((np.asarray(cnt) >= 2) & (W > 0))[0]
        if idx.size == 0:
            return out
        Wk = W[idx]
        mean = G[idx, 0, 1:] / Wk[:, None]
        scatter = G[idx][:, 1:, 1:] - Wk[:, None, None] * (mean[:, :, None] * mean[:, None, :])
        ok = np.isfinite(scatter).all(axis=(1, 2))
        evecs = np.zeros_like(scatter)
        if ok.any():
            evecs[ok] = np.linalg.eigh(scatter[ok])[1]
        for k, b in enumerate(idx):
            if not ok[k]:                         # (a non-finite scatter gets what eigh on it alone raises or returns, whoever shares the batch)
                evecs[k] = np.linalg.eigh(scatter[k])[1]
            nrm = evecs[k][:, 0]
            out[b] = [np.array([nrm[0], nrm[1], -nrm @ mean[k]])]
        return out


# ---------------------------------------------------------------------------------------------------------------------
# 3-D plane (findPlanes; no reference counterpart): the flat family with the line, whose refits differ (see _fit_many)
# ---------------------------------------------------------------------------------------------------------------------
class PlaneEstimator(Estimator):
    model_type = _lib.PLANE3D
    sample_size = 3
    nonminimal_sample_size = 3
    device_minimal = True      # pgx_solve_minimal generates the hypotheses on the GPU (same operation order as minimal())
    cols = 4

    def minimal(self, pts, samples):
        """samples [S, 3] -> unit-normal planes (a, b, c, d), bitwise csrc/solve.hip's solve_minimal for planes: n = u x v in cross3's
        component order, ln = sqrt((n0 n0 + n1 n1) + n2 n2), (a, b, c) = n / ln, d = -((a x0 + b y0) + c z0).  Collinear or
        coincident samples (ln == 0) and a non-finite ln (NaN or Inf coordinates, an overflowing product) give no model."""
        p0, p1, p2 = pts[samples[:, 0]], pts[samples[:, 1]], pts[samples[:, 2]]
        with np.errstate(all="ignore"):
            u, v = p1 - p0, p2 - p0
            n0 = u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1]
            n1 = -(u[:, 0] * v[:, 2] - u[:, 2] * v[:, 0])
            n2 = u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]
            ln = np.sqrt((n0 * n0 + n1 * n1) + n2 * n2)
            ok = (ln > 0) & np.isfinite(ln)
            ln = np.where(ok, ln, 1.0)
            a, b, c = n0 / ln, n1 / ln, n2 / ln
            d = -((a * p0[:, 0] + b * p0[:, 1]) + c * p0[:, 2])
        models = np.column_stack([a, b, c, d])
        return models[ok], np.nonzero(ok)[0]

    def _normal(self, scatter):
        """smallest eigenvectors of the 3x3 scatter matrices [B, 3, 3] (all finite) -> [B, 3]"""
        if self.refit_solver == "jacobi":
            return self._smallest(scatter)
        return np.linalg.eigh(scatter)[1][:, :, 0]

    def _fit_many(self, gram, B, inits):
        """The line's fit one dimension up: one Gram request (sum w [1,x,y,z][1,x,y,z]^T), stacked 3x3 eigen-solves; a non-finite
        scatter gives no model."""
        out = [[] for _ in range(B)]
        G, cnt, _ = gram(_lib.GRAM_AFFINE, None, True, 1, np.arange(B))
        W = G[:, 0, 0]
        idx = np.nonzero((np.asarray(cnt) >= 3) & (W > 0) & np.isfinite(G).all(axis=(1, 2)))[0]
        if idx.size == 0:
            return out
        Wk = W[idx]
        mean = G[idx, 0, 1:] / Wk[:, None]
        scatter = G[idx][:, 1:, 1:] - Wk[:, None, None] * (mean[:, :, None] * mean[:, None, :])
        ok = np.isfinite(scatter).all(axis=(1, 2))
        if not ok.any():
            return out
        nrms = self._normal(scatter[ok])
        for k, b in enumerate(idx[ok]):
            nrm = nrms[k]
            m = mean[ok][k]
            out[b] = [np.array([nrm[0], nrm[1], nrm[2], -nrm @ m])]
        return out


# ---------------------------------------------------------------------------------------------------------------------
# 3-D line (findLines3D; no reference counterpart): the plane's scatter matrix read from the other end of its spectrum
# ---------------------------------------------------------------------------------------------------------------------
class Line3DEstimator(Estimator):
    model_type = _lib.LINE3D
    sample_size = 2
    nonminimal_sample_size = 2
    device_minimal = True      # pgx_solve_minimal generates the hypotheses on the GPU (same operation order as minimal())
    cols = 6

    def minimal(self, pts, samples):
        """samples [S, 2] -> lines (p, d), a point and a unit direction, bitwise csrc/solve.hip's solve_minimal for 3-D lines:
        v = b - a, ln = sqrt((v0 v0 + v1 v1) + v2 v2), d = v / ln, p = a.  Coincident samples (ln == 0) and a length that is not
        finite (NaN or Inf coordinates, an overflowing square) give no model."""
        a, b = pts[samples[:, 0]], pts[samples[:, 1]]
        with np.errstate(all="ignore"):
            v = b - a
            ln = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
            ok = (ln > 0) & np.isfinite(ln)
            d = v / np.where(ok, ln, 1.0)[:, None]
        models = np.column_stack([a, d])
        return models[ok], np.nonzero(ok)[0]

    def _direction(self, scatter):
        """largest eigenvectors of the 3x3 scatter matrices [B, 3, 3] (all finite) -> [B, 3]; the smallest of -scatter under
        "jacobi", so the device eigen-solver serves unchanged"""
        if self.refit_solver == "jacobi":
            return self._smallest(-scatter)
        return np.linalg.eigh(scatter)[1][:, :, -1]

    def _fit_many(self, gram, B, inits):
        """Total least squares: one Gram request (sum w [1,x,y,z][1,x,y,z]^T), the weighted mean is the point and the eigenvector of
        the largest eigenvalue of the scatter about it the direction, signed so that its largest-magnitude component (the first of
        equals) is positive - which makes the two eigen-solvers agree.  A non-finite Gram matrix or scatter gives no model."""
        out = [[] for _ in range(B)]
        G, cnt, _ = gram(_lib.GRAM_AFFINE, None, True, 1, np.arange(B))
        W = G[:, 0, 0]
        idx = np.nonzero((np.asarray(cnt) >= 2) & (W > 0) & np.isfinite(G).all(axis=(1, 2)))[0]
        if idx.size == 0:
            return out
        Wk = W[idx]
        mean = G[idx, 0, 1:] / Wk[:, None]
        scatter = G[idx][:, 1:, 1:] - Wk[:, None, None] * (mean[:, :, None] * mean[:, None, :])
        ok = np.isfinite(scatter).all(axis=(1, 2))
        if not ok.any():
            return out
        dirs = self._direction(scatter[ok])
        for k, b in enumerate(idx[ok]):
            d = dirs[k]
            if d[int(np.argmax(np.abs(d)))] < 0:
                d = -d
            out[b] = [np.concatenate([mean[ok][k], d])]
        return out


# ---------------------------------------------------------------------------------------------------------------------
# The round family (no reference counterpart): 3-D sphere (findSpheres, 4-point minimal solver) and 2-D circle (findCircles, 3-point),
# one algebraic refit on normalised coordinates
# ---------------------------------------------------------------------------------------------------------------------
def _cross3(a, b):
    """csrc/solve.hip cross3's component order on [S, 3] arrays"""
    return (a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], -(a[:, 0] * b[:, 2] - a[:, 2] * b[:, 0]), a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0])


class RoundEstimator(Estimator):
    """What the sphere and the circle share: model (c[DIM], r), DIM = the model type's point dimension, the radius range and the
    algebraic refit.  A subclass adds its model type, sample size, Gram kind and minimal()."""
    device_minimal = True      # pgx_solve_minimal generates the hypotheses on the GPU (same operation order as minimal())
    gram_kind = None           # GRAM_CIRCLE / GRAM_SPHERE: the rows (1, q, |q|^2) of the refit
    radius_range = (0.0, np.inf)   # the radii a model may have (findSpheres / findCircles set it; the device solver reads pgx_set_radius_range)
    takes_radius_range = True

    def context_setup(self, ctx):
        ctx.set_radius_range(*self.radius_range)

    def _in_range(self, r):
        return (r >= self.radius_range[0]) & (r <= self.radius_range[1])

    def _fit_many(self, gram, B, inits):
        """Algebraic fit in two Gram requests: the weighted mean o and the RMS distance s from it (GRAM_AFFINE), then the smallest
        eigenvector theta of the Gram matrix of the rows (1, q, |q|^2), q = (p - o) / s, the last entry summed left to right
        (GRAM_CIRCLE: u u + v v, GRAM_SPHERE: (u u + v v) + w w): theta[0] + theta[1..DIM] . q + theta[-1] |q|^2 = 0 is the sphere
        |q + b|^2 = |b|^2 - theta[0] / theta[-1] with b = theta[1..DIM] / (2 theta[-1]), so c = o - s b and
        r = s sqrt(|b|^2 - theta[0] / theta[-1]).  The normalisation keeps the small matrix well conditioned for scenes far from
        the origin.  `inits` is not used.  The reductions whose order numpy chooses (the trace, b . b) stay per item, so a model
        does not depend on its neighbours."""
        out = [[] for _ in range(B)]
        G, cnt, _ = gram(_lib.GRAM_AFFINE, None, True, 1, np.arange(B))        # sum w [1,p][1,p]^T
        W = G[:, 0, 0]
        rows = np.nonzero((np.asarray(cnt) >= self.sample_size) & (W > 0) & np.isfinite(G).all(axis=(1, 2)))[0]
        if rows.size == 0:
            return out
        W = W[rows]
        o = G[rows, 0, 1:] / W[:, None]
        scatter = G[rows][:, 1:, 1:] - W[:, None, None] * (o[:, :, None] * o[:, None, :])
        var = np.array([np.trace(sc) for sc in scatter]) / W
        # the guard: the root is taken of a positive, finite variance only (coincident points: the trace may round to zero or below it,
        # which must give no model and no RuntimeWarning); s > 0 and finite exactly when var is
        ok = np.isfinite(o).all(axis=1) & (var > 0) & np.isfinite(var)
        if not ok.any():
            return out
        rows, o, s = rows[ok], o[ok], np.sqrt(var[ok])
        G, _, _ = gram(self.gram_kind, np.column_stack([o, s]), True, 1, rows)
        fin = np.isfinite(G).all(axis=(1, 2))
        if not fin.any():
            return out
        rows, o, s = rows[fin], o[fin], s[fin]
        for k, th in enumerate(self._smallest(G[fin])):
            A = th[-1]
            if A == 0:
                continue
            b = th[1:-1] / (2.0 * A)
            rad = b @ b - th[0] / A
            if not rad > 0:
                continue
            r = s[k] * np.sqrt(rad)
            c = o[k] - s[k] * b
            if np.isfinite(c).all() and np.isfinite(r) and self._in_range(r):
                out[rows[k]] = [np.array([*c.tolist(), r])]
        return out


class SphereEstimator(RoundEstimator):
    model_type = _lib.SPHERE3D
    sample_size = 4
    nonminimal_sample_size = 4
    cols = 4
    gram_kind = _lib.GRAM_SPHERE

    def minimal(self, pts, samples):
        """samples [S, 4] -> spheres (cx, cy, cz, r), bitwise csrc/solve.hip's solve_minimal for spheres: a_i = p_i - p0,
        h_i = 0.5 ((a_i0 a_i0 + a_i1 a_i1) + a_i2 a_i2), n1 = a2 x a3, n2 = a3 x a1, n3 = a1 x a2 in cross3's component order,
        det = (a1_0 n1_0 + a1_1 n1_1) + a1_2 n1_2, e_k = ((h1 n1_k + h2 n2_k) + h3 n3_k) / det, r = sqrt((e0 e0 + e1 e1) + e2 e2),
        c = p0 + e.  Coplanar or coincident samples (det == 0), non-finite values and radii outside radius_range give no model."""
        p0 = pts[samples[:, 0]]
        with np.errstate(all="ignore"):
            a = [pts[samples[:, i]] - p0 for i in (1, 2, 3)]
            h = [0.5 * ((ai[:, 0] * ai[:, 0] + ai[:, 1] * ai[:, 1]) + ai[:, 2] * ai[:, 2]) for ai in a]
            n1, n2, n3 = _cross3(a[1], a[2]), _cross3(a[2], a[0]), _cross3(a[0], a[1])
            det = (a[0][:, 0] * n1[0] + a[0][:, 1] * n1[1]) + a[0][:, 2] * n1[2]
            e = [((h[0] * n1[k] + h[1] * n2[k]) + h[2] * n3[k]) / det for k in range(3)]
            r = np.sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2])
            models = np.column_stack([p0[:, 0] + e[0], p0[:, 1] + e[1], p0[:, 2] + e[2], r])
            ok = (det != 0) & np.isfinite(models).all(axis=1) & self._in_range(r)
        return models[ok], np.nonzero(ok)[0]


# ---------------------------------------------------------------------------------------------------------------------
# The iterative refits (cylinder, cone, torus, PnP): the one Gauss-Newton loop, and what the three axial types share besides it
# ---------------------------------------------------------------------------------------------------------------------
def _gauss_newton(gram, kind, wpow, npar, min_count, cutoff, failed, params, update, iterations):
    """The Gauss-Newton loop of the cylinder's, the cone's, the torus' and PnP's `_fit_many`, on B items at once.  `failed` [B] bool
    marks the items that do not start (it is updated in place and returned); the others run.  Per iteration ONE Gram request for the
    running items `act`, gram(kind, params(act), True, wpow, act): the rows are (J, f), so the sums hold the normal matrix
    A = G[:npar, :npar] and the right-hand side -G[:npar, npar].  An item fails with a point that has no row (bad), with fewer than
    min_count points or with non-finite sums; the others take step = pinv(A) rhs with singular values below cutoff eps s_max dropped,
    and update(act, step, prm), prm the parameter rows that were sent for them, applies it to the caller's state and returns which
    of the new iterates are finite.  An item whose iterate is not finite fails at once; one with |step| < 1e-12 stops.  A request
    holds exactly the items still running, so an item's iterates do not depend on its neighbours."""
    running = ~failed
    for _ in range(iterations):
        act = np.nonzero(running)[0]
        if act.size == 0:
            break
        prm = params(act)
        G, cnt, bad = gram(kind, prm, True, wpow, act)
        A, rhs = G[:, :npar, :npar], -G[:, :npar, npar]
        ok = (np.asarray(bad) == 0) & (np.asarray(cnt) >= min_count) & np.isfinite(A).all(axis=(1, 2)) & np.isfinite(rhs).all(axis=1)
        failed[act[~ok]] = True
        running[act[~ok]] = False
        if not ok.any():
            break
        act = act[ok]
        step = np.einsum("bij,bj->bi", np.linalg.pinv(A[ok], rcond=cutoff * np.finfo(np.float64).eps), rhs[ok])
        fin = update(act, step, prm[ok])
        failed[act[~fin]] = True
        running[act[~fin]] = False
        running[act[np.linalg.norm(step, axis=1) < 1e-12]] = False
    return failed


def _cylinder_frame(d):
    """The one rule for the chart's u, [B, 3] unit directions d -> [B, 3]: the coordinate axis of d's smallest-magnitude component (the
    first of equals) crossed with d, normalised.  That axis is the one farthest from d, so |axis x d| >= sqrt(2 / 3)."""
    axis = np.zeros_like(d)
    axis[np.arange(len(d)), np.argmin(np.abs(d), axis=1)] = 1.0
    u = np.cross(axis, d)
    return u / np.linalg.norm(u, axis=1)[:, None]


def _axial_start(inits, blank):
    """The start of a Gauss-Newton refit of models (point[3], d[3], ...): ([B, len(blank)] rows, failed [B]).  An item without an
    init holds `blank` and fails; d is normalised; the caller fails the rows that are not finite once it has prepared them."""
    m = np.tile(np.asarray(blank, dtype=np.float64), (len(inits), 1))
    for b, ini in enumerate(inits):
        if ini is not None:
            m[b] = np.asarray(ini, dtype=np.float64).reshape(len(blank))
    with np.errstate(all="ignore"):
        m[:, 3:6] /= np.linalg.norm(m[:, 3:6], axis=1)[:, None]
    return m, np.array([ini is None for ini in inits], dtype=bool)


def _axial_params(m, act):
    """the parameter rows (model, u) of a GRAM_CYL_GN / GRAM_CONE_GN / GRAM_TORUS_GN request, u = _cylinder_frame(d)"""
    return np.column_stack([m[act], _cylinder_frame(m[act, 3:6])])


def _axial_update(m, act, u, across, along, turn):
    """The chart's step on the axis of the rows m[act], in the frame u, v = d x u: the point moves by across[0] u + across[1] v
    (+ along d, if given), the direction becomes normalise(d + turn[0] u + turn[1] v).  across, along and turn are [len(act), k]
    columns of the step."""
    d = m[act, 3:6]
    v = np.cross(d, u)
    shift = across[:, 0:1] * u + across[:, 1:2] * v
    m[act, 0:3] += shift if along is None else shift + along * d
    d = d + turn[:, 0:1] * u + turn[:, 1:2] * v
    m[act, 3:6] = d / np.linalg.norm(d, axis=1)[:, None]


class OrientedEstimator(Estimator):
    """What the cylinder, the cone and the torus share besides the refit's loop: a device solver that reads per-point `normals`, and a
    `radius_range` that bounds hypotheses and refits (the device solver reads it from pgx_set_radius_range)."""
    device_minimal = True      # pgx_solve_minimal generates the hypotheses on the GPU (same operation order as minimal())
    takes_radius_range = True
    radius_range = (0.0, np.inf)
    normals = None             # [n, 3] float64, in the points' order (the entry point sets it)

    def context_setup(self, ctx):
        ctx.set_radius_range(*self.radius_range)
        ctx.set_normals(self.normals)


# ---------------------------------------------------------------------------------------------------------------------
# Cylinder (findCylinders; no reference counterpart): 2-point solver on oriented points, Gauss-Newton refit on five parameters
# ---------------------------------------------------------------------------------------------------------------------
class CylinderEstimator(OrientedEstimator):
    """Model (p[3], d[3], r): a point on the axis, a unit direction, a radius.  `normals` [n, 3] (per point, neither unit nor
    consistently signed) are read by the minimal solver alone; `radius_range` bounds the radii of hypotheses and refits.

    nonminimal_sample_size is 5, the number of parameters of the chart (a line in space has four, the radius is the fifth): with fewer
    points the 5x5 normal matrix is singular for every configuration, with five it is regular for points in general position.  It is
    not raised above that: the refit always starts from a model that was scored (`init`), the local optimisation draws 14 points, and a
    refit of a small, noisy selection that comes out worse than its start loses to it when both are scored."""
    model_type = _lib.CYLINDER3D
    sample_size = 2
    nonminimal_sample_size = 5
    cols = 7

    def _in_range(self, r):
        return (r >= self.radius_range[0]) & (r <= self.radius_range[1])

    def minimal(self, pts, samples):
        """samples [S, 2] -> cylinders (c, d, r), bitwise csrc/solve.hip's solve_minimal for cylinders, with (a, b) the samples and
        (na, nb) their normals: D = cross3(na, nb), dd = (D0 D0 + D1 D1) + D2 D2, ln = sqrt(dd), d = D / ln, v = b - a,
        k = (v0 d0 + v1 d1) + v2 d2, w = v - k d, x = cross3(w, nb), s = ((x0 D0 + x1 D1) + x2 D2) / dd, c = a + s na,
        r = |s| sqrt((na0 na0 + na1 na1) + na2 na2).  No model unless ln > 0 and finite (parallel or zero normals, the same point
        twice, non-finite input), c and r are finite and r lies in radius_range."""
        a, b = pts[samples[:, 0]], pts[samples[:, 1]]
        nrm = np.asarray(self.normals, dtype=np.float64)
        na, nb = nrm[samples[:, 0]], nrm[samples[:, 1]]
        with np.errstate(all="ignore"):
            D = _cross3(na, nb)
            dd = (D[0] * D[0] + D[1] * D[1]) + D[2] * D[2]
            ln = np.sqrt(dd)
            d = [D[j] / ln for j in range(3)]
            v = b - a
            k = (v[:, 0] * d[0] + v[:, 1] * d[1]) + v[:, 2] * d[2]
            w = np.column_stack([v[:, j] - k * d[j] for j in range(3)])
            x = _cross3(w, nb)
            s = ((x[0] * D[0] + x[1] * D[1]) + x[2] * D[2]) / dd
            r = np.abs(s) * np.sqrt((na[:, 0] * na[:, 0] + na[:, 1] * na[:, 1]) + na[:, 2] * na[:, 2])
            models = np.column_stack([a[:, 0] + s * na[:, 0], a[:, 1] + s * na[:, 1], a[:, 2] + s * na[:, 2], d[0], d[1], d[2], r])
            ok = (ln > 0) & np.isfinite(ln) & np.isfinite(models[:, [0, 1, 2, 6]]).all(axis=1) & self._in_range(r)
        return models[ok], np.nonzero(ok)[0]

    def _fit_many(self, gram, B, inits, iterations=10):
        """Geometric least squares, sum w (|(x - p) x d| - r)^2, by Gauss-Newton from `inits` (the loop is _gauss_newton's):
        at most 10 iterations on [B, ...] stacks, each ONE Gram request (GRAM_CYL_GN, weight power 1) at params (p, d, r, u) with
        u = _cylinder_frame(d) and v = d x u.  The rows are (J, f) with J = df / d(alpha, beta, gamma, eta, rho) in the chart
        p + alpha u + beta v, normalise(d + gamma u + eta v), r + rho (csrc/fit.hip GenCylGn), so delta = pinv(J^T J)(-J^T f) with the
        cut-off 6 eps, then that update; an item stops at |delta| < 1e-12.  An item fails without an init, with fewer than 5 points,
        with a point on its axis (bad) or with non-finite sums.  Afterwards the model is made canonical: p slides along d to the foot
        of the selection's weighted mean (one GRAM_AFFINE request), d is signed like Line3DEstimator's (its largest-magnitude
        component, the first of equals, positive); a model that is not finite or whose radius is outside radius_range is dropped."""
        out = [[] for _ in range(B)]
        m, failed = _axial_start(inits, (0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0))
        failed |= ~np.isfinite(m).all(axis=1)

        def update(act, delta, prm):
            _axial_update(m, act, prm[:, 7:10], delta[:, 0:2], None, delta[:, 2:4])
            m[act, 6] += delta[:, 4]
            return np.isfinite(m[act]).all(axis=1)
        _gauss_newton(gram, _lib.GRAM_CYL_GN, wpow=1, npar=5, min_count=5, cutoff=6, failed=failed, params=lambda act: _axial_params(m, act),
                      update=update, iterations=iterations)
        rows = np.nonzero(~failed)[0]
        if rows.size == 0:
            return out
        G, _, _ = gram(_lib.GRAM_AFFINE, None, True, 1, rows)
        W = G[:, 0, 0]
        with np.errstate(all="ignore"):
            mean = G[:, 0, 1:] / W[:, None]
        for k, b in enumerate(rows):
            p, d, r = m[b, 0:3], m[b, 3:6], m[b, 6]
            if not (W[k] > 0 and np.isfinite(mean[k]).all()):
                continue
            p = p + ((mean[k] - p) @ d) * d
            if d[int(np.argmax(np.abs(d)))] < 0:
                d = -d
            model = np.array([*p.tolist(), *d.tolist(), r])
            if np.isfinite(model).all() and self._in_range(r):
                out[b] = [model]
        return out


# ---------------------------------------------------------------------------------------------------------------------
# Cone (findCones; no reference counterpart): 3-point solver on oriented points, Gauss-Newton refit on six parameters
# ---------------------------------------------------------------------------------------------------------------------
class ConeEstimator(OrientedEstimator):
    """Model (a[3], d[3], c, s): the apex, a unit axis direction pointing into the nappe, the cosine and sine of the half-angle.
    `normals` [n, 3] (per point, neither unit nor consistently signed) are read by the minimal solver alone.  `radius_range` is the
    range of s = sin(half-angle) of hypotheses and refits, (sin theta_min, sin theta_max): a cone has no radius, and the context's radius
    range carries its angle range (include/pgx.h).

    nonminimal_sample_size is 6, the number of parameters of the chart (apex 3, direction 2, angle 1): with fewer points the 6x6 normal
    matrix is singular for every configuration.  As for cylinders it is not raised above that: the refit always starts from a model
    that was scored."""
    model_type = _lib.CONE3D
    sample_size = 3
    nonminimal_sample_size = 6
    cols = 8
    radius_range = (0.0, 1.0)

    def _in_range(self, s):
        return (s >= self.radius_range[0]) & (s <= self.radius_range[1])

    def minimal(self, pts, samples):
        """samples [S, 3] -> cones (a, d, c, s), bitwise csrc/solve.hip's solve_minimal for cones, with p_i the samples and n_i their
        normals: X0 = cross3(n1, n2), X1 = cross3(n2, n0), X2 = cross3(n0, n1), det = (n0_0 X0_0 + n0_1 X0_1) + n0_2 X0_2,
        b_i = (n_i0 p_i0 + n_i1 p_i1) + n_i2 p_i2, a_k = ((b0 X0_k + b1 X1_k) + b2 X2_k) / det, w_i = p_i - a, l_i = |w_i|, g_i = w_i / l_i,
        D = cross3(g1 - g0, g2 - g0), ln = |D|, d = D / ln, negated when ((d . g0) + (d . g1)) + (d . g2) < 0, c = d . g0,
        s = sqrt of the 3-D line's squared residual of g0 about (0, d).  No model unless det != 0, every l_i > 0, ln > 0, everything is
        finite, c > 0 and s lies in radius_range."""
        p = [pts[samples[:, i]] for i in range(3)]
        nrm = np.asarray(self.normals, dtype=np.float64)
        n = [nrm[samples[:, i]] for i in range(3)]
        dot = lambda x, y: (x[0] * y[0] + x[1] * y[1]) + x[2] * y[2]   # noqa: E731  (on component lists)
        comp = lambda x: [x[:, 0], x[:, 1], x[:, 2]]                   # noqa: E731
        with np.errstate(all="ignore"):
            X = [_cross3(n[1], n[2]), _cross3(n[2], n[0]), _cross3(n[0], n[1])]
            det = dot(comp(n[0]), X[0])
            b = [dot(comp(n[i]), comp(p[i])) for i in range(3)]
            a = [((b[0] * X[0][k] + b[1] * X[1][k]) + b[2] * X[2][k]) / det for k in range(3)]
            g, lpos = [], np.ones(len(samples), dtype=bool)
            for i in range(3):
                w = [p[i][:, k] - a[k] for k in range(3)]
                ln_i = np.sqrt(dot(w, w))
                lpos &= ln_i > 0
                g.append([w[k] / ln_i for k in range(3)])
            r1 = np.column_stack([g[1][k] - g[0][k] for k in range(3)])
            r2 = np.column_stack([g[2][k] - g[0][k] for k in range(3)])
            D = _cross3(r1, r2)
            ln = np.sqrt(dot(D, D))
            d = [D[k] / ln for k in range(3)]
            t = [dot(d, g[i]) for i in range(3)]
            flip = (t[0] + t[1]) + t[2] < 0
            d = [np.where(flip, -d[k], d[k]) for k in range(3)]
            c = dot(d, g[0])
            e = [g[0][k] - 0.0 for k in range(3)]
            c0 = e[1] * d[2] - e[2] * d[1]
            c1 = -(e[0] * d[2] - e[2] * d[0])
            c2 = e[0] * d[1] - e[1] * d[0]
            s = np.sqrt((c0 * c0 + c1 * c1) + c2 * c2)
            models = np.column_stack([a[0], a[1], a[2], d[0], d[1], d[2], c, s])
            ok = (det != 0) & lpos & (ln > 0) & np.isfinite(models).all(axis=1) & (c > 0) & self._in_range(s)
        return models[ok], np.nonzero(ok)[0]

    @staticmethod
    def canonical(m):
        """[B, 8] -> the same cones (every residual keeps its value) with s >= 0 and c >= 0: (c, s) -> (-c, -s) negates c rho - s h, and
        so does (d, c) -> (-d, -c).  Afterwards d points into the nappe: that is its sign, there is no other convention."""
        m = np.array(m, dtype=np.float64, copy=True)
        neg = m[:, 7] < 0
        m[neg, 6:8] = -m[neg, 6:8]
        neg = m[:, 6] < 0
        m[neg, 3:7] = -m[neg, 3:7]
        return m

    def _fit_many(self, gram, B, inits, iterations=10):
        """Geometric least squares, sum w (c rho - s h)^2 with rho = |(x - a) x d| and h = (x - a) . d, by Gauss-Newton from `inits`
        (the loop is _gauss_newton's): at most 10 iterations on [B, ...] stacks, each ONE Gram request (GRAM_CONE_GN, weight
        power 1) at params (a, d, c, s, u) with u = _cylinder_frame(d) and v = d x u.  The rows are (J, f) with
        J = df / d(alpha, beta, gamma, delta, eta, tau) in the chart a + alpha u + beta v + gamma d, normalise(d + delta u + eta v),
        (c, s) <- normalise(c - tau s, s + tau c) (csrc/fit.hip GenConeGn), so step = pinv(J^T J)(-J^T f) with the cut-off 6 eps, then
        that update; an item stops at |step| < 1e-12.  An item fails without an init, with fewer than 6 points, with a point on its axis
        (bad) or with non-finite sums.  Afterwards the model is made canonical (canonical(): d unit and pointing into the nappe, (c, s)
        unit with both entries positive); a model that is not finite, has c <= 0 or s <= 0, or whose s is outside radius_range is
        dropped."""
        out = [[] for _ in range(B)]
        m, failed = _axial_start(inits, (0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 1.0, 0.0))
        with np.errstate(all="ignore"):
            m[:, 6:8] /= np.linalg.norm(m[:, 6:8], axis=1)[:, None]
        failed |= ~np.isfinite(m).all(axis=1)

        def update(act, step, prm):
            _axial_update(m, act, prm[:, 8:11], step[:, 0:2], step[:, 2:3], step[:, 3:5])
            cs = np.column_stack([m[act, 6] - step[:, 5] * m[act, 7], m[act, 7] + step[:, 5] * m[act, 6]])
            m[act, 6:8] = cs / np.linalg.norm(cs, axis=1)[:, None]
            return np.isfinite(m[act]).all(axis=1)
        _gauss_newton(gram, _lib.GRAM_CONE_GN, wpow=1, npar=6, min_count=6, cutoff=6, failed=failed, params=lambda act: _axial_params(m, act),
                      update=update, iterations=iterations)
        rows = np.nonzero(~failed)[0]
        if rows.size == 0:
            return out
        mc = self.canonical(m[rows])
        for k, b in enumerate(rows):
            model = mc[k]
            if np.isfinite(model).all() and model[6] > 0 and model[7] > 0 and self._in_range(model[7]):
                out[b] = [model]
        return out


# ---------------------------------------------------------------------------------------------------------------------
# Mixed primitives (findPrimitives; no reference counterpart): planes, spheres, cylinders and cones in one fit
# ---------------------------------------------------------------------------------------------------------------------
# name -> class number, in the slot order of the device solver (and the bit order of pgx_set_primitive_classes)
PRIMITIVE_CLASSES = {"plane": _lib.PLANE3D, "sphere": _lib.SPHERE3D, "cylinder": _lib.CYLINDER3D, "cone": _lib.CONE3D}


class PrimitiveEstimator(Estimator):
    """Model (class, q0 .. q7): the class number of a constituent type (6 plane, 8 sphere, 14 cylinder, 16 cone) and that type's model
    row padded with zeros.  The estimator owns one constituent estimator per enabled class (`parts`, class number -> estimator) and
    adds nothing of its own to their arithmetic: minimal() is their minimal() on the sample prefixes, a refit is their refit on the
    items of their class.  An instance never changes class: a refit reads the class from its init and puts it back in front.

    `radius_range` bounds the radii of spheres and cylinders, `sine_range` the sine of the cones' half-angle (the device solver reads
    the first from pgx_set_radius_range and the second from pgx_set_primitive_classes); `normals` [n, 3] go to the cylinder's and the
    cone's solvers.  nonminimal_sample_size is the largest among the enabled classes: PEARL refits no instance with fewer points,
    whatever its class."""
    model_type = _lib.PRIMITIVE3D
    sample_size = 4
    nonminimal_sample_size = 6
    device_minimal = True      # pgx_solve_minimal generates the hypotheses on the GPU, four slots per sample (same operation order as minimal())
    device_slots = 4
    cols = 9
    takes_radius_range = True
    # per class, in slot order: (class number, constituent, points of the sample it reads)
    _SLOTS = ((_lib.PLANE3D, PlaneEstimator, 3), (_lib.SPHERE3D, SphereEstimator, 4), (_lib.CYLINDER3D, CylinderEstimator, 2),
              (_lib.CONE3D, ConeEstimator, 3))

    def __init__(self, classes=tuple(PRIMITIVE_CLASSES)):
        try:
            classes = list(classes)
        except TypeError:
            classes = []
        unknown = [c for c in classes if c not in PRIMITIVE_CLASSES]
        if unknown or not classes or len(set(classes)) != len(classes):
            raise ValueError("classes should be a non-empty selection of distinct names among " + ", ".join(PRIMITIVE_CLASSES))
        on = {PRIMITIVE_CLASSES[c] for c in classes}
        self.parts = {cls: make() for cls, make, _ in self._SLOTS if cls in on}
        self.class_mask = sum(1 << j for j, (cls, _, _) in enumerate(self._SLOTS) if cls in on)
        self.nonminimal_sample_size = max(p.nonminimal_sample_size for p in self.parts.values())
        self._radius_range = (0.0, np.inf)
        self._sine_range = (0.0, 1.0)
        self._normals = None
        self.radius_range, self.sine_range = self._radius_range, self._sine_range

    @property
    def radius_range(self):
        return self._radius_range

    @radius_range.setter
    def radius_range(self, rng):
        self._radius_range = (float(rng[0]), float(rng[1]))
        for cls in (_lib.SPHERE3D, _lib.CYLINDER3D):
            if cls in self.parts:
                self.parts[cls].radius_range = self._radius_range

    @property
    def sine_range(self):
        return self._sine_range

    @sine_range.setter
    def sine_range(self, rng):
        self._sine_range = (float(rng[0]), float(rng[1]))
        if _lib.CONE3D in self.parts:
            self.parts[_lib.CONE3D].radius_range = self._sine_range     # the cone estimator's range is that of its sine

    @property
    def normals(self):
        return self._normals

    @normals.setter
    def normals(self, nrm):
        self._normals = nrm
        for cls in (_lib.CYLINDER3D, _lib.CONE3D):
            if cls in self.parts:
                self.parts[cls].normals = nrm

    def context_setup(self, ctx):
        ctx.set_normals(self._normals)
        ctx.set_radius_range(*self._radius_range)
        ctx.set_primitive_classes(self.class_mask, *self._sine_range)

    def _row(self, cls, q):
        """(class, q padded with zeros) for one model row or a stack of them"""
        q = np.asarray(q, dtype=np.float64)
        out = np.zeros(q.shape[:-1] + (self.cols,))
        out[..., 0] = cls
        out[..., 1:1 + q.shape[-1]] = q
        return out

    def minimal(self, pts, samples):
        """samples [S, 4] -> the rows csrc/solve.hip's solve_primitive_kernel fills, bit for bit, without its all-NaN rows: slot j of sample
        s (row 4 s + j there) is the j-th constituent's minimal() on the sample's first 3 (plane), 4 (sphere), 2 (cylinder) or 3 (cone)
        indices, behind its class number.  Returned in that order, sample by sample; a class that is off has no slot."""
        samples = np.asarray(samples)
        rows, src, slot = [], [], []
        for j, (cls, _, m) in enumerate(self._SLOTS):
            if cls not in self.parts:
                continue
            models, of = self.parts[cls].minimal(pts, samples[:, :m])
            rows.append(self._row(cls, models).reshape(-1, self.cols))
            src.append(np.asarray(of, dtype=np.int64))
            slot.append(np.full(len(of), j, dtype=np.int64))
        rows, src, slot = np.concatenate(rows), np.concatenate(src), np.concatenate(slot)
        order = np.lexsort((slot, src))
        return rows[order], src[order]

    def _fit_many(self, gram, B, inits):
        """The items are grouped by the class of their init, and each group goes to its constituent's _fit_many with the inits' model
        rows and a Gram provider restricted to the group's items: a request of the constituent for its items `rows` is the request of
        this provider for items group[rows], so no request mixes kinds, and the constituent sees exactly its rows and parameter rows.
        The results come back in place with the class in front.  An item without an init, with a class that is unknown or not
        enabled, gets no model.  The class of a result is the class of its init."""
        out = [[] for _ in range(B)]
        cls_of = np.full(B, np.nan)
        for b, ini in enumerate(inits):
            if ini is not None:
                cls_of[b] = np.asarray(ini, dtype=np.float64).reshape(-1)[0]
        for cls, part in self.parts.items():
            group = np.nonzero(cls_of == float(cls))[0]
            if group.size == 0:
                continue
            part.refit_solver, part._eig_ctx = self.refit_solver, self._eig_ctx

            def sub(kind, prm, use_w, wpow, rows, group=group):
                return gram(kind, prm, use_w, wpow, group[np.asarray(rows, dtype=np.int64)])
            P = part.cols
            fits = part._fit_many(sub, len(group), [np.asarray(inits[b], dtype=np.float64).reshape(-1)[1:1 + P] for b in group])
            for b, models in zip(group, fits):
                out[b] = [self._row(cls, m) for m in models]
        return out


# ---------------------------------------------------------------------------------------------------------------------
# Oriented mixed primitives (findOrientedPrimitives; no reference counterpart): findPrimitives whose inliers agree with the normals
# ---------------------------------------------------------------------------------------------------------------------
def surface_normals(pts, row):
    """g [n, 3], the unnormalised direction of the surface normal of the model row (class, q0 .. q7) at the points pts [n, 3], in the
    operation order of csrc/residuals.hip.h Residual<kOrientedPrimitive3D>::surface_normal; None for a class that is no class."""
    pts = np.asarray(pts, dtype=np.float64)
    row = np.asarray(row, dtype=np.float64).reshape(-1)
    cls, x = row[0], [pts[:, 0], pts[:, 1], pts[:, 2]]
    if cls == _lib.PLANE3D:
        return np.stack([np.full(len(pts), row[1 + k]) for k in range(3)], axis=1)
    if cls == _lib.SPHERE3D:
        return np.stack([x[k] - row[1 + k] for k in range(3)], axis=1)
    if cls not in (_lib.CYLINDER3D, _lib.CONE3D):
        return None
    e = [x[k] - row[1 + k] for k in range(3)]
    d = row[4:7]
    t = (e[0] * d[0] + e[1] * d[1]) + e[2] * d[2]
    if cls == _lib.CYLINDER3D:
        return np.stack([e[k] - t * d[k] for k in range(3)], axis=1)
    c0 = e[1] * d[2] - e[2] * d[1]                 # the 3-D line's squared distance, as the cone's residual computes it
    c1 = -(e[0] * d[2] - e[2] * d[0])
    c2 = e[0] * d[1] - e[1] * d[0]
    with np.errstate(invalid="ignore"):
        rho = np.sqrt((c0 * c0 + c1 * c1) + c2 * c2)
    sr = row[8] * rho
    return np.stack([row[7] * (e[k] - t * d[k]) - sr * d[k] for k in range(3)], axis=1)


def normals_agree(nrm, g, kappa):
    """bool [n]: (n.g)^2 >= kappa (n.n)(g.g) and (n.n)(g.g) > 0, every dot product a left fold (the device's test, bit for bit)."""
    nrm = np.asarray(nrm, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        nn = (nrm[:, 0] * nrm[:, 0] + nrm[:, 1] * nrm[:, 1]) + nrm[:, 2] * nrm[:, 2]
        gg = (g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2]
        ng = (nrm[:, 0] * g[:, 0] + nrm[:, 1] * g[:, 1]) + nrm[:, 2] * g[:, 2]
        w = nn * gg
        return (ng * ng >= kappa * w) & (w > 0.0)


class OrientedPrimitiveEstimator(PrimitiveEstimator):
    """PrimitiveEstimator on model type 20: the same model rows, solvers and refits, but a point supports a model only if its normal
    deviates from the model's surface normal at the point by less than `normal_tolerance` degrees (csrc/residuals.hip.h
    Residual<kOrientedPrimitive3D>: the device reads kappa = cos^2(tolerance) from pgx_set_normal_tolerance).  A hypothesis that does
    not agree with the normals of its own sample's prefix is dropped (Schnabel's candidate test; an all-NaN row on the device).  The
    refits are the constituents' on the inlier lists they are given, which under this type hold compatible points only."""
    model_type = _lib.ORIENTED_PRIMITIVE3D

    def __init__(self, classes=tuple(PRIMITIVE_CLASSES), normal_tolerance=20.0):
        super().__init__(classes)
        tol = float(normal_tolerance)
        if not (0.0 < tol <= 90.0):
            raise ValueError("normal_tolerance should be an angle in degrees with 0 < normal_tolerance <= 90")
        self.normal_tolerance = tol
        c = np.cos(np.deg2rad(tol)) if tol < 90.0 else 0.0
        self.kappa = float(c * c)

    def context_setup(self, ctx):
        super().context_setup(ctx)
        ctx.set_normal_tolerance(self.kappa)

    def minimal(self, pts, samples):
        """PrimitiveEstimator.minimal's rows without those that disagree with the normals of their own prefix: what
        csrc/solve.hip's oriented_slots_kernel leaves, without its all-NaN rows."""
        rows, src = super().minimal(pts, samples)
        samples, pts = np.asarray(samples), np.asarray(pts, dtype=np.float64)
        nrm = np.asarray(self._normals, dtype=np.float64)
        prefix = {cls: m for cls, _, m in self._SLOTS}
        keep = np.zeros(len(rows), dtype=bool)
        for r, (row, s) in enumerate(zip(rows, src)):
            if not row[0] == row[0]:
                continue
            idx = samples[s, :prefix[int(row[0])]]
            g = surface_normals(pts[idx], row)
            keep[r] = g is not None and bool(normals_agree(nrm[idx], g, self.kappa).all())
        return rows[keep], src[keep]


# ---------------------------------------------------------------------------------------------------------------------
# Torus (findTori; no reference counterpart): 4-point solver on oriented points with two slots, Gauss-Newton refit on seven parameters
# ---------------------------------------------------------------------------------------------------------------------
class TorusEstimator(OrientedEstimator):
    """Model (c[3], d[3], R, r): the centre, a unit axis direction, the major radius (axis to the tube's centre circle) and the minor
    (tube) radius of a ring torus, R > r > 0.  `normals` [n, 3] (per point, neither unit nor consistently signed) are read by the
    minimal solver alone, as lines.  `radius_range` bounds r and `major_radius_range` bounds R, of hypotheses and refits.

    nonminimal_sample_size is 7, the number of parameters of the chart (centre 3, direction 2, two radii): with fewer points the 7x7
    normal matrix is singular for every configuration.  As for cylinders and cones it is not raised above that: the refit always starts
    from a model that was scored."""
    model_type = _lib.TORUS3D
    sample_size = 4
    nonminimal_sample_size = 7
    device_slots = 2           # two hypotheses per sample
    cols = 8
    major_radius_range = (0.0, np.inf)

    def context_setup(self, ctx):
        super().context_setup(ctx)
        ctx.set_major_radius_range(*self.major_radius_range)

    def _in_range(self, R, r):
        return ((r >= self.radius_range[0]) & (r <= self.radius_range[1]) & (R >= self.major_radius_range[0]) &
                (R <= self.major_radius_range[1]) & (R > r))

    def minimal_rows(self, pts, samples):
        """samples [S, 4] -> [2 S, 8], row 2 s + j the torus of slot j or NaN: bitwise csrc/solve.hip's solve_minimal for tori, whose
        comment states the operation order (the two transversals of the four normal lines by a quadratic in s, the axis through
        a = p0 + s n0 and b = p1 + t n1, the circle through (h_k, rho_k) of samples 0, 1, 2 by the 3-point circle solver's arithmetic)."""
        samples = np.asarray(samples)
        S = len(samples)
        pts = np.asarray(pts, dtype=np.float64)
        nrm = np.asarray(self.normals, dtype=np.float64)
        # every array below is over the 2 S rows: sample s twice, slot 0 then slot 1
        rows = np.repeat(np.arange(S), 2)
        slot = np.tile(np.arange(2), S)
        comp = lambda x: [x[:, 0], x[:, 1], x[:, 2]]                   # noqa: E731
        dot = lambda x, y: (x[0] * y[0] + x[1] * y[1]) + x[2] * y[2]   # noqa: E731  (on component lists)
        p = [pts[samples[rows, i]] for i in range(4)]
        n = [nrm[samples[rows, i]] for i in range(4)]
        with np.errstate(all="ignore"):
            q = comp(p[1] - p[0])
            n0, n1 = comp(n[0]), comp(n[1])
            A, B, C, D = [], [], [], []
            for i in (2, 3):
                g = p[i] - p[0]
                X = _cross3(n[i], g)
                Y = _cross3(n[i], n[0])
                A.append(-dot(n1, Y))
                B.append(-(dot(q, Y) + dot(n0, X)))
                C.append(dot(n1, X))
                D.append(dot(q, X))
            qa = B[1] * A[0] - A[1] * B[0]
            qb = ((B[1] * C[0] - A[1] * D[0]) - C[1] * B[0]) + D[1] * A[0]
            qc = D[1] * C[0] - C[1] * D[0]
            disc = qb * qb - (4.0 * qa) * qc
            sq = np.sqrt(disc)
            s = np.where(slot == 0, (-qb + sq) / (2.0 * qa), (-qb - sq) / (2.0 * qa))
            den = A[0] * s + C[0]
            t = -(B[0] * s + D[0]) / den
            a = [p[0][:, k] + s * n0[k] for k in range(3)]
            b = [p[1][:, k] + t * n1[k] for k in range(3)]
            Dv = [b[k] - a[k] for k in range(3)]
            ln = np.sqrt(dot(Dv, Dv))
            d = [Dv[k] / ln for k in range(3)]
            h, rho = [], []
            for k in range(3):
                e = [p[k][:, j] - a[j] for j in range(3)]
                h.append(dot(e, d))
                c0 = e[1] * d[2] - e[2] * d[1]
                c1 = -(e[0] * d[2] - e[2] * d[0])
                c2 = e[0] * d[1] - e[1] * d[0]
                rho.append(np.sqrt((c0 * c0 + c1 * c1) + c2 * c2))
            a10, a11, a20, a21 = h[1] - h[0], rho[1] - rho[0], h[2] - h[0], rho[2] - rho[0]
            g1, g2 = 0.5 * (a10 * a10 + a11 * a11), 0.5 * (a20 * a20 + a21 * a21)
            det = a10 * a21 - a11 * a20
            z0, z1 = (g1 * a21 - g2 * a11) / det, (a10 * g2 - a20 * g1) / det
            r = np.sqrt(z0 * z0 + z1 * z1)
            hc, R = h[0] + z0, rho[0] + z1
            c = [a[k] + hc * d[k] for k in range(3)]
            models = np.column_stack([c[0], c[1], c[2], d[0], d[1], d[2], R, r])
            ok = ((disc >= 0) & (qa != 0) & (den != 0) & (ln > 0) & (det != 0) & np.isfinite(models).all(axis=1) & self._in_range(R, r))
        models[~ok] = np.nan
        return models

    def minimal(self, pts, samples):
        """samples [S, 4] -> (tori [H, 8], sample of each [H]): the rows of minimal_rows that hold a model, in its order"""
        models = self.minimal_rows(pts, samples)
        ok = ~np.isnan(models[:, 0])
        return models[ok], np.nonzero(ok)[0] // 2

    def _fit_many(self, gram, B, inits, iterations=10):
        """Geometric least squares, sum w (sqrt((rho - R)^2 + h^2) - r)^2 with rho = |(x - c) x d| and h = (x - c) . d, by Gauss-Newton
        from `inits` (the loop is _gauss_newton's): at most 10 iterations on [B, ...] stacks, each ONE Gram request
        (GRAM_TORUS_GN, weight power 1) at params (c, d, R, r, u) with u = _cylinder_frame(d) and v = d x u.  The rows are (J, f) with
        J = df / d(alpha, beta, gamma, delta, eta, dR, dr) in the chart c + alpha u + beta v + gamma d, normalise(d + delta u + eta v),
        R + dR, r + dr (csrc/fit.hip GenTorusGn), so step = pinv(J^T J)(-J^T f) with the cut-off 7 eps, then that update; an item stops
        at |step| < 1e-12.  An item fails without an init, with fewer than 7 points, with a point on its axis or spine (bad) or with
        non-finite sums.  A model that is not finite, has r <= 0 or R <= r, or whose radii lie outside radius_range /
        major_radius_range is dropped: Gauss-Newton from a ring torus has no reason to leave r > 0, R > 0, and a model that did is
        no ring torus (negating r or R is not a symmetry of the residual)."""
        out = [[] for _ in range(B)]
        m, failed = _axial_start(inits, (0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 2.0, 1.0))
        failed |= ~np.isfinite(m).all(axis=1)

        def update(act, step, prm):
            _axial_update(m, act, prm[:, 8:11], step[:, 0:2], step[:, 2:3], step[:, 3:5])
            m[act, 6] += step[:, 5]
            m[act, 7] += step[:, 6]
            return np.isfinite(m[act]).all(axis=1)
        _gauss_newton(gram, _lib.GRAM_TORUS_GN, wpow=1, npar=7, min_count=7, cutoff=7, failed=failed, params=lambda act: _axial_params(m, act),
                      update=update, iterations=iterations)
        for b in np.nonzero(~failed)[0]:
            model = m[b]
            if np.isfinite(model).all() and model[7] > 0 and bool(self._in_range(model[6], model[7])):
                out[b] = [model.copy()]
        return out


# ---------------------------------------------------------------------------------------------------------------------
# 2-D circle: the round family's other member
# ---------------------------------------------------------------------------------------------------------------------
class CircleEstimator(RoundEstimator):
    model_type = _lib.CIRCLE2D
    sample_size = 3
    nonminimal_sample_size = 3
    cols = 3
    gram_kind = _lib.GRAM_CIRCLE

    def minimal(self, pts, samples):
        """samples [S, 3] -> circles (cx, cy, r), bitwise csrc/solve.hip's solve_minimal for circles: a_i = p_i - p0,
        h_i = 0.5 (a_i0 a_i0 + a_i1 a_i1), det = a_10 a_21 - a_11 a_20, e_0 = (h_1 a_21 - h_2 a_11) / det,
        e_1 = (a_10 h_2 - a_20 h_1) / det, r = sqrt(e_0 e_0 + e_1 e_1), c = p0 + e.  Collinear or coincident samples (det == 0),
        non-finite values and radii outside radius_range give no model."""
        p0 = pts[samples[:, 0]]
        with np.errstate(all="ignore"):
            a1, a2 = pts[samples[:, 1]] - p0, pts[samples[:, 2]] - p0
            h1 = 0.5 * (a1[:, 0] * a1[:, 0] + a1[:, 1] * a1[:, 1])
            h2 = 0.5 * (a2[:, 0] * a2[:, 0] + a2[:, 1] * a2[:, 1])
            det = a1[:, 0] * a2[:, 1] - a1[:, 1] * a2[:, 0]
            e0 = (h1 * a2[:, 1] - h2 * a1[:, 1]) / det
            e1 = (a1[:, 0] * h2 - a2[:, 0] * h1) / det
            r = np.sqrt(e0 * e0 + e1 * e1)
            models = np.column_stack([p0[:, 0] + e0, p0[:, 1] + e1, r])
            ok = (det != 0) & np.isfinite(models).all(axis=1) & self._in_range(r)
        return models[ok], np.nonzero(ok)[0]


# ---------------------------------------------------------------------------------------------------------------------
# vanishing point: solver_vanishing_point_two_lines.h (in-tree, exact restatement)
# ---------------------------------------------------------------------------------------------------------------------
class VanishingPointEstimator(Estimator):
    model_type = _lib.VANISHING_POINT
    sample_size = 2            # solver_vanishing_point_two_lines.h:70-73
    nonminimal_sample_size = 2  # the same solver class is used for both (progressivex_python.cpp:343-346)
    device_minimal = True      # pgx_solve_minimal generates the hypotheses on the GPU (same formulas as minimal())

    @staticmethod
    def _cross(a1, b1, c1, a2, b2, c2):  # :106-121
        return b1 * c2 - c1 * b2, -(a1 * c2 - c1 * a2), a1 * b2 - b1 * a2

    def minimal(self, pts, samples):
        s0, s1 = pts[samples[:, 0]], pts[samples[:, 1]]
        one = np.ones(len(samples))
        with np.errstate(all="ignore"):
            l0 = self._cross(s0[:, 0], s0[:, 1], one, s0[:, 2], s0[:, 3], one)      # :174-176
            l1 = self._cross(s1[:, 0], s1[:, 1], one, s1[:, 2], s1[:, 3], one)      # :177-179
            v = np.column_stack(self._cross(l0[0], l0[1], l0[2], l1[0], l1[1], l1[2]))  # :180-182
            ln = np.sqrt((v * v).sum(axis=1))                                    # :123-131 vec_norm
            ok = (ln > 0) & np.isfinite(ln)        # (a norm that is not finite: v / inf would be the zero vector)
            v = v / np.where(ok, ln, 1.0)[:, None]
        return v[ok], np.nonzero(ok)[0]

    def _fit_many(self, gram, B, inits):
        """Smallest eigenvector of A^T A, rows A = [y0*mz-my, mx-x0*mz, x0*my-y0*mx] * w (:212-218) generated and accumulated on
        the device: one Gram request, stacked 3x3 eigh (:227 SelfAdjointEigenSolver, :230-233; LAPACK per matrix)."""
        out = [[] for _ in range(B)]
        AtA, cnt, _ = gram(_lib.GRAM_VP, None, True, 2, np.arange(B))
        idx = np.nonzero((cnt >= 2) & np.isfinite(AtA).all(axis=(1, 2)))[0]
        if idx.size == 0:
            return out
        if self.refit_solver == "jacobi":
            vs = self._smallest(AtA[idx])
        else:
            evals, evecs = np.linalg.eigh(AtA[idx])
            pick = np.argmin(evals, axis=1)
            vs = np.array([evecs[k][:, int(pick[k])] for k in range(len(idx))])
        for k, b in enumerate(idx):
            v = vs[k]
            n = np.linalg.norm(v)
            if n > 0:
                out[b] = [v / n]
        return out


# ---------------------------------------------------------------------------------------------------------------------
# homography (DefaultHomographyEstimator, progressivex_python.cpp:252)  [UPSTREAM-MEMORY]: 4-point, h33 = 1
# ---------------------------------------------------------------------------------------------------------------------
def _dlt_rows(x1, y1, x2, y2):
    z = np.zeros_like(x1)
    o = np.ones_like(x1)
    r1 = np.stack([-x1, -y1, -o, z, z, z, x2 * x1, x2 * y1, x2], axis=-1)
    r2 = np.stack([z, z, z, -x1, -y1, -o, y2 * x1, y2 * y1, y2], axis=-1)
    return r1, r2


def _hartley_batch(G, cnt):
    """Normalising similarities of both images from one pass of first/second moments (the affine Gram matrices G [B, 5, 5] with
    counts cnt [B], all >= 1; isotropic scaling to an RMS distance of sqrt(2) from the centroid): (T1 [B,3,3], T2 [B,3,3],
    params [B,6] for the DLT / epipolar rows) - elementwise arithmetic, an item's result does not depend on its neighbours."""
    B = G.shape[0]
    cnt = np.asarray(cnt, dtype=np.float64).reshape(B, 1)
    c = G[:, 0, 1:] / cnt
    var = np.maximum(np.diagonal(G, axis1=1, axis2=2)[:, 1:] / cnt - c * c, 0.0)
    rms = np.sqrt(var[:, 0::2] + var[:, 1::2])               # [B, 2]: first image, second image
    pos = rms > 0
    sc = np.where(pos, np.sqrt(2.0) / np.where(pos, rms, 1.0), 1.0)
    T = np.zeros((B, 2, 3, 3))
    T[:, :, 0, 0] = T[:, :, 1, 1] = sc
    T[:, :, 0, 2] = -sc * c[:, 0::2]
    T[:, :, 1, 2] = -sc * c[:, 1::2]
    T[:, :, 2, 2] = 1.0
    prm = np.empty((B, 6))                                   # (sc, cx, cy) of the first image, then of the second
    prm[:, 0::3], prm[:, 1::3], prm[:, 2::3] = sc, c[:, 0::2], c[:, 1::2]
    return T[:, 0], T[:, 1], prm


def _dlt_homography(p):
    """normalised DLT homography of correspondences p [k, 4] (host, k small: DEGENSAC's plane refit) or None"""
    x1, x2 = p[:, 0:2], p[:, 2:4]
    def norm(x):
        c = x.mean(0)
        d = np.sqrt(((x - c) ** 2).sum(1)).mean()
        if not (d > 0):
            return None, None
        sc = np.sqrt(2.0) / d
        T = np.array([[sc, 0, -sc * c[0]], [0, sc, -sc * c[1]], [0, 0, 1.0]])
        return (x - c) * sc, T
    a, T1 = norm(x1)
    b, T2 = norm(x2)
    if a is None or b is None:
        return None
    z = np.zeros(len(p))
    o = np.ones(len(p))
    r1 = np.stack([a[:, 0], a[:, 1], o, z, z, z, -b[:, 0] * a[:, 0], -b[:, 0] * a[:, 1], -b[:, 0]], axis=1)
    r2 = np.stack([z, z, z, a[:, 0], a[:, 1], o, -b[:, 1] * a[:, 0], -b[:, 1] * a[:, 1], -b[:, 1]], axis=1)
    A = np.vstack([r1, r2])
    try:
        h = np.linalg.svd(A)[2][-1].reshape(3, 3)
        H = np.linalg.inv(T2) @ h @ T1
    except np.linalg.LinAlgError:
        return None
    return H if np.isfinite(H).all() else None


class HomographyEstimator(Estimator):
    model_type = _lib.HOMOGRAPHY
    sample_size = 4
    nonminimal_sample_size = 4
    rows_per_model = 3
    device_minimal = True      # pgx_solve_minimal: 8x8 Gaussian elimination per sample on the GPU

    def minimal(self, pts, samples):
        largest = float(np.abs(pts).max())
        scale = max(1.0, largest)                      # isotropic pre-scaling: coordinates O(1) for the 8x8 solve
        p = pts[samples] / scale                       # [S,4,4]
        r1, r2 = _dlt_rows(p[..., 0], p[..., 1], p[..., 2], p[..., 3])
        A = np.concatenate([r1, r2], axis=1)           # [S,8,9]
        lhs, rhs = A[:, :, :8], -A[:, :, 8]
        # the determinant of a regular sample scales with the eighth power of the coordinates (four columns linear, two quadratic in
        # them), so for a point set below 1 - where the pre-scaling does nothing - the threshold follows it (a set that reaches 1: unchanged)
        ok = np.abs(np.linalg.det(lhs)) > 1e-14 * min(1.0, largest) ** 8
        h = np.zeros((len(samples), 9))
        if ok.any():
            h[ok, :8] = np.linalg.solve(lhs[ok], rhs[ok][..., None])[..., 0]
            h[ok, 8] = 1.0
            # undo the scaling: H = S^-1 Hn S with S = diag(1/scale, 1/scale, 1)
            h[ok, 2] *= scale
            h[ok, 5] *= scale
            h[ok, 6] /= scale
            h[ok, 7] /= scale
        ok &= np.isfinite(h).all(axis=1)
        return h[ok], np.nonzero(ok)[0]

    def _fit_many(self, gram, B, inits):
        """Normalised DLT: two Gram requests (the moments for the normalisation, then the normalised DLT rows), stacked eigh /
        inv (numpy runs LAPACK per matrix, so an item's model does not depend on its neighbours)."""
        out = [[] for _ in range(B)]
        G, cnt, _ = gram(_lib.GRAM_AFFINE, None, False, 2, np.arange(B))
        rows = np.nonzero((cnt >= 4) & np.isfinite(G).all(axis=(1, 2)))[0]
        if rows.size == 0:
            return out
        T1, T2, prm = _hartley_batch(G[rows], cnt[rows])
        AtA, _, _ = gram(_lib.GRAM_DLT_H, prm, True, 2, rows)
        fin = np.isfinite(AtA).all(axis=(1, 2)) & np.isfinite(T2).all(axis=(1, 2))
        if not fin.any():
            return out
        sel = np.nonzero(fin)[0]
        Hn = self._smallest(AtA[sel]).reshape(-1, 3, 3)
        H = np.linalg.inv(T2[sel]) @ Hn @ T1[sel]
        for k, r in enumerate(sel):
            Hb = H[k]
            if np.isfinite(Hb).all() and abs(Hb[2, 2]) >= 1e-300:
                out[rows[r]] = [(Hb / Hb[2, 2]).reshape(-1)]
        return out


class SymmetricHomographyEstimator(HomographyEstimator):
    """Same solvers; the model carried to the kernels is [H | H^-1] (symmetric transfer error switch)."""
    model_type = _lib.HOMOGRAPHY_SYM
    device_minimal = False     # 18-parameter models: generated on the host

    @staticmethod
    def _augment(models):
        out = []
        keep = []
        for k, h in enumerate(models):
            H = h.reshape(3, 3)
            if abs(np.linalg.det(H)) < 1e-300:
                continue
            out.append(np.concatenate([h, np.linalg.inv(H).reshape(-1)]))
            keep.append(k)
        return (np.array(out).reshape(-1, 18), np.array(keep, dtype=np.int64))

    def minimal(self, pts, samples):
        models, src = super().minimal(pts, samples)
        aug, keep = self._augment(models)
        return aug, src[keep]

    def _fit_many(self, gram, B, inits):
        return [[m for m in self._augment(np.array(res).reshape(-1, 9))[0]] for res in super()._fit_many(gram, B, inits)]

    def output(self, model):
        return np.asarray(model[:9], dtype=np.float64).reshape(3, 3)


# ---------------------------------------------------------------------------------------------------------------------
# fundamental matrix (DefaultFundamentalMatrixEstimator, progressivex_python.cpp:616)  [UPSTREAM-MEMORY]
# 7-point minimal (up to 3 solutions), normalised 8-point non-minimal
# ---------------------------------------------------------------------------------------------------------------------
class FundamentalEstimator(Estimator):
    model_type = _lib.FUNDAMENTAL
    sample_size = 7
    nonminimal_sample_size = 8
    rows_per_model = 3
    device_minimal = True      # pgx_solve_minimal: Gauss-Jordan null space + cubic by bisection, three slots per sample
    device_slots = 3

    @staticmethod
    def _rows(p):
        x1, y1, x2, y2 = p[..., 0], p[..., 1], p[..., 2], p[..., 3]
        o = np.ones_like(x1)
        return np.stack([x2 * x1, x2 * y1, x2, y2 * x1, y2 * y1, y2, x1, y1, o], axis=-1)

    def minimal(self, pts, samples):
        p = pts[samples]
        scale = max(1.0, float(np.abs(pts).max()))
        A = self._rows(p / scale)                      # [S,7,9], isotropic pre-scaling for conditioning
        _, sv, vt = np.linalg.svd(A, full_matrices=True)
        F1, F2 = vt[:, 7].reshape(-1, 3, 3), vt[:, 8].reshape(-1, 3, 3)
        # det(l F1 + (1-l) F2) is a cubic in l: interpolate it at 4 nodes
        ls = np.array([0.0, 1.0, -1.0, 2.0])
        vals = np.stack([np.linalg.det(l * F1 + (1 - l) * F2) for l in ls], axis=1)
        V = np.vander(ls, 4)
        coef = np.linalg.solve(V, vals.T).T            # [S,4] highest power first
        D = np.diag([1 / scale, 1 / scale, 1.0])
        # roots of all cubics at once: eigenvalues of the stacked companion matrices (np.roots does the same one by
        # one); samples with a vanishing leading coefficient (a quadratic) take the slow path
        # a rank-deficient sample (a repeated point, seven points of one plane) has no two-dimensional null space to take a pencil
        # from: no model, as the device's 1e-12 pivot test answers (the last two right singular vectors alone would give arbitrary ones)
        finite = np.isfinite(coef).all(axis=1) & (sv[:, 6] >= 1e-12)
        lead = np.abs(coef[:, 0]) > 1e-14 * np.abs(coef).max(axis=1)
        reg = np.nonzero(finite & lead)[0]
        sidx, roots = [], []
        if len(reg):
            comp = np.zeros((len(reg), 3, 3))
            comp[:, 0, :] = -coef[reg, 1:] / coef[reg, :1]
            comp[:, 1, 0] = 1.0
            comp[:, 2, 1] = 1.0
            ev = np.linalg.eigvals(comp)                                   # [R,3]
            real = np.abs(ev.imag) <= 1e-9 * np.maximum(1.0, np.abs(ev.real))
            rr, cc = np.nonzero(real)
            sidx.append(reg[rr])
            roots.append(ev.real[rr, cc])
        for s in np.nonzero(finite & ~lead)[0]:
            for r in np.roots(coef[s, 1:]):
                if abs(r.imag) <= 1e-9 * max(1.0, abs(r.real)):
                    sidx.append(np.array([s]))
                    roots.append(np.array([r.real]))
        if not sidx:
            return np.zeros((0, 9)), np.zeros(0, dtype=np.int64)
        sidx, roots = np.concatenate(sidx), np.concatenate(roots)
        o = np.argsort(sidx, kind="stable")                                # by sample; roots keep LAPACK's order (as np.roots)
        sidx, roots = sidx[o], roots[o]
        F = D @ (roots[:, None, None] * F1[sidx] + (1.0 - roots)[:, None, None] * F2[sidx]) @ D
        nrm = np.sqrt((F * F).sum(axis=(1, 2)))
        ok = (nrm > 0) & np.isfinite(nrm)
        models = (F[ok] / nrm[ok][:, None, None]).reshape(-1, 9)
        return models, sidx[ok].astype(np.int64)

    # -- validity [U-14] ------------------------------------------------------------------------------------------------------
    # DefaultFundamentalMatrixEstimator (progressivex_python.cpp:616) = gcransac's FundamentalMatrixEstimator, whose source is
    # absent from the snapshot.  Restated from the literature the upstream comments cite [UPSTREAM-MEMORY]:
    #   "oriented"  Chum, Werner, Matas, "Epipolar geometry estimation via RANSAC benefits from the oriented epipolar
    #               constraint" (ICPR 2004): e' x x' and F x must point the same way for every correspondence of the
    #               minimal sample - a hypothesis whose sample disagrees is dropped before it is scored;
    #   "symmetric" every so-far-best F must keep at least max(7, ratio * |inliers|) of its Sampson inliers (r^2 < T^2, the
    #               scorer's threshold) when they are tested with the SYMMETRIC EPIPOLAR distance d(x', F x)^2 + d(x, F^T x')^2
    #               - the Sampson distance stays small next to a degenerate (near rank-one) F's pseudo-epipoles, where one of
    #               the two point-line distances explodes; ratio = 0.5 upstream.  The symmetric distance is 4 x the Sampson
    #               distance when both gradients are equal, so it is compared with 4 T^2: against threshold^2 (what the
    #               recollection of upstream says) the CLEAN ground-truth models of the bundled cubetoy scene keep only
    #               48-60 % of their inliers and are rejected (docs/experiments-cubetoy.md);
    #   "degensac"  Chum, Werner, Matas, "Two-view geometry estimation unaffected by a dominant plane" (CVPR 2005): if five of
    #               the seven sample points agree with a homography H compatible with F, F is H-degenerate: H is re-estimated
    #               on its inliers, epipoles are drawn from pairs of off-plane correspondences (plane and parallax:
    #               e' = (x1' x H x1) x (x2' x H x2), F = [e']x H) and the best-scoring F replaces the model.
    # validity = "off" | "oriented" | "symmetric" (oriented + symmetric) | "full" (all three).  Default "off": nothing of these
    # stages can be checked against the snapshot, and on the three bundled AdelaideRMF scenes plus C3 no setting measures better
    # than none (docs/experiments-cubetoy.md section 1, round-4 rows) - a recollection does not get to change default results.
    validity = "off"
    minimum_inlier_ratio_in_validity_check = 0.5
    homography_threshold = 2.0

    @staticmethod
    def _hom(p):
        o = np.ones(p.shape[:-1] + (1,))
        return np.concatenate([p[..., 0:2], o], axis=-1), np.concatenate([p[..., 2:4], o], axis=-1)

    def valid_samples(self, pts, samples, models, src):
        ok = np.isfinite(models).all(axis=1)
        if self.validity == "off" or not ok.any():
            return ok
        idx = np.nonzero(ok)[0]
        F = models[idx].reshape(-1, 3, 3)
        x1, x2 = self._hom(pts[np.asarray(samples)[src[idx]]])                 # [H, 7, 3] each
        e2 = np.linalg.svd(F)[0][:, :, 2]                                       # left null vector: e2^T F = 0
        l = np.einsum("hij,hkj->hki", F, x1)                                    # F x1
        m = np.cross(e2[:, None, :], x2)                                        # e2 x x2
        sg = np.sign((l * m).sum(-1))
        good = (sg > 0).all(axis=1) | (sg < 0).all(axis=1)
        ok[idx[~good]] = False
        return ok

    @staticmethod
    def _sampson_and_symmetric(F, pts):
        x1, x2 = FundamentalEstimator._hom(pts)
        l2 = x1 @ F.T                                                           # F x1: lines in image 2
        l1 = x2 @ F                                                             # F^T x2: lines in image 1
        r = (x2 * l2).sum(-1)
        a = l2[:, 0] ** 2 + l2[:, 1] ** 2
        b = l1[:, 0] ** 2 + l1[:, 1] ** 2
        with np.errstate(divide="ignore", invalid="ignore"):
            return r * r / (a + b), r * r * (1.0 / a + 1.0 / b)

    def _h_from_f(self, F, e2, x1, x2):
        """H compatible with F through three correspondences (Hartley & Zisserman, result 13.6): H = A - e2 (M^-1 b)^T,
        A = [e2]x F, M = rows x1_i, b_i = (x2_i x A x1_i) . (x2_i x e2) / |x2_i x e2|^2."""
        ex = np.array([[0.0, -e2[2], e2[1]], [e2[2], 0.0, -e2[0]], [-e2[1], e2[0], 0.0]])
        A = ex @ F
        c1 = np.cross(x2, (A @ x1.T).T)
        c2 = np.cross(x2, e2[None, :])
        den = (c2 * c2).sum(-1)
        if not np.all(den > 0):
            return None
        b = (c1 * c2).sum(-1) / den
        try:
            return A - np.outer(e2, np.linalg.solve(x1, b))
        except np.linalg.LinAlgError:
            return None

    @staticmethod
    def _transfer2(H, x1, x2):
        y = x1 @ H.T
        with np.errstate(divide="ignore", invalid="ignore"):
            d = (y[:, 0] / y[:, 2] - x2[:, 0]) ** 2 + (y[:, 1] / y[:, 2] - x2[:, 1]) ** 2
        return np.where(np.isfinite(d), d, np.inf)

    def valid_best(self, ctx, pts, model, sample, threshold, rescore):
        if self.validity in ("off", "oriented"):
            return True, model
        F = np.asarray(model, dtype=np.float64).reshape(3, 3)
        T2 = 2.25 * threshold * threshold
        inliers, supported = ctx.epipolar_support(F, T2, 4.0 * T2)           # one pass over all points on the device
        need = max(self.sample_size, int(inliers * self.minimum_inlier_ratio_in_validity_check))
        if supported < need:
            return False, model
        if self.validity != "full" or sample is None:
            return True, model
        # ---- DEGENSAC: is the sample H-degenerate?
        x1, x2 = self._hom(pts[np.asarray(sample)])
        e2 = np.linalg.svd(F)[0][:, 2]
        h2 = self.homography_threshold ** 2
        H = None
        for tri in ((0, 1, 2), (3, 4, 5), (0, 1, 6), (3, 4, 6), (2, 5, 6)):
            cand = self._h_from_f(F, e2, x1[list(tri)], x2[list(tri)])
            if cand is not None and np.isfinite(cand).all() and int((self._transfer2(cand, x1, x2) < h2).sum()) >= 5:
                H = cand
                break
        if H is None:
            return True, model
        # the plane: inliers of H among all correspondences, H refitted on them (normalised DLT)
        a1, a2 = self._hom(pts)
        on = self._transfer2(H, a1, a2) < h2
        if int(on.sum()) >= 4:
            Hr = _dlt_homography(pts[on])
            if Hr is not None and int((self._transfer2(Hr, a1, a2) < h2).sum()) >= int(on.sum()):
                H = Hr
                on = self._transfer2(H, a1, a2) < h2
        off = np.nonzero(~on)[0]
        if len(off) < 2:
            return True, model
        # plane and parallax: epipoles from pairs of off-plane correspondences
        rng = np.random.default_rng(int(on.sum()) * 7919 + len(off))            # deterministic in the data (no stream consumed)
        trials = min(100, len(off) * (len(off) - 1) // 2)
        pa = rng.integers(0, len(off), trials)
        pb = (pa + 1 + rng.integers(0, len(off) - 1, trials)) % len(off)
        la = np.cross(a2[off[pa]], (a1[off[pa]] @ H.T))
        lb = np.cross(a2[off[pb]], (a1[off[pb]] @ H.T))
        e = np.cross(la, lb)
        nrm = np.linalg.norm(e, axis=1)
        e = e[nrm > 0] / nrm[nrm > 0][:, None]
        if len(e) == 0:
            return True, model
        ex = np.zeros((len(e), 3, 3))
        ex[:, 0, 1], ex[:, 0, 2], ex[:, 1, 0], ex[:, 1, 2], ex[:, 2, 0], ex[:, 2, 1] = -e[:, 2], e[:, 1], e[:, 2], -e[:, 0], -e[:, 1], e[:, 0]
        cands = ex @ H
        cn = np.linalg.norm(cands.reshape(len(e), -1), axis=1)
        cands = (cands[cn > 0] / cn[cn > 0][:, None, None]).reshape(-1, 9)
        if len(cands) == 0:
            return True, model
        sc = np.asarray(rescore(np.vstack([np.asarray(model, dtype=np.float64)[None, :], cands])), dtype=np.float64)
        k = int(np.argmax(sc[1:])) + 1
        if np.isfinite(sc[k]) and sc[k] > sc[0]:
            return True, cands[k - 1].copy()
        return True, model

    def _fit_many(self, gram, B, inits):
        """Normalised 8-point: two Gram requests (the moments for the normalisation, then the normalised epipolar rows), stacked
        eigh / svd for the rank-2 projection - LAPACK per matrix, so an item's model does not depend on its neighbours (a
        local-optimisation round refits 50 samples, a PEARL iteration every instance: 5 200 single eigh + svd calls were a third
        of findTwoViewMotions' proposal time at C3)."""
        out = [[] for _ in range(B)]
        G, cnt, _ = gram(_lib.GRAM_AFFINE, None, False, 2, np.arange(B))
        rows = np.nonzero((cnt >= 8) & np.isfinite(G).all(axis=(1, 2)))[0]
        if rows.size == 0:
            return out
        T1, T2, prm = _hartley_batch(G[rows], cnt[rows])
        AtA, _, _ = gram(_lib.GRAM_EPI_F, prm, True, 2, rows)
        sel = np.nonzero(np.isfinite(AtA).all(axis=(1, 2)))[0]
        if sel.size == 0:
            return out
        F = self._smallest(AtA[sel]).reshape(-1, 3, 3)
        okf = np.isfinite(F).all(axis=(1, 2))
        sel, F = sel[okf], F[okf]
        if sel.size == 0:
            return out
        u, sv, v = np.linalg.svd(F)
        D = np.zeros_like(F)
        D[:, 0, 0], D[:, 1, 1] = sv[:, 0], sv[:, 1]
        F = u @ D @ v
        F = T2[sel].transpose(0, 2, 1) @ F @ T1[sel]
        for k, r in enumerate(sel):
            nrm = np.linalg.norm(F[k])
            if np.isfinite(nrm) and nrm != 0:
                out[rows[r]] = [(F[k] / nrm).reshape(-1)]
        return out


# ---------------------------------------------------------------------------------------------------------------------
# PnP (DefaultPnPEstimator, progressivex_python.cpp:119)  [UPSTREAM-MEMORY]: P3P minimal (Grunert's quartic + Horn
# alignment, up to 4 solutions), Gauss-Newton reprojection refinement as the non-minimal fit
# ---------------------------------------------------------------------------------------------------------------------
def _kabsch(A, B):
    """Batched rigid alignment B ~ R A + t for [S,3,3] point triples (rows = points)."""
    ca, cb = A.mean(axis=1, keepdims=True), B.mean(axis=1, keepdims=True)
    H = np.einsum("sij,sik->sjk", A - ca, B - cb)
    U, _, Vt = np.linalg.svd(H)
    d = np.sign(np.linalg.det(np.einsum("sij,sjk->sik", Vt.transpose(0, 2, 1), U.transpose(0, 2, 1))))
    Dm = np.zeros_like(H)
    Dm[:, 0, 0] = 1
    Dm[:, 1, 1] = 1
    Dm[:, 2, 2] = d
    R = Vt.transpose(0, 2, 1) @ Dm @ U.transpose(0, 2, 1)
    t = cb[:, 0] - np.einsum("sij,sj->si", R, ca[:, 0])
    return R, t


class PnPEstimator(Estimator):
    model_type = _lib.PNP
    sample_size = 3
    nonminimal_sample_size = 6
    rows_per_model = 3
    cols = 4
    device_minimal = True      # pgx_solve_minimal: Grunert's quartic by bisection, pose from the triangle frames; 4 slots
    device_slots = 4

    def minimal(self, pts, samples):
        p = pts[samples]                                     # [S,3,5]
        f = np.concatenate([p[..., :2], np.ones(p.shape[:2] + (1,))], axis=-1)
        f = f / np.linalg.norm(f, axis=-1, keepdims=True)    # unit bearings
        X = p[..., 2:]
        a = np.linalg.norm(X[:, 1] - X[:, 2], axis=1)
        b = np.linalg.norm(X[:, 0] - X[:, 2], axis=1)
        c = np.linalg.norm(X[:, 0] - X[:, 1], axis=1)
        ca = (f[:, 1] * f[:, 2]).sum(axis=1)
        cb = (f[:, 0] * f[:, 2]).sum(axis=1)
        cg = (f[:, 0] * f[:, 1]).sum(axis=1)
        ok = (a > 0) & (b > 0) & (c > 0)
        with np.errstate(all="ignore"):
            a2, b2, c2 = a * a, b * b, c * c
            q = (a2 - c2) / b2
            r = (a2 + c2) / b2
            # Grunert / Fischler-Bolles quartic in v = s3 / s1
            A4 = (q - 1) ** 2 - 4 * c2 / b2 * ca ** 2
            A3 = 4 * (q * (1 - q) * cb - (1 - r) * ca * cg + 2 * c2 / b2 * ca ** 2 * cb)
            A2 = 2 * (q ** 2 - 1 + 2 * q ** 2 * cb ** 2 + 2 * (b2 - c2) / b2 * ca ** 2
                      - 4 * r * ca * cb * cg + 2 * (b2 - a2) / b2 * cg ** 2)
            A1 = 4 * (-q * (1 + q) * cb + 2 * a2 / b2 * cg ** 2 * cb - (1 - r) * ca * cg)
            A0 = (1 + q) ** 2 - 4 * a2 / b2 * cg ** 2
        coef = np.stack([A4, A3, A2, A1, A0], axis=1)
        ok &= np.isfinite(coef).all(axis=1) & (np.abs(A4) > 1e-14)
        S = len(samples)
        comp = np.zeros((S, 4, 4))
        comp[:, 1, 0] = comp[:, 2, 1] = comp[:, 3, 2] = 1.0
        safeA4 = np.where(ok, A4, 1.0)
        comp[:, 0, 3] = -A0 / safeA4
        comp[:, 1, 3] = -A1 / safeA4
        comp[:, 2, 3] = -A2 / safeA4
        comp[:, 3, 3] = -A3 / safeA4
        comp[~ok] = 0
        roots = np.linalg.eigvals(comp)                      # [S,4]
        models, src = [], []
        for k in range(4):
            v = roots[:, k]
            real = ok & (np.abs(v.imag) < 1e-8 * np.maximum(1.0, np.abs(v.real))) & (v.real > 0)
            if not real.any():
                continue
            sidx = np.nonzero(real)[0]
            vv = v.real[sidx]
            qq, cga, cba, caa = q[sidx], cg[sidx], cb[sidx], ca[sidx]
            a2s, b2s, c2s = a2[sidx], b2[sidx], c2[sidx]
            with np.errstate(all="ignore"):
                u = ((-1 + qq) * vv * vv - 2 * qq * cba * vv + 1 + qq) / (2 * (cga - vv * caa))
                s1 = np.sqrt(b2s / (1 + vv * vv - 2 * vv * cba))
            s3 = vv * s1

            def gates(u):
                # positive finite depths and consistency with the two unused side constraints -> (passes, |e2|)
                with np.errstate(all="ignore"):
                    s2 = u * s1
                    e1 = s1 ** 2 + s2 ** 2 - 2 * s1 * s2 * cga - c2s
                    e2 = s2 ** 2 + s3 ** 2 - 2 * s2 * s3 * caa - a2s
                    ok = np.isfinite(s1) & np.isfinite(s2) & (s1 > 0) & (s2 > 0) & (s3 > 0)
                    return ok & (np.abs(e1) < 1e-6 * c2s) & (np.abs(e2) < 1e-6 * a2s), np.abs(e2)

            good, _ = gates(u)
            if not good.all():
                # the second way to u where the linear one fails its gates (0 / 0 when two poses share v, solve.hip solve_p3p):
                # u^2 - 2 cg u + 1 - c2 / s1^2 = 0, of its roots through the gates the one with the smaller |e2|
                with np.errstate(all="ignore"):
                    disc = cga * cga - 1 + c2s / (s1 * s1)
                    sq = np.sqrt(np.where(disc >= 0, disc, np.nan))
                oka, ea = gates(cga - sq)
                okb, eb = gates(cga + sq)
                second = okb & (~oka | (eb < ea))
                u = np.where(good, u, np.where(second, cga + sq, cga - sq))
                good = good | oka | okb
            if not good.any():
                continue
            sidx = sidx[good]
            s2 = u * s1
            depth = np.stack([s1[good], s2[good], s3[good]], axis=1)
            Y = f[sidx] * depth[..., None]                    # camera-frame points
            R, t = _kabsch(X[sidx], Y)
            P = np.concatenate([R, t[..., None]], axis=2).reshape(-1, 12)
            fin = np.isfinite(P).all(axis=1)
            models.append(P[fin])
            src.append(sidx[fin])
        if not models:
            return np.zeros((0, 12)), np.zeros(0, dtype=np.int64)
        models, src = np.vstack(models), np.concatenate(src)
        o = np.argsort(src, kind="stable")
        return models[o], src[o]

    def nonminimal(self, ctx, sel, weights=None, init=None):
        """Gauss-Newton on the reprojection error from `init` (PEARL and the local optimisation always have one; the
        DLT start of an un-initialised fit is not needed on this path).  Per iteration the device accumulates the
        normal equations  sum (J,r)^T (J,r)  (rows in fit.hip GenPnpGn, one pgx_gram call), the 6x6 solve and the pose update
        run here."""
        # The one refit with two statements.  This single-item one solves with lstsq and the vector forms of norm; `_fit_many`
        # (labels, batches) solves with pinv on stacks.  The two agree to rounding only (the tests say 1e-9), and the local
        # optimisation runs this one on the product path, so its bits stay: folding it into `_fit_many` would change results.
        if init is None:
            return []
        P = np.asarray(init, dtype=np.float64).reshape(3, 4).copy()
        R, t = P[:, :3], P[:, 3]
        for _ in range(10):
            G, cnt, bad = ctx.gram(_lib.GRAM_PNP_GN, sel, params=np.column_stack([R, t]).reshape(-1), weights=weights, wpow=2)
            if cnt < 4 or bad > 0:
                return []
            try:
                delta = np.linalg.lstsq(G[:6, :6], -G[:6, 6], rcond=None)[0]
            except np.linalg.LinAlgError:
                return []
            om = delta[:3]
            ang = np.linalg.norm(om)
            if ang > 0:                                       # R <- exp([omega]_x) R ; t <- t + dt
                k = om / ang
                Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
                R = (np.eye(3) + np.sin(ang) * Kx + (1 - np.cos(ang)) * (Kx @ Kx)) @ R
            t = t + delta[3:]
            if np.linalg.norm(delta) < 1e-12:
                break
        out = np.column_stack([R, t])
        return [out.reshape(-1)] if np.isfinite(out).all() else []

    def nonminimal_batch(self, ctx, index, weights=None, init=None):
        """The local optimisation's B refits from one start: ONE pgx_pnp_refine_batch launch that runs all Gauss-Newton steps
        on the device when the context offers it (the GPU context); otherwise - the CPU oracle context of the tests - the
        stacked iteration of `_fit_many`, whose iterates the kernel reproduces up to rounding."""
        refine = getattr(ctx, "pnp_refine_batch", None)
        if refine is None or init is None:
            return super().nonminimal_batch(ctx, index, weights, init)
        index = np.asarray(index)
        B = index.shape[0]
        start = np.tile(np.asarray(init, dtype=np.float64).reshape(1, 12), (B, 1))
        P, ok = refine(start, index, weights=weights, wpow=2, iterations=10)
        return [[P[b]] if ok[b] else [] for b in range(B)]

    def _fit_many(self, gram, B, inits, iterations=10):
        """The Gauss-Newton iteration of `nonminimal` for B items at once (the loop is _gauss_newton's), with the 6x6 solves, the rotation
        updates and the convergence tests done on [B, ...] arrays - 50 refits x 10 iterations per graph-cut round were 13 us of lstsq + 15 us
        of small-array numpy each, a third of C4's proposal time.  The solve is the pseudo-inverse with lstsq's cut-off
        (singular values below eps * 6 * s_max dropped), so an item's iterates are those of `nonminimal` up to rounding."""
        have = np.array([ini is not None for ini in inits], dtype=bool)
        R = np.zeros((B, 3, 3))
        t = np.zeros((B, 3))
        for b in np.nonzero(have)[0]:
            P0 = np.asarray(inits[b], dtype=np.float64).reshape(3, 4)
            R[b], t[b] = P0[:, :3], P0[:, 3]
        eye = np.eye(3)

        def params(act):
            return np.concatenate([R[act], t[act][:, :, None]], axis=2).reshape(act.size, 12)

        def update(act, delta, prm):
            om = delta[:, :3]
            ang = np.linalg.norm(om, axis=1)
            k = om / np.where(ang > 0, ang, 1.0)[:, None]
            Kx = np.zeros((act.size, 3, 3))
            Kx[:, 0, 1], Kx[:, 0, 2] = -k[:, 2], k[:, 1]
            Kx[:, 1, 0], Kx[:, 1, 2] = k[:, 2], -k[:, 0]
            Kx[:, 2, 0], Kx[:, 2, 1] = -k[:, 1], k[:, 0]
            rot = eye + np.sin(ang)[:, None, None] * Kx + (1 - np.cos(ang))[:, None, None] * (Kx @ Kx)
            rot[ang == 0] = eye                   # R <- exp([omega]_x) R ; t <- t + dt
            Rn, tn = rot @ R[act], t[act] + delta[:, 3:]
            R[act], t[act] = Rn, tn
            return np.isfinite(Rn).all(axis=(1, 2)) & np.isfinite(tn).all(axis=1)
        # a start that is not finite is sent like any other: its sums fail it
        failed = _gauss_newton(gram, _lib.GRAM_PNP_GN, wpow=2, npar=6, min_count=4, cutoff=6, failed=~have, params=params, update=update,
                               iterations=iterations)
        P = np.concatenate([R, t[:, :, None]], axis=2).reshape(B, 12)
        good = ~failed & np.isfinite(P).all(axis=1)
        return [[P[b]] if good[b] else [] for b in range(B)]


ESTIMATORS = {
    "line": LineEstimator,
    "plane": PlaneEstimator,
    "sphere": SphereEstimator,
    "circle": CircleEstimator,
    "line3d": Line3DEstimator,
    "cylinder": CylinderEstimator,
    "cone": ConeEstimator,
    "torus": TorusEstimator,
    "primitive": PrimitiveEstimator,
    "oriented_primitive": OrientedPrimitiveEstimator,
    "vanishing_point": VanishingPointEstimator,
    "homography": HomographyEstimator,
    "homography_sym": SymmetricHomographyEstimator,
    "fundamental": FundamentalEstimator,
    "pnp": PnPEstimator,
}
