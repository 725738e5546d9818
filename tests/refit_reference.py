"""The single-item statements of the least-squares refits as pyprogressivex/_estimators.py held them before its stacked
`_fit_many` became the only one: the readable scalar form, one generator per estimator that yields Gram requests
(kind, params, use_weights, wpow) and receives (G, count, bad), and the driver that feeds one from a context's `gram`.
TEST INFRASTRUCTURE: tests/test_refit_statements_cpu.py holds the product to these bodies, byte for byte, on the LAPACK of the
machine the test runs on.  `self` is the product's estimator (its `_smallest`, `_normal`, `refit_solver`, `radius_range`, `_augment`).  PnP is
not here: its single-item statement is still the product's own `PnPEstimator.nonminimal`."""
import numpy as np

from pyprogressivex import _estimators, _lib


def _hartley_from_moments(G, cnt):
    """Normalising similarities of both images from one pass of first/second moments (the affine Gram matrix G;
    isotropic scaling to an RMS distance of sqrt(2) from the centroid).  Returns (T1, T2, params for the DLT /
    epipolar rows, count)."""
    if cnt < 1:
        return None, None, None, 0
    c = G[0, 1:] / cnt
    var = np.maximum(np.diag(G)[1:] / cnt - c * c, 0.0)
    Ts, prm = [], []
    for k in (0, 2):
        rms = np.sqrt(var[k] + var[k + 1])
        sc = np.sqrt(2.0) / rms if rms > 0 else 1.0
        Ts.append(np.array([[sc, 0, -sc * c[k]], [0, sc, -sc * c[k + 1]], [0, 0, 1.0]]))
        prm += [sc, c[k], c[k + 1]]
    return Ts[0], Ts[1], np.array(prm), cnt


def _smallest_eigenvector(G):
    evals, evecs = np.linalg.eigh(G)
    return evecs[:, 0]


def line_fit(self, init):
    G, cnt, _ = yield (_lib.GRAM_AFFINE, None, True, 1)                    # sum w [1,x,y][1,x,y]^T
    W = G[0, 0]
    if cnt < 2 or not W > 0:
        return []
    mean = G[0, 1:] / W
    evals, evecs = np.linalg.eigh(G[1:, 1:] - W * np.outer(mean, mean))     # weighted scatter about the mean
    nrm = evecs[:, 0]
    return [np.array([nrm[0], nrm[1], -nrm @ mean])]


def plane_fit(self, init):
    G, cnt, _ = yield (_lib.GRAM_AFFINE, None, True, 1)                    # sum w [1,x,y,z][1,x,y,z]^T
    W = G[0, 0]
    if cnt < 3 or not W > 0:
        return []
    mean = G[0, 1:] / W
    scatter = G[1:, 1:] - W * np.outer(mean, mean)                          # weighted scatter about the mean
    if not np.isfinite(scatter).all():
        return []
    nrm = self._normal(scatter[None])[0]
    return [np.array([nrm[0], nrm[1], nrm[2], -nrm @ mean])]


def round_fit(self, init):
    """Algebraic fit in two Gram passes: the weighted mean o and the RMS distance s from it (GRAM_AFFINE), then the smallest
    eigenvector theta of the Gram matrix of the rows (1, q, |q|^2), q = (p - o) / s, the last entry summed left to right
    (GRAM_CIRCLE: u u + v v, GRAM_SPHERE: (u u + v v) + w w): theta[0] + theta[1..DIM] . q + theta[-1] |q|^2 = 0 is the sphere
    |q + b|^2 = |b|^2 - theta[0] / theta[-1] with b = theta[1..DIM] / (2 theta[-1]), so c = o - s b and
    r = s sqrt(|b|^2 - theta[0] / theta[-1]).  The normalisation keeps the small matrix well conditioned for scenes far from
    the origin.  `init` is not used."""
    G, cnt, _ = yield (_lib.GRAM_AFFINE, None, True, 1)                    # sum w [1,p][1,p]^T
    W = G[0, 0]
    if cnt < self.sample_size or not W > 0:
        return []
    o = G[0, 1:] / W
    scatter = G[1:, 1:] - W * np.outer(o, o)
    var = np.trace(scatter) / W
    # the guard: the root is taken of a positive, finite variance only (coincident points: the trace may round to zero or below it,
    # which must give no model and no RuntimeWarning); s > 0 and finite exactly when var is
    if not (np.isfinite(o).all() and var > 0 and np.isfinite(var)):
        return []
    s = np.sqrt(var)
    G, _, _ = yield (self.gram_kind, np.array([*o.tolist(), s]), True, 1)
    if not np.isfinite(G).all():
        return []
    th = self._smallest(G[None])[0]
    A = th[-1]
    if A == 0:
        return []
    b = th[1:-1] / (2.0 * A)
    rad = b @ b - th[0] / A
    if not rad > 0:
        return []
    r = s * np.sqrt(rad)
    c = o - s * b
    if not (np.isfinite(c).all() and np.isfinite(r) and self._in_range(r)):
        return []
    return [np.array([*c.tolist(), r])]


def vanishing_point_fit(self, init):
    # rows A = [y0*mz-my, mx-x0*mz, x0*my-y0*mx] * w (:212-218) are generated and accumulated on the device
    AtA, cnt, _ = yield (_lib.GRAM_VP, None, True, 2)
    if cnt < 2:
        return []
    if self.refit_solver == "jacobi":
        v = self._smallest(AtA[None])[0]
    else:
        evals, evecs = np.linalg.eigh(AtA)                                    # :227 SelfAdjointEigenSolver
        v = evecs[:, int(np.argmin(evals))]                                   # :230-233
    n = np.linalg.norm(v)
    return [v / n] if n > 0 else []


def homography_fit(self, init):
    G, cnt, _ = yield (_lib.GRAM_AFFINE, None, False, 2)
    T1, T2, prm, cnt = _hartley_from_moments(G, cnt)
    if cnt < 4:
        return []
    AtA, _, _ = yield (_lib.GRAM_DLT_H, prm, True, 2)                                  # normalised DLT rows
    Hn = (self._smallest(AtA[None])[0] if self.refit_solver == "jacobi" else _smallest_eigenvector(AtA)).reshape(3, 3)
    H = np.linalg.inv(T2) @ Hn @ T1
    if not np.isfinite(H).all() or abs(H[2, 2]) < 1e-300:
        return []
    return [(H / H[2, 2]).reshape(-1)]


def symmetric_homography_fit(self, init):
    res = yield from homography_fit(self, init)
    return [m for m in self._augment(np.array(res).reshape(-1, 9))[0]]


def fundamental_fit(self, init):
    G, cnt, _ = yield (_lib.GRAM_AFFINE, None, False, 2)
    T1, T2, prm, cnt = _hartley_from_moments(G, cnt)
    if cnt < 8:
        return []
    AtA, _, _ = yield (_lib.GRAM_EPI_F, prm, True, 2)                                  # normalised 8-point rows
    F = (self._smallest(AtA[None])[0] if self.refit_solver == "jacobi" else _smallest_eigenvector(AtA)).reshape(3, 3)
    u, s, v = np.linalg.svd(F)
    F = u @ np.diag([s[0], s[1], 0.0]) @ v
    F = T2.T @ F @ T1
    nrm = np.linalg.norm(F)
    if not np.isfinite(nrm) or nrm == 0:
        return []
    return [(F / nrm).reshape(-1)]


FIT = {
    _estimators.LineEstimator: line_fit,
    _estimators.PlaneEstimator: plane_fit,
    _estimators.SphereEstimator: round_fit,
    _estimators.CircleEstimator: round_fit,
    _estimators.VanishingPointEstimator: vanishing_point_fit,
    _estimators.HomographyEstimator: homography_fit,
    _estimators.SymmetricHomographyEstimator: symmetric_homography_fit,
    _estimators.FundamentalEstimator: fundamental_fit,
}


def nonminimal(est, ctx, sel, weights=None, init=None):
    """one refit of the selection sel = ("index", indices) | ("label", k): one ctx.gram call per request of the generator"""
    est._eig_ctx = ctx
    gen = FIT[type(est)](est, init)
    try:
        req = next(gen)
        while True:
            kind, params, use_w, wpow = req
            req = gen.send(ctx.gram(kind, sel, params=params, weights=weights if use_w else None, wpow=wpow))
    except StopIteration as done:
        return done.value
