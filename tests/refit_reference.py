"""The single-item statements of the least-squares refits as pyprogressivex/_estimators.py held them before its stacked
`_fit_many` became the only one: the readable scalar form, one generator per estimator that yields Gram requests
(kind, params, use_weights, wpow) and receives (G, count, bad), and the driver that feeds one from a context's `gram`.
TEST INFRASTRUCTURE: tests/test_refit_statements_cpu.py holds the product to these bodies, byte for byte, on the LAPACK of the
machine the test runs on.  `self` is the product's estimator (its `_smallest`, `_normal`, `refit_solver`, `radius_range`, `_augment`).  PnP is
not among them: its single-item statement is still the product's own `PnPEstimator.nonminimal`.  Below them, the four stacked
Gauss-Newton refits (cylinder, cone, torus, PnP) as each held its own copy of the loop."""
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


# ---- the four Gauss-Newton refits as _estimators.py held them, each with its own copy of the loop, before _gauss_newton owned it ------
# The bodies of CylinderEstimator / ConeEstimator / TorusEstimator / PnPEstimator._fit_many, verbatim, as functions of
# (self, gram, B, inits); tests/test_refit_statements_cpu.py holds the product to them: the same bytes, the same requests.
_cylinder_frame = _estimators._cylinder_frame


def cylinder_fit_many(self, gram, B, inits, iterations=10):
    out = [[] for _ in range(B)]
    have = np.array([ini is not None for ini in inits], dtype=bool)
    if not have.any():
        return out
    m = np.zeros((B, 7))
    m[:, 5] = 1.0
    for b in np.nonzero(have)[0]:
        m[b] = np.asarray(inits[b], dtype=np.float64).reshape(7)
    with np.errstate(all="ignore"):
        m[:, 3:6] /= np.linalg.norm(m[:, 3:6], axis=1)[:, None]
    failed = ~have | ~np.isfinite(m).all(axis=1)
    running = ~failed
    for _ in range(iterations):
        act = np.nonzero(running)[0]
        if act.size == 0:
            break
        u = _cylinder_frame(m[act, 3:6])
        G, cnt, bad = gram(_lib.GRAM_CYL_GN, np.column_stack([m[act], u]), True, 1, act)
        A, rhs = G[:, :5, :5], -G[:, :5, 5]
        ok = (np.asarray(bad) == 0) & (np.asarray(cnt) >= 5) & np.isfinite(A).all(axis=(1, 2)) & np.isfinite(rhs).all(axis=1)
        failed[act[~ok]] = True
        running[act[~ok]] = False
        if not ok.any():
            break
        act, A, rhs, u = act[ok], A[ok], rhs[ok], u[ok]
        d = m[act, 3:6]
        v = np.cross(d, u)
        delta = np.einsum("bij,bj->bi", np.linalg.pinv(A, rcond=6 * np.finfo(np.float64).eps), rhs)
        m[act, 0:3] += delta[:, 0:1] * u + delta[:, 1:2] * v
        d = d + delta[:, 2:3] * u + delta[:, 3:4] * v
        m[act, 3:6] = d / np.linalg.norm(d, axis=1)[:, None]
        m[act, 6] += delta[:, 4]
        fin = np.isfinite(m[act]).all(axis=1)
        failed[act[~fin]] = True
        running[act[~fin]] = False
        running[act[np.linalg.norm(delta, axis=1) < 1e-12]] = False
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


def cone_fit_many(self, gram, B, inits, iterations=10):
    out = [[] for _ in range(B)]
    have = np.array([ini is not None for ini in inits], dtype=bool)
    if not have.any():
        return out
    m = np.zeros((B, 8))
    m[:, 5] = m[:, 6] = 1.0
    for b in np.nonzero(have)[0]:
        m[b] = np.asarray(inits[b], dtype=np.float64).reshape(8)
    with np.errstate(all="ignore"):
        m[:, 3:6] /= np.linalg.norm(m[:, 3:6], axis=1)[:, None]
        m[:, 6:8] /= np.linalg.norm(m[:, 6:8], axis=1)[:, None]
    failed = ~have | ~np.isfinite(m).all(axis=1)
    running = ~failed
    for _ in range(iterations):
        act = np.nonzero(running)[0]
        if act.size == 0:
            break
        u = _cylinder_frame(m[act, 3:6])
        G, cnt, bad = gram(_lib.GRAM_CONE_GN, np.column_stack([m[act], u]), True, 1, act)
        A, rhs = G[:, :6, :6], -G[:, :6, 6]
        ok = (np.asarray(bad) == 0) & (np.asarray(cnt) >= 6) & np.isfinite(A).all(axis=(1, 2)) & np.isfinite(rhs).all(axis=1)
        failed[act[~ok]] = True
        running[act[~ok]] = False
        if not ok.any():
            break
        act, A, rhs, u = act[ok], A[ok], rhs[ok], u[ok]
        d = m[act, 3:6]
        v = np.cross(d, u)
        step = np.einsum("bij,bj->bi", np.linalg.pinv(A, rcond=6 * np.finfo(np.float64).eps), rhs)
        m[act, 0:3] += step[:, 0:1] * u + step[:, 1:2] * v + step[:, 2:3] * d
        d = d + step[:, 3:4] * u + step[:, 4:5] * v
        m[act, 3:6] = d / np.linalg.norm(d, axis=1)[:, None]
        cs = np.column_stack([m[act, 6] - step[:, 5] * m[act, 7], m[act, 7] + step[:, 5] * m[act, 6]])
        m[act, 6:8] = cs / np.linalg.norm(cs, axis=1)[:, None]
        fin = np.isfinite(m[act]).all(axis=1)
        failed[act[~fin]] = True
        running[act[~fin]] = False
        running[act[np.linalg.norm(step, axis=1) < 1e-12]] = False
    rows = np.nonzero(~failed)[0]
    if rows.size == 0:
        return out
    mc = self.canonical(m[rows])
    for k, b in enumerate(rows):
        model = mc[k]
        if np.isfinite(model).all() and model[6] > 0 and model[7] > 0 and self._in_range(model[7]):
            out[b] = [model]
    return out


def torus_fit_many(self, gram, B, inits, iterations=10):
    out = [[] for _ in range(B)]
    have = np.array([ini is not None for ini in inits], dtype=bool)
    if not have.any():
        return out
    m = np.zeros((B, 8))
    m[:, 5] = 1.0
    m[:, 6], m[:, 7] = 2.0, 1.0
    for b in np.nonzero(have)[0]:
        m[b] = np.asarray(inits[b], dtype=np.float64).reshape(8)
    with np.errstate(all="ignore"):
        m[:, 3:6] /= np.linalg.norm(m[:, 3:6], axis=1)[:, None]
    failed = ~have | ~np.isfinite(m).all(axis=1)
    running = ~failed
    for _ in range(iterations):
        act = np.nonzero(running)[0]
        if act.size == 0:
            break
        u = _cylinder_frame(m[act, 3:6])
        G, cnt, bad = gram(_lib.GRAM_TORUS_GN, np.column_stack([m[act], u]), True, 1, act)
        A, rhs = G[:, :7, :7], -G[:, :7, 7]
        ok = (np.asarray(bad) == 0) & (np.asarray(cnt) >= 7) & np.isfinite(A).all(axis=(1, 2)) & np.isfinite(rhs).all(axis=1)
        failed[act[~ok]] = True
        running[act[~ok]] = False
        if not ok.any():
            break
        act, A, rhs, u = act[ok], A[ok], rhs[ok], u[ok]
        d = m[act, 3:6]
        v = np.cross(d, u)
        step = np.einsum("bij,bj->bi", np.linalg.pinv(A, rcond=7 * np.finfo(np.float64).eps), rhs)
        m[act, 0:3] += step[:, 0:1] * u + step[:, 1:2] * v + step[:, 2:3] * d
        d = d + step[:, 3:4] * u + step[:, 4:5] * v
        m[act, 3:6] = d / np.linalg.norm(d, axis=1)[:, None]
        m[act, 6] += step[:, 5]
        m[act, 7] += step[:, 6]
        fin = np.isfinite(m[act]).all(axis=1)
        failed[act[~fin]] = True
        running[act[~fin]] = False
        running[act[np.linalg.norm(step, axis=1) < 1e-12]] = False
    for b in np.nonzero(~failed)[0]:
        model = m[b]
        if np.isfinite(model).all() and model[7] > 0 and bool(self._in_range(model[6], model[7])):
            out[b] = [model.copy()]
    return out


def pnp_fit_many(self, gram, B, inits, iterations=10):
    out = [[] for _ in range(B)]
    have = np.array([ini is not None for ini in inits], dtype=bool)
    if not have.any():
        return out
    R = np.zeros((B, 3, 3))
    t = np.zeros((B, 3))
    for b in np.nonzero(have)[0]:
        P0 = np.asarray(inits[b], dtype=np.float64).reshape(3, 4)
        R[b], t[b] = P0[:, :3], P0[:, 3]
    running = have.copy()                   # still iterating
    failed = ~have
    eye = np.eye(3)
    for _ in range(iterations):
        act = np.nonzero(running)[0]
        if act.size == 0:
            break
        prm = np.concatenate([R[act], t[act][:, :, None]], axis=2).reshape(act.size, 12)
        G, cnt, bad = gram(_lib.GRAM_PNP_GN, prm, True, 2, act)
        A, b = G[:, :6, :6], -G[:, :6, 6]
        ok = (bad == 0) & (cnt >= 4) & np.isfinite(A).all(axis=(1, 2)) & np.isfinite(b).all(axis=1)
        failed[act[~ok]] = True
        running[act[~ok]] = False
        if not ok.any():
            break
        act, A, b = act[ok], A[ok], b[ok]
        delta = np.einsum("bij,bj->bi", np.linalg.pinv(A, rcond=6 * np.finfo(np.float64).eps), b)
        om = delta[:, :3]
        ang = np.linalg.norm(om, axis=1)
        k = om / np.where(ang > 0, ang, 1.0)[:, None]
        Kx = np.zeros((act.size, 3, 3))
        Kx[:, 0, 1], Kx[:, 0, 2] = -k[:, 2], k[:, 1]
        Kx[:, 1, 0], Kx[:, 1, 2] = k[:, 2], -k[:, 0]
        Kx[:, 2, 0], Kx[:, 2, 1] = -k[:, 1], k[:, 0]
        rot = eye + np.sin(ang)[:, None, None] * Kx + (1 - np.cos(ang))[:, None, None] * (Kx @ Kx)
        rot[ang == 0] = eye                   # R <- exp([omega]_x) R ; t <- t + dt
        R[act] = rot @ R[act]
        t[act] = t[act] + delta[:, 3:]
        running[act[np.linalg.norm(delta, axis=1) < 1e-12]] = False
    P = np.concatenate([R, t[:, :, None]], axis=2).reshape(B, 12)
    good = ~failed & np.isfinite(P).all(axis=1)
    return [[P[b]] if good[b] else [] for b in range(B)]


FIT_MANY = {
    _estimators.CylinderEstimator: cylinder_fit_many,
    _estimators.ConeEstimator: cone_fit_many,
    _estimators.TorusEstimator: torus_fit_many,
    _estimators.PnPEstimator: pnp_fit_many,
}


def with_reference_fit_many(est):
    """`est` with its class's reference body above as its `_fit_many`, for the entry points that call it (nonminimal_labels,
    nonminimal_batch, PrimitiveEstimator._fit_many's constituents); the estimator is changed in place and returned"""
    body = FIT_MANY[type(est)]
    est._fit_many = lambda gram, B, inits, iterations=10: body(est, gram, B, inits, iterations)
    return est
