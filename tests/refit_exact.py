"""The least-squares refits restated from their definitions at 50 digits: what the product's non-minimal fits are held to.

TEST INFRASTRUCTURE, never imported by the product.  Every fit is written from its objective - minimise
sum_i w_i^p sum_rows (a . theta)^2 over unit theta, p the weight power the product passes to its Gram calls - and not from the
product's route: the design matrix is formed row by row from the points in mpmath, the minimiser is an eigenvector of its 50-digit
A^T A, and no Gram matrix of the product or of the oracle, no call into pgx_oracle and no helper of _estimators.py is used.  Every
fit returns, next to the model, the vector in the normalised space where the eigenproblem is posed, the normalisation, and the
eigenvalues the tolerance is made of (tolerance(): 32 eps lambda_max / (lambda_2 - lambda_1)).

mpmath is imported when a fit is called, not when the module is: tests/golden/make_golden_refits.py runs the fits and writes
tests/golden/kat_refits_v1.npz, and the comparisons (tests/refit_accuracy_cases.py) read that file.  The one statement that runs
at test time is the pose's Gauss-Newton step at a pose the product returned: pnp_terms() and solve6() are written over an abstract
number type, mpmath's mpf in the generator and the standard library's decimal (50 digits) in the tests; pnp_jacobian_check() holds
the analytic Jacobian they use to central differences of the 50-digit projection, which is what makes it independent of the
Jacobian the kernel, the oracle and the host share.
"""
import decimal

import numpy as np

DIGITS = 50
EPS = 2.0 ** -52
FACTOR = 32.0           # Davis-Kahan: 2 x (row products + a summation tree of < 12 levels + the rounded normalisation) < 2 x 16 eps


def _mp():
    import mpmath
    mpmath.mp.dps = DIGITS
    return mpmath


def tolerance(lam_max, gap, factor=1.0):
    return FACTOR * EPS * float(lam_max) / float(gap) * float(factor)


# ---- 50-digit building blocks --------------------------------------------------------------------------------------------------
def _rows_to_gram(mp, rows):
    """A^T A of the rows (lists of mpf), q x q"""
    q = len(rows[0])
    M = mp.zeros(q, q)
    for a in rows:
        for i in range(q):
            if a[i] == 0:
                continue
            for j in range(i, q):
                M[i, j] += a[i] * a[j]
    for i in range(q):
        for j in range(i):
            M[i, j] = M[j, i]
    return M


def _eig(mp, M):
    """(eigenvalues ascending, eigenvectors as lists in that order) of the symmetric M"""
    E, Q = mp.eigsy(M)
    order = sorted(range(len(E)), key=lambda k: E[k])
    return [E[k] for k in order], [[Q[r, k] for r in range(M.rows)] for k in order]


def _unit(mp, v):
    n = mp.sqrt(sum(x * x for x in v))
    return [x / n for x in v]


def _mpf_rows(mp, pts):
    return [[mp.mpf(float(x)) for x in row] for row in np.asarray(pts, dtype=np.float64)]


def _weights(mp, w, m, power):
    """w_i^power as mpf, 1 when there are no weights"""
    if w is None:
        return [mp.mpf(1)] * m
    return [mp.mpf(float(x)) ** power for x in np.asarray(w, dtype=np.float64)]


def _hartley(mp, xy):
    """(scale, cx, cy): the similarity that takes the points to centroid 0 and RMS distance sqrt(2); unweighted"""
    m = len(xy)
    cx = sum(p[0] for p in xy) / m
    cy = sum(p[1] for p in xy) / m
    ms = sum((p[0] - cx) ** 2 + (p[1] - cy) ** 2 for p in xy) / m
    return mp.sqrt(2) / mp.sqrt(ms), cx, cy


def _T(mp, s, cx, cy):
    return mp.matrix([[s, 0, -s * cx], [0, s, -s * cy], [0, 0, 1]])


def _floats(v):
    return np.array([float(x) for x in v], dtype=np.float64)


def _result(mp, lam, theta, model, norm=(), factor=1.0, zero_smallest=False, sens=()):
    lam1 = mp.mpf(0) if zero_smallest else lam[0]
    gap = lam[1] - lam1
    return dict(model=_floats(model), theta=_floats(theta), norm=_floats(norm), lam_max=float(lam[-1]), gap=float(gap),
                factor=float(factor), tol=tolerance(lam[-1], gap, factor), sens=_floats(sens))


# ---- the fits ------------------------------------------------------------------------------------------------------------------
def _two_view(mp, pts, w):
    p = _mpf_rows(mp, pts)
    n1 = _hartley(mp, [(r[0], r[1]) for r in p])
    n2 = _hartley(mp, [(r[2], r[3]) for r in p])
    q = [((r[0] - n1[1]) * n1[0], (r[1] - n1[2]) * n1[0], (r[2] - n2[1]) * n2[0], (r[3] - n2[2]) * n2[0]) for r in p]
    return q, n1, n2, [mp.sqrt(x) for x in _weights(mp, w, len(p), 2)]


def homography(pts, w=None):
    """normalised DLT: x2 = (h1 . x) / (h3 . x), y2 = (h2 . x) / (h3 . x) cleared of the denominator, weight w^2; model H / H[2,2]"""
    mp = _mp()
    q, n1, n2, sw = _two_view(mp, pts, w)
    rows = []
    for (x1, y1, x2, y2), s in zip(q, sw):
        rows.append([s * v for v in (x1, y1, 1, 0, 0, 0, -x2 * x1, -x2 * y1, -x2)])
        rows.append([s * v for v in (0, 0, 0, x1, y1, 1, -y2 * x1, -y2 * y1, -y2)])
    lam, vec = _eig(mp, _rows_to_gram(mp, rows))
    theta = vec[0]
    Hn = mp.matrix([theta[0:3], theta[3:6], theta[6:9]])
    H = _T(mp, *n2) ** -1 * Hn * _T(mp, *n1)
    H = H / H[2, 2]
    return _result(mp, lam, theta, [H[r, c] for r in range(3) for c in range(3)], norm=list(n1) + list(n2),
                   zero_smallest=len(q) == 4)       # 8 rows: the ninth eigenvalue is exactly 0


def fundamental(pts, w=None):
    """normalised 8-point: one epipolar row per correspondence, weight w^2; the nearest rank-2 matrix; T2^T F T1 at unit norm.
    theta is the rank-2 matrix in normalised coordinates at unit norm; factor = 1 + 2 s3 / (s2 - s3) of the unprojected one."""
    mp = _mp()
    q, n1, n2, sw = _two_view(mp, pts, w)
    rows = [[s * v for v in (x2 * x1, x2 * y1, x2, y2 * x1, y2 * y1, y2, x1, y1, 1)] for (x1, y1, x2, y2), s in zip(q, sw)]
    lam, vec = _eig(mp, _rows_to_gram(mp, rows))
    f = vec[0]
    U, S, V = mp.svd_r(mp.matrix([f[0:3], f[3:6], f[6:9]]))
    sv = sorted([S[k] for k in range(3)], reverse=True)
    order = sorted(range(3), key=lambda k: -S[k])
    D = mp.zeros(3, 3)
    D[order[0], order[0]], D[order[1], order[1]] = S[order[0]], S[order[1]]
    F2 = U * D * V
    theta = _unit(mp, [F2[r, c] for r in range(3) for c in range(3)])
    F = _T(mp, *n2).T * F2 * _T(mp, *n1)
    model = _unit(mp, [F[r, c] for r in range(3) for c in range(3)])
    return _result(mp, lam, theta, model, norm=list(n1) + list(n2), factor=1 + 2 * sv[2] / (sv[1] - sv[2]), sens=sv)


def vanishing_point(pts, w=None):
    """the line through a segment's end point and its midpoint m, (y0 - my, mx - x0, x0 my - y0 mx), weight w^2"""
    mp = _mp()
    p = _mpf_rows(mp, pts)
    sw = [mp.sqrt(x) for x in _weights(mp, w, len(p), 2)]
    rows = []
    for (x0, y0, x1, y1), s in zip(p, sw):
        mx, my = (x0 + x1) / 2, (y0 + y1) / 2
        rows.append([s * (y0 - my), s * (mx - x0), s * (x0 * my - y0 * mx)])
    lam, vec = _eig(mp, _rows_to_gram(mp, rows))
    theta = _unit(mp, vec[0])
    return _result(mp, lam, theta, theta)


def flat(pts, w=None):
    """total least squares line / plane: weighted mean (weight w), scatter about it in a second pass, normal = its smallest
    eigenvector, c = -n . mean.  lam_max is the 2-norm of the UN-centred second-moment matrix sum w p p^T, which is what the
    product subtracts W mean mean^T from; gap is the centred scatter's.  sens = (|mean|,)."""
    mp = _mp()
    p = _mpf_rows(mp, pts)
    ww = _weights(mp, w, len(p), 1)
    d = len(p[0])
    W = sum(ww)
    mean = [sum(wi * r[k] for wi, r in zip(ww, p)) / W for k in range(d)]
    lam, vec = _eig(mp, _rows_to_gram(mp, [[mp.sqrt(wi) * (r[k] - mean[k]) for k in range(d)] for wi, r in zip(ww, p)]))
    raw, _ = _eig(mp, _rows_to_gram(mp, [[mp.sqrt(wi) * r[k] for k in range(d)] for wi, r in zip(ww, p)]))
    n = _unit(mp, vec[0])
    c = -sum(a * b for a, b in zip(n, mean))
    mean_norm = mp.sqrt(sum(x * x for x in mean))
    res = _result(mp, lam, n, n + [c], norm=mean, sens=[mean_norm])
    res["lam_max"] = float(raw[-1])
    res["tol"] = tolerance(raw[-1], res["gap"])
    return res


def round_(pts, w=None):
    """algebraic circle / sphere: o = weighted mean, s = weighted RMS distance from it (weight w), rows (1, q, |q|^2) of
    q = (p - o) / s, weight w; theta[0] + theta[1..d] . q + theta[-1] |q|^2 = 0 is |q + b|^2 = |b|^2 - theta[0] / theta[-1],
    b = theta[1..d] / (2 theta[-1]): c = o - s b, r = s sqrt(|b|^2 - theta[0] / theta[-1])"""
    mp = _mp()
    p = _mpf_rows(mp, pts)
    ww = _weights(mp, w, len(p), 1)
    d = len(p[0])
    W = sum(ww)
    o = [sum(wi * r[k] for wi, r in zip(ww, p)) / W for k in range(d)]
    s = mp.sqrt(sum(wi * sum((r[k] - o[k]) ** 2 for k in range(d)) for wi, r in zip(ww, p)) / W)
    rows = []
    for wi, r in zip(ww, p):
        q = [(r[k] - o[k]) / s for k in range(d)]
        rows.append([mp.sqrt(wi) * v for v in [1] + q + [sum(x * x for x in q)]])
    lam, vec = _eig(mp, _rows_to_gram(mp, rows))
    th = _unit(mp, vec[0])
    b = [x / (2 * th[-1]) for x in th[1:-1]]
    rad = sum(x * x for x in b) - th[0] / th[-1]
    model = [o[k] - s * b[k] for k in range(d)] + [s * mp.sqrt(rad)]
    return _result(mp, lam, th, model, norm=o + [s])


# ---- the pose: weighted reprojection cost sum w^2 ((u^ - u)^2 + (v^ - v)^2), R <- exp([omega]x) R, t <- t + dt -----------------------
def pnp_terms(pts, w, P, num):
    """(residual [2m], Jacobian [2m][6]) of the weighted reprojection residuals w (u^ - u), w (v^ - v) at the pose P [12] with
    respect to (omega, dt) at 0, in the arithmetic of `num` (mpf or decimal.Decimal; the inputs are doubles, converted exactly; a
    pose given as a list may hold numbers of that arithmetic already):
    Xc = R X + t, u^ = xc / zc, v^ = yc / zc; d Xc / d omega = -[R X]x (exp([omega]x) R X = R X + omega x R X + ..), d Xc / d t = I."""
    P = [num(float(x)) if isinstance(x, (float, np.floating)) else x for x in (P if isinstance(P, list) else np.asarray(P, dtype=np.float64).reshape(12))]
    res, jac = [], []
    for i, row in enumerate(np.asarray(pts, dtype=np.float64)):
        u, v, X, Y, Z = (num(float(x)) for x in row)
        wi = num(1) if w is None else num(float(w[i]))
        rx, ry, rz = (P[4 * k] * X + P[4 * k + 1] * Y + P[4 * k + 2] * Z for k in range(3))
        xc, yc, zc = rx + P[3], ry + P[7], rz + P[11]
        # d u^ / d Xc = (1 / zc, 0, -xc / zc^2), d v^ / d Xc = (0, 1 / zc, -yc / zc^2); omega x RX = (wy rz - wz ry, wz rx - wx rz, wx ry - wy rx)
        dX = [(0, rz, -ry, 1, 0, 0), (-rz, 0, rx, 0, 1, 0), (ry, -rx, 0, 0, 0, 1)]     # d (xc, yc, zc) / d (omega, t), by row
        gu, gv = (1 / zc, 0, -xc / (zc * zc)), (0, 1 / zc, -yc / (zc * zc))
        res += [wi * (xc / zc - u), wi * (yc / zc - v)]
        jac.append([wi * sum(gu[a] * dX[a][k] for a in range(3)) for k in range(6)])
        jac.append([wi * sum(gv[a] * dX[a][k] for a in range(3)) for k in range(6)])
    return res, jac


def normal_equations(res, jac):
    """(J^T J [6][6], J^T r [6])"""
    A = [[sum(row[i] * row[j] for row in jac) for j in range(6)] for i in range(6)]
    g = [sum(row[i] * r for row, r in zip(jac, res)) for i in range(6)]
    return A, g


def solve6(A, g):
    """delta with A delta = -g: Gaussian elimination with partial pivoting in the arithmetic of the entries"""
    n = len(g)
    M = [list(A[i]) + [-g[i]] for i in range(n)]
    for c in range(n):
        piv = max(range(c, n), key=lambda r: abs(M[r][c]))
        M[c], M[piv] = M[piv], M[c]
        for r in range(c + 1, n):
            f = M[r][c] / M[c][c]
            for k in range(c, n + 1):
                M[r][k] -= f * M[c][k]
    x = [0] * n
    for r in range(n - 1, -1, -1):
        x[r] = (M[r][n] - sum(M[r][k] * x[k] for k in range(r + 1, n))) / M[r][r]
    return x


def pnp_step_decimal(pts, w, P):
    """the Gauss-Newton step (omega, dt) [6] at the pose P in 50-digit decimal arithmetic: the statement the tests run at the
    poses the product returns (no mpmath needed; tests/test_refit_accuracy_cpu.py holds it to the mpmath one where mpmath is)"""
    with decimal.localcontext() as dc:
        dc.prec = DIGITS
        res, jac = pnp_terms(pts, w, P, decimal.Decimal)
        return np.array([float(x) for x in solve6(*normal_equations(res, jac))])


def _rodrigues(mp, om):
    ang = mp.sqrt(sum(x * x for x in om))
    if ang == 0:
        return mp.eye(3)
    k = [x / ang for x in om]
    K = mp.matrix([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return mp.eye(3) + mp.sin(ang) * K + (1 - mp.cos(ang)) * (K * K)


def _moved(mp, P, delta):
    """the pose (mpf [12]) after R <- exp([omega]x) R, t <- t + dt"""
    R = _rodrigues(mp, delta[:3]) * mp.matrix([[P[4 * r + c] for c in range(3)] for r in range(3)])
    return [R[r, c] if c < 3 else P[4 * r + 3] + delta[3 + r] for r in range(3) for c in range(4)]


def _residual_at(mp, p, ww, P):
    out = []
    for (u, v, X, Y, Z), wi in zip(p, ww):
        xc, yc, zc = (P[4 * k] * X + P[4 * k + 1] * Y + P[4 * k + 2] * Z + P[4 * k + 3] for k in range(3))
        out += [wi * (xc / zc - u), wi * (yc / zc - v)]
    return out


def pnp_jacobian_check(pts, w, P):
    """max |analytic - central difference| over the Jacobian's entries: the differences are of the 50-digit residuals under
    the pose update itself, at step 1e-20 (truncation ~ 1e-40, rounding ~ 1e-30)"""
    mp = _mp()
    p = _mpf_rows(mp, pts)
    ww = [mp.mpf(1)] * len(p) if w is None else [mp.mpf(float(x)) for x in w]
    P0 = [mp.mpf(float(x)) for x in np.asarray(P, dtype=np.float64).reshape(12)]
    _, jac = pnp_terms(pts, w, P, lambda x: mp.mpf(x))
    h = mp.mpf(10) ** -20
    worst = mp.mpf(0)
    for k in range(6):
        d = [mp.mpf(0)] * 6
        d[k] = h
        plus = _residual_at(mp, p, ww, _moved(mp, P0, d))
        d[k] = -h
        minus = _residual_at(mp, p, ww, _moved(mp, P0, d))
        for r in range(len(plus)):
            worst = max(worst, abs((plus[r] - minus[r]) / (2 * h) - jac[r][k]))
    return float(worst)


def pnp_state(pts, w, P):
    """at the pose P: the Gauss-Newton step and what the bounds are made of -
    dict(delta [6], inv = |(J^T J)^-1|_2, J = |J|_2, JtJ = |J^T J|_2, r = |r|, kappa = kappa(J^T J))"""
    mp = _mp()
    res, jac = pnp_terms(pts, w, P, lambda x: mp.mpf(x))
    A, g = normal_equations(res, jac)
    lam, _ = _eig(mp, mp.matrix(A))
    return dict(delta=_floats(solve6(A, g)), inv=float(1 / lam[0]), J=float(mp.sqrt(lam[-1])), JtJ=float(lam[-1]),
                r=float(mp.sqrt(sum(x * x for x in res))), kappa=float(lam[-1] / lam[0]))


def pnp_run(pts, w, P, iterations=6, until=None):
    """the reference's own Gauss-Newton run from P: (pose as mpf [12] after `iterations` steps, or after the first step below
    `until`; the number of steps after which |delta| first fell below 1e-12, or None)"""
    mp = _mp()
    cur = [mp.mpf(float(x)) for x in np.asarray(P, dtype=np.float64).reshape(12)]
    first = None
    for it in range(iterations):
        res, jac = pnp_terms(pts, w, cur, lambda x: mp.mpf(x))
        d = solve6(*normal_equations(res, jac))
        cur = _moved(mp, cur, d)
        nd = mp.sqrt(sum(x * x for x in d))
        if first is None and nd < mp.mpf(10) ** -12:
            first = it + 1
        if until is not None and nd < until:
            break
    return cur, first


def pnp_moved(P, delta):
    """the pose P (mpf [12]) after the motion delta = (omega, dt), rounded to doubles"""
    mp = _mp()
    return _floats(_moved(mp, list(P), [mp.mpf(float(x)) for x in delta]))
