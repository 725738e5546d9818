"""The iterative minimal solvers restated from their definitions at 50 digits: what pgx_solve_minimal's 4-point homography, 7-point
fundamental matrix and P3P (solve.hip: solve_h4_kernel, solve_f7_kernel, solve_p3p) and the host routes of _estimators.py are held to.

TEST INFRASTRUCTURE, never imported by the product; mpmath is imported when a function is called.  tests/golden/make_golden_minimal.py
runs this module and writes tests/golden/kat_minimal_v1.npz; the comparisons (tests/minimal_accuracy_cases.py) read that file.
The committed float64 inputs are taken as exact.  Three things are kept apart:

  what the answer is          *_definition(): from the problem's statement, by a method that is not the product's -
                              H: the null vector of the 8 x 9 DLT system of the unscaled points (50-digit SVD), in the h33 = 1 chart and
                                 at unit norm, and [H | H^-1];
                              F: the 2-dimensional null space of the 7 x 9 system (SVD), det(l F1 + (1 - l) F2) by interpolation, all its
                                 roots by polyroots at raised precision, the real ones as unit-norm F; the basis must not matter;
                              P3P: every depth triple (s1, s2, s3) > 0 of the three cosine-law equations - the resultant in x = s2 / s1 of
                                 the two conics in (s2 / s1, s3 / s1) (the product eliminates the other way, to v = s3 / s1), its roots by
                                 polyroots at raised precision, both y of each root, Newton on the three equations - and the pose from
                                 the camera-frame points Y_i = s_i f_i as the R, t with Y = R X + t (R = E D^-1 of the edge triads);
  how accurately the product's ROUTE can deliver it
                              *_route(): the stages of solve.hip restated once, with a hook at every stage interface that multiplies
                              that stage's outputs by (1 + delta); kappa_route = sum over stages of (roundings on the stage's longest
                              chain) x max_i sum_j |d out_i / d delta_j|, by differences of step 1e-20 at 50 digits; for the 8 x 8 elimination the
                              standard bound 3 n rho cond_inf |h|_inf instead.  The tolerance is 32 eps kappa_route; the expected values
                              never come from the route.  At delta = 0 the route must land on the definition's answer to 1e-40
                              (asserted by the generator: a wrong Grunert coefficient ends there);
  the problem's own condition *_condition(): |J|_2 |x|_2 / |y|_2, J the Jacobian of the answer y with respect to the inputs x (in the
                              solver's scaled coordinates for H and F), by differences at 50 digits.
"""
import numpy as np

DIGITS = 50
EPS = 2.0 ** -52
FACTOR = 32.0
# roundings on the longest dependency chain inside each stage, counted from solve.hip (DESIGN.md 4.5b lists the chains)
P3P_WEIGHTS = {"bearings": 5, "cosines, squared sides": 4, "terms of A0..A4": 8, "m0..m3": 16, "v": 1, "terms of u and s1": 3,
               "u, s1": 6, "depths, camera-frame points": 2, "frames": 14, "R": 3, "t": 4}
H4_WEIGHTS = {"scaled rows": 2, "solved h": 1, "unscaled h": 1, "unit norm (the comparison's own rounding)": 12}


def _mp():
    import mpmath
    mpmath.mp.dps = DIGITS
    return mpmath


class digits:
    """with digits(80): the working precision for a block (the generator compares route and definition at delta = 0 there, so that
    the 1e-40 it asks for is not lost to the conditioning of a near-double root)"""

    def __init__(self, n):
        self.n = n

    def __enter__(self):
        global DIGITS
        self.old, DIGITS = DIGITS, self.n

    def __exit__(self, *a):
        global DIGITS
        DIGITS = self.old
        _mp()


def _f(x):
    return float(x)


def no_hook(stage, values):
    return values


def _relative(J, x, y):
    """the normwise relative condition number |J|_2 |x|_2 / |y|_2"""
    return float(np.linalg.norm(J, 2) * np.linalg.norm([_f(v) for v in x]) / np.linalg.norm([_f(v) for v in y]))


# ---- P3P: the definition --------------------------------------------------------------------------------------------------------
def _p3p_setup(mp, rows):
    """bearings f [3][3], object points X [3][3], cosines (ca, cb, cg) and squared sides (a2, b2, c2) of rows (u, v, X, Y, Z)"""
    return _p3p_setup_mp(mp, [[mp.mpf(float(x)) for x in r] for r in rows])


def _p3p_equations(s, cos, side):
    ca, cb, cg = cos
    a2, b2, c2 = side
    s1, s2, s3 = s
    F = [s1 * s1 + s2 * s2 - 2 * s1 * s2 * cg - c2, s1 * s1 + s3 * s3 - 2 * s1 * s3 * cb - b2, s2 * s2 + s3 * s3 - 2 * s2 * s3 * ca - a2]
    J = [[2 * s1 - 2 * s2 * cg, 2 * s2 - 2 * s1 * cg, 0], [2 * s1 - 2 * s3 * cb, 0, 2 * s3 - 2 * s1 * cb],
         [0, 2 * s2 - 2 * s3 * ca, 2 * s3 - 2 * s2 * ca]]
    return F, J


def _p3p_polish(mp, s, cos, side, steps=12):
    """Newton on the three cosine-law equations; (depths, relative residual)"""
    s = list(s)
    for _ in range(steps):
        F, J = _p3p_equations(s, cos, side)
        try:
            d = mp.lu_solve(mp.matrix(J), mp.matrix(F))
        except ZeroDivisionError:
            break
        s = [s[k] - d[k] for k in range(3)]
        if max(abs(d[k]) for k in range(3)) <= mp.mpf(10) ** -(DIGITS - 3) * max(abs(x) for x in s):
            break
    F, _ = _p3p_equations(s, cos, side)
    return s, max(abs(F[k]) / side[(2, 1, 0)[k]] for k in range(3))


def _p3p_pose(mp, s, f, X):
    """[R | t] row-major (12) with s_i f_i = R X_i + t: R carries the edge triad of the object triangle onto the camera-frame one"""
    Y = [[s[r] * f[r][k] for k in range(3)] for r in range(3)]

    def triad(P):
        a = [P[1][k] - P[0][k] for k in range(3)]
        b = [P[2][k] - P[0][k] for k in range(3)]
        n = [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]
        return mp.matrix([[a[0], b[0], n[0]], [a[1], b[1], n[1]], [a[2], b[2], n[2]]])
    R = triad(Y) * mp.inverse(triad(X))
    t = [Y[0][i] - sum(R[i, j] * X[0][j] for j in range(3)) for i in range(3)]
    return [x for i in range(3) for x in (R[i, 0], R[i, 1], R[i, 2], t[i])]


def p3p_depths(rows):
    """every (s1, s2, s3) > 0 of the three cosine-law equations, ascending in v = s3 / s1; 50-digit mpf"""
    mp = _mp()
    f, X, cos, side = _p3p_setup(mp, rows)
    ca, cb, cg = cos
    a2, b2, c2 = side
    if min(side) == 0:                    # two of the three object points coincide: no triangle, no pose
        return []
    # E1(x, y) = b2 (1 + x^2 - 2 x cg) - c2 (1 + y^2 - 2 y cb), E2(x, y) = a2 (1 + x^2 - 2 x cg) - c2 (x^2 + y^2 - 2 x y ca), x = s2/s1, y = s3/s1:
    # quadratics in y with the same leading coefficient; their resultant in y is a quartic in x, interpolated at five nodes
    def res(x):
        w = 1 + x * x - 2 * x * cg
        p2, p1, p0 = -c2, 2 * c2 * cb, b2 * w - c2
        q2, q1, q0 = -c2, 2 * c2 * ca * x, a2 * w - c2 * x * x
        return (p2 * q0 - p0 * q2) ** 2 - (p2 * q1 - p1 * q2) * (p1 * q0 - p0 * q1)
    nodes = [mp.mpf(k) for k in (0, 1, -1, 2, -2)]
    V = mp.matrix([[x ** (4 - j) for j in range(5)] for x in nodes])
    coef = mp.lu_solve(V, mp.matrix([res(x) for x in nodes]))
    roots = mp.polyroots([coef[k] for k in range(5)], maxsteps=500, extraprec=4 * mp.mp.prec)
    found = []
    for x in roots:
        if abs(mp.im(x)) > mp.mpf(10) ** -18 * max(1, abs(mp.re(x))) or mp.re(x) <= 0:
            continue
        x = mp.re(x)
        w = 1 + x * x - 2 * x * cg
        disc = cb * cb - 1 + b2 * w / c2            # E1 in y: y^2 - 2 cb y + 1 - b2 w / c2 = 0
        if disc < 0:
            if disc < -mp.mpf(10) ** -18:
                continue
            disc = mp.mpf(0)
        for y in (cb - mp.sqrt(disc), cb + mp.sqrt(disc)):
            if y <= 0 or w <= 0:
                continue
            e2 = a2 * w - c2 * (x * x + y * y - 2 * x * y * ca)
            if abs(e2) > mp.mpf(10) ** -12 * (a2 + c2):
                continue
            s1 = mp.sqrt(c2 / w)
            s, r = _p3p_polish(mp, [s1, x * s1, y * s1], cos, side)
            if r > mp.mpf(10) ** -(DIGITS - 6) or min(s) <= 0:
                continue
            if all(max(abs(s[k] - o[k]) for k in range(3)) > mp.mpf(10) ** -25 * max(s) for o in found):
                found.append(s)
    return sorted(found, key=lambda s: s[2] / s[0])


def p3p_definition(rows):
    """[(depths, pose)] of one sample, ascending in v = s3 / s1 (mpf lists)"""
    mp = _mp()
    f, X, _, _ = _p3p_setup(mp, rows)
    return [(s, _p3p_pose(mp, s, f, X)) for s in p3p_depths(rows)]


def p3p_den(rows, s):
    """2 (cg - v ca) at the solution s: the denominator of the product's linear formula for u"""
    mp = _mp()
    _, _, cos, _ = _p3p_setup(mp, rows)
    return 2 * (cos[2] - s[2] / s[0] * cos[0])


def p3p_condition(rows, s):
    """|d pose / d rows|_2 at the solution s (12 x 15, central differences, step 1e-20; the perturbed problem is solved by Newton from s)"""
    mp = _mp()
    h = mp.mpf(10) ** -20
    base = [[mp.mpf(float(x)) for x in r] for r in rows]

    def pose(rr):
        f, X, cos, side = _p3p_setup_mp(mp, rr)
        s2, _ = _p3p_polish(mp, s, cos, side)
        return _p3p_pose(mp, s2, f, X)
    J = np.zeros((12, 15))
    for r in range(3):
        for c in range(5):
            hi = [list(x) for x in base]
            lo = [list(x) for x in base]
            hi[r][c] += h
            lo[r][c] -= h
            a, b = pose(hi), pose(lo)
            J[:, 5 * r + c] = [_f((a[k] - b[k]) / (2 * h)) for k in range(12)]
    return _relative(J, [x for r in base for x in r], pose(base))


def _p3p_setup_mp(mp, rows):
    """_p3p_setup on rows that are mpf already"""
    f = []
    for r in rows:
        ln = mp.sqrt(r[0] * r[0] + r[1] * r[1] + 1)
        f.append([r[0] / ln, r[1] / ln, 1 / ln])
    X = [r[2:5] for r in rows]
    dot = lambda a, b: a[0] * b[0] + a[1] * b[1] + a[2] * b[2]
    sub = lambda a, b: [a[k] - b[k] for k in range(3)]
    cos = (dot(f[1], f[2]), dot(f[0], f[2]), dot(f[0], f[1]))
    side = (dot(sub(X[1], X[2]), sub(X[1], X[2])), dot(sub(X[0], X[2]), sub(X[0], X[2])), dot(sub(X[0], X[1]), sub(X[0], X[1])))
    return f, X, cos, side


# ---- P3P: the product's route, stage by stage -----------------------------------------------------------------------------------
def p3p_quartic(rows, hook=no_hook):
    """(f, X, (ca, cb, cg), (a2, b2, c2), q, [m0..m3]) as solve_p3p forms them; hooks: bearings; cosines, squared sides; terms of A0..A4; m0..m3"""
    mp = _mp()
    rows = [[mp.mpf(float(x)) for x in r] for r in rows]
    flat = hook("bearings", [x for r in rows for x in (lambda ln: (r[0] / ln, r[1] / ln, 1 / ln))(mp.sqrt(r[0] * r[0] + r[1] * r[1] + 1))])
    f = [flat[0:3], flat[3:6], flat[6:9]]
    X = [r[2:5] for r in rows]
    dot = lambda a, b: a[0] * b[0] + a[1] * b[1] + a[2] * b[2]
    sub = lambda a, b: [a[k] - b[k] for k in range(3)]
    d12, d02, d01 = sub(X[1], X[2]), sub(X[0], X[2]), sub(X[0], X[1])
    ca, cb, cg, a2, b2, c2 = hook("cosines, squared sides", [dot(f[1], f[2]), dot(f[0], f[2]), dot(f[0], f[1]), dot(d12, d12), dot(d02, d02), dot(d01, d01)])
    q, rr = (a2 - c2) / b2, (a2 + c2) / b2
    T = hook("terms of A0..A4", [
        (q - 1) * (q - 1), -4 * c2 / b2 * ca * ca,                                                               # A4
        q * (1 - q) * cb, -(1 - rr) * ca * cg, 2 * c2 / b2 * ca * ca * cb,                                       # A3 / 4
        q * q, mp.mpf(-1), 2 * q * q * cb * cb, 2 * (b2 - c2) / b2 * ca * ca, -4 * rr * ca * cb * cg, 2 * (b2 - a2) / b2 * cg * cg,   # A2 / 2
        -q * (1 + q) * cb, 2 * a2 / b2 * cg * cg * cb, -(1 - rr) * ca * cg,                                      # A1 / 4
        (1 + q) * (1 + q), -4 * a2 / b2 * cg * cg])                                                              # A0
    A4, A3, A2, A1, A0 = T[0] + T[1], 4 * (T[2] + T[3] + T[4]), 2 * sum(T[5:11]), 4 * (T[11] + T[12] + T[13]), T[14] + T[15]
    m = hook("m0..m3", [A0 / A4, A1 / A4, A2 / A4, A3 / A4])
    return f, X, (ca, cb, cg), (a2, b2, c2), q, m


def p3p_route_roots(rows):
    """the positive real roots v of the route's monic quartic at 50 digits, ascending"""
    mp = _mp()
    m = p3p_quartic(rows)[5]
    roots = mp.polyroots([1, m[3], m[2], m[1], m[0]], maxsteps=500, extraprec=4 * mp.mp.prec)
    return sorted(mp.re(v) for v in roots if abs(mp.im(v)) <= mp.mpf(10) ** -18 * max(1, abs(mp.re(v))) and mp.re(v) > 0)


def p3p_route(rows, v_start, hook=no_hook, quadratic_u=None):
    """The pose (12) the route makes of the root next to v_start, or None where a gate refuses it.  quadratic_u = -1 / +1: u from the
    second way (u^2 - 2 cg u + 1 - c2 / s1^2 = 0, that root) in place of the linear formula."""
    mp = _mp()
    f, X, (ca, cb, cg), (a2, b2, c2), q, m = p3p_quartic(rows, hook)
    v = v_start
    for _ in range(60):                                        # the root of the (hooked) quartic next to v_start
        p = (((v + m[3]) * v + m[2]) * v + m[1]) * v + m[0]
        dp = ((4 * v + 3 * m[3]) * v + 2 * m[2]) * v + m[1]
        if dp == 0:
            break
        step = p / dp
        v = v - step
        if abs(step) <= mp.mpf(10) ** -(DIGITS - 3) * abs(v):
            break
    v, = hook("v", [v])
    t = hook("terms of u and s1", [(-1 + q) * v * v, -2 * q * cb * v, 1 + q, cg, -v * ca, mp.mpf(1), v * v, -2 * v * cb])
    s1 = mp.sqrt(b2 / (t[5] + t[6] + t[7]))
    if quadratic_u is None:
        u = (t[0] + t[1] + t[2]) / (2 * (t[3] + t[4]))
    else:
        disc = cg * cg - 1 + c2 / (s1 * s1)
        if disc < 0:
            return None
        u = cg + quadratic_u * mp.sqrt(disc)
    u, s1 = hook("u, s1", [u, s1])
    s2, s3 = u * s1, v * s1
    if not (s1 > 0 and s2 > 0 and s3 > 0):
        return None
    dep = hook("depths, camera-frame points", [s1, s2, s3])
    Y = hook("depths, camera-frame points", [f[r][k] * dep[r] for r in range(3) for k in range(3)])
    Y = [Y[0:3], Y[3:6], Y[6:9]]
    E = []
    for P in (X, Y):
        p1 = [P[1][k] - P[0][k] for k in range(3)]
        p2 = [P[2][k] - P[0][k] for k in range(3)]
        n1 = mp.sqrt(p1[0] * p1[0] + p1[1] * p1[1] + p1[2] * p1[2])
        e0 = [x / n1 for x in p1]
        cr = [e0[1] * p2[2] - e0[2] * p2[1], e0[2] * p2[0] - e0[0] * p2[2], e0[0] * p2[1] - e0[1] * p2[0]]
        n3 = mp.sqrt(cr[0] * cr[0] + cr[1] * cr[1] + cr[2] * cr[2])
        e2 = [x / n3 for x in cr]
        e1 = [e2[1] * e0[2] - e2[2] * e0[1], e2[2] * e0[0] - e2[0] * e0[2], e2[0] * e0[1] - e2[1] * e0[0]]
        E.append(e0 + e1 + e2)
    E = hook("frames", E[0] + E[1])
    EX, EY = [E[0:3], E[3:6], E[6:9]], [E[9:12], E[12:15], E[15:18]]
    R = hook("R", [EY[0][i] * EX[0][j] + EY[1][i] * EX[1][j] + EY[2][i] * EX[2][j] for i in range(3) for j in range(3)])
    t = hook("t", [Y[0][i] - (R[3 * i] * X[0][0] + R[3 * i + 1] * X[0][1] + R[3 * i + 2] * X[0][2]) for i in range(3)])
    return [x for i in range(3) for x in (R[3 * i], R[3 * i + 1], R[3 * i + 2], t[i])]


def kappa_route(route, weights, absolute=None, nout=None, extra_skips=()):
    """sum over stages of weight x max_i sum_j |d out_i / d delta_j| (the deltas of that stage's hook; forward differences of step
    1e-20 at 50 digits, so exact to 1e-20 relative); route(hook) -> the outputs.  absolute = {stage: size}: that stage's outputs
    move by delta x size instead of by the factor 1 + delta (a normwise bound: the elimination stages).  Also {stage: its share}.
    nout: the maximum runs over the first nout outputs only; each further output gets its own sum over the stages outside
    extra_skips, returned third (an invariant of the model and the stages that can break it)."""
    mp = _mp()
    h = mp.mpf(10) ** -20
    sizes = []
    absolute = absolute or {}
    extra = 0.0

    def count(stage, values):
        sizes.append((stage, len(values)))
        return values
    base = route(count)
    total, shares = 0.0, {}
    for call, (stage, size) in enumerate(sizes):
        acc = np.zeros(len(base))
        for j in range(size):
            seen = [0]

            def hook(st, values, j=j):
                seen[0] += 1
                if seen[0] - 1 != call:
                    return values
                values = list(values)
                values[j] = values[j] + h * absolute[st] if st in absolute else values[j] * (1 + h)
                return values
            out = route(hook)
            acc += [abs(_f((out[k] - base[k]) / h)) for k in range(len(base))]
        worst = float(acc[:nout].max())
        shares[stage] = shares.get(stage, 0.0) + weights[stage] * worst
        total += weights[stage] * worst
        if nout is not None:
            extra += weights[stage] * acc[nout:] * (stage not in extra_skips)
    return (total, shares) if nout is None else (total, shares, extra)


def p3p_kappa_route(rows, s):
    """kappa_route of the solution with depths s (the root v = s3 / s1 of the route's quartic)"""
    v = s[2] / s[0]
    return kappa_route(lambda hook: p3p_route(rows, v, hook), P3P_WEIGHTS)


# ---- the 4-point homography -----------------------------------------------------------------------------------------------------
def _h4_rows(mp, p):
    """the 8 x 9 DLT system of four correspondences (x1, y1, x2, y2): x2 (h6 x1 + h7 y1 + h8) = h0 x1 + h1 y1 + h2 and the same for y2"""
    A = []
    for x1, y1, x2, y2 in p:
        A.append([-x1, -y1, -1, 0, 0, 0, x2 * x1, x2 * y1, x2])
    for x1, y1, x2, y2 in p:
        A.append([0, 0, 0, -x1, -y1, -1, y2 * x1, y2 * y1, y2])
    return mp.matrix(A)


def h4_definition(p4, scale=1.0):
    """The null vector of the exact DLT system of p4 / scale: dict(rank_deficient, sv (the two smallest singular values over the
    largest), unit (9, unit norm, largest entry positive), chart (9, h33 = 1, None where h33 is 0), sym (18, [H | H^-1], None where
    singular))."""
    mp = _mp()
    p = [[mp.mpf(float(x)) / mp.mpf(float(scale)) for x in r] for r in p4]
    A = _h4_rows(mp, p)
    _, S, V = mp.svd_r(A.T * A, compute_uv=True)          # 9 x 9, symmetric: the singular values are those of A squared
    sv = sorted([mp.sqrt(abs(S[k])) for k in range(9)], reverse=True)
    out = dict(sv=(sv[7] / sv[0], sv[8] / sv[0]), rank_deficient=bool(sv[7] <= mp.mpf(10) ** -20 * sv[0]), unit=None, chart=None, sym=None)
    if out["rank_deficient"]:
        return out
    k = min(range(9), key=lambda i: abs(S[i]))
    h = [V[k, j] for j in range(9)]
    # the null vector again from the definition A h = 0 directly (inverse iteration cleans what the squared system lost)
    big = max(range(9), key=lambda j: abs(h[j]))
    cols = [j for j in range(9) if j != big]
    sol = mp.lu_solve(mp.matrix([[A[i, j] for j in cols] for i in range(8)]), mp.matrix([-A[i, big] for i in range(8)]))
    h = [mp.mpf(0)] * 9
    for n, j in enumerate(cols):
        h[j] = sol[n]
    h[big] = mp.mpf(1)
    nrm = mp.sqrt(sum(x * x for x in h))
    out["unit"] = [x / nrm for x in h]
    if h[8] != 0:
        out["chart"] = [x / h[8] for x in h]
        H = mp.matrix(3, 3)
        for i in range(9):
            H[i // 3, i % 3] = out["chart"][i]
        if mp.det(H) != 0:
            Hi = mp.inverse(H)
            out["sym"] = out["chart"] + [Hi[i // 3, i % 3] for i in range(9)]
    return out


def h4_route(p4, scale, hook=no_hook):
    """solve_h4_kernel's stages at 50 digits: the rows of the points over `scale`, the h33 = 1 solve, the unscaling; the solved h
    in SCALED coordinates is what is returned (the comparison is made there), after the unscaling's rounding."""
    mp = _mp()
    p = [[mp.mpf(float(x)) / mp.mpf(float(scale)) for x in r] for r in p4]
    ent = []
    for x1, y1, x2, y2 in p:
        ent += [-x1, -y1, x2 * x1, x2 * y1, -x2]
    for x1, y1, x2, y2 in p:
        ent += [-x1, -y1, y2 * x1, y2 * y1, -y2]
    ent = hook("scaled rows", ent)
    M, rhs = mp.zeros(8, 8), mp.zeros(8, 1)
    for r in range(4):
        a, b = ent[5 * r:5 * r + 5], ent[20 + 5 * r:25 + 5 * r]
        M[r, 0], M[r, 1], M[r, 2], M[r, 6], M[r, 7], rhs[r] = a[0], a[1], -1, a[2], a[3], a[4]
        M[r + 4, 3], M[r + 4, 4], M[r + 4, 5], M[r + 4, 6], M[r + 4, 7], rhs[r + 4] = b[0], b[1], -1, b[2], b[3], b[4]
    h = hook("solved h", [x for x in mp.lu_solve(M, rhs)])
    h = hook("unscaled h", h) + [mp.mpf(1)]
    nrm = mp.sqrt(sum(x * x for x in h))
    return hook("unit norm (the comparison's own rounding)", [x / nrm for x in h])


def h4_elimination(p4, scale):
    """(growth factor of the exact elimination with partial pivoting, cond_inf of the 8 x 8 block), both at 50 digits"""
    mp = _mp()
    p = [[mp.mpf(float(x)) / mp.mpf(float(scale)) for x in r] for r in p4]
    A = _h4_rows(mp, p)
    M = mp.matrix([[A[i, j] for j in range(8)] for i in range(8)])
    norm = lambda B: max(sum(abs(B[i, j]) for j in range(B.cols)) for i in range(B.rows))
    cond = norm(M) * norm(mp.inverse(M))
    W = M.copy()
    top = big = max(abs(W[i, j]) for i in range(8) for j in range(8))
    for c in range(8):
        pr = max(range(c, 8), key=lambda i: abs(W[i, c]))
        if pr != c:
            for j in range(8):
                W[c, j], W[pr, j] = W[pr, j], W[c, j]
        for i in range(c + 1, 8):
            fct = W[i, c] / W[c, c]
            for j in range(c, 8):
                W[i, j] -= fct * W[c, j]
        big = max(big, max(abs(W[i, j]) for i in range(8) for j in range(8)))
    return _f(big / top), _f(cond)


def h4_kappa_route(p4, scale):
    """rows and unscaling by their deltas; the solved h moves by 3 n rho cond_inf |h|_inf (n = 8), the standard bound of the solve"""
    rho, cond = h4_elimination(p4, scale)
    size = []
    h4_route(p4, scale, lambda stage, values: (size.append(max(abs(x) for x in values)) if stage == "solved h" else None, values)[1])
    weights = dict(H4_WEIGHTS)
    weights["solved h"] = 3 * 8 * rho * cond
    return kappa_route(lambda hook: h4_route(p4, scale, hook), weights, absolute={"solved h": size[0]})


def h4_condition(p4, scale):
    """the relative condition of the unit-norm null vector with respect to p4 / scale (9 x 16, central differences)"""
    mp = _mp()
    h = mp.mpf(10) ** -20
    base = [[mp.mpf(float(x)) / mp.mpf(float(scale)) for x in r] for r in p4]

    def solve(p):
        A = _h4_rows(mp, p)
        sol = mp.lu_solve(mp.matrix([[A[i, j] for j in range(8)] for i in range(8)]), mp.matrix([-A[i, 8] for i in range(8)]))
        v = [sol[k] for k in range(8)] + [mp.mpf(1)]
        nrm = mp.sqrt(sum(x * x for x in v))
        return [x / nrm for x in v]
    J = np.zeros((9, 16))
    for r in range(4):
        for c in range(4):
            hi = [list(x) for x in base]
            lo = [list(x) for x in base]
            hi[r][c] += h
            lo[r][c] -= h
            a, b = solve(hi), solve(lo)
            J[:, 4 * r + c] = [_f((a[k] - b[k]) / (2 * h)) for k in range(9)]
    return _relative(J, [x for r in base for x in r], solve(base))


# ---- the 7-point fundamental matrix ---------------------------------------------------------------------------------------------
# roundings on the longest chain of each stage of solve_f7_kernel; the null vectors take the elimination bound
F7_WEIGHTS = {"scaled rows": 2, "null vectors": 1, "c0..c3": 15, "first root": 1, "qb, qc": 3, "terms of the other roots": 2,
              "other roots": 1, "F before unscaling": 3, "normalised F": 16}


def _f7_rows(mp, p7, scale):
    A = []
    for r in p7:
        x1, y1, x2, y2 = [mp.mpf(float(x)) / mp.mpf(float(scale)) for x in r]
        A.append([x2 * x1, x2 * y1, x2, y2 * x1, y2 * y1, y2, x1, y1, mp.mpf(1)])
    return A


def _det3(a):
    return a[0] * (a[4] * a[8] - a[5] * a[7]) - a[1] * (a[3] * a[8] - a[5] * a[6]) + a[2] * (a[3] * a[7] - a[4] * a[6])


def _unit_signed(mp, F):
    nrm = mp.sqrt(sum(x * x for x in F))
    # the sign: the first entry of at least half the largest magnitude is positive (not "the largest": a skew-symmetric F has its
    # entries in pairs of equal magnitude and opposite sign, and which of a pair is the larger is decided in the last digit)
    top = max(abs(x) for x in F)
    big = min(k for k in range(9) if 2 * abs(F[k]) >= top)
    sign = 1 if F[big] > 0 else -1
    return [sign * x / nrm for x in F]


def _gauss_jordan(mp, A):
    """Gauss-Jordan with full pivoting on the 7 x 9 rows (first maximum in row-major order, as solve_f7_kernel): (F1, F2, col, growth
    factor, cond_inf of the pivoted 7 x 7 block), or None where a pivot vanishes (rank < 7)"""
    M = [list(r) for r in A]
    col = list(range(9))
    top = big = max(abs(x) for r in M for x in r)
    for r in range(7):
        best, pr, pc = mp.mpf(-1), r, r
        for i in range(r, 7):
            for j in range(r, 9):
                if abs(M[i][j]) > best:
                    best, pr, pc = abs(M[i][j]), i, j
        if best <= mp.mpf(10) ** -30 * top:
            return None
        M[r], M[pr] = M[pr], M[r]
        if pc != r:
            for i in range(7):
                M[i][r], M[i][pc] = M[i][pc], M[i][r]
            col[r], col[pc] = col[pc], col[r]
        piv = M[r][r]
        M[r] = [x / piv for x in M[r]]
        for i in range(7):
            if i != r:
                fct = M[i][r]
                M[i] = [M[i][j] - fct * M[r][j] for j in range(9)]
        big = max(big, max(abs(x) for row in M for x in row))
    F1, F2 = [mp.mpf(0)] * 9, [mp.mpf(0)] * 9
    for k in range(7):
        F1[col[k]], F2[col[k]] = -M[k][7], -M[k][8]
    F1[col[7]], F2[col[8]] = mp.mpf(1), mp.mpf(1)
    B = mp.matrix([[A[i][col[j]] for j in range(7)] for i in range(7)])
    norm = lambda Z: max(sum(abs(Z[i, j]) for j in range(Z.cols)) for i in range(Z.rows))
    return F1, F2, col, _f(big / top), _f(norm(B) * norm(mp.inverse(B)))


def _pencil_cubic(mp, F1, F2):
    """(c3, c2, c1, c0) of det(l F1 + (1 - l) F2), by interpolation at four nodes"""
    nodes = [mp.mpf(k) for k in (0, 1, -1, 2)]
    vals = [_det3([l * F1[k] + (1 - l) * F2[k] for k in range(9)]) for l in nodes]
    c = mp.lu_solve(mp.matrix([[l ** 3, l ** 2, l, 1] for l in nodes]), mp.matrix(vals))
    return [c[k] for k in range(4)]


def _real_roots(mp, coef):
    """the real roots of the polynomial (highest power first; leading zeros dropped), by polyroots at raised precision"""
    top = max(abs(x) for x in coef)
    coef = list(coef)
    while coef and abs(coef[0]) <= mp.mpf(10) ** -35 * top:
        coef.pop(0)
    if len(coef) <= 1:
        return []
    roots = mp.polyroots(coef, maxsteps=500, extraprec=4 * mp.mp.prec)
    return sorted(mp.re(x) for x in roots if abs(mp.im(x)) <= mp.mpf(10) ** -30 * max(1, abs(x)))


def f7_solutions(F1, F2):
    """every singular member of the pencil spanned by F1, F2, as unit-norm F with the largest entry positive; None where the
    cubic vanishes (every member singular: no finite solution set)"""
    mp = _mp()
    c = _pencil_cubic(mp, F1, F2)
    scale3 = (max(abs(x) for x in F1) + max(abs(x) for x in F2)) ** 3
    if max(abs(x) for x in c) <= mp.mpf(10) ** -35 * scale3:
        return None
    out = [_unit_signed(mp, [l * F1[k] + (1 - l) * F2[k] for k in range(9)]) for l in _real_roots(mp, c)]
    if abs(c[0]) <= mp.mpf(10) ** -35 * max(abs(x) for x in c):         # the root at infinity of this chart: F1 - F2 itself
        out.append(_unit_signed(mp, [F1[k] - F2[k] for k in range(9)]))
    return out


def f7_definition(p7, scale, basis="svd"):
    """dict(rank_deficient, sv (the smallest singular value over the largest), sols [unit-norm F in the coordinates over `scale`] or
    None where the cubic vanishes).  basis: the null space from the 50-digit SVD, "mixed" = those two vectors rotated, "gj" = the
    two vectors of Gauss-Jordan with a free variable at 1: the solution set must not depend on it (asserted by the generator)."""
    mp = _mp()
    A = _f7_rows(mp, p7, scale)
    _, S, V = mp.svd_r(mp.matrix(A), full_matrices=True, compute_uv=True)
    sv = [S[k] for k in range(7)]
    out = dict(sv=_f(min(sv) / max(sv)), rank_deficient=bool(min(sv) <= mp.mpf(10) ** -20 * max(sv)), sols=None)
    if out["rank_deficient"]:
        return out
    F1, F2 = [V[7, k] for k in range(9)], [V[8, k] for k in range(9)]
    if basis == "mixed":
        c, s = mp.cos(mp.mpf("0.7")), mp.sin(mp.mpf("0.7"))
        F1, F2 = [c * F1[k] + s * F2[k] for k in range(9)], [-s * F1[k] + c * F2[k] for k in range(9)]
    if basis == "gj":
        F1, F2 = _gauss_jordan(mp, A)[:2]
    out["sols"] = f7_solutions(F1, F2)
    return out


def f7_route(p7, scale, which, hook=no_hook):
    """solve_f7_kernel's stages at 50 digits; `which` = (branch, slot): the slot whose F is returned - unit norm in the coordinates
    over `scale`, the largest entry positive.  Returns None where that slot is empty."""
    mp = _mp()
    ent = hook("scaled rows", [x for r in _f7_rows(mp, p7, scale) for x in r[:8]])
    A = [ent[8 * r:8 * r + 8] + [mp.mpf(1)] for r in range(7)]
    F1, F2, col = _gauss_jordan(mp, A)[:3]
    free = hook("null vectors", [F1[col[k]] for k in range(7)] + [F2[col[k]] for k in range(7)])
    for k in range(7):
        F1[col[k]], F2[col[k]] = free[k], free[7 + k]
    D = [F1[k] - F2[k] for k in range(9)]
    c0, c3 = _det3(F2), _det3(D)
    c1 = c2 = mp.mpf(0)
    for r in range(3):
        T = list(F2)
        T[3 * r:3 * r + 3] = D[3 * r:3 * r + 3]
        c1 += _det3(T)
        T = list(D)
        T[3 * r:3 * r + 3] = F2[3 * r:3 * r + 3]
        c2 += _det3(T)
    c0, c1, c2, c3 = hook("c0..c3", [c0, c1, c2, c3])
    branch, slot = which[0], which[1]
    if branch == "cubic":
        a, b, c = c2 / c3, c1 / c3, c0 / c3
        l0 = which[2]
        for _ in range(60):                         # the root of the (hooked) cubic next to the one the bisection lands on
            p, dp = ((l0 + a) * l0 + b) * l0 + c, (3 * l0 + 2 * a) * l0 + b
            if dp == 0:
                break
            step = p / dp
            l0 -= step
            if abs(step) <= mp.mpf(10) ** -(DIGITS - 3) * max(1, abs(l0)):
                break
        l0, = hook("first root", [l0])
        if slot == 0:
            l = l0
        else:
            qb = a + l0
            qb, qc = hook("qb, qc", [qb, b + qb * l0])
            t = hook("terms of the other roots", [qb * qb, 4 * qc])
            if t[0] - t[1] < 0:
                return None
            t = hook("terms of the other roots", [-qb, mp.sqrt(t[0] - t[1])])
            l, = hook("other roots", [(t[0] - t[1]) / 2 if slot == 1 else (t[0] + t[1]) / 2])
    elif branch == "quadratic":
        disc = c1 * c1 - 4 * c2 * c0
        if disc < 0:
            return None
        l, = hook("other roots", [(-c1 - mp.sqrt(disc)) / (2 * c2) if slot == 0 else (-c1 + mp.sqrt(disc)) / (2 * c2)])
    elif branch == "linear":
        l, = hook("other roots", [-c0 / c1])
    if branch == "infinity":                    # c3 vanishes: F1 - F2 itself, the root at infinity of this chart
        F = hook("F before unscaling", D)
    else:
        F = hook("F before unscaling", [l * F1[k] + (1 - l) * F2[k] for k in range(9)])
    return hook("normalised F", _unit_signed(mp, F))


def f7_route_plan(p7, scale):
    """what the route does on this sample at 50 digits: (branch, [which per filled slot], growth, cond, |null vectors|_inf); the
    first root of the cubic branch is the one 200 bisection steps inside the Cauchy bound land on"""
    mp = _mp()
    A = _f7_rows(mp, p7, scale)
    gj = _gauss_jordan(mp, A)
    if gj is None:
        return None
    F1, F2, col, growth, cond = gj
    D = [F1[k] - F2[k] for k in range(9)]
    c = _pencil_cubic(mp, F1, F2)            # (c3, c2, c1, c0): the same numbers as the route's expansion by rows
    c3, c2, c1, c0 = c
    cm = max(abs(x) for x in c)
    size = max(abs(x) for x in F1 + F2)
    if cm == 0:
        return ("none", [], growth, cond, size)
    if abs(c3) > mp.mpf(10) ** -14 * cm:
        a, b, cc = c2 / c3, c1 / c3, c0 / c3
        lo = -(1 + max(abs(a), abs(b), abs(cc)))
        hi = -lo
        for _ in range(400):
            mid = (lo + hi) / 2
            if ((mid + a) * mid + b) * mid + cc < 0:
                lo = mid
            else:
                hi = mid
        l0 = (lo + hi) / 2
        qb = a + l0
        disc = qb * qb - 4 * (b + qb * l0)
        plan = [("cubic", 0, l0)] + ([("cubic", 1, l0), ("cubic", 2, l0)] if disc >= 0 else [])
        return ("cubic", plan, growth, cond, size)
    # c3 vanishes (to the route's 1e-14): F1 - F2 is returned after the finite roots.  It is the solution only as far as c3 is zero:
    # the exact root is l = -c2 / c3 (+ ...), so the unit-norm F is off by at most 2 |c3 / c2| |F2| / |F1 - F2| and has det = c3 / |F1 - F2|^3;
    # both ride on the plan entry and are added to the slot's tolerance and det bound (f7_kappa_route)
    nD = mp.sqrt(sum(x * x for x in D))
    lead = c2 if abs(c2) > mp.mpf(10) ** -14 * cm else c1 if abs(c1) > mp.mpf(10) ** -14 * cm else c0
    inf = [("infinity", 0, _f(2 * abs(c3 / lead) * mp.sqrt(sum(x * x for x in F2)) / nD), _f(abs(c3) / nD ** 3))]
    def finite(branch, slot, l):
        """a finite root of the truncated polynomial: the same figures, against the root of the whole cubic next to it"""
        le = l
        for _ in range(60):
            step = (((c3 * le + c2) * le + c1) * le + c0) / ((3 * c3 * le + 2 * c2) * le + c1)
            le -= step
            if abs(step) <= mp.mpf(10) ** -(DIGITS - 3) * max(1, abs(le)):
                break
        Ft = _unit_signed(mp, [l * F1[k] + (1 - l) * F2[k] for k in range(9)])
        Fe = _unit_signed(mp, [le * F1[k] + (1 - le) * F2[k] for k in range(9)])
        return (branch, slot, _f(2 * max(abs(Ft[k] - Fe[k]) for k in range(9))), _f(abs(_det3(Ft))))
    if abs(c2) > mp.mpf(10) ** -14 * cm:
        disc = c1 * c1 - 4 * c2 * c0
        two = [finite("quadratic", 0, (-c1 - mp.sqrt(disc)) / (2 * c2)), finite("quadratic", 1, (-c1 + mp.sqrt(disc)) / (2 * c2))] if disc >= 0 else []
        return ("quadratic", two + inf, growth, cond, size)
    if abs(c1) > mp.mpf(10) ** -14 * cm:
        return ("linear", [finite("linear", 0, -c0 / c1)] + inf, growth, cond, size)
    return ("infinity", inf, growth, cond, size)


def f7_kappa_route(p7, scale, which, plan):
    """(kappa_route of one slot, {stage: share}, the same sum for det F of the returned model); the null vectors move by
    3 n rho cond_inf |x|_inf (n = 7).  det F does not see the stages before the cubic: the cubic is formed from the null vectors as
    they are, so its root makes THEIR pencil singular - what is left is the rounding from c0..c3 on."""
    _, _, growth, cond, size = plan
    weights = dict(F7_WEIGHTS)
    weights["null vectors"] = 3 * 7 * growth * cond

    def route(hook):
        F = f7_route(p7, scale, which, hook)
        return F + [_det3(F)]
    total, shares, extra = kappa_route(route, weights, absolute={"null vectors": size}, nout=9)
    if which[0] != "cubic":                     # what dropping c3 l^3 leaves in a root of the truncated polynomial, in units of 32 eps
        shares["c3 taken as zero"] = which[2] / (FACTOR * EPS)
        return total + shares["c3 taken as zero"], shares, float(extra[0]) + which[3] / (FACTOR * EPS)
    return total, shares, float(extra[0])


def f7_condition(p7, scale, F):
    """|d F / d (p7 / scale)|_2 of the solution F (unit norm; 9 x 28, differences of step 1e-20; the perturbed problem is solved from
    its definition with the Gauss-Jordan basis and the nearest solution is taken)"""
    mp = _mp()
    h = mp.mpf(10) ** -20
    base = [[mp.mpf(float(x)) / mp.mpf(float(scale)) for x in r] for r in p7]

    def solve(p):
        A = [[x2 * x1, x2 * y1, x2, y2 * x1, y2 * y1, y2, x1, y1, mp.mpf(1)] for x1, y1, x2, y2 in p]
        F1, F2 = _gauss_jordan(mp, A)[:2]
        sols = f7_solutions(F1, F2)
        return min(sols, key=lambda G: max(abs(G[k] - F[k]) for k in range(9)))
    J = np.zeros((9, 28))
    for r in range(7):
        for c in range(4):
            hi = [list(x) for x in base]
            hi[r][c] += h
            G = solve(hi)
            J[:, 4 * r + c] = [_f((G[k] - F[k]) / h) for k in range(9)]
    return _relative(J, [x for r in base for x in r], F)
