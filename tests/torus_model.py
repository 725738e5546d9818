"""The torus type restated for its tests (test_tori_cpu.py, test_gpu_tori.py).  TEST INFRASTRUCTURE, never imported by the product.

* sq_torus: Residual<kTorus3D> (csrc/residuals.hip.h) in numpy, operation for operation: the 3-D line's q (sq_line3d of
  line3d_filter_model.py), rho = sqrt(q), h = (e0 d0 + e1 d1) + e2 d2, t = rho - R, w = sqrt(t t + h h), |w - r| and its square.
  rho_h_rows and e_rows give the rows on which the oracle's 2-D circle type with the model (R, 0, r) and its plane type with the model
  (d, 0) evaluate the last step and h.
* solve_scalar: solve.hip's 4-point torus solver in scalar numpy floats, operation for operation, one slot.
* transversal_reference: the same answer by ANOTHER route at 50 digits - the null space of the four Pluecker incidence conditions and
  the Klein quadric for the axis, a linear system for the circle.  route_sensitivity: the product's route restated in mpmath with a
  hook at every stage interface, which gives the tolerance 32 eps kappa_route in the manner of DESIGN.md 4.5b.
* gn_rows / numpy_gram: fit.hip GenTorusGn's rows in numpy and a Gram provider over them; f_value: the function they differentiate.
* gn_reference: plain Gauss-Newton on sum w (w - r)^2 at 50 digits from the same start, with the condition number of its own 7x7 normal
  matrix at the solution; refit_ratios compares a model with it and defines the parameters' scales.
* prep / reject / group_reject: Filter32<kTorus3D> (csrc/score_filters.hip.h) in the header's operation order and with the header's
  literals (header_literals reads them out of the header's text), f32 arithmetic as in line3d_filter_model.py (mpmath at 24 bits, fma
  one rounding).
"""
import numpy as np

import line3d_filter_model as L3
from line3d_filter_model import EPS, cross_components, f32, f32_up, group_row, morton_order, point_row, sq_line3d  # noqa: F401
from pyprogressivex import _estimators, _lib


# ---- the exact path -----------------------------------------------------------------------------------------------------------------
def rho_h(pts, m):
    """(rho, h) of Residual<kTorus3D>"""
    with np.errstate(invalid="ignore", over="ignore"):
        e0, e1, e2 = pts[:, 0] - m[0], pts[:, 1] - m[1], pts[:, 2] - m[2]
        rho = np.sqrt(sq_line3d(pts, m))
        h = (e0 * m[3] + e1 * m[4]) + e2 * m[5]
    return rho, h


def signed_torus(pts, m):
    rho, h = rho_h(pts, m)
    with np.errstate(invalid="ignore", over="ignore"):
        t = rho - m[6]
        w = np.sqrt(t * t + h * h)
        return w - m[7]


def sq_torus(pts, m):
    with np.errstate(invalid="ignore", over="ignore"):
        plain = np.abs(signed_torus(pts, m))
        return plain * plain


def rho_h_rows(pts, m):
    """[n, 2] rows (rho, h): the 2-D circle (R, 0, r) has the residual |sqrt((rho - R)^2 + (h - 0)^2) - r| on them"""
    return np.ascontiguousarray(np.column_stack(rho_h(pts, m)))


def e_rows(pts, m):
    """[n, 3] rows e = x - c: the plane (d, 0) has the residual |((d0 e0 + d1 e1) + d2 e2) + 0| on them"""
    return np.ascontiguousarray(np.column_stack([pts[:, 0] - m[0], pts[:, 1] - m[1], pts[:, 2] - m[2]]))


# ---- the minimal solver ---------------------------------------------------------------------------------------------------------------
def _cross3(a, b):
    return [a[1] * b[2] - a[2] * b[1], -(a[0] * b[2] - a[2] * b[0]), a[0] * b[1] - a[1] * b[0]]


def _dot3(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def solve_scalar(p, n, slot, rmin=0.0, rmax=np.inf, Rmin=0.0, Rmax=np.inf):
    """solve_minimal(Type<kTorus3D>) on numpy float64 scalars, p and n the four samples and their normals: the model [8] or None"""
    p = [np.asarray(v, dtype=np.float64) for v in p]
    n = [np.asarray(v, dtype=np.float64) for v in n]
    with np.errstate(all="ignore"):
        q = [p[1][k] - p[0][k] for k in range(3)]
        A, B, C, D = [], [], [], []
        for i in (2, 3):
            g = [p[i][k] - p[0][k] for k in range(3)]
            X, Y = _cross3(n[i], g), _cross3(n[i], n[0])
            A.append(-_dot3(n[1], Y))
            B.append(-(_dot3(q, Y) + _dot3(n[0], X)))
            C.append(_dot3(n[1], X))
            D.append(_dot3(q, X))
        qa = B[1] * A[0] - A[1] * B[0]
        qb = ((B[1] * C[0] - A[1] * D[0]) - C[1] * B[0]) + D[1] * A[0]
        qc = D[1] * C[0] - C[1] * D[0]
        disc = qb * qb - (4.0 * qa) * qc
        if not disc >= 0.0 or qa == 0.0:
            return None
        sq = np.sqrt(disc)
        s = (-qb + sq) / (2.0 * qa) if slot == 0 else (-qb - sq) / (2.0 * qa)
        den = A[0] * s + C[0]
        if den == 0.0:
            return None
        t = -(B[0] * s + D[0]) / den
        a = [p[0][k] + s * n[0][k] for k in range(3)]
        b = [p[1][k] + t * n[1][k] for k in range(3)]
        Dv = [b[k] - a[k] for k in range(3)]
        ln = np.sqrt(_dot3(Dv, Dv))
        if not ln > 0.0:
            return None
        d = [Dv[k] / ln for k in range(3)]
        h, rho = [], []
        for k in range(3):
            e = [p[k][j] - a[j] for j in range(3)]
            h.append(_dot3(e, d))
            c0 = e[1] * d[2] - e[2] * d[1]
            c1 = -(e[0] * d[2] - e[2] * d[0])
            c2 = e[0] * d[1] - e[1] * d[0]
            rho.append(np.sqrt((c0 * c0 + c1 * c1) + c2 * c2))
        a10, a11, a20, a21 = h[1] - h[0], rho[1] - rho[0], h[2] - h[0], rho[2] - rho[0]
        g1, g2 = 0.5 * (a10 * a10 + a11 * a11), 0.5 * (a20 * a20 + a21 * a21)
        det = a10 * a21 - a11 * a20
        if det == 0.0:
            return None
        z0, z1 = (g1 * a21 - g2 * a11) / det, (a10 * g2 - a20 * g1) / det
        r = np.sqrt(z0 * z0 + z1 * z1)
        hc, R = h[0] + z0, rho[0] + z1
        m = np.array([a[0] + hc * d[0], a[1] + hc * d[1], a[2] + hc * d[2], d[0], d[1], d[2], R, r])
        if not (np.isfinite(m).all() and R > r and r >= rmin and r <= rmax and R >= Rmin and R <= Rmax):
            return None
    return m


def frame_of(d):
    e1 = np.cross(d, [1.0, 0.0, 0.0] if abs(d[0]) < 0.9 else [0.0, 1.0, 0.0])
    e1 /= np.linalg.norm(e1)
    return e1, np.cross(d, e1)


def on_torus(rng, torus, n, phi_range=(0.0, 2 * np.pi)):
    """n exact points of the torus (c, d, R, r) and their outward unit normals cos(theta) rhohat + sin(theta) d"""
    c, d, R, r = torus[:3], torus[3:6], torus[6], torus[7]
    e1, e2 = frame_of(d)
    phi, theta = rng.uniform(phi_range[0], phi_range[1], n), rng.uniform(0, 2 * np.pi, n)
    rad = np.cos(phi)[:, None] * e1 + np.sin(phi)[:, None] * e2
    nrm = np.cos(theta)[:, None] * rad + np.sin(theta)[:, None] * d
    return c + R * rad + r * nrm, nrm


def random_torus(rng, coord=1.0, offset=0.0, ratio=None):
    d = rng.normal(size=3)
    d /= np.linalg.norm(d)
    R = rng.uniform(0.8, 2.0) * coord
    r = rng.uniform(0.2, 0.5) * coord if ratio is None else R / ratio
    return np.concatenate([rng.uniform(3, 7, 3) * coord + offset, d, [R, r]])


def same_torus(m, gt, rel):
    """m is the torus gt within rel, relative to gt's R (d up to sign)"""
    R = gt[6]
    dd = min(np.linalg.norm(m[3:6] - gt[3:6]), np.linalg.norm(m[3:6] + gt[3:6]))
    return bool(np.linalg.norm(m[:3] - gt[:3]) <= rel * max(R, np.abs(gt[:3]).max()) and dd <= rel and abs(m[6] - R) <= rel * R
                and abs(m[7] - gt[7]) <= rel * R)


# ---- the solver by another route, at 50 digits -----------------------------------------------------------------------------------------
def _mp50():
    import mpmath
    mp = mpmath.mp.clone()
    mp.dps = 50
    return mp


def transversal_reference(p, n):
    """Every torus whose axis is a common transversal of the four lines (p_i, n_i) and whose tube circle passes through samples 0, 1, 2,
    at 50 digits and NOT by the product's route: a line with direction l and moment m meets the line (n_i, p_i x n_i) iff
    l . (p_i x n_i) + m . n_i = 0; the four conditions leave a 2-dimensional null space of Pluecker vectors (the eigenvectors of the two
    smallest eigenvalues of A^T A), and the members that are lines satisfy the Klein quadric l . m = 0, a homogeneous quadratic on the
    pencil.  Per real root: the axis (point l x m / l.l, direction l / |l|), the samples' (h, rho) about it, and the circle
    h^2 + rho^2 + D h + E rho + F = 0 through three of them as a 3x3 linear system.  Returns a list of (c, d, R, r) as floats, not
    filtered by any range, with the relative gap of the null space as a conditioning figure."""
    mp = _mp50()
    P = [[mp.mpf(float(x)) for x in v] for v in p]
    N = [[mp.mpf(float(x)) for x in v] for v in n]

    def cross(a, b):
        return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]

    def dot(a, b):
        return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]

    A = mp.zeros(4, 6)
    for i in range(4):
        mom = cross(P[i], N[i])
        nn = mp.sqrt(dot(N[i], N[i]) + dot(mom, mom))
        for k in range(3):
            A[i, k] = mom[k] / nn
            A[i, 3 + k] = N[i][k] / nn
    ev, V = mp.eigsy(A.T * A)
    order = sorted(range(6), key=lambda k: ev[k])
    x1 = [V[k, order[0]] for k in range(6)]
    x2 = [V[k, order[1]] for k in range(6)]
    gap = float(ev[order[2]] / ev[order[5]])
    q11, q22 = dot(x1[:3], x1[3:]), dot(x2[:3], x2[3:])
    q12 = (dot(x1[:3], x2[3:]) + dot(x2[:3], x1[3:])) / 2
    # q11 al^2 + 2 q12 al be + q22 be^2 = 0 on x = al x1 + be x2
    disc = q12 * q12 - q11 * q22
    if disc < 0:
        return [], gap
    sq = mp.sqrt(disc)
    if abs(q11) >= abs(q22):
        roots = [((-q12 + sg * sq) / q11, mp.mpf(1)) for sg in (1, -1)] if q11 != 0 else []
    else:
        roots = [(mp.mpf(1), (-q12 + sg * sq) / q22) for sg in (1, -1)]
    out = []
    for al, be in roots:
        x = [al * x1[k] + be * x2[k] for k in range(6)]
        l, m = x[:3], x[3:]
        ll = dot(l, l)
        if ll == 0:
            continue
        pt = [v / ll for v in cross(l, m)]
        ln = mp.sqrt(ll)
        d = [v / ln for v in l]
        hr = []
        for k in range(3):
            e = [P[k][j] - pt[j] for j in range(3)]
            h = dot(e, d)
            perp = [e[j] - h * d[j] for j in range(3)]
            hr.append((h, mp.sqrt(dot(perp, perp))))
        M = mp.matrix([[h, rho, 1] for h, rho in hr])
        rhs = mp.matrix([-(h * h + rho * rho) for h, rho in hr])
        try:
            sol = mp.lu_solve(M, rhs)
        except ZeroDivisionError:
            continue
        hc, R = -sol[0] / 2, -sol[1] / 2
        r2 = hc * hc + R * R - sol[2]
        if r2 < 0:
            continue
        c = [pt[j] + hc * d[j] for j in range(3)]
        out.append(np.array([float(v) for v in c] + [float(v) for v in d] + [float(R), float(mp.sqrt(r2))]))
    return out, gap


# the product's route with a hook behind every stage: (name, outputs, roundings on the stage's longest chain, counted from solve.hip)
ROUTE_STAGES = [("coefficients", 8, 7),     # a difference, a cross product (2), a dot product (3), the sum of two of them
                ("quadratic terms", 8, 2),  # the eight products of qa, qb, qc, each summed at most three times: charged per term
                ("quadratic", 3, 3),
                ("root terms", 2, 4),       # -qb; qb qb, 4 qa qc, their difference, the root
                ("s", 1, 2), ("t", 1, 5), ("a, b", 6, 2), ("d", 3, 7), ("h, rho", 6, 8), ("circle", 3, 9), ("c, R", 4, 2)]


def _route_mp(mp, P, N, slot, delta):
    def hook(stage, vals):
        dl = delta.get(stage)
        return [v * (1 + dl[i]) for i, v in enumerate(vals)] if dl is not None else vals

    def cross(a, b):
        return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]

    def dot(a, b):
        return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]

    q = [P[1][k] - P[0][k] for k in range(3)]
    co = []
    for i in (2, 3):
        g = [P[i][k] - P[0][k] for k in range(3)]
        X, Y = cross(N[i], g), cross(N[i], N[0])
        co += [-dot(N[1], Y), -(dot(q, Y) + dot(N[0], X)), dot(N[1], X), dot(q, X)]
    A1, B1, C1, D1, A2, B2, C2, D2 = hook("coefficients", co)
    tm = hook("quadratic terms", [B2 * A1, A2 * B1, B2 * C1, A2 * D1, C2 * B1, D2 * A1, D2 * C1, C2 * D1])
    qa, qb, qc = hook("quadratic", [tm[0] - tm[1], ((tm[2] - tm[3]) - tm[4]) + tm[5], tm[6] - tm[7]])
    mqb, sq = hook("root terms", [-qb, mp.sqrt(qb * qb - 4 * qa * qc)])
    s, = hook("s", [(mqb + sq) / (2 * qa) if slot == 0 else (mqb - sq) / (2 * qa)])
    t, = hook("t", [-(B1 * s + D1) / (A1 * s + C1)])
    ab = hook("a, b", [P[0][k] + s * N[0][k] for k in range(3)] + [P[1][k] + t * N[1][k] for k in range(3)])
    a = ab[:3]
    Dv = [ab[3 + k] - a[k] for k in range(3)]
    ln = mp.sqrt(dot(Dv, Dv))
    d = hook("d", [v / ln for v in Dv])
    hr = []
    for k in range(3):
        e = [P[k][j] - a[j] for j in range(3)]
        cr = cross(e, d)
        hr += [dot(e, d), mp.sqrt(dot(cr, cr))]
    h0, r0, h1, r1, h2, r2 = hook("h, rho", hr)
    a10, a11, a20, a21 = h1 - h0, r1 - r0, h2 - h0, r2 - r0
    g1, g2 = (a10 * a10 + a11 * a11) / 2, (a20 * a20 + a21 * a21) / 2
    det = a10 * a21 - a11 * a20
    z0 = (g1 * a21 - g2 * a11) / det
    z1 = (a10 * g2 - a20 * g1) / det
    z0, z1, r = hook("circle", [z0, z1, mp.sqrt(z0 * z0 + z1 * z1)])
    hc = h0 + z0
    out = hook("c, R", [a[k] + hc * d[k] for k in range(3)] + [r0 + z1])
    return out[:3], d, out[3], r


def route_sensitivity(p, n, slot):
    """(model at 50 digits by the product's route, kappa_route per parameter group): kappa = sum over the stages of
    w x max_i sum_j |d out_i / d delta_j| with delta a relative perturbation of the stage's j-th output (differences of step 1e-20), the
    outputs scaled as same_torus and the tests scale them: the centre by max(R, the largest |coordinate| of the samples), the direction
    by 1, both radii by R."""
    mp = _mp50()
    P = [[mp.mpf(float(x)) for x in v] for v in p]
    N = [[mp.mpf(float(x)) for x in v] for v in n]
    c0, d0, R0, r0 = _route_mp(mp, P, N, slot, {})
    scale_c = max(R0, max(abs(x) for v in P for x in v))
    step = mp.mpf(10) ** -20

    def groups(res):
        c, d, R, r = res
        return [[(c[k] - c0[k]) / scale_c for k in range(3)], [d[k] - d0[k] for k in range(3)], [(R - R0) / R0, (r - r0) / R0]]

    kappa = [mp.mpf(0)] * 3
    for name, nout, w in ROUTE_STAGES:
        sums = None
        for j in range(nout):
            dl = [mp.mpf(0)] * nout
            dl[j] = step
            gr = groups(_route_mp(mp, P, N, slot, {name: dl}))
            ab = [[abs(x) / step for x in g] for g in gr]
            sums = ab if sums is None else [[x + y for x, y in zip(g0, g1)] for g0, g1 in zip(sums, ab)]
        kappa = [kappa[k] + w * max(sums[k]) for k in range(3)]
    model = np.array([float(v) for v in c0] + [float(v) for v in d0] + [float(R0), float(r0)])
    return model, [float(k) for k in kappa]


def route_ratios(m, ref, kappa, p):
    """the model's distance from the reference in the three groups over 32 eps kappa_route"""
    scale_c = max(ref[6], float(np.abs(np.asarray(p)).max()))
    dd = min(np.linalg.norm(m[3:6] - ref[3:6]), np.linalg.norm(m[3:6] + ref[3:6]))
    err = (float(np.linalg.norm(m[:3] - ref[:3])) / scale_c, float(dd), float(max(abs(m[6] - ref[6]), abs(m[7] - ref[7])) / ref[6]))
    return tuple(e / (32.0 * EPS * k) for e, k in zip(err, kappa))


# ---- the Gauss-Newton rows ------------------------------------------------------------------------------------------------------------
def gn_rows(pts, prm, plant_sign=None):
    """GenTorusGn's rows [n, 8] at prm = (c, d, R, r, u) and which points have none (bad); plant_sign = a column whose sign is reversed"""
    m, u = prm[:8], prm[8:11]
    R, r = m[6], m[7]
    v = _cross3(m[3:6], u)
    e0, e1, e2 = pts[:, 0] - m[0], pts[:, 1] - m[1], pts[:, 2] - m[2]
    c0, c1, c2 = cross_components(pts, m)
    with np.errstate(all="ignore"):
        rho = np.sqrt((c0 * c0 + c1 * c1) + c2 * c2)
        bad = ~(rho > 0.0) | ~np.isfinite(rho)
        h = (e0 * m[3] + e1 * m[4]) + e2 * m[5]
        t = rho - R
        w = np.sqrt(t * t + h * h)
        bad |= ~(w > 0.0) | ~np.isfinite(w)
        tw, hw = t / w, h / w
        g0 = tw * ((e0 - h * m[3]) / rho) + hw * m[3]
        g1 = tw * ((e1 - h * m[4]) / rho) + hw * m[4]
        g2 = tw * ((e2 - h * m[5]) / rho) + hw * m[5]
        gu = (g0 * u[0] + g1 * u[1]) + g2 * u[2]
        gv = (g0 * v[0] + g1 * v[1]) + g2 * v[2]
        gd = (g0 * m[3] + g1 * m[4]) + g2 * m[5]
        eu = (e0 * u[0] + e1 * u[1]) + e2 * u[2]
        ev = (e0 * v[0] + e1 * v[1]) + e2 * v[2]
        k = (h * R) / (w * rho)
        rows = np.column_stack([-gu, -gv, -gd, eu * k, ev * k, -tw, np.full(len(pts), -1.0), w - r])
    if plant_sign is not None:
        rows[:, plant_sign] = -rows[:, plant_sign]
    return rows, bad


def numpy_gram(pts, w=None, plant_sign=None, log=None):
    """a Gram provider for TorusEstimator._fit_many with one item over all of pts"""
    w = np.ones(len(pts)) if w is None else np.asarray(w, dtype=np.float64)

    def gram(kind, prm, use_w, wpow, rows):
        assert list(rows) == [0]
        if log is not None:
            log.append((kind, None if prm is None else prm.copy(), use_w, wpow))
        assert kind == _lib.GRAM_TORUS_GN and prm.shape == (1, 11)
        A, bad = gn_rows(pts, prm[0], plant_sign)
        A, ww = A[~bad], w[~bad]
        return ((A * ww[:, None]).T @ A)[None], np.array([len(pts)]), np.array([int(bad.sum())])
    return gram


def chart(m):
    """(u, v) of the chart at the model m: _estimators._cylinder_frame's u and v = d x u"""
    u = _estimators._cylinder_frame(np.asarray(m[3:6], dtype=np.float64)[None])[0]
    return u, np.cross(m[3:6], u)


# ---- the refit at 50 digits -----------------------------------------------------------------------------------------------------------
def refit_fixture(n, offset, weighted, seed):
    """n noisy points on at least a third of the ring (and the whole tube) of a torus with R in (0.8, 2) and r in (0.2, 0.5), its centre
    `offset` from the origin, the true model and a start 1e-3 .. 1e-1.5 away from it (absolute in the centre and the direction, relative
    to R in the radii)"""
    rng = np.random.default_rng(seed)
    gt = random_torus(rng, offset=offset)
    cov = rng.uniform(1.0 / 3.0, 1.0)
    if n == 7:                                               # seven points in general position: spread over the ring and the tube
        e1, e2 = frame_of(gt[3:6])
        phi = np.array([-0.9, -0.6, -0.3, 0.0, 0.3, 0.6, 0.9]) * np.pi * cov
        theta = np.array([0.3, 2.5, 4.4, 1.2, 5.6, 3.4, 0.9])
        rad = np.cos(phi)[:, None] * e1 + np.sin(phi)[:, None] * e2
        nrm = np.cos(theta)[:, None] * rad + np.sin(theta)[:, None] * gt[3:6]
        pts = gt[:3] + gt[6] * rad + gt[7] * nrm
    else:
        pts, nrm = on_torus(rng, gt, n, (-np.pi * cov, np.pi * cov))
    pts = pts + nrm * rng.normal(0, 0.005, n)[:, None]
    w = rng.uniform(0.5, 1.5, n) if weighted else None
    mag = 10.0 ** rng.uniform(-3, -1.5)
    start = gt.copy()
    start[:3] += mag * rng.normal(size=3) / np.sqrt(3)
    start[3:6] += mag * rng.normal(size=3) / np.sqrt(3)
    start[3:6] /= np.linalg.norm(start[3:6])
    start[6] *= 1.0 + mag * rng.uniform(-1, 1)
    start[7] += gt[6] * mag * rng.uniform(-0.2, 0.2)
    return np.ascontiguousarray(pts), w, gt, start


def gn_reference(pts, w, start, iterations=80):
    """Plain Gauss-Newton on sum w (sqrt((rho - R)^2 + h^2) - r)^2 at 50 digits from `start`, in the chart of the estimator rebuilt at
    every iterate; the Jacobian is written from the chain rule on (rho, h) and is checked against differences of the 50-digit f in
    test_tori_cpu.py.  Returns (c, d, (R, r), cond, converged): the 2-norm condition number of the 7x7 normal matrix at the solution and
    whether the last step was below 1e-30."""
    mp = _mp50()
    P = [[mp.mpf(float(x)) for x in row] for row in np.asarray(pts, dtype=np.float64)]
    ww = [mp.mpf(1)] * len(P) if w is None else [mp.mpf(float(x)) for x in w]

    def cross(a, b):
        return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]

    def dot(a, b):
        return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]

    def unit(a):
        ln = mp.sqrt(sum(x * x for x in a))
        return [x / ln for x in a]

    def frame(d):
        k = min(range(3), key=lambda j: abs(d[j]))
        ax = [mp.mpf(0)] * 3
        ax[k] = mp.mpf(1)
        u = unit(cross(ax, d))
        return u, cross(d, u)

    def normal_equations(c, d, R, r, u, v):
        A, g = mp.zeros(7, 7), mp.zeros(7, 1)
        for wi, x in zip(ww, P):
            e = [x[k] - c[k] for k in range(3)]
            h = dot(e, d)
            perp = [e[k] - h * d[k] for k in range(3)]
            rho = mp.sqrt(dot(perp, perp))
            t = rho - R
            wd = mp.sqrt(t * t + h * h)
            # df/drho = t / wd, df/dh = h / wd; moving c by z: drho = -rhohat . z, dh = -d . z; tilting d by del u: dh = del e.u,
            # drho = -del h e.u / rho
            frho, fh = t / wd, h / wd
            rhat = [perp[k] / rho for k in range(3)]
            row = [-(frho * dot(rhat, u) + fh * dot(d, u)), -(frho * dot(rhat, v) + fh * dot(d, v)), -(frho * dot(rhat, d) + fh),
                   (fh - frho * h / rho) * dot(e, u), (fh - frho * h / rho) * dot(e, v), -frho, mp.mpf(-1)]
            f = wd - r
            for i in range(7):
                wr = wi * row[i]
                g[i] += wr * f
                for j in range(i, 7):
                    A[i, j] += wr * row[j]
        for i in range(7):
            for j in range(i):
                A[i, j] = A[j, i]
        return A, g

    c = [mp.mpf(float(x)) for x in start[:3]]
    d = unit([mp.mpf(float(x)) for x in start[3:6]])
    R, r = mp.mpf(float(start[6])), mp.mpf(float(start[7]))
    step = mp.mpf(1)
    for _ in range(iterations):
        u, v = frame(d)
        A, g = normal_equations(c, d, R, r, u, v)
        delta = mp.lu_solve(A, -g)
        c = [c[k] + delta[0] * u[k] + delta[1] * v[k] + delta[2] * d[k] for k in range(3)]
        d = unit([d[k] + delta[3] * u[k] + delta[4] * v[k] for k in range(3)])
        R, r = R + delta[5], r + delta[6]
        step = mp.sqrt(sum(x * x for x in delta))
        if step < mp.mpf(10) ** -30:
            break
    u, v = frame(d)
    A, _ = normal_equations(c, d, R, r, u, v)
    sv = mp.svd_r(A, compute_uv=False)
    cond = float(max(sv) / min(sv))
    return (np.array([float(x) for x in c]), np.array([float(x) for x in d]), np.array([float(R), float(r)]), cond,
            bool(step < mp.mpf(10) ** -30))


_REFIT_CACHE = {}


def refit_case(n, offset, weighted):
    """(pts, w, gt, start, 50-digit reference) of one of REFIT_CASES, computed once per process: the CPU and the GPU tests share it"""
    key = (n, offset, weighted)
    if key not in _REFIT_CACHE:
        pts, w, gt, start = refit_fixture(n, offset, weighted, seed=n + int(offset) + weighted)
        _REFIT_CACHE[key] = (pts, w, gt, start, gn_reference(pts, w, start))
    return _REFIT_CACHE[key]


def f_value_mp(pts, m, u, v, x):
    """f = w - r at 50 digits at the chart point x = (alpha, beta, gamma, delta, eta, dR, dr) about m, per point (mpmath numbers)"""
    mp = _mp50()
    M = [mp.mpf(float(t)) for t in m]
    U, V, X = [mp.mpf(float(t)) for t in u], [mp.mpf(float(t)) for t in v], [mp.mpf(t) for t in x]
    c = [M[k] + X[0] * U[k] + X[1] * V[k] + X[2] * M[3 + k] for k in range(3)]
    d = [M[3 + k] + X[3] * U[k] + X[4] * V[k] for k in range(3)]
    ln = mp.sqrt(sum(t * t for t in d))
    d = [t / ln for t in d]
    out = []
    for row in pts:
        e = [mp.mpf(float(row[k])) - c[k] for k in range(3)]
        h = sum(e[k] * d[k] for k in range(3))
        perp = [e[k] - h * d[k] for k in range(3)]
        rho = mp.sqrt(sum(t * t for t in perp))
        out.append(mp.sqrt((rho - (M[6] + X[5])) ** 2 + h * h) - (M[7] + X[6]))
    return out


def refit_ratios(model, ref, pts):
    """The fitted model's distance from the reference in the chart's three parameter groups, each over its tolerance
    32 eps cond x scale: the centre (scale: the largest |coordinate| of the points, what x - c is formed from), the direction (scale 1,
    up to sign: d has none of its own) and the radii (scale R)."""
    c, d, Rr, cond, _ = ref
    tol = 32.0 * EPS * cond
    dd = min(float(np.linalg.norm(model[3:6] - d)), float(np.linalg.norm(model[3:6] + d)))
    return (float(np.linalg.norm(model[:3] - c)) / (tol * float(np.abs(pts).max())), dd / tol,
            float(np.linalg.norm(model[6:8] - Rr)) / (tol * float(Rr[0])))


# ---- the f32 filter -------------------------------------------------------------------------------------------------------------------
# the torus' shape, TorusShape32; the shared part (AxialFilter32) is line3d_filter_model's
MODEL_LITERALS = dict(L3.SHARED_LITERALS, e1=4.0, e0=2.0, e0_pn=2.0, e0_R=3.0, floor=2e-18, e2=18.0, R_max=1e17, r_max=1e17)

_LITERAL_PATTERNS = [
    (("e1",), r"ln\.e1 = f32_up\(NUM \* u \* dn\);"),
    (("e0", "e0_pn", "e0_R", "floor"),
     r"ln\.e0 = big \? __builtin_inff\(\) : f32_up\(NUM \* u \* \(\(NUM \* dn \* pn \+ NUM \* fabs\(R\)\) \+ fabs\(r\)\) \+ NUM\);"),
    (("e2",), r"ln\.e2 = f32_up\(NUM \* u \* dn\);"),
    (("R_max", "r_max"), r"const bool big = out \|\| !\(fabs\(R\) <= NUM\) \|\| !\(fabs\(r\) <= NUM\);"),
]

# the header's statements of the f32 test's operation order, as prep and _magnitude below restate them, behind the shared block's
OPERATION_LINES = L3.SHARED_OPERATION_LINES + [
    "const double R = m[6] * sc, r = m[7] * sc;",
    "ln.R = (float)R;",
    "ln.r = (float)r;",
    "ln.nrm = f32_up(dn);",
    "const float s = axial_dist(p, ln, l1);",
    "const float h = axial_height(p, ln);",
    "const float t = s - ln.R;",
    "const float w = sqrtf(__builtin_fmaf(t, t, h * h));",
    "return fabsf(w - ln.r);",
]


def header_block():
    return L3.axial_header_block("TorusShape32")


def header_literals():
    return L3.axial_header_literals("TorusShape32", _LITERAL_PATTERNS)


def prep(m, pscale, T2, plant_zero_budget=False, lit=None):
    """Filter32<kTorus3D>::prep in float64, the lane's floats as Python floats holding f32 values"""
    L = MODEL_LITERALS if lit is None else lit

    def budget(ln, m, sc, dn, pn, u, out):
        R, r = np.float64(m[6]) * sc, np.float64(m[7]) * sc
        ln["R"], ln["r"] = f32(R), f32(r)
        big = out or not (abs(R) <= L["R_max"]) or not (abs(r) <= L["r_max"])
        ln["e1"] = f32_up(L["e1"] * u * dn)
        ln["e0"] = float("inf") if big else f32_up(L["e0"] * u * ((L["e0_pn"] * dn * pn + L["e0_R"] * abs(R)) + abs(r)) + L["floor"])
        ln["e2"] = f32_up(L["e2"] * u * dn)
        ln["nrm"] = f32_up(dn)
    return L3.axial_prep(m, pscale, T2, L, budget, plant_zero_budget)


def _magnitude(row, ln):
    """TorusShape32::magnitude: (|n~|, l~)"""
    c = L3._mp24()
    s, l1 = L3._dist(row, ln)
    h = L3._height(row, ln)
    t = s - c.mpf(ln["R"])
    w = c.sqrt(L3._fma(c, t, t, h * h))
    return abs(w - c.mpf(ln["r"])), l1


def reject(row, ln):
    """row = (x~, y~, z~, P): Filter32<kTorus3D>::reject"""
    return L3.axial_reject(_magnitude, row, ln)


def group_reject(g, ln):
    """g = (centre[3], rho, Pmax): Filter32<kTorus3D>::group_reject"""
    return L3.axial_group_reject(_magnitude, g, ln)


RATIOS = (1.05, 2.0, 5.0, 20.0, 50.0)
D_EXPONENTS = (-40, 0, 40)


def sweep_is_crossed(seen):
    """seen = the (exponent of d's scale, R / r, coordinate scale, offset class) of the cases a sweep ran: every scale of d met every
    ratio, and every coordinate scale met every offset"""
    return (all({q for x, q, _, _ in seen if x == e} == set(RATIOS) for e in D_EXPONENTS) and {x for x, _, _, _ in seen} == set(D_EXPONENTS)
            and {(c, o) for _, _, c, o in seen} == {(c, o) for c in (1.0, 1e3, 1e6) for o in (0, 1, 2)})


# ---- the cases the CPU and the GPU tests share ----
# the end-to-end scene: fixed on the CPU (test_tori_cpu.py) before the device runs it (test_gpu_tori.py)
E2E = dict(n_per_torus=800, n_tori=2, n_outliers=800, sigma=0.01, major_radius=(0.8, 2.0), minor_radius=(0.2, 0.5), normal_noise_deg=2.0)
E2E_SEEDS = (0, 1, 2)
E2E_T = 0.05
REFIT_CASES = [(n, offset, weighted) for n in (7, 64, 1000) for offset in (0.0, 1e3) for weighted in (False, True)]


def near_threshold_cases():
    """(rng, ground truth, T, exponent of d's scale, R / r, coordinate scale, offset class): coordinate scales 1, 1e3, 1e6, scenes at
    the origin, 1e3 scene scales and 1e6 units from it, thresholds 1e-3 x, 1 x nominal and half the tube radius, R / r from 1.05 to 50,
    d scaled by 2^-40 .. 2^40 by the caller (the caller divides R, r and T by the same factor's inverse: see scaled_model); 81 cases
    in which every scale of d meets all five ratios"""
    rng = np.random.default_rng(41)
    k = 0
    for coord in (1.0, 1e3, 1e6):
        for oc, offset in enumerate((0.0, 1e3 * coord, 1e6)):
            for tf in (1e-3, 1.0, None):
                for e in D_EXPONENTS:
                    ratio = RATIOS[(k // 3) % 5]
                    k += 1
                    gt = random_torus(rng, coord, offset, ratio)
                    T = 0.5 * gt[7] if tf is None else min(1.5 * 0.05 * coord * tf, 0.5 * gt[7])
                    yield rng, gt, T, e, ratio, coord, oc


def scaled_model(gt, T, e):
    """the torus gt with d times 2^e: the residual is homogeneous in (d, R, r) together, so R, r and T are multiplied along and the
    inlier sets are those of (gt, T)"""
    f = float(np.ldexp(1.0, e))
    m = np.array(gt, dtype=np.float64, copy=True)
    m[3:8] *= f
    return m, T * f


def near_threshold_points(rng, torus, T, n, arc=2 * np.pi):
    """n points whose signed distance to the surface of the unit-direction ring torus is +-T (1 +- 0.5e-4), outside and inside the tube
    in turn, anywhere on the tube and on an arc of `arc` radians of the ring (T <= r / 2, so that the inner ones stay off the spine)"""
    c, d, R, r = np.asarray(torus[:3]), np.asarray(torus[3:6]), float(torus[6]), float(torus[7])
    e1, e2 = frame_of(d)
    phi, theta = rng.uniform(0, arc, n), rng.uniform(0, 2 * np.pi, n)
    target = T * (1.0 + rng.uniform(-0.99e-4 / 2, 0.99e-4 / 2, n)) * np.where(np.arange(n) % 2 == 1, -1.0, 1.0)
    rad = np.cos(phi)[:, None] * e1 + np.sin(phi)[:, None] * e2
    nrm = np.cos(theta)[:, None] * rad + np.sin(theta)[:, None] * d
    return np.ascontiguousarray(c + R * rad + (r + target)[:, None] * nrm)
