"""The cone type restated for its tests (test_cones_cpu.py, test_gpu_cones.py).  TEST INFRASTRUCTURE, never imported by the product.

* sq_cone: Residual<kCone3D> (csrc/residuals.hip.h) in numpy, operation for operation: the 3-D line's q (sq_line3d of
  line3d_filter_model.py), rho = sqrt(q), h = (e0 d0 + e1 d1) + e2 d2, |c rho - s h| and its square.  rho_h_rows and e_rows give the rows
  on which the oracle's 2-D line type with the model (c, -s, 0) and its plane type with the model (d, 0) evaluate the last step and h.
* solve_scalar: solve.hip's 3-point cone solver in scalar numpy floats, operation for operation.
* gn_rows / numpy_gram: fit.hip GenConeGn's rows in numpy and a Gram provider over them; f_value: the function they differentiate.
* gn_reference: plain Gauss-Newton on sum w (c rho - s h)^2 at 50 digits from the same start, with the condition number of its own 6x6
  normal matrix at the solution; refit_ratios compares a model with it and defines the parameters' scales.
* prep / reject / group_reject: Filter32<kCone3D> (csrc/score_filters.hip.h) in the header's operation order and with the header's
  literals (header_literals reads them out of the header's text), f32 arithmetic as in line3d_filter_model.py (mpmath at 24 bits, fma
  one rounding).
"""
import numpy as np

import line3d_filter_model as L3
from line3d_filter_model import EPS, cross_components, f32, f32_up, group_row, morton_order, point_row, sq_line3d  # noqa: F401
from pyprogressivex import _estimators, _lib


# ---- the exact path -----------------------------------------------------------------------------------------------------------------
def rho_h(pts, m):
    """(rho, h) of Residual<kCone3D>"""
    with np.errstate(invalid="ignore", over="ignore"):
        e0, e1, e2 = pts[:, 0] - m[0], pts[:, 1] - m[1], pts[:, 2] - m[2]
        rho = np.sqrt(sq_line3d(pts, m))
        h = (e0 * m[3] + e1 * m[4]) + e2 * m[5]
    return rho, h


def signed_cone(pts, m):
    rho, h = rho_h(pts, m)
    with np.errstate(invalid="ignore", over="ignore"):
        return m[6] * rho - m[7] * h


def sq_cone(pts, m):
    with np.errstate(invalid="ignore", over="ignore"):
        plain = np.abs(signed_cone(pts, m))
        return plain * plain


def rho_h_rows(pts, m):
    """[n, 2] rows (rho, h): the 2-D line (c, -s, 0) has the residual |(c rho + (-s) h) + 0| on them"""
    return np.ascontiguousarray(np.column_stack(rho_h(pts, m)))


def e_rows(pts, m):
    """[n, 3] rows e = x - a: the plane (d, 0) has the residual |((d0 e0 + d1 e1) + d2 e2) + 0| on them"""
    return np.ascontiguousarray(np.column_stack([pts[:, 0] - m[0], pts[:, 1] - m[1], pts[:, 2] - m[2]]))


# ---- the minimal solver ---------------------------------------------------------------------------------------------------------------
def _cross3(a, b):
    return [a[1] * b[2] - a[2] * b[1], -(a[0] * b[2] - a[2] * b[0]), a[0] * b[1] - a[1] * b[0]]


def _dot3(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def solve_scalar(p, n, rmin=0.0, rmax=np.inf):
    """solve_minimal(Type<kCone3D>) on numpy float64 scalars, p and n the three samples and their normals: the model [8] or None"""
    p = [np.asarray(v, dtype=np.float64) for v in p]
    n = [np.asarray(v, dtype=np.float64) for v in n]
    with np.errstate(all="ignore"):
        X = [_cross3(n[1], n[2]), _cross3(n[2], n[0]), _cross3(n[0], n[1])]
        det = _dot3(n[0], X[0])
        if det == 0.0:
            return None
        b = [_dot3(n[i], p[i]) for i in range(3)]
        a = [((b[0] * X[0][k] + b[1] * X[1][k]) + b[2] * X[2][k]) / det for k in range(3)]
        g = []
        for i in range(3):
            w = [p[i][0] - a[0], p[i][1] - a[1], p[i][2] - a[2]]
            ln = np.sqrt(_dot3(w, w))
            if not ln > 0.0:
                return None
            g.append([w[0] / ln, w[1] / ln, w[2] / ln])
        D = _cross3([g[1][k] - g[0][k] for k in range(3)], [g[2][k] - g[0][k] for k in range(3)])
        ln = np.sqrt(_dot3(D, D))
        if not ln > 0.0:
            return None
        d = [D[0] / ln, D[1] / ln, D[2] / ln]
        t = [_dot3(d, g[i]) for i in range(3)]
        if (t[0] + t[1]) + t[2] < 0.0:
            d = [-d[0], -d[1], -d[2]]
        c = _dot3(d, g[0])
        e = [g[0][0] - 0.0, g[0][1] - 0.0, g[0][2] - 0.0]
        c0 = e[1] * d[2] - e[2] * d[1]
        c1 = -(e[0] * d[2] - e[2] * d[0])
        c2 = e[0] * d[1] - e[1] * d[0]
        s = np.sqrt((c0 * c0 + c1 * c1) + c2 * c2)
        m = np.array([a[0], a[1], a[2], d[0], d[1], d[2], c, s])
        if not (np.isfinite(m).all() and c > 0.0 and s >= rmin and s <= rmax):
            return None
    return m


def on_cone(rng, cone, n, hlo=1.0, hhi=4.0):
    """n exact points of the cone (a, d, c, s) at heights in [hlo, hhi] and their outward unit normals c rhohat - s d"""
    a, d, c, s = cone[:3], cone[3:6], cone[6], cone[7]
    e1 = np.cross(d, [1.0, 0.0, 0.0] if abs(d[0]) < 0.9 else [0.0, 1.0, 0.0])
    e1 /= np.linalg.norm(e1)
    e2 = np.cross(d, e1)
    phi, h = rng.uniform(0, 2 * np.pi, n), rng.uniform(hlo, hhi, n)
    rad = np.cos(phi)[:, None] * e1 + np.sin(phi)[:, None] * e2
    return a + h[:, None] * d + (h * s / c)[:, None] * rad, c * rad - s * d


# ---- the Gauss-Newton rows ------------------------------------------------------------------------------------------------------------
def gn_rows(pts, prm, plant_sign=None):
    """GenConeGn's rows [n, 7] at prm = (a, d, c, s, u) and which points have none (bad); plant_sign = a column whose sign is reversed"""
    m, u = prm[:8], prm[8:11]
    c, s = m[6], m[7]
    v = _cross3(m[3:6], u)
    e0, e1, e2 = pts[:, 0] - m[0], pts[:, 1] - m[1], pts[:, 2] - m[2]
    c0, c1, c2 = cross_components(pts, m)
    with np.errstate(all="ignore"):
        rho = np.sqrt((c0 * c0 + c1 * c1) + c2 * c2)
        bad = ~(rho > 0.0) | ~np.isfinite(rho)
        h = (e0 * m[3] + e1 * m[4]) + e2 * m[5]
        g0 = c * ((e0 - h * m[3]) / rho) - s * m[3]
        g1 = c * ((e1 - h * m[4]) / rho) - s * m[4]
        g2 = c * ((e2 - h * m[5]) / rho) - s * m[5]
        gu = (g0 * u[0] + g1 * u[1]) + g2 * u[2]
        gv = (g0 * v[0] + g1 * v[1]) + g2 * v[2]
        gd = (g0 * m[3] + g1 * m[4]) + g2 * m[5]
        eu = (e0 * u[0] + e1 * u[1]) + e2 * u[2]
        ev = (e0 * v[0] + e1 * v[1]) + e2 * v[2]
        k = (c * h) / rho + s
        rows = np.column_stack([-gu, -gv, -gd, -(eu * k), -(ev * k), -(rho * s + h * c), c * rho - s * h])
    if plant_sign is not None:
        rows[:, plant_sign] = -rows[:, plant_sign]
    return rows, bad


def numpy_gram(pts, w=None, plant_sign=None, log=None):
    """a Gram provider for ConeEstimator._fit_many with one item over all of pts"""
    w = np.ones(len(pts)) if w is None else np.asarray(w, dtype=np.float64)

    def gram(kind, prm, use_w, wpow, rows):
        assert list(rows) == [0]
        if log is not None:
            log.append((kind, None if prm is None else prm.copy(), use_w, wpow))
        assert kind == _lib.GRAM_CONE_GN and prm.shape == (1, 11)
        A, bad = gn_rows(pts, prm[0], plant_sign)
        A, ww = A[~bad], w[~bad]
        return ((A * ww[:, None]).T @ A)[None], np.array([len(pts)]), np.array([int(bad.sum())])
    return gram


def chart(m):
    """(u, v) of the chart at the model m: _estimators._cylinder_frame's u and v = d x u"""
    u = _estimators._cylinder_frame(np.asarray(m[3:6], dtype=np.float64)[None])[0]
    return u, np.cross(m[3:6], u)


def f_value(pts, m, u, v, x):
    """f = c rho - s h at the chart point x = (alpha, beta, gamma, delta, eta, tau) about m"""
    a = m[:3] + x[0] * u + x[1] * v + x[2] * m[3:6]
    d = m[3:6] + x[3] * u + x[4] * v
    d = d / np.linalg.norm(d)
    cs = np.array([m[6] - x[5] * m[7], m[7] + x[5] * m[6]])
    cs = cs / np.linalg.norm(cs)
    e = pts - a
    return cs[0] * np.linalg.norm(np.cross(e, d), axis=1) - cs[1] * (e @ d)


# ---- the refit at 50 digits -----------------------------------------------------------------------------------------------------------
def refit_fixture(n, offset, weighted, seed):
    """n noisy points on an arc of at least a third of a cone of half-angle 15 .. 40 degrees between the heights 1 and 4, its apex
    `offset` from the origin, the true model and a start 1e-3 .. 1e-1.5 away from it (absolute in the apex, the direction and the angle)"""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=3)
    d /= np.linalg.norm(d)
    theta = np.deg2rad(rng.uniform(15.0, 40.0))
    c, s = np.cos(theta), np.sin(theta)
    apex = rng.uniform(3, 7, 3) + offset
    e1 = np.cross(d, rng.normal(size=3))
    e1 /= np.linalg.norm(e1)
    e2 = np.cross(d, e1)
    cov = rng.uniform(1.0 / 3.0, 1.0)
    h = np.sqrt(rng.uniform(1.0, 16.0, n))
    phi = rng.uniform(-np.pi * cov, np.pi * cov, n)
    if n == 6:                                               # six points in general position: spread over the arc and the heights
        h = np.array([1.0, 3.7, 1.9, 3.1, 1.3, 4.0])
        phi = np.array([-0.9, -0.55, -0.15, 0.2, 0.6, 0.95]) * np.pi * cov
    rad = np.cos(phi)[:, None] * e1 + np.sin(phi)[:, None] * e2
    pts = apex + h[:, None] * d + (h * s / c)[:, None] * rad + (c * rad - s * d) * rng.normal(0, 0.005, n)[:, None]
    w = rng.uniform(0.5, 1.5, n) if weighted else None
    gt = np.concatenate([apex, d, [c, s]])
    mag = 10.0 ** rng.uniform(-3, -1.5)
    start = gt.copy()
    start[:3] += mag * rng.normal(size=3) / np.sqrt(3)
    start[3:6] += mag * rng.normal(size=3) / np.sqrt(3)
    start[3:6] /= np.linalg.norm(start[3:6])
    t2 = theta + mag * rng.uniform(-1, 1)
    start[6:8] = np.cos(t2), np.sin(t2)
    return np.ascontiguousarray(pts), w, gt, start


def gn_reference(pts, w, start, iterations=80):
    """Plain Gauss-Newton on sum w (c rho - s h)^2 at 50 digits from `start`, in the chart of the estimator rebuilt at every iterate.
    Returns (a, d, (c, s), cond, converged): the apex, the unit direction, the unit (c, s) (floats, canonical: both entries of (c, s)
    positive), the 2-norm condition number of the 6x6 normal matrix at the solution and whether the last step was below 1e-30
    (fourteen orders below what float64 resolves)."""
    import mpmath
    mp = mpmath.mp.clone()
    mp.dps = 50
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

    def normal_equations(a, d, c, s, u, v):
        A, g = mp.zeros(6, 6), mp.zeros(6, 1)
        for wi, x in zip(ww, P):
            e = [x[k] - a[k] for k in range(3)]
            h = dot(e, d)
            r = [e[k] - h * d[k] for k in range(3)]
            rho = mp.sqrt(dot(r, r))
            gr = [c * r[k] / rho - s * d[k] for k in range(3)]
            kk = c * h / rho + s
            row = [-dot(gr, u), -dot(gr, v), -dot(gr, d), -dot(e, u) * kk, -dot(e, v) * kk, -(rho * s + h * c)]
            f = c * rho - s * h
            for i in range(6):
                wr = wi * row[i]
                g[i] += wr * f
                for j in range(i, 6):
                    A[i, j] += wr * row[j]
        for i in range(6):
            for j in range(i):
                A[i, j] = A[j, i]
        return A, g

    a = [mp.mpf(float(x)) for x in start[:3]]
    d = unit([mp.mpf(float(x)) for x in start[3:6]])
    c, s = unit([mp.mpf(float(x)) for x in start[6:8]])
    step = mp.mpf(1)
    for _ in range(iterations):
        u, v = frame(d)
        A, g = normal_equations(a, d, c, s, u, v)
        delta = mp.lu_solve(A, -g)
        a = [a[k] + delta[0] * u[k] + delta[1] * v[k] + delta[2] * d[k] for k in range(3)]
        d = unit([d[k] + delta[3] * u[k] + delta[4] * v[k] for k in range(3)])
        c, s = unit([c - delta[5] * s, s + delta[5] * c])
        step = mp.sqrt(sum(x * x for x in delta))
        if step < mp.mpf(10) ** -30:
            break
    u, v = frame(d)
    A, _ = normal_equations(a, d, c, s, u, v)
    sv = mp.svd_r(A, compute_uv=False)
    cond = float(max(sv) / min(sv))
    m = _estimators.ConeEstimator.canonical(np.array([[float(x) for x in a] + [float(x) for x in d] + [float(c), float(s)]]))[0]
    return m[:3], m[3:6], m[6:8], cond, bool(step < mp.mpf(10) ** -30)


def refit_ratios(model, ref, pts):
    """The fitted (canonical) model's distance from the reference in the chart's three parameter groups, each over its tolerance
    32 eps cond x scale: the apex (scale: the largest |coordinate| of the points, what x - a is formed from), the direction (scale 1: a
    unit vector with a sign of its own, into the nappe) and (c, s) (scale 1: a unit vector)."""
    a, d, cs, cond, _ = ref
    tol = 32.0 * EPS * cond
    return (float(np.linalg.norm(model[:3] - a)) / (tol * float(np.abs(pts).max())), float(np.linalg.norm(model[3:6] - d)) / tol,
            float(np.linalg.norm(model[6:8] - cs)) / tol)


# ---- the f32 filter -------------------------------------------------------------------------------------------------------------------
# the cone's shape, ConeShape32; the shared part (AxialFilter32) is line3d_filter_model's
MODEL_LITERALS = dict(L3.SHARED_LITERALS, e1=2.0, e0=2.0, floor=1e-18, e2=10.5, k_inflate=1.001, k1_min=0.0009765625, k1_max=1024.0)

_LITERAL_PATTERNS = [
    (("e1",), r"ln\.e1 = f32_up\(NUM \* u \* dn \* K\);"),
    (("e0", "floor"), r"ln\.e0 = big \? __builtin_inff\(\) : f32_up\(NUM \* u \* dn \* K \* pn \+ NUM \* \(K \+ 1\.0\)\);"),
    (("e2",), r"ln\.e2 = f32_up\(NUM \* u \* dn \* K\);"),
    (("k_inflate",), r"const double K = k1 \* NUM;"),
    (("k1_min", "k1_max"), r"const bool big = out \|\| !\(k1 >= NUM\) \|\| !\(k1 <= NUM\);"),
]

# the header's statements of the f32 test's operation order, as prep and _magnitude below restate them, behind the shared block's
OPERATION_LINES = L3.SHARED_OPERATION_LINES + [
    "ln.c = (float)m[6];",
    "ln.s = (float)m[7];",
    "const double k1 = fabs(m[6]) + fabs(m[7]);",
    "ln.nrm = f32_up(dn * sqrt(m[6] * m[6] + m[7] * m[7]));",
    "const float s = axial_dist(p, ln, l1);",
    "const float h = axial_height(p, ln);",
    "const float n = __builtin_fmaf(s, ln.c, -(h * ln.s));",
    "return fabsf(n);",
]


def header_block():
    return L3.axial_header_block("ConeShape32")


def header_literals():
    return L3.axial_header_literals("ConeShape32", _LITERAL_PATTERNS)


def prep(m, pscale, T2, plant_zero_budget=False, lit=None):
    """Filter32<kCone3D>::prep in float64, the lane's floats as Python floats holding f32 values"""
    L = MODEL_LITERALS if lit is None else lit

    def budget(ln, m, sc, dn, pn, u, out):
        ln["c"], ln["s"] = f32(m[6]), f32(m[7])
        k1 = np.float64(abs(m[6])) + abs(m[7])
        K = k1 * L["k_inflate"]
        big = out or not (k1 >= L["k1_min"]) or not (k1 <= L["k1_max"])
        ln["e1"] = f32_up(L["e1"] * u * dn * K)
        ln["e0"] = float("inf") if big else f32_up(L["e0"] * u * dn * K * pn + L["floor"] * (K + 1.0))
        ln["e2"] = f32_up(L["e2"] * u * dn * K)
        ln["nrm"] = f32_up(dn * np.sqrt(np.float64(m[6]) * m[6] + np.float64(m[7]) * m[7]))
    return L3.axial_prep(m, pscale, T2, L, budget, plant_zero_budget)


def _magnitude(row, ln):
    """ConeShape32::magnitude: (|n~|, l~)"""
    c = L3._mp24()
    s, l1 = L3._dist(row, ln)
    h = L3._height(row, ln)
    return abs(L3._fma(c, s, c.mpf(ln["c"]), -(h * c.mpf(ln["s"])))), l1


def reject(row, ln):
    """row = (x~, y~, z~, P): Filter32<kCone3D>::reject"""
    return L3.axial_reject(_magnitude, row, ln)


def group_reject(g, ln):
    """g = (centre[3], rho, Pmax): Filter32<kCone3D>::group_reject"""
    return L3.axial_group_reject(_magnitude, g, ln)


def sweep_is_crossed(seen):
    """seen = the (e, f, angle in whole degrees) of the cases a sweep ran: every scale of d met every angle and every scale of (c, s)"""
    return all({a for x, _, a in seen if x == e} == {2, 15, 30, 45, 75, 88} and {f for x, f, _ in seen if x == e} == {-8, 0, 3, 8}
               for e in (-40, 0, 40)) and {x for x, _, _ in seen} == {-40, 0, 40}


# ---- the cases the CPU and the GPU tests share ----
# the end-to-end scene: fixed on the CPU (test_cones_cpu.py) before the device runs it (test_gpu_cones.py)
E2E = dict(n_per_cone=800, n_cones=3, n_outliers=800, sigma=0.01, half_angle_deg=(15.0, 40.0), extent=(1.0, 4.0), normal_noise_deg=5.0)
REFIT_CASES = [(n, offset, weighted) for n in (6, 64, 1000) for offset in (0.0, 1e3) for weighted in (False, True)]


def random_cone(rng, coord, offset, angle_deg):
    d = rng.normal(size=3)
    d /= np.linalg.norm(d)
    t = np.deg2rad(angle_deg)
    return np.concatenate([rng.uniform(3, 7, 3) * coord + offset, d, [np.cos(t), np.sin(t)]])


def near_threshold_cases():
    """(rng, ground truth, T, exponent of d's scale, exponent of (c, s)'s scale, coordinate scale): coordinate scales 1, 1e3, 1e6, scenes
    at the origin, 1e3 scene scales and 1e6 units from it, thresholds 1e-3 .. 1 x nominal (and 1e1 x: larger ones leave no room beside
    the apex), half-angles 2 .. 88 degrees, d scaled by 2^-40 .. 2^40 and (c, s) by 2^-8 .. 2^8 by the caller; 81 cases in which every
    scale of d meets all six angles and all four scales of (c, s)"""
    rng = np.random.default_rng(37)
    k = 0
    for coord in (1.0, 1e3, 1e6):
        for offset in (0.0, 1e3 * coord, 1e6):
            for tf in (1e-3, 1.0, 1e1):
                for e in (-40, 0, 40):
                    # e is the innermost loop (k % 3): angle and (c, s) scale go by k // 3, so that every scale of d meets every
                    # angle and every scale of (c, s) (an index k % 6 would tie each d scale to two angles)
                    ang = (2.0, 15.0, 45.0, 75.0, 88.0, 30.0)[(k // 3) % 6]
                    f = (0, -8, 8, 3)[(k // 3 + k // 27) % 4]
                    k += 1
                    yield rng, random_cone(rng, coord, offset, ang), 1.5 * 0.05 * coord * tf, e, f, coord


def near_threshold_points(rng, cone, T, n, along):
    """n points whose signed distance to the generatrix of the unit cone (a, d, c, s) is +-T (1 +- 0.5e-4), outside and inside the nappe
    in turn, at heights between 2 T / min(c, s) + 0.2 along and that plus `along`: far enough from the apex and the axis that the foot lies
    on the nappe and rho stays positive"""
    a, d, c, s = np.asarray(cone[:3]), np.asarray(cone[3:6]), float(cone[6]), float(cone[7])
    e1 = np.cross(d, [1.0, 0.0, 0.0] if abs(d[0]) < 0.9 else [0.0, 1.0, 0.0])
    e1 /= np.linalg.norm(e1)
    e2 = np.cross(d, e1)
    phi = rng.uniform(0, 2 * np.pi, n)
    h0 = 2.0 * T / min(c, s) + 0.2 * along
    t = rng.uniform(h0, h0 + along, n)                       # position along the generatrix
    target = T * (1.0 + rng.uniform(-0.99e-4 / 2, 0.99e-4 / 2, n)) * np.where(np.arange(n) % 2 == 1, -1.0, 1.0)
    rad = np.cos(phi)[:, None] * e1 + np.sin(phi)[:, None] * e2
    return np.ascontiguousarray(a + (t * c - target * s)[:, None] * d + (t * s + target * c)[:, None] * rad)
