"""The cylinder type restated for its tests (test_cylinders_cpu.py, test_gpu_cylinders.py).  TEST INFRASTRUCTURE, never imported by the
product.

* sq_cylinder: Residual<kCylinder3D> (csrc/residuals.hip.h) in numpy, operation for operation: the 3-D line's q (sq_line3d of
  line3d_filter_model.py), then |sqrt(q) - r| and its square.  cross_rows gives the rows C = e x d on which the oracle's sphere type
  with the model (0, 0, 0, r) evaluates that last step bit for bit (C - 0 is exact).
* solve_scalar: solve.hip's 2-point cylinder solver in scalar Python floats, operation for operation.
* gn_rows / numpy_gram: fit.hip GenCylGn's rows in numpy and a Gram provider over them; f_value: the function they differentiate.
* gn_reference: plain Gauss-Newton on sum w (|(x - p) x d| - r)^2 at 50 digits from the same start, with the condition number of its
  own 5x5 normal matrix at the solution; refit_ratios compares a model with it.
* prep / reject / group_reject: Filter32<kCylinder3D> (csrc/score_filters.hip.h) in the header's operation order and with the header's
  literals (header_literals reads them out of the header's text), f32 arithmetic as in line3d_filter_model.py (mpmath at 24 bits, fma
  one rounding).
"""
import numpy as np

import line3d_filter_model as L3
from line3d_filter_model import EPS, cross_components, f32, f32_up, group_row, morton_order, point_row, sq_line3d  # noqa: F401
from pyprogressivex import _estimators, _lib


# ---- the exact path -----------------------------------------------------------------------------------------------------------------
def sq_cylinder(pts, m):
    with np.errstate(invalid="ignore", over="ignore"):
        plain = np.abs(np.sqrt(sq_line3d(pts, m)) - m[6])
        return plain * plain


def cross_rows(pts, m):
    """C = e x d in cross3's component order, [n, 3]"""
    return np.ascontiguousarray(np.column_stack(cross_components(pts, m)))


# ---- the minimal solver ---------------------------------------------------------------------------------------------------------------
def _cross3(a, b):
    return [a[1] * b[2] - a[2] * b[1], -(a[0] * b[2] - a[2] * b[0]), a[0] * b[1] - a[1] * b[0]]


def solve_scalar(a, b, na, nb, rmin=0.0, rmax=np.inf):
    """solve_minimal(Type<kCylinder3D>) on numpy float64 scalars: the model [7] or None"""
    a, b, na, nb = (np.asarray(v, dtype=np.float64) for v in (a, b, na, nb))
    with np.errstate(all="ignore"):
        D = _cross3(na, nb)
        dd = (D[0] * D[0] + D[1] * D[1]) + D[2] * D[2]
        ln = np.sqrt(dd)
        if not (ln > 0.0) or not np.isfinite(ln):
            return None
        d = [D[0] / ln, D[1] / ln, D[2] / ln]
        v = [b[0] - a[0], b[1] - a[1], b[2] - a[2]]
        k = (v[0] * d[0] + v[1] * d[1]) + v[2] * d[2]
        x = _cross3([v[0] - k * d[0], v[1] - k * d[1], v[2] - k * d[2]], nb)
        s = ((x[0] * D[0] + x[1] * D[1]) + x[2] * D[2]) / dd
        c = [a[0] + s * na[0], a[1] + s * na[1], a[2] + s * na[2]]
        r = np.abs(s) * np.sqrt((na[0] * na[0] + na[1] * na[1]) + na[2] * na[2])
        if not (np.isfinite(c).all() and np.isfinite(r) and r >= rmin and r <= rmax):
            return None
    return np.array([c[0], c[1], c[2], d[0], d[1], d[2], r])


# ---- the Gauss-Newton rows ------------------------------------------------------------------------------------------------------------
def gn_rows(pts, prm, plant_sign=None):
    """GenCylGn's rows [n, 6] at prm = (p, d, r, u) and which points have none (bad); plant_sign = a column whose sign is reversed"""
    m, u = prm[:7], prm[7:10]
    v = _cross3(m[3:6], u)
    e0, e1, e2 = pts[:, 0] - m[0], pts[:, 1] - m[1], pts[:, 2] - m[2]
    c0, c1, c2 = cross_components(pts, m)
    with np.errstate(all="ignore"):
        s = np.sqrt((c0 * c0 + c1 * c1) + c2 * c2)
        bad = ~(s > 0.0) | ~np.isfinite(s)
        t = (e0 * m[3] + e1 * m[4]) + e2 * m[5]
        gu = ((c0 * v[0] + c1 * v[1]) + c2 * v[2]) / s
        gv = -(((c0 * u[0] + c1 * u[1]) + c2 * u[2]) / s)
        rows = np.column_stack([gu, gv, t * gu, t * gv, -np.ones(len(pts)), s - m[6]])
    if plant_sign is not None:
        rows[:, plant_sign] = -rows[:, plant_sign]
    return rows, bad


def numpy_gram(pts, w=None, plant_sign=None, log=None):
    """a Gram provider for CylinderEstimator._fit_many with one item over all of pts"""
    w = np.ones(len(pts)) if w is None else np.asarray(w, dtype=np.float64)

    def gram(kind, prm, use_w, wpow, rows):
        assert list(rows) == [0]
        if log is not None:
            log.append((kind, None if prm is None else prm.copy(), use_w, wpow))
        if kind == _lib.GRAM_AFFINE:
            A, bad = np.column_stack([np.ones(len(pts)), pts]), np.zeros(len(pts), bool)
        else:
            assert kind == _lib.GRAM_CYL_GN and prm.shape == (1, 10)
            A, bad = gn_rows(pts, prm[0], plant_sign)
        A, ww = A[~bad], w[~bad]
        return ((A * ww[:, None]).T @ A)[None], np.array([len(pts)]), np.array([int(bad.sum())])
    return gram


def chart(m):
    """(u, v) of the chart at the model m: _estimators._cylinder_frame's u and v = d x u"""
    u = _estimators._cylinder_frame(np.asarray(m[3:6], dtype=np.float64)[None])[0]
    return u, np.cross(m[3:6], u)


def f_value(pts, m, u, v, x):
    """f = s - r at the chart point x = (alpha, beta, gamma, eta, rho) about m"""
    p = m[:3] + x[0] * u + x[1] * v
    d = m[3:6] + x[2] * u + x[3] * v
    d = d / np.linalg.norm(d)
    return np.linalg.norm(np.cross(pts - p, d), axis=1) - (m[6] + x[4])


# ---- the refit at 50 digits -----------------------------------------------------------------------------------------------------------
def refit_fixture(n, offset, weighted, seed):
    """n noisy points on an arc of at least a third of a cylinder of length at least 4 r, `offset` from the origin, the true model and a
    start 1e-3 .. 1e-1 away from it (relative to r in position and radius, absolute in the direction)"""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=3)
    d /= np.linalg.norm(d)
    r = rng.uniform(0.3, 1.0)
    mid = rng.uniform(3, 7, 3) + offset
    e1 = np.cross(d, rng.normal(size=3))
    e1 /= np.linalg.norm(e1)
    e2 = np.cross(d, e1)
    cov = rng.uniform(1.0 / 3.0, 1.0)
    ln = rng.uniform(4.0, 8.0) * r
    t = rng.uniform(-0.5 * ln, 0.5 * ln, n)
    phi = rng.uniform(-np.pi * cov, np.pi * cov, n)
    if n == 5:                                               # five points in general position: spread over the arc and the length
        t = np.array([-0.5, -0.2, 0.1, 0.3, 0.5]) * ln
        phi = np.array([-0.9, 0.7, -0.3, 0.1, 0.95]) * np.pi * cov
    rad = np.cos(phi)[:, None] * e1 + np.sin(phi)[:, None] * e2
    pts = mid + t[:, None] * d + rad * (r + rng.normal(0, 0.005, n))[:, None]
    w = rng.uniform(0.5, 1.5, n) if weighted else None
    gt = np.concatenate([mid, d, [r]])
    mag = 10.0 ** rng.uniform(-3, -1)
    start = gt.copy()
    start[:3] += mag * r * rng.normal(size=3) / np.sqrt(3)
    start[3:6] += mag * rng.normal(size=3) / np.sqrt(3)
    start[3:6] /= np.linalg.norm(start[3:6])
    start[6] *= 1.0 + mag * rng.uniform(-1, 1)
    return np.ascontiguousarray(pts), w, gt, start


def gn_reference(pts, w, start, iterations=60):
    """Plain Gauss-Newton on sum w (|(x - p) x d| - r)^2 at 50 digits from `start`, in a chart rebuilt at every iterate from an
    arbitrary orthonormal pair (the minimiser does not depend on it).  Returns (p, d, r, cond, converged): a point of the axis, the unit
    direction, the radius (floats), the 2-norm condition number of the 5x5 normal matrix at the solution in the estimator's chart and
    whether the last step was below 1e-30 (fourteen orders below what float64 resolves)."""
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
        ln = mp.sqrt(dot(a, a))
        return [x / ln for x in a]

    def frame(d):
        k = min(range(3), key=lambda j: abs(d[j]))
        ax = [mp.mpf(0)] * 3
        ax[k] = mp.mpf(1)
        u = unit(cross(ax, d))
        return u, cross(d, u)

    def normal_equations(p, d, r, u, v):
        A, g = mp.zeros(5, 5), mp.zeros(5, 1)
        for wi, x in zip(ww, P):
            e = [x[k] - p[k] for k in range(3)]
            c = cross(e, d)
            s = mp.sqrt(dot(c, c))
            t = dot(e, d)
            gu, gv = dot(c, v) / s, -dot(c, u) / s
            row = [gu, gv, t * gu, t * gv, mp.mpf(-1)]
            f = s - r
            for i in range(5):
                wr = wi * row[i]
                g[i] += wr * f
                for j in range(i, 5):
                    A[i, j] += wr * row[j]
        for i in range(5):
            for j in range(i):
                A[i, j] = A[j, i]
        return A, g

    p = [mp.mpf(float(x)) for x in start[:3]]
    d = unit([mp.mpf(float(x)) for x in start[3:6]])
    r = mp.mpf(float(start[6]))
    step = mp.mpf(1)
    for _ in range(iterations):
        u, v = frame(d)
        A, g = normal_equations(p, d, r, u, v)
        delta = mp.lu_solve(A, -g)
        p = [p[k] + delta[0] * u[k] + delta[1] * v[k] for k in range(3)]
        d = unit([d[k] + delta[2] * u[k] + delta[3] * v[k] for k in range(3)])
        r = r + delta[4]
        step = mp.sqrt(sum(x * x for x in delta))
        if step < mp.mpf(10) ** -30:
            break
    u, v = frame(d)
    A, _ = normal_equations(p, d, r, u, v)
    sv = mp.svd_r(A, compute_uv=False)
    cond = float(max(sv) / min(sv))
    return (np.array([float(x) for x in p]), np.array([float(x) for x in d]), float(r), cond, bool(step < mp.mpf(10) ** -30))


def refit_ratios(model, ref, pts):
    """The fitted model's distance from the reference in the five chart parameters, each over its tolerance 32 eps cond x scale: the
    axis' offset perpendicular to the reference axis (scale: the largest |coordinate| of the points, what x - p is formed from), the
    direction (scale 1: a unit vector, compared up to its sign) and the radius (scale r)."""
    p, d, r, cond, _ = ref
    tol = 32.0 * EPS * cond
    md = model[3:6] if model[3:6] @ d > 0 else -model[3:6]
    off = (model[:3] - p) - ((model[:3] - p) @ d) * d
    return (float(np.linalg.norm(off)) / (tol * float(np.abs(pts).max())), float(np.linalg.norm(md - d)) / tol,
            abs(float(model[6]) - r) / (tol * r))


# ---- the f32 filter -------------------------------------------------------------------------------------------------------------------
# the cylinder's shape, CylinderShape32; the shared part (AxialFilter32) is line3d_filter_model's
MODEL_LITERALS = dict(L3.SHARED_LITERALS, e1=2.0, e0=2.0, floor=1e-18, e2=8.0, r_max=1e17)

_LITERAL_PATTERNS = [
    (("e1",), r"ln\.e1 = f32_up\(NUM \* u \* dn\);"),
    (("e0", "floor"), r"ln\.e0 = big \? __builtin_inff\(\) : f32_up\(NUM \* u \* \(dn \* pn \+ fabs\(R\)\) \+ NUM\);"),
    (("e2",), r"ln\.e2 = f32_up\(NUM \* u \* dn\);"),
    (("r_max",), r"const bool big = out \|\| !\(fabs\(R\) <= NUM\);"),
]

# the header's statements of the f32 test's operation order, as prep and _magnitude below restate them, behind the shared block's
OPERATION_LINES = L3.SHARED_OPERATION_LINES + [
    "const double R = m[6] * sc;",
    "ln.r = (float)R;",
    "ln.nrm = f32_up(dn);",
    "const float s = axial_dist(p, ln, l1);",
    "return fabsf(s - ln.r);",
]


def header_block():
    return L3.axial_header_block("CylinderShape32")


def header_literals():
    return L3.axial_header_literals("CylinderShape32", _LITERAL_PATTERNS)


def prep(m, pscale, T2, plant_zero_budget=False, lit=None):
    """Filter32<kCylinder3D>::prep in float64, the lane's floats as Python floats holding f32 values"""
    L = MODEL_LITERALS if lit is None else lit

    def budget(ln, m, sc, dn, pn, u, out):
        R = np.float64(m[6]) * sc
        ln["r"] = f32(R)
        big = out or not (abs(R) <= L["r_max"])
        ln["e1"] = f32_up(L["e1"] * u * dn)
        ln["e0"] = float("inf") if big else f32_up(L["e0"] * u * (dn * pn + abs(R)) + L["floor"])
        ln["e2"] = f32_up(L["e2"] * u * dn)
        ln["nrm"] = f32_up(dn)
    return L3.axial_prep(m, pscale, T2, L, budget, plant_zero_budget)


def _magnitude(row, ln):
    """CylinderShape32::magnitude: (|s~ - r~|, l~)"""
    s, l1 = L3._dist(row, ln)
    return abs(s - L3._mp24().mpf(ln["r"])), l1


def reject(row, ln):
    """row = (x~, y~, z~, P): Filter32<kCylinder3D>::reject"""
    return L3.axial_reject(_magnitude, row, ln)


def group_reject(g, ln):
    """g = (centre[3], rho, Pmax): Filter32<kCylinder3D>::group_reject"""
    return L3.axial_group_reject(_magnitude, g, ln)


# ---- the cases the CPU and the GPU tests share ----
REFIT_CASES = [(n, offset, weighted) for n in (5, 64, 1000) for offset in (0.0, 1e3) for weighted in (False, True)]


def random_cylinder(rng, coord, offset, radius):
    d = rng.normal(size=3)
    d /= np.linalg.norm(d)
    return np.concatenate([rng.uniform(3, 7, 3) * coord + offset, d, [radius]])


def near_threshold_cases():
    """(ground truth, T, radius factor): coordinate scales 1, 1e3, 1e6, scenes at the origin, 1e3 scene scales and 1e6 units from it,
    thresholds 1e-3 .. 1e3 x nominal, radii 1e-3 .. 1e3 x the scale, d scaled by 2^-40 .. 2^40 by the caller"""
    rng = np.random.default_rng(31)
    k = 0
    for coord in (1.0, 1e3, 1e6):
        for offset in (0.0, 1e3 * coord, 1e6):
            for tf in (1e-3, 1.0, 1e3):
                for e in (-40, 0, 40):
                    rf = (1e-3, 1.0, 1e3, 0.05)[k % 4]
                    k += 1
                    yield rng, random_cylinder(rng, coord, offset, rf * coord), 1.5 * 0.05 * coord * tf, e, coord


# ---- pairs near the threshold ---------------------------------------------------------------------------------------------------------
def near_threshold_points(rng, cyl, T, n, along):
    """n points whose distance to the surface of the unit-direction cylinder (p, d, r) is T (1 +- 0.5e-4), outside it and - where
    r > T - inside it in turn, at positions uniform in +-along along the axis"""
    p, d, r = np.asarray(cyl[:3]), np.asarray(cyl[3:6]), float(cyl[6])
    a = np.cross(d, [1.0, 0.0, 0.0] if abs(d[0]) < 0.9 else [0.0, 1.0, 0.0])
    a /= np.linalg.norm(a)
    b = np.cross(d, a)
    phi = rng.uniform(0, 2 * np.pi, n)
    target = T * (1.0 + rng.uniform(-0.99e-4 / 2, 0.99e-4 / 2, n))
    side = np.where((np.arange(n) % 2 == 1) & (r > 1.001 * T), -1.0, 1.0)
    perp = np.cos(phi)[:, None] * a + np.sin(phi)[:, None] * b
    return np.ascontiguousarray(p + rng.uniform(-along, along, n)[:, None] * d + (r + side * target)[:, None] * perp)
