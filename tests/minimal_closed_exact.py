"""The nine closed-form minimal solvers restated from their definitions at 50 digits: what the lane-per-model solvers of
csrc/solve.hip (solve_minimal(Type<...>) behind solve_kernel<MT>: 2-D line, vanishing point, plane, sphere, circle, 3-D line, 2-point
oriented cylinder, 3-point oriented cone, the two slots of the 4-point oriented torus) and Estimator.minimal of _estimators.py are
held to.  The sibling of tests/minimal_exact.py, whose digits, no_hook, _relative and kappa_route it uses.

TEST INFRASTRUCTURE, never imported by the product; mpmath is imported when a function is called.
tests/golden/make_golden_minimal_closed.py runs this module and writes tests/golden/kat_minimal_closed_v1.npz; the comparisons
(tests/minimal_closed_cases.py) read that file.  The committed float64 inputs are taken as exact.  Kept apart:

  what the answer is          definition(name, P, N, ranges): by a method that is not the product's -
      line, plane             the null vector of the m x (m + 1) system of homogeneous points by SVD, at unit normal, up to one sign;
      vanishing point         each segment's line the null vector of its two homogeneous endpoints, the point the null vector of the
                              two lines (SVD), unit norm, up to sign;
      circle, sphere          the algebraic form on the UNTRANSLATED coordinates, 2 c . p_i + k = |p_i|^2 by LU, r = sqrt(k + |c|^2)
                              (the product translates to p0 and uses Cramer's rule);
      3-D line                d = (b - a) / |b - a|, p = a;
      cylinder                d the null vector of [na; nb] by SVD (no cross product), (s, t, u) of s na - t nb - u d = b - a by LU,
                              c = a + s na, r = |s| |na|; d up to sign;
      cone                    the apex the LU solution of n_i . a = n_i . p_i, d the null vector of [g1 - g0; g2 - g0] by SVD (g_i the unit
                              vectors from the apex), signed by sum d . g_i >= 0, c = d . g0, s = sqrt(1 - c^2);
      torus                   both common transversals of the four normal lines in Pluecker coordinates: the 2-dimensional null space
                              of the 4 x 6 incidence system by SVD, the Klein quadric's quadratic on it, its roots by polyroots at
                              raised precision (the basis must not matter); per real transversal a point and the unit direction, the
                              three (h_k, rho_k), the circle through them by the algebraic circle definition, R, r, c; kept where the
                              solver's stated acceptance holds (R > r, finite, inside the ranges); d up to sign, the slots as a set;
  how accurately the product's ROUTE can deliver it
                              route(name, P, N, ranges, slot, hook): the stages of solve.hip's comments restated once, a hook at every
                              stage interface; kappa_route = sum over stages of WEIGHTS (the roundings on the stage's longest chain,
                              counted from the code) x max_i sum_j |d out_i / d delta_j| (minimal_exact.kappa_route); the tolerance is
                              32 eps kappa_route.  At delta = 0 the route must land on the definition to 1e-40 (the generator asserts it);
  the problem's own condition condition(name, P, N, slot): |J|_2 |x|_2 / |y|_2 of the answer with respect to every input
                              (points and, where read, normals), by central differences at 50 digits.
"""
import numpy as np

import minimal_exact as X
from minimal_exact import _relative, digits, kappa_route, no_hook  # noqa: F401  (digits: re-exported for the generator)

EPS, FACTOR = X.EPS, X.FACTOR
TYPES = ["line", "vanishing_point", "plane", "sphere", "circle", "line3d", "cylinder", "cone", "torus"]
ORIENTED = ("cylinder", "cone", "torus")
FULL = (0.0, float("inf"), 0.0, float("inf"))       # (rmin, rmax, Rmin, Rmax): the context's ranges at creation
# the entries whose common sign is free in the comparison (None: nothing is)
FLIP = dict(line=[-1, -1, -1], vanishing_point=[-1, -1, -1], plane=[-1, -1, -1, -1], sphere=None, circle=None, line3d=None,
            cylinder=[1, 1, 1, -1, -1, -1, 1], cone=None, torus=[1, 1, 1, -1, -1, -1, 1, 1])

# roundings on the longest dependency chain inside each stage, counted from solve.hip (DESIGN.md 4.5b lists the chains).  A product
# that enters a sum or a difference is a stage of its own, "<stage> (products)", of weight 1 (2 where an unhooked difference feeds it:
# the torus' e = p_k - a, hc = h_0 + z_0): the stage's own weight counts what follows the products
class _Weights(dict):
    def __missing__(self, stage):
        assert stage.endswith(" (products)"), stage
        return 1


WEIGHTS = {name: _Weights(w) for name, w in dict(
    line={"d": 1, "ln": 3, "normal": 1, "c": 1},
    vanishing_point={"lines": 1, "v": 1, "ln": 4, "unit": 1},
    plane={"edges": 1, "n": 1, "ln": 4, "normal": 1, "d": 2},
    sphere={"a": 1, "h": 3, "crosses": 1, "det": 2, "e": 3, "r": 4, "c": 1},
    circle={"a": 1, "h": 2, "det": 1, "e": 2, "r": 3, "c": 1},
    line3d={"v": 1, "ln": 4, "d": 1},
    cylinder={"D": 1, "dd": 3, "ln": 1, "d": 1, "v": 1, "k": 2, "w": 1, "x": 1, "s": 3, "c": 1, "r": 5},
    cone={"X": 1, "det": 2, "b": 2, "a": 3, "w": 1, "l": 4, "g": 1, "differences": 1, "D": 1, "ln": 4, "d": 1, "c": 2, "s": 5},
    torus={"q, g": 1, "X, Y": 1, "A..D": 3, "qa, qb, qc": 3, "disc": 1, "sq": 1, "s": 2, "den": 1, "t": 2, "a, b": 1, "d": 6,
           "h, rho": 5, "h, rho (products)": 2, "circle a": 1, "circle g": 2, "circle det": 1, "z": 2, "c, R, r": 3, "c, R, r (products)": 2}).items()}


def _mp():
    return X._mp()


def _m(mp, a):
    return [[mp.mpf(float(x)) for x in r] for r in np.atleast_2d(np.asarray(a, dtype=np.float64))]


def _dot(a, b):
    return sum(x * y for x, y in zip(a, b))


def _sub(a, b):
    return [x - y for x, y in zip(a, b)]


def _cross(a, b):
    """cross3's component order (solve.hip)"""
    return [a[1] * b[2] - a[2] * b[1], -(a[0] * b[2] - a[2] * b[0]), a[0] * b[1] - a[1] * b[0]]


def _norm(mp, a):
    return mp.sqrt(_dot(a, a))


def _null(mp, rows, dim=1):
    """the last `dim` right singular vectors of the m x n system `rows` (n = m + dim) by SVD, or None where its rank is below m"""
    A = mp.matrix(rows)
    m, n = A.rows, A.cols
    if max(abs(A[i, j]) for i in range(m) for j in range(n)) == 0:
        return None
    _, S, V = mp.svd_r(A, full_matrices=True, compute_uv=True)
    sv = [S[k] for k in range(m)]
    if min(sv) <= mp.mpf(10) ** -(X.DIGITS - 20) * max(sv):
        return None
    out = [[V[n - dim + k, j] for j in range(n)] for k in range(dim)]
    return out[0] if dim == 1 else out


def _lu(mp, A, b):
    """the LU solution of A x = b, or None where A is singular"""
    try:
        A = mp.matrix(A)
        n = A.rows
        E = A.copy()                                    # singular = det 0 after the rows, then the columns, are brought to largest entry 1
        for i in range(n):
            top = max(abs(E[i, j]) for j in range(n))
            if top == 0:
                return None
            for j in range(n):
                E[i, j] /= top
        for j in range(n):
            top = max(abs(E[i, j]) for i in range(n))
            if top == 0:
                return None
            for i in range(n):
                E[i, j] /= top
        if abs(mp.det(E)) <= mp.mpf(10) ** -(X.DIGITS - 20):
            return None
        x = mp.lu_solve(A, mp.matrix(b))
    except ZeroDivisionError:
        return None
    return [x[k] for k in range(A.rows)]


def _round_definition(mp, P):
    """(c, r) of the circle / sphere through the rows of P: 2 c . p + k = |p|^2 by LU on the untranslated coordinates"""
    sol = _lu(mp, [[2 * x for x in p] + [1] for p in P], [_dot(p, p) for p in P])
    if sol is None:
        return None
    c, k = sol[:-1], sol[-1]
    rr = k + _dot(c, c)
    return (c, mp.sqrt(rr)) if rr > 0 else None


def _inside(v, lo, hi):
    return v >= lo and v <= hi


# ---- the definitions -------------------------------------------------------------------------------------------------------------
def torus_transversals(P, N, basis="svd"):
    """the real common transversals of the four normal lines as (a point, the unit direction), or None where the incidence system
    has rank below 4 (a zero normal, lines in special position: no finite solution set).  basis "mixed": the null space rotated."""
    mp = _mp()
    P, N = _m(mp, P), _m(mp, N)
    # line i = (direction n_i, moment p_i x n_i); a line (t, m) meets it iff t . (p_i x n_i) + m . n_i = 0
    B = _null(mp, [_cross(P[i], N[i]) + N[i] for i in range(4)], dim=2)
    if B is None:
        return None
    u, v = B
    if basis == "mixed":
        c, s = mp.cos(mp.mpf("0.7")), mp.sin(mp.mpf("0.7"))
        u, v = [c * u[k] + s * v[k] for k in range(6)], [-s * u[k] + c * v[k] for k in range(6)]
    # the Klein quadric t . m = 0 on l u + v: al l^2 + be l + ga = 0
    al, be, ga = _dot(u[:3], u[3:]), _dot(u[:3], v[3:]) + _dot(v[:3], u[3:]), _dot(v[:3], v[3:])
    top = max(abs(al), abs(be), abs(ga))
    if top <= mp.mpf(10) ** -(X.DIGITS - 15):
        return None
    lines = []
    if abs(al) <= mp.mpf(10) ** -(X.DIGITS - 15) * top:                 # a root at infinity of this chart: u itself
        lines.append(u)
        roots = [] if abs(be) <= mp.mpf(10) ** -(X.DIGITS - 15) * top else [-ga / be]
    else:
        roots = mp.polyroots([al, be, ga], maxsteps=500, extraprec=4 * mp.mp.prec)
        roots = [mp.re(x) for x in roots if abs(mp.im(x)) <= mp.mpf(10) ** -(X.DIGITS // 2 - 5) * max(1, abs(x))]
    lines += [[l * u[k] + v[k] for k in range(6)] for l in roots]
    out = []
    for L in lines:
        t, m = L[:3], L[3:]
        tt = _dot(t, t)
        if tt <= mp.mpf(10) ** -(X.DIGITS - 15) * _dot(L, L):           # a line at infinity: no axis
            continue
        ln = mp.sqrt(tt)
        out.append(([x / tt for x in _cross_plain(t, m)], [x / ln for x in t]))
    return out


def _cross_plain(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def definition(name, P, N=None, ranges=FULL, basis="svd"):
    """every solution of the sample (point rows P, normal rows N) as a list of 50-digit models; [] where there is none"""
    mp = _mp()
    rmin, rmax, Rmin, Rmax = ranges
    if name == "torus":
        axes = torus_transversals(P, N, basis)
        P = _m(mp, P)
        out = []
        for a0, d in axes or []:
            hr = []
            for k in range(3):
                e = _sub(P[k], a0)
                h = _dot(e, d)
                hr.append([h, _norm(mp, [e[j] - h * d[j] for j in range(3)])])
            circ = _round_definition(mp, hr)
            if circ is None:
                continue
            (hc, R), r = circ
            if R > r and _inside(r, rmin, rmax) and _inside(R, Rmin, Rmax):
                out.append([a0[j] + hc * d[j] for j in range(3)] + d + [R, r])
        return out
    P = _m(mp, P)
    if name in ("line", "plane"):
        v = _null(mp, [p + [mp.mpf(1)] for p in P])
        if v is None:
            return []
        ln = _norm(mp, v[:-1])
        return [[x / ln for x in v]]
    if name == "vanishing_point":
        lines = [_null(mp, [[s[0], s[1], mp.mpf(1)], [s[2], s[3], mp.mpf(1)]]) for s in P]
        v = None if None in lines else _null(mp, lines)
        return [] if v is None else [v]
    if name in ("circle", "sphere"):
        circ = _round_definition(mp, P)
        return [circ[0] + [circ[1]]] if circ is not None and _inside(circ[1], rmin, rmax) else []
    if name == "line3d":
        v = _sub(P[1], P[0])
        ln = _norm(mp, v)
        return [P[0] + [x / ln for x in v]] if ln > 0 else []
    N = _m(mp, N)
    if name == "cylinder":
        d = _null(mp, [N[0], N[1]])
        if d is None:
            return []
        stu = _lu(mp, [[N[0][j], -N[1][j], -d[j]] for j in range(3)], _sub(P[1], P[0]))
        if stu is None:
            return []
        r = abs(stu[0]) * _norm(mp, N[0])
        return [[P[0][j] + stu[0] * N[0][j] for j in range(3)] + d + [r]] if _inside(r, rmin, rmax) else []
    assert name == "cone"
    a = _lu(mp, N, [_dot(N[i], P[i]) for i in range(3)])
    if a is None:
        return []
    g = []
    for i in range(3):
        w = _sub(P[i], a)
        if _norm(mp, w) <= mp.mpf(10) ** -(X.DIGITS - 15) * (1 + _norm(mp, P[i])):          # a sample at the apex
            return []
        g.append([x / _norm(mp, w) for x in w])
    d = _null(mp, [_sub(g[1], g[0]), _sub(g[2], g[0])])
    if d is None:
        return []
    if sum(_dot(d, g[i]) for i in range(3)) < 0:
        d = [-x for x in d]
    c = _dot(d, g[0])
    if not c > mp.mpf(10) ** -(X.DIGITS - 15):                    # c <= 0 is refused (c = 0 exactly: the apex in the samples' plane)
        return []
    s = mp.sqrt(1 - c * c)
    return [a + d + [c, s]] if _inside(s, rmin, rmax) else []


def unflipped(P, N):
    """the cone's sum of D . g_i before its sign flip (D = (g1 - g0) x (g2 - g0), the apex by LU): negative = the flip is taken"""
    mp = _mp()
    P, N = _m(mp, P), _m(mp, N)
    a = _lu(mp, N, [_dot(N[i], P[i]) for i in range(3)])
    g = [[x / _norm(mp, _sub(P[i], a)) for x in _sub(P[i], a)] for i in range(3)]
    D = _cross(_sub(g[1], g[0]), _sub(g[2], g[0]))
    return sum(_dot(D, g[i]) for i in range(3))


def surface_residual(name, P, N, model):
    """what the generator asserts of every reference solution (each <= 1e-40 relative): the samples on the surface and the normal
    relation the solver uses -> the largest residual, relative to the sample's size"""
    mp = _mp()
    P = _m(mp, P)
    size = max(abs(x) for p in P for x in p) or mp.mpf(1)
    m = list(model)
    if name in ("line", "plane"):
        return max(abs(_dot(m[:-1], p) + m[-1]) for p in P) / size
    if name == "vanishing_point":                        # the point on both segments' lines
        return max(abs(_dot(m, _cross_plain([s[0], s[1], 1], [s[2], s[3], 1]))) for s in P) / size ** 2
    if name in ("circle", "sphere"):
        return max(abs(_norm(mp, _sub(p, m[:-1])) - m[-1]) for p in P) / size
    if name == "line3d":
        return max(_norm(mp, _cross_plain(_sub(p, m[:3]), m[3:])) for p in P) / size
    N = _m(mp, N)
    c, d = m[:3], m[3:6]
    if name == "cylinder":
        on = abs(_norm(mp, _cross_plain(_sub(P[0], c), d)) - m[6]) / size          # (r is the first sample's distance)
        meet = max(abs(_dot(d, _cross_plain(N[i], _sub(P[i], c)))) / (_norm(mp, N[i]) * size) for i in range(2))
        return max(on, meet, max(abs(_dot(n, d)) / _norm(mp, n) for n in N))
    if name == "cone":
        on = max(abs(_dot(_sub(p, c), d) - m[6] * _norm(mp, _sub(p, c))) for p in P) / size
        return max(on, max(abs(_dot(N[i], _sub(P[i], c))) / (_norm(mp, N[i]) * size) for i in range(3)), abs(m[6] ** 2 + m[7] ** 2 - 1))
    on = 0
    for p in P[:3]:                                      # the fourth sample enters through the transversal alone
        e = _sub(p, c)
        h = _dot(e, d)
        on = max(on, abs(mp.sqrt((_norm(mp, _cross_plain(e, d)) - m[6]) ** 2 + h * h) - m[7]) / size)
    meet = max(abs(_dot(d, _cross_plain(N[i], _sub(P[i], c)))) / (_norm(mp, N[i]) * size) for i in range(4))
    return max(on, meet)


# ---- the product's routes, stage by stage (solve.hip's comments) -------------------------------------------------------------------------
class _Ops:
    """the sums of products of one route: every product that enters a sum or a difference is hooked on its own, as the stage
    "<stage> (products)" - its rounding is relative to the product, not to what the cancellation leaves - before the stage's outputs are"""

    def __init__(self, hook):
        self.hook = hook

    def dot(self, stage, a, b):
        return sum(self.hook(stage + " (products)", [x * y for x, y in zip(a, b)]))

    def cross(self, stage, a, b):
        t = self.hook(stage + " (products)", [a[1] * b[2], a[2] * b[1], a[0] * b[2], a[2] * b[0], a[0] * b[1], a[1] * b[0]])
        return [t[0] - t[1], -(t[2] - t[3]), t[4] - t[5]]

    def axpy(self, stage, a, s, x):
        """a + s x, componentwise"""
        t = self.hook(stage + " (products)", [s * v for v in x])
        return [a[k] + t[k] for k in range(len(a))]


def _circle_route(mp, p0, p1, p2, hook, pre=""):
    """the 3-point circle solver's arithmetic on three 2-D points -> (e0, e1), or None where det is 0"""
    a10, a11, a20, a21 = hook(pre + "a", [p1[0] - p0[0], p1[1] - p0[1], p2[0] - p0[0], p2[1] - p0[1]])
    h1, h2 = hook(pre + ("g" if pre else "h"), [(a10 * a10 + a11 * a11) / 2, (a20 * a20 + a21 * a21) / 2])
    t = hook(pre + "det (products)", [a10 * a21, a11 * a20])
    det, = hook(pre + "det", [t[0] - t[1]])
    if det == 0:
        return None
    t = hook(("z" if pre else "e") + " (products)", [h1 * a21, h2 * a11, a10 * h2, a20 * h1])
    return hook("z" if pre else "e", [(t[0] - t[1]) / det, (t[2] - t[3]) / det])


def route(name, P, N=None, ranges=FULL, slot=0, hook=no_hook, inputs=None):
    """the model the route makes of the sample (a list of 50-digit numbers), or None where a gate refuses it.  inputs: the sample
    as one flat list of mpf (points, then normals) in place of P and N - the condition's differences."""
    mp = _mp()
    o = _Ops(hook)
    rmin, rmax, Rmin, Rmax = ranges
    if inputs is None:
        P, N = _m(mp, P), (_m(mp, N) if N is not None else None)
    else:
        D = {"line": 2, "vanishing_point": 4, "circle": 2}.get(name, 3)
        m = len(inputs) // (D + 3) if name in ORIENTED else len(inputs) // D
        P = [list(inputs[D * i:D * i + D]) for i in range(m)]
        N = [list(inputs[D * m + 3 * i:D * m + 3 * i + 3]) for i in range(m)] if name in ORIENTED else None
    if name == "line":
        dx, dy = hook("d", [P[1][0] - P[0][0], P[1][1] - P[0][1]])
        ln, = hook("ln", [mp.sqrt(dx * dx + dy * dy)])
        if not ln > 0:
            return None
        n = hook("normal", [-dy / ln, dx / ln])
        return n + hook("c", [-o.dot("c", n, P[0])])
    if name == "vanishing_point":
        one = mp.mpf(1)
        L = hook("lines", o.cross("lines", [P[0][0], P[0][1], one], [P[0][2], P[0][3], one]) + o.cross("lines", [P[1][0], P[1][1], one], [P[1][2], P[1][3], one]))
        v = hook("v", o.cross("v", L[:3], L[3:]))
        ln, = hook("ln", [_norm(mp, v)])
        return hook("unit", [x / ln for x in v]) if ln > 0 else None
    if name == "plane":
        e = hook("edges", _sub(P[1], P[0]) + _sub(P[2], P[0]))
        n = hook("n", o.cross("n", e[:3], e[3:]))
        ln, = hook("ln", [_norm(mp, n)])
        if not ln > 0:
            return None
        n = hook("normal", [x / ln for x in n])
        return n + hook("d", [-o.dot("d", n, P[0])])
    if name == "sphere":
        a = hook("a", [x for i in (1, 2, 3) for x in _sub(P[i], P[0])])
        a = [a[0:3], a[3:6], a[6:9]]
        h = hook("h", [_dot(x, x) / 2 for x in a])
        n = hook("crosses", o.cross("crosses", a[1], a[2]) + o.cross("crosses", a[2], a[0]) + o.cross("crosses", a[0], a[1]))
        n = [n[0:3], n[3:6], n[6:9]]
        det, = hook("det", [o.dot("det", a[0], n[0])])
        if det == 0:
            return None
        e = hook("e", [o.dot("e", h, [n[0][k], n[1][k], n[2][k]]) / det for k in range(3)])
        r, = hook("r", [_norm(mp, e)])
        c = hook("c", [P[0][k] + e[k] for k in range(3)])
        return c + [r] if _inside(r, rmin, rmax) else None
    if name == "circle":
        e = _circle_route(mp, P[0], P[1], P[2], hook)
        if e is None:
            return None
        r, = hook("r", [_norm(mp, e)])
        c = hook("c", [P[0][0] + e[0], P[0][1] + e[1]])
        return c + [r] if _inside(r, rmin, rmax) else None
    if name == "line3d":
        v = hook("v", _sub(P[1], P[0]))
        ln, = hook("ln", [_norm(mp, v)])
        return P[0] + hook("d", [x / ln for x in v]) if ln > 0 else None
    if name == "cylinder":
        a, b, na, nb = P[0], P[1], N[0], N[1]
        D = hook("D", o.cross("D", na, nb))
        dd, = hook("dd", [_dot(D, D)])
        ln, = hook("ln", [mp.sqrt(dd)])
        if not ln > 0:
            return None
        d = hook("d", [x / ln for x in D])
        v = hook("v", _sub(b, a))
        k, = hook("k", [o.dot("k", v, d)])
        w = hook("w", o.axpy("w", v, -k, d))
        x = hook("x", o.cross("x", w, nb))
        s, = hook("s", [o.dot("s", x, D) / dd])
        c = hook("c", o.axpy("c", a, s, na))
        r, = hook("r", [abs(s) * _norm(mp, na)])
        return c + d + [r] if _inside(r, rmin, rmax) else None
    if name == "cone":
        Xc = hook("X", o.cross("X", N[1], N[2]) + o.cross("X", N[2], N[0]) + o.cross("X", N[0], N[1]))
        Xc = [Xc[0:3], Xc[3:6], Xc[6:9]]
        det, = hook("det", [o.dot("det", N[0], Xc[0])])
        if det == 0:
            return None
        b = hook("b", [o.dot("b", N[i], P[i]) for i in range(3)])
        a = hook("a", [o.dot("a", b, [Xc[0][k], Xc[1][k], Xc[2][k]]) / det for k in range(3)])
        w = hook("w", [x for i in range(3) for x in _sub(P[i], a)])
        w = [w[0:3], w[3:6], w[6:9]]
        l = hook("l", [_norm(mp, x) for x in w])
        if not min(l) > 0:
            return None
        g = hook("g", [w[i][k] / l[i] for i in range(3) for k in range(3)])
        g = [g[0:3], g[3:6], g[6:9]]
        df = hook("differences", _sub(g[1], g[0]) + _sub(g[2], g[0]))
        D = hook("D", o.cross("D", df[:3], df[3:]))
        ln, = hook("ln", [_norm(mp, D)])
        if not ln > 0:
            return None
        d = hook("d", [x / ln for x in D])
        if sum(_dot(d, g[i]) for i in range(3)) < 0:
            d = [-x for x in d]
        c, = hook("c", [o.dot("c", d, g[0])])
        s, = hook("s", [_norm(mp, o.cross("s", g[0], d))])
        return a + d + [c, s] if c > 0 and _inside(s, rmin, rmax) else None
    assert name == "torus"
    p0, p1, n0, n1 = P[0], P[1], N[0], N[1]
    qg = hook("q, g", _sub(p1, p0) + _sub(P[2], p0) + _sub(P[3], p0))
    q, g = qg[:3], [qg[3:6], qg[6:9]]
    XY = hook("X, Y", o.cross("X, Y", N[2], g[0]) + o.cross("X, Y", N[2], n0) + o.cross("X, Y", N[3], g[1]) + o.cross("X, Y", N[3], n0))
    co = []
    for i in range(2):
        Xv, Yv = XY[6 * i:6 * i + 3], XY[6 * i + 3:6 * i + 6]
        co += [-o.dot("A..D", n1, Yv), -(o.dot("A..D", q, Yv) + o.dot("A..D", n0, Xv)), o.dot("A..D", n1, Xv), o.dot("A..D", q, Xv)]
    co = hook("A..D", co)
    A, B, C, Dc = [co[0], co[4]], [co[1], co[5]], [co[2], co[6]], [co[3], co[7]]
    t = hook("qa, qb, qc (products)", [B[1] * A[0], A[1] * B[0], B[1] * C[0], A[1] * Dc[0], C[1] * B[0], Dc[1] * A[0], Dc[1] * C[0], C[1] * Dc[0]])
    qa, qb, qc = hook("qa, qb, qc", [t[0] - t[1], t[2] - t[3] - t[4] + t[5], t[6] - t[7]])
    t = hook("disc (products)", [qb * qb, 4 * qa * qc])
    disc, = hook("disc", [t[0] - t[1]])
    if disc < 0 or qa == 0:
        return None
    sq, = hook("sq", [mp.sqrt(disc)])
    s, = hook("s", [(-qb + sq) / (2 * qa) if slot == 0 else (-qb - sq) / (2 * qa)])
    den, = hook("den", [o.dot("den", [A[0]], [s]) + C[0]])
    if den == 0:
        return None
    t, = hook("t", [-(o.dot("t", [B[0]], [s]) + Dc[0]) / den])
    ab = hook("a, b", o.axpy("a, b", p0, s, n0) + o.axpy("a, b", p1, t, n1))
    a, Dv = ab[:3], _sub(ab[3:], ab[:3])
    ln = _norm(mp, Dv)
    if not ln > 0:
        return None
    d = hook("d", [x / ln for x in Dv])
    hr = []
    for k in range(3):
        e = _sub(P[k], a)
        hr += [o.dot("h, rho", e, d), _norm(mp, o.cross("h, rho", e, d))]
    hr = hook("h, rho", hr)
    z = _circle_route(mp, hr[0:2], hr[2:4], hr[4:6], hook, pre="circle ")
    if z is None:
        return None
    hc = hr[0] + z[0]
    out = hook("c, R, r", o.axpy("c, R, r", a, hc, d) + [hr[1] + z[1], _norm(mp, z)])
    R, r = out[3], out[4]
    return out[:3] + d + [R, r] if R > r and _inside(r, rmin, rmax) and _inside(R, Rmin, Rmax) else None


def aligned(name, model, ref):
    """model with its free sign chosen next to ref"""
    f = FLIP[name]
    if f is None:
        return list(model)
    other = [x * s for x, s in zip(model, f)]
    dist = lambda m: max(abs(a - b) for a, b in zip(m, ref))
    return other if dist(other) < dist(model) else list(model)


def kappa(name, P, N=None, ranges=FULL, slot=0):
    """(kappa_route, {stage: share}) of the slot's model; without the ranges, so that a model at a bound keeps both sides"""
    return kappa_route(lambda hook: route(name, P, N, FULL, slot, hook), WEIGHTS[name])


def condition(name, P, N=None, slot=0):
    """the relative condition of the slot's answer with respect to every input (central differences of 1e-20 of the largest input of
    the points and of the normals each; the answer as the route's closed form at delta = 0, which the generator holds to the
    definition at 1e-40; no range, so that a solution at a bound has both sides)"""
    mp = _mp()
    x = [v for r in _m(mp, P) for v in r]
    steps = [mp.mpf(10) ** -20 * max(abs(v) for v in x)] * len(x)
    if name in ORIENTED:
        nx = [v for r in _m(mp, N) for v in r]
        steps += [mp.mpf(10) ** -20 * max(abs(v) for v in nx)] * len(nx)
        x += nx
    base = route(name, None, None, FULL, slot, inputs=x)
    # (the torus route's R > r gate is part of FULL: a solution kept by the definition passes it on both sides of a small step)
    J = np.zeros((len(base), len(x)))
    for j in range(len(x)):
        hi, lo = list(x), list(x)
        hi[j] += steps[j]
        lo[j] -= steps[j]
        a, b = route(name, None, None, FULL, slot, inputs=hi), route(name, None, None, FULL, slot, inputs=lo)
        J[:, j] = [float((a[k] - b[k]) / (2 * steps[j])) for k in range(len(base))]
    return _relative(J, x, base)
