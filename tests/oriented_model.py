"""The oriented mixed-primitive type (PGX_ORIENTED_PRIMITIVE3D = 20) in numpy.  A model row is type 18's (class, q0 .. q7) and the
distance is type 18's (tests/primitive_model.py sq_primitive: nothing is restated twice); what is stated here is the compatibility
test of a point's normal n with the model's surface normal at the point.  g, the unnormalised direction of that normal:

    plane    (a, b, c, d)     g = (a, b, c)
    sphere   (c, r)           g = x - c
    cylinder (p, d, r)        e = x - p,  t = (e0 d0 + e1 d1) + e2 d2,  g_k = e_k - t d_k
    cone     (a, d, c, s)     e = x - a,  h = (e0 d0 + e1 d1) + e2 d2,  w_k = e_k - h d_k,
                              rho = the root the cone's residual computes (the 3-D line's distance in its cross-product form),
                              g_k = c w_k - (s rho) d_k

Every dot product is a left fold, (u0 v0 + u1 v1) + u2 v2.  With nn = n.n, gg = g.g, ng = n.g and w = nn gg a point is COMPATIBLE iff
ng ng >= kappa w and w > 0, kappa = cos^2(tolerance): no division, no root besides the cone's own; every comparison is false on NaN.
squared = type 18's where compatible, +inf where not; a class that is no class gives NaN.  plain (pgx_residual_sum(s)) is type 18's."""
import numpy as np

from primitive_model import CONE, CYLINDER, PLANE, PREFIX, SPHERE, class_of, sq_primitive


def kappa_of(tolerance_deg):
    """cos^2 of the tolerance, as OrientedPrimitiveEstimator computes it (90 degrees: exactly 0)"""
    if tolerance_deg == 90.0:
        return 0.0
    c = np.cos(np.deg2rad(tolerance_deg))
    return float(c * c)


def _fold(u, v):
    return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]


def surface_normal(pts, m):
    """g as a list of three [n] arrays, or None for a class that is no class"""
    c = class_of(m)
    if c is None:
        return None
    x = [pts[:, 0], pts[:, 1], pts[:, 2]]
    with np.errstate(invalid="ignore", over="ignore"):
        if c == PLANE:
            return [np.full(len(pts), m[1 + k]) for k in range(3)]
        if c == SPHERE:
            return [x[k] - m[1 + k] for k in range(3)]
        e = [x[k] - m[1 + k] for k in range(3)]
        d = m[4:7]
        t = _fold(e, d)
        if c == CYLINDER:
            return [e[k] - t * d[k] for k in range(3)]
        assert c == CONE
        c0 = e[1] * d[2] - e[2] * d[1]
        c1 = -(e[0] * d[2] - e[2] * d[0])
        c2 = e[0] * d[1] - e[1] * d[0]
        rho = np.sqrt((c0 * c0 + c1 * c1) + c2 * c2)
        sr = m[8] * rho
        return [m[7] * (e[k] - t * d[k]) - sr * d[k] for k in range(3)]


def compatible(pts, nrm, m, kappa):
    """bool [n]"""
    g = surface_normal(pts, m)
    if g is None:
        return np.zeros(len(pts), dtype=bool)
    n = [nrm[:, 0], nrm[:, 1], nrm[:, 2]]
    with np.errstate(invalid="ignore", over="ignore"):
        nn, gg, ng = _fold(n, n), _fold(g, g), _fold(n, g)
        w = nn * gg
        return (ng * ng >= kappa * w) & (w > 0.0)


def sq_oriented(pts, nrm, m, kappa):
    """squared residuals of the union row m [9] under type 20"""
    sq = sq_primitive(pts, m)
    if class_of(m) is None:
        return sq                                                                 # NaN
    return np.where(compatible(pts, nrm, m, kappa), sq, np.inf)


def sq_fn(nrm, kappa):
    """sq_oriented as the (pts, model) function primitive_helpers.ref_score takes; pts must be the rows the normals belong to"""
    def fn(pts, m):
        assert len(pts) == len(nrm)
        return sq_oriented(pts, nrm, m, kappa)
    return fn


def prefix_compatible(pts, nrm, sample, m, kappa):
    """the solver's candidate test: the slot's model agrees with every point of its own prefix of the four-point sample"""
    c = class_of(m)
    if c is None:
        return False
    idx = np.asarray(sample)[:PREFIX[c]]
    return bool(compatible(pts[idx], nrm[idx], m, kappa).all())
