"""The 3-D line type restated for its tests (test_lines3d_cpu.py, test_gpu_lines3d.py).  TEST INFRASTRUCTURE, never imported by the
product.

* sq_line3d: Residual<kLine3D> (csrc/residuals.hip.h) in numpy, operation for operation.
* sym_points / SYM_MODEL: the same residual through the oracle's symmetric-homography type.  With H = H^-1 = (0 0 0; 0 0 0; 0 0 1)
  both maps send every finite point to (0, 0), and the point (c2, 0, c0, c1) has the residual (c0 c0 + c1 c1) + (c2 c2 + 0): every
  added operation is exact, so the oracle evaluates the line residual bit for bit without knowing the type.  Needs finite c.
* prep / reject / group_reject: Filter32<kLine3D> (csrc/score_filters.hip.h) in the header's operation order and with the header's
  literals.  header_literals() reads the literals out of the header's text and OPERATION_LINES are the header's statements of the
  operation order, so a test can hold model and header together: a coefficient or a statement changed on one side only fails it.
  The part the header states once for the four axial types (AxialFilter32, axial_dist, axial_height) is restated once, here
  (SHARED_*, axial_prep, axial_reject, axial_group_reject); cylinder_model.py, cone_model.py and torus_model.py add their shapes.
  f32 arithmetic is mpmath at 24 bits of precision, fma an exact product and a sum rounded once (numpy has no fmaf, and an
  fma emulated through float64 rounds twice).  mpmath has no exponent limits: the model is for operands inside the f32 range, which
  is what prep's switch-off leaves.
* point_row / group_row: the f32 rows of setpoints.hip (coordinates and P; the stored centre, the inflated radius about it, Pmax).
* refit_reference: the total-least-squares line from the points alone at 50 digits, with the tolerance of DESIGN.md 4.5a at the top
  of the spectrum.
"""
import os
import re

import numpy as np

EPS = 2.0 ** -52
U32 = 2.0 ** -24
SYM_MODEL = np.zeros(18)
SYM_MODEL[8] = SYM_MODEL[17] = 1.0


# ---- the exact path ---------------------------------------------------------------------------------------------------------------
def cross_components(pts, m):
    e0, e1, e2 = pts[:, 0] - m[0], pts[:, 1] - m[1], pts[:, 2] - m[2]
    c0 = e1 * m[5] - e2 * m[4]
    c1 = -(e0 * m[5] - e2 * m[3])
    c2 = e0 * m[4] - e1 * m[3]
    return c0, c1, c2


def sq_line3d(pts, m):
    with np.errstate(invalid="ignore", over="ignore"):
        c0, c1, c2 = cross_components(pts, m)
        return (c0 * c0 + c1 * c1) + c2 * c2


def sym_points(pts, m):
    """the points whose symmetric-transfer residual under SYM_MODEL is sq_line3d(pts, m)"""
    c0, c1, c2 = cross_components(pts, m)
    return np.ascontiguousarray(np.column_stack([c2, np.zeros(len(pts)), c0, c1]))


# ---- the f32 filter ---------------------------------------------------------------------------------------------------------------
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "progressive-x_amd", "csrc", "score_filters.hip.h")

# The four axial filters (3-D line, cylinder, cone, torus) share AxialFilter32 in the header, and their restatements share this part:
# the literals and statements of the shared block, prep's opening and end, the tails of reject and group_reject.  A type's module
# (this one for the 3-D line) states its shape: its own literals and statements, its budget lines and the quantity that is compared.
SHARED_LITERALS = dict(u=5.9604644775390625e-8, dn_inflate=1.001, pn_inflate=1.001, pscale_max=1e17, pn_max=1e17, ts_min=1e-30,
                       ts_max=1e30, margin_inv=64.0, group_l1_rho=1.74, group_rho=1.001, group_tpp=1.001)

_NUM = r"([0-9][0-9.e+-]*)"
_SHARED_PATTERNS = [
    (("u",), r"const double u = NUM;"),
    (("dn_inflate",), r"const double dn = sqrt\(\(d\[0\] \* d\[0\] \+ d\[1\] \* d\[1\]\) \+ d\[2\] \* d\[2\]\) \* NUM;"),
    (("pn_inflate",), r"const double pn = sqrt\(\(m\[0\] \* m\[0\] \+ m\[1\] \* m\[1\]\) \+ m\[2\] \* m\[2\]\) \* NUM;"),
    (("pscale_max", "pn_max", "ts_min", "ts_max"),
     r"const bool out = !\(pscale <= NUM\) \|\| !\(pn <= NUM\) \|\| !\(Ts > NUM\) \|\| !\(Ts < NUM\) \|\| off;"),
    (("margin_inv",), r"ln\.tpp = f32_up\(Ts \* \(1\.0 \+ 1\.0 / NUM\)\);"),
    (("group_l1_rho",), r"__builtin_fmaf\(NUMf, g\[3\], l1\)"),
    (("group_rho",), r"- ln\.nrm \* g\[3\] \* NUMf;"),
    (("group_tpp",), r"return m > ln\.tpp \* NUMf;"),
]

# the shared block's statements of the f32 test's operation order, as prep_open, dist, height, reject_tail and group_tail restate them
SHARED_OPERATION_LINES = [
    "const double Ts = sqrt(T2) * sc;",
    "const float e0 = p[0] - ln.p[0], e1 = p[1] - ln.p[1], e2 = p[2] - ln.p[2];",
    "const float c0 = __builtin_fmaf(e1, d[2], -(e2 * d[1]));",
    "const float c1 = __builtin_fmaf(e2, d[0], -(e0 * d[2]));",
    "const float c2 = __builtin_fmaf(e0, d[1], -(e1 * d[0]));",
    "*l1 = (fabsf(e0) + fabsf(e1)) + fabsf(e2);",
    "return sqrtf(__builtin_fmaf(c0, c0, __builtin_fmaf(c1, c1, c2 * c2)));",
    "return __builtin_fmaf(e2, ln.d[2], __builtin_fmaf(e1, ln.d[1], e0 * ln.d[0]));",
    "const float a = Shape::magnitude(p, ln, &l1);",
    "const float m = a - __builtin_fmaf(ln.e2, l1, __builtin_fmaf(ln.e1, p[5], ln.e0));",
    "return m > ln.tpp;",
    "if (ln.nanh != 0.0f) return true;",
    "const float a = Shape::magnitude(g, ln, &l1);",
    "const float m = a - __builtin_fmaf(ln.e2, __builtin_fmaf(1.74f, g[3], l1), __builtin_fmaf(ln.e1, g[4], ln.e0)) - ln.nrm * g[3] * 1.001f;",
    "return m > ln.tpp * 1.001f;",
]

# the 3-D line's shape: LineShape32
MODEL_LITERALS = dict(SHARED_LITERALS, e1=2.0, e0=2.0, floor=1e-18, e2=8.0)
_LITERAL_PATTERNS = [
    (("e1",), r"ln\.e1 = f32_up\(NUM \* u \* dn\);"),
    (("e0", "floor"), r"ln\.e0 = big \? __builtin_inff\(\) : f32_up\(NUM \* u \* dn \* pn \+ NUM\);"),
    (("e2",), r"ln\.e2 = f32_up\(NUM \* u \* dn\);"),
]
OPERATION_LINES = SHARED_OPERATION_LINES + [
    "ln.nrm = f32_up(dn);",
    "static __device__ __forceinline__ float magnitude(const float* p, const Lane& ln, float* l1) { return axial_dist(p, ln, l1); }",
]


def shared_block():
    """the header's text from the axial family's opening comment to the end of `template <class Shape> struct AxialFilter32 { ... };`"""
    text = open(HEADER).read()
    start = text.index("// ---- the axial family:")
    return text[start:text.index("\n};\n", text.index("template <class Shape> struct AxialFilter32 : Shape {", start))]


def shape_block(shape):
    """the text of `struct <shape> { ... };` in score_filters.hip.h"""
    text = open(HEADER).read()
    start = text.index("struct %s {" % shape)
    return text[start:text.index("\n};\n", start)]


def read_literals(block, patterns):
    """the patterns' literals as `block` has them, each pattern found exactly once"""
    out = {}
    for names, pat in patterns:
        found = re.findall(pat.replace("NUM", _NUM), block)
        assert len(found) == 1, (names, found)
        values = found[0] if isinstance(found[0], tuple) else (found[0],)
        for k, v in zip(names, values):
            out[k] = float(v)
    return out


def axial_header_block(shape):
    """the shared block followed by the shape's: where a type's statements stand"""
    return shared_block() + "\n" + shape_block(shape)


def axial_header_literals(shape, patterns):
    """a type's MODEL_LITERALS as the header's text has them: the shared ones read from the shared block, its own from its shape's"""
    return dict(read_literals(shared_block(), _SHARED_PATTERNS), **read_literals(shape_block(shape), patterns))


def header_block():
    return axial_header_block("LineShape32")


def header_literals():
    return axial_header_literals("LineShape32", _LITERAL_PATTERNS)


_ctx = None


def _mp24():
    global _ctx
    if _ctx is None:
        import mpmath
        _ctx = mpmath.mp.clone()
        _ctx.prec = 24
    return _ctx


def f32(x):
    with np.errstate(over="ignore"):
        return float(np.float32(x))


def f32_up(x):
    return f32(x * 1.000001)           # kInflate


def pow2_normaliser(d):
    mx = 0.0
    for v in d:
        a = abs(float(v))
        if a > mx:                     # NaN entries are skipped by the comparison
            mx = a
    off = not (mx >= 1e-75) or not (mx <= 1e75)
    if not (mx > 0.0) or not (mx < 1.7976931348623157e308):
        return 1.0, off
    _, e = np.frexp(mx)
    return float(np.ldexp(1.0, -int(e))), off


def axial_prep(m, pscale, T2, L, budget, plant_zero_budget=False):
    """AxialFilter32<Shape>::prep in float64, the lane's floats as Python floats holding f32 values: the shared opening, then
    budget(ln, m, sc, dn, pn, u, out) - the shape's own fields, e1, e0, e2 and nrm - and tpp.  plant_zero_budget: E = 0, for the test
    that shows a missing budget is seen."""
    m = [float(v) for v in m]
    sc, off = pow2_normaliser(m[3:6])
    with np.errstate(over="ignore", invalid="ignore"):
        d = [np.float64(m[3 + k]) * sc for k in range(3)]
        ln = dict(p=[f32(m[k]) for k in range(3)], d=[f32(d[k]) for k in range(3)])
        ln["nanh"] = 1.0 if any(v != v for v in m) else 0.0
        Ts = np.sqrt(np.float64(T2)) * sc
        dn = np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]) * L["dn_inflate"]
        pn = np.sqrt((np.float64(m[0]) * m[0] + np.float64(m[1]) * m[1]) + np.float64(m[2]) * m[2]) * L["pn_inflate"]
        out = not (pscale <= L["pscale_max"]) or not (pn <= L["pn_max"]) or not (Ts > L["ts_min"]) or not (Ts < L["ts_max"]) or off
        budget(ln, m, sc, dn, pn, L["u"], out)
        ln["tpp"] = f32_up(Ts * (1.0 + 1.0 / L["margin_inv"]))
        ln["lit"] = L
    if plant_zero_budget:
        ln["e1"] = ln["e0"] = ln["e2"] = 0.0
    return ln


def prep(m, pscale, T2, plant_zero_budget=False, lit=None):
    """Filter32<kLine3D>::prep"""
    L = MODEL_LITERALS if lit is None else lit

    def budget(ln, m, sc, dn, pn, u, big):
        ln["e1"] = f32_up(L["e1"] * u * dn)
        ln["e0"] = float("inf") if big else f32_up(L["e0"] * u * dn * pn + L["floor"])
        ln["e2"] = f32_up(L["e2"] * u * dn)
        ln["nrm"] = f32_up(dn)
    return axial_prep(m, pscale, T2, L, budget, plant_zero_budget)


def _fma(c, a, b, d):
    return c.fadd(c.fmul(a, b, exact=True), d)      # one rounding, to the context's 24 bits


def _dist(row, ln):
    """axial_dist: (s~, l~)"""
    c = _mp24()
    x = [c.mpf(v) for v in row[:3]]
    p = [c.mpf(v) for v in ln["p"]]
    d = [c.mpf(v) for v in ln["d"]]
    e0, e1, e2 = x[0] - p[0], x[1] - p[1], x[2] - p[2]
    c0 = _fma(c, e1, d[2], -(e2 * d[1]))
    c1 = _fma(c, e2, d[0], -(e0 * d[2]))
    c2 = _fma(c, e0, d[1], -(e1 * d[0]))
    l1 = (abs(e0) + abs(e1)) + abs(e2)
    return c.sqrt(_fma(c, c0, c0, _fma(c, c1, c1, c2 * c2))), l1


def _height(row, ln):
    """axial_height: h~"""
    c = _mp24()
    x = [c.mpf(v) for v in row[:3]]
    p = [c.mpf(v) for v in ln["p"]]
    d = [c.mpf(v) for v in ln["d"]]
    e0, e1, e2 = x[0] - p[0], x[1] - p[1], x[2] - p[2]
    return _fma(c, e2, d[2], _fma(c, e1, d[1], e0 * d[0]))


def axial_reject(magnitude, row, ln):
    """row = (x~, y~, z~, P): AxialFilter32<Shape>::reject with the shape's magnitude(row, ln) = (the compared quantity, l~)"""
    c = _mp24()
    a, l1 = magnitude(row, ln)
    m = a - _fma(c, c.mpf(ln["e2"]), l1, _fma(c, c.mpf(ln["e1"]), c.mpf(row[3]), c.mpf(ln["e0"])))
    return bool(m > c.mpf(ln["tpp"]))


def axial_group_reject(magnitude, g, ln):
    """g = (centre[3], rho, Pmax): AxialFilter32<Shape>::group_reject"""
    if ln["nanh"] != 0.0:
        return True
    c = _mp24()
    a, l1 = magnitude(g, ln)
    rho, L = c.mpf(g[3]), ln["lit"]
    E = _fma(c, c.mpf(ln["e2"]), _fma(c, c.mpf(f32(L["group_l1_rho"])), rho, l1), _fma(c, c.mpf(ln["e1"]), c.mpf(g[4]), c.mpf(ln["e0"])))
    m = a - E - c.mpf(ln["nrm"]) * rho * c.mpf(f32(L["group_rho"]))
    return bool(m > c.mpf(ln["tpp"]) * c.mpf(f32(L["group_tpp"])))


def reject(row, ln):
    """Filter32<kLine3D>::reject: s~ itself is compared"""
    return axial_reject(_dist, row, ln)


def group_reject(g, ln):
    """Filter32<kLine3D>::group_reject"""
    return axial_group_reject(_dist, g, ln)


def point_row(x):
    return [f32(x[0]), f32(x[1]), f32(x[2]), f32(max(1.0, abs(x[0]), abs(x[1]), abs(x[2])) * 1.000001)]


def group_row(pts):
    """sp_line_bounds_kernel<SPAN, 3>: the box centre in f32, the radius about the STORED centre and the largest P, inflated"""
    centre = np.float32(0.5 * (pts.min(axis=0) + pts.max(axis=0))).astype(np.float64)
    df = pts - centre
    R2 = ((df[:, 0] * df[:, 0] + df[:, 1] * df[:, 1]) + df[:, 2] * df[:, 2]).max()
    return [float(centre[0]), float(centre[1]), float(centre[2]), f32(np.sqrt(R2) * 1.00001 + 1e-30),
            f32(max(1.0, np.abs(pts).max()) * 1.000002)]


# ---- pairs near the threshold -------------------------------------------------------------------------------------------------------
def near_threshold_points(rng, line, T, n, along):
    """n points at distance T (1 +- 0.5e-4) from the unit-direction line (p, d), at positions uniform in +-along along it: a point on
    the axis moved along a random perpendicular"""
    p, d = np.asarray(line[:3]), np.asarray(line[3:])
    a = np.cross(d, [1.0, 0.0, 0.0] if abs(d[0]) < 0.9 else [0.0, 1.0, 0.0])
    a /= np.linalg.norm(a)
    b = np.cross(d, a)
    phi = rng.uniform(0, 2 * np.pi, n)
    target = T * (1.0 + rng.uniform(-0.99e-4 / 2, 0.99e-4 / 2, n))
    perp = np.cos(phi)[:, None] * a + np.sin(phi)[:, None] * b
    return np.ascontiguousarray(p + rng.uniform(-along, along, n)[:, None] * d + target[:, None] * perp)


def morton_order(pts, bits=10):
    lo, hi = pts.min(axis=0), pts.max(axis=0)
    q = np.minimum(((pts - lo) / np.where(hi > lo, hi - lo, 1.0) * (1 << bits)).astype(np.int64), (1 << bits) - 1)
    key = np.zeros(len(pts), np.int64)
    for b in range(bits):
        for k in range(3):
            key |= ((q[:, k] >> b) & 1) << (3 * b + k)
    return np.argsort(key, kind="stable")


# ---- refit fixtures -------------------------------------------------------------------------------------------------------------------
def known_line(rng, n, offset=0.0):
    d = rng.normal(size=3)
    d /= np.linalg.norm(d)
    if d[int(np.argmax(np.abs(d)))] < 0:
        d = -d
    p = rng.uniform(3, 7, 3) + offset
    t = rng.uniform(-4, 4, n)
    return np.ascontiguousarray(p + t[:, None] * d), p, d


REFIT_N = (2, 3, 63, 64, 65, 129, 1000)


def refit_fixture(n, offset, weights, seed):
    """a noisy line with 20 % outliers (where n allows), `offset` from the origin; weights: None, "mild" in [0.5, 1.5], "wide" over
    1e-3 .. 1e3 with one exact zero (n >= 3)"""
    rng = np.random.default_rng(seed)
    pts, _, _ = known_line(rng, n, offset)
    pts = pts + rng.normal(0, 0.01, pts.shape)
    k = n // 5
    if k:
        pts[:k] = rng.uniform(0, 10, (k, 3)) + offset
    w = None
    if weights == "mild":
        w = rng.uniform(0.5, 1.5, n)
    elif weights == "wide":
        w = 10.0 ** rng.uniform(-3, 3, n)
        if n >= 3:
            w[n // 2] = 0.0
    return np.ascontiguousarray(pts), w


# ---- the refit at 50 digits ---------------------------------------------------------------------------------------------------------
def refit_reference(pts, w=None):
    """(mean, direction, tol, |mean|): the weighted mean, the unit eigenvector of the largest eigenvalue of the centred weighted
    scatter (largest-magnitude component positive), and tol = 32 eps lambda_max / (lambda_1 - lambda_2) with lambda_max the 2-norm of
    the un-centred moments sum w p p^T and lambda_1 >= lambda_2 the two largest eigenvalues of the scatter - all from the points alone
    at 50 digits"""
    import mpmath
    mp = mpmath.mp.clone()
    mp.dps = 50
    P = [[mp.mpf(float(x)) for x in row] for row in np.asarray(pts, dtype=np.float64)]
    ww = [mp.mpf(1)] * len(P) if w is None else [mp.mpf(float(x)) for x in w]
    W = sum(ww)
    mean = [sum(wi * p[k] for wi, p in zip(ww, P)) / W for k in range(3)]
    S, M = mp.zeros(3, 3), mp.zeros(3, 3)
    for wi, p in zip(ww, P):
        if wi == 0:
            continue
        q = [p[k] - mean[k] for k in range(3)]
        for i in range(3):
            for j in range(3):
                S[i, j] += wi * q[i] * q[j]
                M[i, j] += wi * p[i] * p[j]
    E, Q = mp.eigsy(S)
    order = sorted(range(3), key=lambda k: E[k])
    d = [Q[r, order[2]] for r in range(3)]
    big = max(range(3), key=lambda k: (abs(d[k]), -k))
    if d[big] < 0:
        d = [-x for x in d]
    lam_max = max(abs(x) for x in mp.eigsy(M, eigvals_only=True))
    tol = 32.0 * EPS * float(lam_max) / float(E[order[2]] - E[order[1]])
    mean_f = np.array([float(x) for x in mean])
    return mean_f, np.array([float(x) for x in d]), tol, float(np.linalg.norm(mean_f))


def refit_ratios(model, ref):
    """(direction error / tol, perpendicular mean error / its bound) of a fitted model (p, d) against refit_reference's result"""
    mean, d, tol, mn = ref
    de = float(np.linalg.norm(model[3:] - d))
    diff = model[:3] - mean
    perp = float(np.linalg.norm(diff - (diff @ d) * d))
    return de / tol, perp / (tol * mn + 4.0 * EPS * mn) if mn > 0 else (0.0 if perp == 0 else np.inf)
