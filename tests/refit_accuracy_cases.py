"""The refit accuracy fixtures (tests/golden/kat_refits_v1.npz, written by tests/golden/make_golden_refits.py from the 50-digit
restatement tests/refit_exact.py) and the comparisons that hold a context's refits to them: shared by the CPU file
(tests/test_refit_accuracy_cpu.py, OracleContext) and the GPU file (tests/test_gpu_refit_accuracy.py).  TEST INFRASTRUCTURE; next to the
product's estimators it needs numpy and the standard library only (no mpmath).

Per type: one point set; two resident weight vectors shared by all types (uniform in [0.5, 1.5]; spanning 1e-3 .. 1e3 with an exact
zero at ZERO_AT); one labelling; the selections -
  index lists of the minimal size and one more, of 9, 21, 63, 64, 65, 128, 129, 200 points (one wave per selection in pgx_gram_batch
  and pgx_pnp_refine_batch: below, at and above 64 and 128), one with a repeated index, 100 inliers of one structure ("inliers"),
  80 inliers and 20 outliers ("mixed"), labels 0 (200 points spread over the set: pgx_gram reduces across blocks) and 1, and a copy
  of one list moved by 1e4 (H, F, VP) or 1e3 (line, plane);
every selection without weights and with the uniform ones, three of them with the wide ones.  A fixture row holds the reference's
answer and the tolerance (the C_ columns).

What is compared: the forward error in the normalised space where the eigenproblem is posed - the product's model
is carried there in exact rational arithmetic with the reference's normalisation, scaled to unit norm, aligned in sign - against
tol = 32 eps lambda_max / (lambda_2 - lambda_1) of the reference's A^T A (line and plane: the un-centred moments' norm over the
centred scatter's gap, and |dc| <= tol |mean| + 4 eps |mean|; fundamental: times 1 + 2 s3 / (s2 - s3)); the plain invariants of
each model; and for the pose a single Gauss-Newton step against the reference's and the reference's step at the pose the
product's 10 iterations return."""
import os
from fractions import Fraction

import numpy as np

import refit_exact
from pyprogressivex import _estimators, _lib

FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kat_refits_v1.npz")
SEED = 3
BASE, NMAX, ZERO_AT, WIDTH = 300, 364, 7, 44
STORED = ["line", "homography", "fundamental", "pnp", "vanishing_point", "plane", "sphere", "circle"]
TYPES = STORED + ["homography_sym"]
FAMILY = dict(line="flat", plane="flat", circle="round", sphere="round", vanishing_point="vp", homography="two_view",
              homography_sym="two_view", fundamental="two_view", pnp="pnp")
MINIMAL = dict(line=2, plane=3, circle=3, sphere=4, vanishing_point=2, homography=4, fundamental=8, pnp=4)
EPS = 2.0 ** -52
# fixture row: the eigen-fits ...
C_TOL, C_LMAX, C_GAP, C_FAC, C_SENS = 0, 1, 2, 3, 4
C_NORM, C_THETA, C_MODEL = slice(5, 11), slice(11, 20), slice(20, 32)
# ... and the pose: at the start (0) and at the reference's converged pose (S)
C_INV0, C_J0, C_R0, C_JTJ0, C_ND0, C_KAPPA, C_FIRST, C_INVS, C_JS, C_RS = 1, 2, 3, 4, 5, 6, 7, 8, 9, 10
C_D0, C_START = slice(11, 17), slice(32, 44)


class Case:
    """one type's fixtures: pts, labels, K, sels [(index | None, label)], fixtures [(selection number, weighting, row)]"""


def load():
    z = np.load(FILE)
    W = z["w"]
    out = {}
    for name in TYPES:
        t = STORED.index("homography" if name == "homography_sym" else name)
        c = Case()
        c.name, c.n = name, int(z["npts"][t, 0])
        c.d = _lib.POINT_DIM[_estimators.ESTIMATORS[name].model_type]
        c.pts = np.ascontiguousarray(z["pts"][t, :c.n, :c.d])
        c.labels = z["labels"][t, :c.n].astype(np.int32)
        c.K = 3
        c.weights = [None, np.ascontiguousarray(W[0, :c.n]), np.ascontiguousarray(W[1, :c.n])]
        numbers = [k for k in range(len(z["selinfo"])) if z["selinfo"][k, 0] == t]
        c.sels = []
        for k in numbers:
            _, start, length, label = z["selinfo"][k]
            c.sels.append((None, int(label)) if label >= 0 else (z["sel"][start:start + length].astype(np.int64), -1))
        c.fixtures = [(numbers.index(int(s)), int(wt), z["fx"][f]) for f, (tt, s, wt) in enumerate(z["meta"]) if tt == t]
        c.start = z["pnp_start"] if name == "pnp" else None          # the start of the pose's single steps (a run starts at C_START)
        out[name] = c
    return out


def members(case, s):
    idx, label = case.sels[s]
    return np.flatnonzero(case.labels == label) if idx is None else idx


# ---- a model in the normalised space, exactly ---------------------------------------------------------------------------------
def _frac(a):
    return [[Fraction(float(x)) for x in r] for r in np.asarray(a, dtype=np.float64)]


def _mul(A, B):
    return [[sum(A[i][k] * B[k][j] for k in range(len(B))) for j in range(len(B[0]))] for i in range(len(A))]


def _unit_aligned(v, ref):
    v = np.array([float(x) for x in v])
    v = v / np.linalg.norm(v)
    return v if float(v @ ref) >= 0 else -v


def theta_of(name, model, row):
    """the model as the unit vector of the reference's normalised space, signed like the reference's (rational arithmetic up to the
    last scaling, so that what is measured is the product's error and not the mapping's)"""
    fam = FAMILY[name]
    q = dict(flat=0, vp=3, two_view=9)
    ref = row[C_THETA]
    model = np.asarray(model, dtype=np.float64)
    if fam == "vp":
        return _unit_aligned(model, ref[:3])
    if fam == "flat":
        d = len(model) - 1
        return _unit_aligned(model[:d], ref[:d])
    if fam == "round":
        d = len(model) - 1
        o, s = [Fraction(float(x)) for x in row[C_NORM][:d]], Fraction(float(row[C_NORM][d]))
        c, r = [Fraction(float(x)) for x in model[:d]], Fraction(float(model[d]))
        b = [(o[k] - c[k]) / s for k in range(d)]
        th = [sum(x * x for x in b) - (r / s) ** 2] + [2 * x for x in b] + [Fraction(1)]
        big = max(abs(x) for x in th)
        return _unit_aligned([x / big for x in th], ref[:d + 2])
    s1, cx1, cy1, s2, cx2, cy2 = [Fraction(float(x)) for x in row[C_NORM]]
    T1i = [[1 / s1, 0, cx1], [0, 1 / s1, cy1], [0, 0, 1]]
    M = _frac(model[:9].reshape(3, 3))
    if name == "fundamental":                                   # F = T2^T Fn T1
        T2it = [[1 / s2, 0, 0], [0, 1 / s2, 0], [cx2, cy2, 1]]
        N = _mul(_mul(T2it, M), T1i)
    else:                                                       # H = T2^-1 Hn T1
        T2 = [[s2, 0, -s2 * cx2], [0, s2, -s2 * cy2], [0, 0, 1]]
        N = _mul(_mul(T2, M), T1i)
    flat = [x for r in N for x in r]
    big = max(abs(x) for x in flat)
    return _unit_aligned([x / big for x in flat], ref[:q[fam]])


def ratio_of(name, model, row):
    """error / tolerance of one model against one fixture row (the larger of the two for a line or plane: normal and offset)"""
    th = theta_of(name, model, row)
    ref = row[C_THETA][:len(th)]
    ratio = float(np.linalg.norm(th - ref)) / row[C_TOL]
    if FAMILY[name] == "flat":
        d = len(th)
        sign = 1.0 if float(np.asarray(model[:d]) @ ref) >= 0 else -1.0
        ctol = row[C_TOL] * row[C_SENS] + 4 * EPS * row[C_SENS]
        if ctol > 0:
            ratio = max(ratio, abs(sign * model[d] - row[C_MODEL][d]) / ctol)
    return ratio


def check_invariants(name, model, where):
    model = np.asarray(model, dtype=np.float64)
    if name in ("homography", "homography_sym"):
        assert model[8] == 1.0, where
    if name == "homography_sym":
        H, Hi = model[:9].reshape(3, 3), model[9:].reshape(3, 3)
        assert np.abs(H @ Hi - np.eye(3)).max() <= 32 * EPS * np.linalg.cond(H), where
    if name == "fundamental":
        F = model.reshape(3, 3)
        assert abs(np.linalg.norm(F) - 1.0) <= 4 * EPS, where
        assert abs(np.linalg.det(F)) <= 32 * EPS, where
    if name == "pnp":
        R = model.reshape(3, 4)[:, :3]
        assert np.abs(R.T @ R - np.eye(3)).max() <= 64 * EPS, where        # ten Rodrigues updates of a few eps each
        assert np.linalg.det(R) > 0, where


# ---- the entry points ---------------------------------------------------------------------------------------------------------
def _one(models, where):
    assert len(models) == 1, where + ("no model",)
    return models[0]


def eigen_ratios(name, case, ctx, solver, strict=True, before=None):
    """Every fixture of an eigen-type through every entry point of one context: {(entry, selection number, weighting): ratio}.
    index selections: nonminimal (pgx_gram), nonminimal_batch (pgx_gram_batch, two rows: the list and the list reversed);
    label selections: nonminimal with the label, with the label's members as an index list, and nonminimal_labels
    (pgx_gram_labels, all labels in one call).  strict=False (the planted errors): a missing model or a broken invariant is
    the ratio inf instead of a failure, and before(weights) is called ahead of every fixture."""
    est = _estimators.ESTIMATORS[name]()
    est.refit_solver = solver
    ctx.set_points(est.model_type, case.pts)
    ctx.set_labels(case.labels)
    out = {}

    def note(entry, s, wt, row, models):
        where = (name, solver, entry, s, wt)
        try:
            model = _one(models, where)
            check_invariants(name, model, where)
            out[(entry, s, wt)] = ratio_of(name, model, row)
        except AssertionError:
            if strict:
                raise
            out[(entry, s, wt)] = np.inf

    by_labels = {}
    for s, wt, row in case.fixtures:
        idx, label = case.sels[s]
        w = case.weights[wt]
        if before is not None:
            before(w)
        if idx is None:
            note("nonminimal/label", s, wt, row, est.nonminimal(ctx, ("label", label), w))
            note("nonminimal/index", s, wt, row, est.nonminimal(ctx, ("index", members(case, s)), w))
            if wt not in by_labels:
                by_labels[wt] = est.nonminimal_labels(ctx, case.K, w)
            note("nonminimal_labels", s, wt, row, by_labels[wt][label])
        else:
            note("nonminimal/index", s, wt, row, est.nonminimal(ctx, ("index", idx), w))
            both = est.nonminimal_batch(ctx, np.stack([idx, idx[::-1]]), w)
            note("nonminimal_batch", s, wt, row, both[0])
            note("nonminimal_batch/reversed", s, wt, row, both[1])
    return out


def _delta_of(P0, P1):
    """(omega, dt) with R1 = exp([omega]x) R0, t1 = t0 + dt; R1 R0^T is formed exactly"""
    A, B = np.asarray(P0).reshape(3, 4), np.asarray(P1).reshape(3, 4)
    rel = _mul(_frac(B[:, :3]), [list(r) for r in zip(*_frac(A[:, :3]))])
    a = np.array([float(rel[2][1] - rel[1][2]), float(rel[0][2] - rel[2][0]), float(rel[1][0] - rel[0][1])]) / 2.0
    sn = float(np.linalg.norm(a))
    om = a * (np.arcsin(min(sn, 1.0)) / sn) if sn > 0 else a
    return np.concatenate([om, B[:, 3] - A[:, 3]])


def _host_one_step(est, ctx, idx, w, start):
    """one pass of PnPEstimator._fit_many over the context's pgx_gram_batch"""
    def gram(kind, prm, use_w, wpow, rows):
        G, bad = ctx.gram_batch(kind, idx[None], params=prm, weights=w if use_w else None, wpow=wpow)
        return G, np.full(len(rows), len(idx), dtype=np.int64), bad
    return est._fit_many(gram, 1, [start], iterations=1)[0]


def pose_ratios(case, ctx, strict=True):
    """Every pose fixture through every entry point: {(entry, selection number, weighting): ratio}.
    one step ("step/..."): pgx_pnp_refine_batch at iterations = 1 and one pass of _fit_many over pgx_gram_batch, against the
    reference's step from the same start, bound 32 eps |(JtJ)^-1| (|J| |r| + |JtJ| |delta|) - at every size.
    convergence ("run/..."), from the fixture's own start (the reference's run from it is below 1e-12 within 6 iterations): the 50-digit step at the pose returned after 10
    iterations by nonminimal (pgx_gram), nonminimal_labels (pgx_gram_labels) and nonminimal_batch (pgx_pnp_refine_batch),
    bound 1e-12 (the stop rule) + 32 eps |(JtJ)^-1| |J| |r| (the rounding of J^T r)."""
    est = _estimators.PnPEstimator()
    ctx.set_points(est.model_type, case.pts)
    ctx.set_labels(case.labels)
    out = {}

    def guarded(fn):
        def inner(entry, s, wt, row, models):
            try:
                fn(entry, s, wt, row, models)
            except AssertionError:
                if strict:
                    raise
                out[(entry, s, wt)] = np.inf
        return inner

    @guarded
    def step(entry, s, wt, row, models):
        where = ("pnp", entry, s, wt)
        P1 = _one(models, where)
        check_invariants("pnp", P1, where)
        out[(entry, s, wt)] = float(np.linalg.norm(_delta_of(case.start, P1) - row[C_D0])) / row[C_TOL]

    @guarded
    def run(entry, s, wt, row, models):
        where = ("pnp", entry, s, wt)
        P = _one(models, where)
        check_invariants("pnp", P, where)
        idx = members(case, s)
        w = case.weights[wt]
        left = refit_exact.pnp_step_decimal(case.pts[idx], None if w is None else w[idx], P)
        out[(entry, s, wt)] = float(np.linalg.norm(left)) / (1e-12 + 32 * EPS * row[C_INVS] * row[C_JS] * row[C_RS])

    for s, wt, row in case.fixtures:
        sel, label = case.sels[s]
        idx = members(case, s)
        w = case.weights[wt]
        start = case.start.copy()
        P1, ok = ctx.pnp_refine_batch(start[None], idx[None], weights=w, wpow=2, iterations=1)
        step("step/pnp_refine_batch", s, wt, row, [P1[0]] if ok[0] else [])
        step("step/_fit_many", s, wt, row, _host_one_step(est, ctx, idx, w, start))
        start = row[C_START].copy()
        if sel is None:
            run("run/nonminimal/label", s, wt, row, est.nonminimal(ctx, ("label", label), w, init=start))
            run("run/nonminimal_labels", s, wt, row, est.nonminimal_labels(ctx, case.K, w, inits=[start] * case.K)[label])
        else:
            run("run/nonminimal/index", s, wt, row, est.nonminimal(ctx, ("index", idx), w, init=start))
        both = est.nonminimal_batch(ctx, np.stack([idx, idx[::-1]]), w, init=start)
        run("run/nonminimal_batch", s, wt, row, both[0])
        run("run/nonminimal_batch/reversed", s, wt, row, both[1])
    return out


def report(name, where, ratios):
    """the line the tests print: the worst error / tolerance of a type, and where"""
    key = max(ratios, key=ratios.get)
    return f"refit accuracy [{where}] {name}: worst error/tolerance {ratios[key]:.3g} over {len(ratios)} comparisons, at {key}"
