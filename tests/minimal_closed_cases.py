"""The closed-form minimal solvers' accuracy fixtures (tests/golden/kat_minimal_closed_v1.npz, written by
tests/golden/make_golden_minimal_closed.py from the 50-digit statements of tests/minimal_closed_exact.py) and what holds
pgx_solve_minimal's nine lane-per-model solvers and Estimator.minimal to them: the sibling of tests/minimal_accuracy_cases.py, whose
Case, read_case, match, batch_of, device_ratios and report it uses - the set comparison is written there, once.  Shared by the CPU
file (tests/test_minimal_closed_accuracy_cpu.py) and the GPU file (tests/test_gpu_minimal_closed_accuracy.py).  TEST INFRASTRUCTURE;
numpy and the standard library only (no mpmath).

Per type, point sets (with normals where the type reads them) by the ranges that are resident with them - pgx_set_radius_range and
pgx_set_major_radius_range are context state, so a class that needs a range is a set of its own -, the minimal samples as index rows
into their set, and per sample the reference's solution set (NaN padded), each solution's problem condition, kappa_route and
tolerance 32 eps kappa_route.  The kinds ACCURACY, COVERAGE and NO_MODEL are minimal_accuracy_cases'; one more:
  RANGE      coordinates whose squares overflow (>= 1e155) or differences whose squares or cubes underflow: every slot is all NaN or
             within tolerance of a reference solution of its own; a finite or partly NaN row that is neither is a defect.
Compared as returned, in max-entry distance; the line, the plane and the vanishing point up to one overall sign, the cylinder's and
the torus' d up to sign (the cone's d points into the nappe; the 3-D line's follows b - a).  Per returned model (CHECKS): unit
vectors within 4 eps, c^2 + s^2 = 1 within the bound its two stages leave, r >= 0, R > r; and the exact contracts - the line's normal
has the signs of (-dy, dx), the plane's those of (p1 - p0) x (p2 - p0), wherever the component exceeds its tolerance (rational
arithmetic), the 3-D line's point is the first sample's bits."""
import os
from fractions import Fraction

import numpy as np

import minimal_accuracy_cases as cases
from minimal_accuracy_cases import ACCURACY, COVERAGE, NO_MODEL, RANGE
from pyprogressivex import _estimators

FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kat_minimal_closed_v1.npz")
SEED = 23
EPS = 2.0 ** -52
INF = float("inf")
TYPES = ["line", "vanishing_point", "plane", "sphere", "circle", "line3d", "cylinder", "cone", "torus"]
ORIENTED = ("cylinder", "cone", "torus")
KEY = dict(line="l", vanishing_point="v", plane="pl", sphere="s", circle="c", line3d="l3", cylinder="cy", cone="co", torus="t")
SLOTS = dict(line=1, vanishing_point=1, plane=1, sphere=1, circle=1, line3d=1, cylinder=1, cone=1, torus=2)
PARAMS = dict(line=3, vanishing_point=3, plane=4, sphere=4, circle=3, line3d=6, cylinder=7, cone=8, torus=8)
SAMPLE = dict(line=2, vanishing_point=2, plane=3, sphere=4, circle=3, line3d=2, cylinder=2, cone=3, torus=4)
DIM = dict(line=2, vanishing_point=4, plane=3, sphere=3, circle=2, line3d=3, cylinder=3, cone=3, torus=3)
FLIP = dict(line=[-1, -1, -1], vanishing_point=[-1, -1, -1], plane=[-1, -1, -1, -1], cylinder=[1, 1, 1, -1, -1, -1, 1],
            torus=[1, 1, 1, -1, -1, -1, 1, 1])
FULL = (0.0, INF, 0.0, INF)
# rows = slots x S crosses the 256-thread block of solve_kernel at these S
BATCHES = {name: (1, 255, 256, 257) for name in TYPES}
BATCHES["torus"] = (1, 127, 128, 129, 255, 256, 257)
# (set, (rmin, rmax, Rmin, Rmax)): the ranges resident with the set
_ROUND_SETS = [("general", FULL), ("excluded", (2.5, 3.5, 0.0, INF)), ("bound", (1.5, 1.5, 0.0, INF))]
SETS = dict(line=[("general", FULL)], vanishing_point=[("general", FULL)], plane=[("general", FULL)], sphere=_ROUND_SETS,
            circle=_ROUND_SETS, line3d=[("general", FULL)], cylinder=[("general", FULL)], cone=[("general", FULL)],
            torus=[("general", FULL), ("major capped", (0.0, INF, 0.0, 100.0)), ("tube", (0.4, 0.6, 0.0, INF)),
                   ("major", (0.0, INF, 1.8, 2.2))])


def _table(degenerate, more=()):
    """(class, set, samples, kind): the classes every type has, its exact degeneracies, its own classes, the RANGE classes"""
    rows = [("coordinates of order 1", "general", 8, ACCURACY), ("coordinates of order 1e3", "general", 8, ACCURACY),
            ("coordinates of order 2^-10", "general", 8, ACCURACY), ("scene offset 1e6, size 1", "general", 8, ACCURACY),
            ("repeated index", "general", 8, NO_MODEL), ("out-of-range index", "general", 8, NO_MODEL)]
    rows += [(c, "general", 8, NO_MODEL) for c in degenerate] + list(more)
    return rows + [("huge coordinates, squares overflow", "general", 8, RANGE), ("tiny differences, squares underflow", "general", 8, RANGE),
                   ("tiny differences, cubes underflow", "general", 8, RANGE)]


def _round(flat, nearly):
    return _table(["coincident points", flat], [(nearly, "general", 8, ACCURACY), ("radius range excludes the solution", "excluded", 8, NO_MODEL),
                                                ("radius exactly at both bounds", "bound", 8, ACCURACY)])


CLASSES = dict(
    line=_table(["coincident points"]),
    # (two parallel segments on distinct lines HAVE a vanishing point, the direction at infinity: by the definition that is a model)
    vanishing_point=_table(["collinear segments", "a segment of length zero"], [("parallel segments", "general", 8, ACCURACY)]),
    plane=_table(["coincident points", "collinear points"]),
    sphere=_round("coplanar points", "nearly coplanar points"),
    circle=_round("collinear points", "nearly collinear points"),
    line3d=_table(["coincident points"]),
    cylinder=_table(["a zero normal", "parallel normals"],
                    [("normals flipped", "general", 8, ACCURACY), ("normals rescaled by 2^+-20", "general", 8, ACCURACY),
                     ("normals 1 degree apart", "general", 8, ACCURACY), ("coincident points, different normals", "general", 8, ACCURACY)]),
    cone=_table(["a zero normal", "the same point twice", "c <= 0 refused", "a sample at the apex"],
                [("normals flipped", "general", 8, ACCURACY), ("normals rescaled by 2^+-20", "general", 8, ACCURACY),
                 ("half-angle 5 degrees", "general", 8, ACCURACY), ("half-angle 85 degrees", "general", 8, ACCURACY),
                 ("the sign flip is taken", "general", 8, ACCURACY)]),
    torus=_table(["a zero normal in each place", "no real transversal"],
                 [("two transversals, both accepted", "general", 8, ACCURACY), ("two transversals, one accepted", "general", 8, ACCURACY),
                  ("discriminant near zero", "general", 8, ACCURACY), ("second transversal far away", "major capped", 8, ACCURACY),
                  ("tube-radius range cuts a slot", "tube", 8, ACCURACY), ("major-radius range cuts a slot", "major", 8, ACCURACY)]))
FIELDS = cases.FIELDS


# ---- per returned model: the invariants and the exact contracts ---------------------------------------------------------------------
def _unit(v, what):
    assert abs(np.linalg.norm(v) - 1.0) <= 4 * EPS, (what, float(np.linalg.norm(v)) - 1.0)


def _sample_rows(case, f):
    return case.sets[case.set_of[f]][1][case.samples[f]]


def _signs_follow(model, ref, tol, exact, what):
    for k, e in enumerate(exact):
        if abs(ref[k]) > tol:
            assert e != 0 and (model[k] > 0) == (e > 0), (what, k, float(model[k]), float(e))


def _check(name):
    def check(case, f, model, ref, tol):
        m = np.asarray(model, dtype=np.float64)
        if name in ("line", "plane"):
            _unit(m[:-1], "unit normal")
            P = [[Fraction(float(x)) for x in r] for r in _sample_rows(case, f)]
            if name == "line":
                exact = [-(P[1][1] - P[0][1]), P[1][0] - P[0][0]]
            else:
                u, v = [P[1][k] - P[0][k] for k in range(3)], [P[2][k] - P[0][k] for k in range(3)]
                exact = [u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]]
            _signs_follow(m, ref if (m[:-1] @ ref[:-1]) > 0 else -ref, tol, exact, "the normal's sign")
        if name == "vanishing_point":
            _unit(m, "unit norm")
        if name in ("sphere", "circle", "cylinder"):
            assert m[-1] >= 0, ("r >= 0", m[-1])
        if name == "line3d":
            assert m[:3].tobytes() == _sample_rows(case, f)[0].tobytes(), "p is the first sample's bits"
        if name in ("line3d", "cylinder", "cone", "torus"):
            _unit(m[3:6], "unit direction")
        if name == "cone":
            c, s = m[6], m[7]
            # |g0|^2 |d|^2 = 1 within 7 eps (two unit vectors of 3.5 roundings each); c = d . g0 adds 3, s = |g0 x d| adds 6 roundings
            # of eps / 2, times 2 c and 2 s: the bound the stages "c" and "s" leave
            assert c > 0 and s >= 0 and abs(c * c + s * s - 1.0) <= EPS * (8 + 3 * c + 6 * s), ("c^2 + s^2", c * c + s * s - 1.0)
        if name == "torus":
            assert m[6] > m[7] >= 0, ("R > r >= 0", m[6], m[7])
    return check


for _name in TYPES:
    cases.CLASSES[_name], cases.SLOTS[_name], cases.PARAMS[_name], cases.COMPARED[_name] = CLASSES[_name], SLOTS[_name], PARAMS[_name], PARAMS[_name]
    cases.AS_RETURNED.add(_name)
    cases.CHECKS[_name] = _check(_name)
    if _name in FLIP:
        cases.FLIP[_name] = [float(x) for x in FLIP[_name]]


def class_number(name, cname):
    return [c[0] for c in CLASSES[name]].index(cname)


def load():
    """{type: Case}: minimal_accuracy_cases.Case with, besides its fields, ranges [sets, 4], normals [per set, or None] and
    prepare(ctx, s) - what device_ratios makes resident with set s (s = None: the ranges as at creation)"""
    z = np.load(FILE)
    out = {}
    for name in TYPES:
        k = KEY[name]
        c = cases.read_case(z, name, k, [s for s, _ in SETS[name]], FIELDS)
        c.ranges = np.array([r for _, r in SETS[name]])
        c.normals = [np.ascontiguousarray(z[k + "_nrm"][z[k + "_ptset"] == s]) for s in range(len(c.sets))] if name in ORIENTED else None

        def prepare(ctx, s, c=c):
            rng = FULL if s is None else c.ranges[s]
            ctx.set_radius_range(rng[0], rng[1])
            if hasattr(ctx, "set_major_radius_range"):
                ctx.set_major_radius_range(rng[2], rng[3])
            if s is not None and c.normals is not None:
                ctx.set_normals(c.normals[s])
        c.prepare = prepare
        out[name] = c
    return out


def device_ratios(name, case, ctx, strict=True, batches=None):
    """every fixture through ctx.solve_minimal at every batch size: {(set, S, fixture): error / tolerance}"""
    return cases.device_ratios(name, case, ctx, strict, batches or BATCHES[name])


def estimator(name, case, s):
    est = _estimators.ESTIMATORS[name]()
    rng = case.ranges[s]
    if getattr(est, "takes_radius_range", False):
        est.radius_range = (rng[0], rng[1])
    if name == "torus":
        est.major_radius_range = (rng[2], rng[3])
    if case.normals is not None:
        est.normals = case.normals[s]
    return est


def host_ratios(name, case, strict=True, make=estimator):
    """every fixture with in-range indices through Estimator.minimal (the torus: minimal_rows): {(set, 'host', fixture): ratio}"""
    out = {}
    for s, (sname, pts, scale) in enumerate(case.sets):
        mine = np.flatnonzero(case.set_of == s)
        mine = mine[[bool((case.samples[f] >= 0).all() and (case.samples[f] < len(pts)).all()) for f in mine]]
        est = make(name, case, s)
        got = np.full((len(mine), SLOTS[name], PARAMS[name]), np.nan)
        if name == "torus":
            got = np.asarray(est.minimal_rows(pts, case.samples[mine].astype(np.int64))).reshape(len(mine), 2, 8)
        else:
            models, src = est.minimal(pts, case.samples[mine].astype(np.int64))
            got[np.asarray(src, dtype=np.int64), 0] = np.asarray(models).reshape(-1, PARAMS[name])
        for j, f in enumerate(mine):
            out[(sname, "host", int(f))] = cases.match(name, case, f, got[j], scale, (sname, "host"), strict)
    return out
