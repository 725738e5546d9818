"""Regenerates tests/golden/kat_minimal_closed_v1.npz: the samples of the closed-form minimal solvers' accuracy tests and, per
sample, what tests/minimal_closed_exact.py - the nine solvers' problems restated from their definitions in mpmath at 50 digits -
answers: the solution set, each solution's problem condition, kappa_route and tolerance (tests/minimal_closed_cases.py says what the
kinds and columns mean).  Run from the repository root: `python tests/golden/make_golden_minimal_closed.py` (needs mpmath).
Fixture = data only.

As in make_golden_minimal.py a sample is draw number k of its class: rows(name, class, k) makes it from numpy's generator seeded by
(SEED, type, class, k) and nothing else; a draw is kept if the REFERENCE says that it meets the class's conditions, the number of the
kept draw is recorded, and the regeneration check replays the kept draws alone.  A fixture that does not meet its kind is refused
(the next draw is tried), never relabelled.  Asserted here, on the reference alone, for every reference solution:
  the sample points lie on the surface and the normal relation its solver uses holds, to 1e-40 (cylinder: the first sample at r, both
  normal lines through the axis, both normals orthogonal to d; cone: the samples at the half-angle, every tangent plane through the
  apex; torus: samples 0, 1, 2 on the surface, all four normal lines through the axis);
  the route restated at 50 digits with every delta = 0 lands on the definition's solutions to 1e-40, on all of them and on nothing else;
  the torus' solution set is the same from two bases of the null space;
  ACCURACY fixtures have 0 < tolerance <= 1e-6 and solutions 1000 tolerances apart; COVERAGE fixtures have problem condition <= 1e4.
The RANGE classes (coordinates of 2^522, differences of 2^-550 and 2^-404) are answered at 450 digits, where the SVDs still
resolve them."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.join(ROOT, "oracle"), os.path.join(ROOT, "progressive-x_amd"), os.path.join(ROOT, "tests"), HERE]
import minimal_closed_exact as C  # noqa: E402
from make_golden_minimal import _meets, _rotation  # noqa: E402
from minimal_closed_cases import (ACCURACY, CLASSES, COVERAGE, DIM, FIELDS, FILE, KEY, NO_MODEL, ORIENTED, PARAMS, RANGE, SAMPLE, SEED,  # noqa: E402
                                  SETS, SLOTS, TYPES)

EPS = 2.0 ** -52
MAX_DRAWS = 400000
HUGE, TINY2, TINY3 = 2.0 ** 522, 2.0 ** -550, 2.0 ** -404
SIZES = {"coordinates of order 1e3": 1000.0, "coordinates of order 2^-10": 2.0 ** -10, "huge coordinates, squares overflow": HUGE,
         "tiny differences, squares underflow": TINY2, "tiny differences, cubes underflow": TINY3}
# every other huge fixture of the vanishing point and the plane: v (cubic in the coordinates) and n (quadratic) are finite there and their
# norms are not - at 2^522 the products themselves overflow to Inf - Inf = NaN, which `ln > 0` refused before the guard
ALSO_HUGE = dict(vanishing_point=2.0 ** 335, plane=2.0 ** 300)
FAR_TRANSVERSAL = (1e6, 1e7)          # |s2 / s1| of the class "second transversal far away"


def _frame(rng):
    Q = _rotation(rng)
    return Q[:, 0], Q[:, 1], Q[:, 2]


def _scales(rng, m):
    return rng.uniform(0.5, 2.0, m) * rng.choice([-1.0, 1.0], m)


def _dyadic(rng, shape, lo=-64, hi=64, den=32.0):
    return rng.integers(lo, hi, shape) / den


def oriented(name, rng, cname):
    """a sample of points and normals on one cylinder / cone / torus (consistent up to the rounding of its float64 rows; the normals
    neither unit nor consistently signed)"""
    d, u, v = _frame(rng)
    o = rng.uniform(-1, 1, 3)
    ring = lambda a: np.cos(a) * u + np.sin(a) * v           # noqa: E731
    if name == "cylinder":
        r = rng.uniform(0.3, 1.5)
        a0 = rng.uniform(0, 2 * np.pi)
        ang = [a0, a0 + (np.deg2rad(1.0) if cname == "normals 1 degree apart" else rng.uniform(0.5, 2.6))]
        P = np.array([o + rng.uniform(-1, 1) * d + r * ring(a) for a in ang])
        N = np.array([ring(a) for a in ang]) * _scales(rng, 2)[:, None]
        return P, N
    if name == "cone":
        th = np.deg2rad({"half-angle 5 degrees": 5.0, "half-angle 85 degrees": 85.0}.get(cname, rng.uniform(20.0, 60.0)))
        ang = rng.uniform(0, 2 * np.pi) + np.cumsum(rng.uniform(0.6, 2.4, 3))
        P = np.array([o + t * (np.cos(th) * d + np.sin(th) * ring(a)) for a, t in zip(ang, rng.uniform(0.5, 2.0, 3))])
        N = np.array([np.cos(th) * ring(a) - np.sin(th) * d for a in ang]) * _scales(rng, 3)[:, None]
        order = rng.permutation(3)                            # (the order of the samples decides whether the solver's D points into the nappe)
        return P[order], N[order]
    R, r = rng.uniform(1.9, 2.1), rng.uniform(0.45, 0.55)
    ua = rng.uniform(0, 2 * np.pi, 4)
    va = rng.uniform(0, 2 * np.pi, 4)
    if cname == "second transversal far away":
        # the normals orthogonal to m = (mx, 0, mz) (in the frame u, v, d) all meet the line at infinity of the planes m . x = const: a
        # second transversal there; tilted by 1e-7 it comes back to a distance of 1e6 .. 1e7
        mx, mz = np.cos(0.6), np.sin(0.6)
        va = np.arctan(-np.cos(ua) * mx / mz) + rng.uniform(0.5, 2.0, 4) * rng.choice([-1, 1], 4) * 1e-7
    P = np.array([o + R * ring(a) + r * (np.cos(b) * ring(a) + np.sin(b) * d) for a, b in zip(ua, va)])
    N = np.array([np.cos(b) * ring(a) + np.sin(b) * d for a, b in zip(ua, va)]) * _scales(rng, 4)[:, None]
    return P, N


def rows(name, cls, k, fnum=0):
    """draw k of class cls: (point rows [m, D], normal rows [m, 3] or None), float64: taken as exact from here on"""
    rng = np.random.default_rng([SEED, TYPES.index(name), cls, k])
    cname = CLASSES[name][cls][0]
    m, D = SAMPLE[name], DIM[name]
    size = SIZES.get(cname, 1.0)
    if name in ORIENTED:
        if cname == "no real transversal":
            P, N = rng.uniform(-1, 1, (4, 3)), rng.normal(size=(4, 3))
        elif cname == "c <= 0 refused":
            # the apex in the plane z = 0 of the samples (dyadic, so that every product is exact): the unit vectors to the samples span
            # that plane, d is its normal and c = 0 exactly
            a = np.append(_dyadic(rng, 2), 0.0)
            P = np.column_stack([_dyadic(rng, (3, 2)), np.zeros(3)])
            N = _dyadic(rng, (3, 3), -8, 8, 4.0)
            for i in range(3):                              # n_i . (p_i - a) = 0: n_i = (-wy, wx, anything) times a dyadic factor
                w = P[i] - a
                N[i, :2] = np.array([-w[1], w[0]]) * rng.choice([0.5, 1.0, 2.0])
        elif cname == "a sample at the apex":
            # normals along the three axes (powers of two), so that Cramer's rule is exact and the apex comes out as the sample's bits
            a = _dyadic(rng, 3)
            perm = rng.permutation(3)
            N = np.zeros((3, 3))
            P = np.tile(a, (3, 1))
            for i in range(3):
                N[i, perm[i]] = rng.choice([-1.0, 1.0]) * 2.0 ** rng.integers(-3, 4)
                if i < 2:                                   # samples 0 and 1 move inside their tangent planes; sample 2 IS the apex
                    P[i, [j for j in range(3) if j != perm[i]]] += _dyadic(rng, 2, 1, 64)
        else:
            P, N = oriented(name, rng, cname)
        if cname == "normals flipped":
            N = N * np.where(np.arange(m) == rng.integers(m), -1.0, rng.choice([-1.0, 1.0], m))[:, None]
        if cname == "normals rescaled by 2^+-20":
            N = N * (2.0 ** (20 * rng.choice([-1, 1], m)))[:, None]
        if cname == "a zero normal" or cname == "a zero normal in each place":
            N[fnum % m] = 0.0
        if cname == "parallel normals":
            N[1] = 2.0 * N[0]
        if cname == "the same point twice":
            P[1 + fnum % 2] = P[0]
        if cname == "coincident points, different normals":
            P[1] = P[0]
        if cname == "scene offset 1e6, size 1":
            P = P + 1e6 * rng.uniform(0.5, 1.0, 3) * rng.choice([-1.0, 1.0], 3)
        return P * size, N
    if cname in ("coincident points", "collinear points", "coplanar points", "collinear segments", "a segment of length zero", "parallel segments"):
        p0, e1, e2 = _dyadic(rng, D), _dyadic(rng, D, 1, 32), _dyadic(rng, D, -32, 32)
        if name == "vanishing_point":
            q, e = p0[:2], e1[:2]
            if cname == "collinear segments":
                return np.array([[*q, *(q + e)], [*(q + 2 * e), *(q + 5 * e)]]), None
            if cname == "a segment of length zero":
                seg = [[*q, *q], [*(q + e2[:2]), *(q + e2[:2] + e)]]
                return np.array(seg if fnum % 2 else seg[::-1]), None
            return np.array([[*q, *(q + e)], [*(q + e2[:2] + [0.25, 0.0]), *(q + e2[:2] + [0.25, 0.0] + 2 * e)]]), None
        P = np.array([p0, p0 + e1, p0 + e2, p0 + 2 * e1 + 3 * e2][:m])
        if cname == "coincident points":
            P[1 + fnum % (m - 1)] = P[0]
        elif name in ("plane", "circle"):
            P[2] = p0 + 3 * e1
        return P, None
    if cname == "radius exactly at both bounds":            # dyadic centre, r = 1.5, samples on the axes through the centre: every step is exact
        c = _dyadic(rng, D, den=8.0)
        E = np.eye(D) * 1.5
        P = np.array([c + E[0], c + E[1], c - E[0]] if D == 2 else [c + E[0], c + E[1], c + E[2], c - E[rng.integers(3)]])
        return P[rng.permutation(m)], None
    if name in ("circle", "sphere") and cname in ("radius range excludes the solution", "nearly collinear points", "nearly coplanar points"):
        if cname == "radius range excludes the solution":
            c, r = rng.uniform(-1, 1, D), rng.uniform(1.0, 2.0) if fnum % 2 else rng.uniform(4.0, 5.0)
            g = rng.normal(size=(m, D))
            return c + r * g / np.linalg.norm(g, axis=1, keepdims=True), None
        P = rng.uniform(-1, 1, (m, D))
        E = P[1:m - 1] - P[0]
        nrm = np.array([-E[0][1], E[0][0]]) if D == 2 else np.cross(E[0], E[1])
        P[m - 1] = P[0] + rng.uniform(0.2, 0.8, m - 2) @ E + 10.0 ** rng.uniform(-5, -2) * nrm / np.linalg.norm(nrm)
        return P, None
    P = rng.uniform(-1, 1, (m, D))
    if name in ALSO_HUGE and size == HUGE and fnum % 2:
        size = ALSO_HUGE[name]
    if cname == "scene offset 1e6, size 1":
        off = 1e6 * rng.uniform(0.5, 1.0, 2 if D == 4 else D) * rng.choice([-1.0, 1.0], 2 if D == 4 else D)
        P = P + (np.tile(off, 2) if D == 4 else off)
    return P * size, None


def screen(name, cname, P, N):
    """float64 only: False = not worth the reference's time (the reference decides what is kept)"""
    if name != "torus" or cname not in ("discriminant near zero", "no real transversal"):
        return True
    q = P[1] - P[0]
    co = []
    for i in (2, 3):
        Xv, Yv = np.cross(N[i], P[i] - P[0]), np.cross(N[i], N[0])
        co.append((-N[1] @ Yv, -(q @ Yv + N[0] @ Xv), N[1] @ Xv, q @ Xv))
    (A1, B1, C1, D1), (A2, B2, C2, D2) = co
    qa, qb, qc = B2 * A1 - A2 * B1, B2 * C1 - A2 * D1 - C2 * B1 + D2 * A1, D2 * C1 - C2 * D1
    disc = qb * qb - 4 * qa * qc
    return disc < 0 if cname == "no real transversal" else 0 <= disc <= 1e-3 * qb * qb


# ---- what the reference says of one sample ---------------------------------------------------------------------------------------
def _floats(v):
    return [float(x) for x in v]


def empty(name):
    slots = SLOTS[name]
    return dict(nref=0, ref=np.full((slots, PARAMS[name]), np.nan), cond=np.full(slots, np.nan), kappa=np.full(slots, np.nan),
                tol=np.full(slots, np.nan))


def _canonical(name, sol):
    """the free sign: the largest of the entries it moves is positive"""
    f = C.FLIP[name]
    if f is None:
        return list(sol)
    moved = [k for k in range(len(sol)) if f[k] < 0]
    big = max(moved, key=lambda k: abs(sol[k]))
    return [x * (f[k] if sol[big] < 0 else 1) for k, x in enumerate(sol)]


def _near(name, a, b, rel):
    a = C.aligned(name, a, b)
    return max(abs(x - y) for x, y in zip(a, b)) <= rel * max(abs(y) for y in b)


def reference(name, cls, P, N, ranges):
    """The fixture of the sample - dict(nref, ref, cond, kappa, tol) - or None where the sample does not meet its class's conditions.
    The assertions on the reference itself are made here."""
    cname, _, _, kind = CLASSES[name][cls]
    out = empty(name)
    with C.digits(450 if kind == RANGE else 80):
        sols = C.definition(name, P, N, ranges)
        n = len(sols)
        if kind == NO_MODEL:
            return out if n == 0 and (cname != "no real transversal" or C.torus_transversals(P, N) == []) else None
        if n == 0:
            return None
        for s in sols:
            assert C.surface_residual(name, P, N, s) <= 1e-40, (name, cname, "a reference solution off its surface")
        made = [(slot, C.route(name, P, N, ranges, slot)) for slot in range(SLOTS[name])]
        made = [(slot, r) for slot, r in made if r is not None]
        assert len(made) == n and all(any(_near(name, r, s, 1e-40) for _, r in made) for s in sols), (name, cname, "the route misses the definition")
        if name == "torus":
            other = C.definition(name, P, N, ranges, basis="mixed")
            assert len(other) == n and all(any(_near(name, o, s, 1e-40) for o in other) for s in sols), "the basis matters"
            both = len(C.torus_transversals(P, N) or [])
            full = len(C.definition(name, P, N))
            want = {"two transversals, both accepted": (2, 2, 2), "two transversals, one accepted": (2, 1, 1),
                    "tube-radius range cuts a slot": (2, 2, 1), "major-radius range cuts a slot": (2, 2, 1)}.get(cname)
            if want is not None and (both, full, n) != want:
                return None
            if cname == "second transversal far away":
                seen = []
                for slot in (0, 1):
                    C.route(name, P, N, C.FULL, slot, lambda st, v: (seen.append(v[0]) if st == "s" else None, v)[1])
                if len(seen) != 2 or n != 1:
                    return None
                ratio = abs(seen[0] / seen[1])
                if not FAR_TRANSVERSAL[0] <= max(ratio, 1 / ratio) <= FAR_TRANSVERSAL[1]:
                    return None
        if name == "cone" and cname == "the sign flip is taken" and not C.unflipped(P, N) < 0:
            return None
    out["nref"] = n
    for slot, r in made:
        j = min(range(n), key=lambda j: max(abs(x - y) for x, y in zip(C.aligned(name, r, sols[j]), sols[j])))      # slot of the route = solution j
        out["ref"][j] = _floats(_canonical(name, sols[j]))
        out["kappa"][j] = C.kappa(name, P, N, slot=slot)[0]
        out["tol"][j] = C.FACTOR * EPS * out["kappa"][j]
        if kind != RANGE:
            out["cond"][j] = C.condition(name, P, N, slot)
    if kind == RANGE:
        return out
    if cname.startswith("nearly co") and not (out["tol"][:n] >= 1e-8).all():      # at the edge of admissibility: 1e-8 <= tolerance <= 1e-6
        return None
    if cname == "second transversal far away" and not (out["cond"][:n] <= 1e4).all():
        return None
    return out if _meets(out, n, kind) else None


# ---- the file --------------------------------------------------------------------------------------------------------------------
def generate(verbose=True, draws=None, only=None, fixtures=None):
    """every array of the file.  draws = {type: the stored draw numbers [F]}: replay exactly those; fixtures = {type: fixture numbers}:
    the reference of those fixtures alone (the consistency test), the others left NaN"""
    data = dict(seed=np.array([SEED]))
    for name in TYPES if only is None else only:
        key, m, D = KEY[name], SAMPLE[name], DIM[name]
        setnames = [s for s, _ in SETS[name]]
        pts, nrm = {s: [] for s in setnames}, {s: [] for s in setnames}
        rec = {f: [] for f in FIELDS}
        for cls, (cname, sname, count, kind) in enumerate(CLASSES[name]):
            ranges = dict(SETS[name])[sname]
            k = 0
            for _ in range(count):
                fnum = len(rec["cls"])
                while True:
                    if draws is not None:
                        k = int(draws[name][fnum])
                    P, N = rows(name, cls, k, fnum)
                    ref = None
                    if fixtures is not None and fnum not in fixtures.get(name, ()):
                        ref = empty(name)
                    elif draws is not None or screen(name, cname, P, N):
                        if cname == "out-of-range index":
                            ref = empty(name)
                        elif cname == "repeated index":
                            ref = reference(name, cls, np.vstack([P[:1], P[:1], P[2:]]), None if N is None else np.vstack([N[:1], N[:1], N[2:]]), ranges)
                        else:
                            ref = reference(name, cls, P, N, ranges)
                    if ref is not None:
                        break
                    assert draws is None, (name, cname, k, "a stored draw fails its class's conditions")
                    k += 1
                    assert k < MAX_DRAWS, (name, cname)
                start = len(pts[sname])
                pts[sname] += list(P)
                nrm[sname] += list(N if N is not None else np.zeros((m, 3)))
                idx = np.arange(start, start + m)
                if cname == "repeated index":
                    idx[1] = idx[0]
                if cname == "out-of-range index":
                    idx[fnum % m] = -1 if fnum % 2 else 10 ** 6
                for f, v in dict(ref, samples=idx, set_of=setnames.index(sname), cls=cls, kind=kind, draw=k).items():
                    rec[f].append(v)
                if verbose:
                    print(name, "/", cname, "draw", k, "nref", ref["nref"], "tol", ref["tol"][:max(1, ref["nref"])], "cond", ref["cond"][:max(1, ref["nref"])],
                          flush=True)
                k += 1
        data[key + "_pts"] = np.concatenate([np.array(pts[s]).reshape(-1, D) for s in setnames])
        data[key + "_ptset"] = np.concatenate([np.full(len(pts[s]), i, dtype=np.int32) for i, s in enumerate(setnames)])
        if name in ORIENTED:
            data[key + "_nrm"] = np.concatenate([np.array(nrm[s]).reshape(-1, 3) for s in setnames])
        for f in FIELDS:
            data[key + "_" + f] = np.array(rec[f], dtype=np.int32 if f in ("samples", "set_of", "cls", "kind", "draw", "nref") else np.float64)
    return data


if __name__ == "__main__":
    only = sys.argv[1:] or None
    data = generate(only=only)
    if only is None:
        np.savez_compressed(FILE, **data)
        print("wrote", os.path.basename(FILE), os.path.getsize(FILE), "bytes;", {KEY[t]: len(data[KEY[t] + "_cls"]) for t in TYPES}, "fixtures")
