"""Regenerates tests/golden/kat_minimal_v1.npz: the samples of the minimal-solver accuracy tests and, per sample, what
tests/minimal_exact.py - the solvers' problems restated from their definitions in mpmath at 50 digits - answers: the solution set,
each solution's problem condition, kappa_route and tolerance (tests/minimal_accuracy_cases.py says what the kinds and columns
mean).  Run from the repository root: `python tests/golden/make_golden_minimal.py` (needs mpmath).  Fixture = data only.

A sample is draw number k of its class: rows(name, class, k) makes it from numpy's generator seeded by (SEED, type, class, k) and
nothing else.  A draw is kept if the REFERENCE says that it meets the class's conditions (reference() returns None otherwise);
then the next draw is tried, and the number of the kept draw is recorded in the file, so that the regeneration check replays the
kept draws alone.  A cheap float64 screen (screen()) only spares the search 50-digit work on hopeless draws; it decides nothing
that is stored.  Asserted here, on the reference alone:
  the route restated at 50 digits with every delta = 0 lands on the definition's solutions to 1e-40, on all of them and on nothing else;
  the fundamental matrix's solution set is the same from three bases of the null space;
  ACCURACY fixtures have 0 < tolerance <= 1e-6 and solutions 1000 tolerances apart;
  COVERAGE fixtures have problem condition <= 1e4 and solutions >= 1e-3 apart (relative).

p3p_parent_models is recorded data: what the oracle of the commit before the P3P change answered on the P3P samples (the change
must keep the bits of every sample that was complete there).  It is read back from the existing file, with the P3P draws it
belongs to, and is never made here: without it the generator refuses."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.join(ROOT, "oracle"), os.path.join(ROOT, "progressive-x_amd"), os.path.join(ROOT, "tests")]
import minimal_exact as X  # noqa: E402
from minimal_accuracy_cases import (ACCURACY, CLASSES, COMPARED, COVERAGE, DIM, EXTRA, FIELDS, FILE, KEY, MAX_ROWS, NO_MODEL, SAMPLE,  # noqa: E402
                                    SEED, SETS, SLOTS, TYPES)

EPS = 2.0 ** -52
MAX_DRAWS = 400000
INDEX_CLASSES = ("repeated index", "out-of-range index")


def _rotation(rng, small=None):
    if small is not None:                       # a rotation by `small` radians about a random axis
        a = rng.normal(size=3)
        a *= small / np.linalg.norm(a)
        K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
        th = np.linalg.norm(a)
        return np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * (K @ K)
    Q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    if np.linalg.det(Q) < 0:
        Q[:, 0] = -Q[:, 0]
    return Q


def rows(name, cls, k):
    """draw k of class cls: the sample's point rows [m, D] (float64: taken as exact from here on)"""
    rng = np.random.default_rng([SEED, TYPES.index(name), cls, k])
    cname, sname, _, _ = CLASSES[name][cls]
    if cname in INDEX_CLASSES:
        cname = CLASSES[name][0][0]               # a general sample; the index row makes the case
    if name == "pnp":
        size = {"coordinates of order 1e3": 1000.0, "coordinates of order 2^-10": 2.0 ** -10}.get(cname, 1.0)
        Xo = rng.uniform(-1, 1, (3, 3))
        Q = _rotation(rng)
        depth = rng.uniform(8, 16) if cname == "far camera" else rng.uniform(1.8, 3.0) if cname.endswith("solution") or \
            cname.endswith("solutions") else rng.uniform(3, 6)
        t = np.array([rng.uniform(-0.5, 0.5), rng.uniform(-0.5, 0.5), depth])
        if cname == "isosceles, q = 1":       # a right isosceles triangle on dyadic coordinates: a2 = b2 + c2 and b2 = c2 exactly, so q = 1
            L = float(rng.integers(32, 96)) / 64.0
            ax = rng.permutation(3)
            Xo = np.tile(rng.integers(-32, 32, 3) / 64.0, (3, 1))
            Xo[1, ax[0]] += L
            Xo[2, ax[1]] += L
        Y = (Xo @ Q.T + t) * size
        return np.column_stack([Y[:, 0] / Y[:, 2], Y[:, 1] / Y[:, 2], Xo * size])
    c = dict(unit=1.0, pixel=1000.0, tiny=2.0 ** -10)[sname]
    if name == "fundamental":
        if cname == "planar scene":           # dyadic points under a dyadic affine map: exact in float64, a plane's homography, rank <= 6
            x1 = rng.integers(-96, 96, (7, 2)) / 128.0
            x2 = x1 @ (rng.integers(-8, 8, (2, 2)) / 16.0 + np.eye(2)).T + rng.integers(-8, 8, 2) / 16.0
            return np.column_stack([x1, x2])
        Xw = rng.uniform(-1, 1, (7, 3)) + [0, 0, 4]
        R = {"pure translation": np.eye(3), "near-pure translation": _rotation(rng, 1e-4)}.get(cname)
        if R is None:
            R = _rotation(rng, rng.uniform(0.05, 0.4))
        Y = Xw @ R.T + rng.uniform(-0.5, 0.5, 3)
        return np.column_stack([Xw[:, :2] / Xw[:, 2:], Y[:, :2] / Y[:, 2:]]) * (2.0 * c)
    if cname == "three collinear points":     # dyadic points under a dyadic affine map: exact in float64, consistent, rank 7
        p0 = rng.integers(-64, 64, 2) / 128.0
        d = rng.integers(1, 32, 2) / 128.0
        x1 = np.array([p0, p0 + d, p0 + 3 * d, rng.integers(-64, 64, 2) / 128.0])
        x2 = x1 @ (rng.integers(-8, 8, (2, 2)) / 8.0 + np.eye(2)).T + rng.integers(-8, 8, 2) / 16.0
        return np.column_stack([x1, x2])
    x1 = rng.uniform(-1, 1, (4, 2)) * c
    H = np.eye(3) + np.array([[0.3, 0.3, 0.0], [0.3, 0.3, 0.0], [0.0, 0.0, 0.0]]) * rng.normal(size=(3, 3))
    H[:2, 2] = rng.uniform(-0.3, 0.3, 2) * c
    persp = 0.4 if cname in ("strong perspective row", "h33 near zero") else 0.05
    H[2, :2] = rng.uniform(-persp, persp, 2) / c
    if cname == "h33 near zero":
        H[2, 2] = rng.choice([-1.0, 1.0]) * rng.uniform(1e-4, 4e-4)
    y = np.column_stack([x1, np.ones(4)]) @ H.T
    return np.column_stack([x1, y[:, :2] / y[:, 2:]])


def screen(name, cls, r):
    """float64 only: False = not worth the reference's time (the reference decides what is kept)"""
    cname, sname, _, _ = CLASSES[name][cls]
    if not np.isfinite(r).all():
        return False
    if name != "pnp":
        if not np.abs(r).max() <= dict(SETS[name])[sname]:
            return False
        if cname in ("pure translation", "two roots within 2e-3") and name == "fundamental":
            s = max(1.0, dict(SETS[name])[sname])
            x1, y1, x2, y2 = (r / s).T
            A = np.column_stack([x2 * x1, x2 * y1, x2, y2 * x1, y2 * y1, y2, x1, y1, np.ones(7)])
            if cname == "pure translation":      # the two columns elimination leaves free are each other's transposes: c3 vanishes there
                M, free = A.copy(), list(range(9))
                for k in range(7):
                    i, j = np.unravel_index(np.argmax(np.abs(M[k:, :][:, free])), (7 - k, len(free)))
                    M[[k, k + i]] = M[[k + i, k]]
                    c = free.pop(j)
                    M[k + 1:] -= np.outer(M[k + 1:, c] / M[k, c], M[k])
                return sorted(free) in ([1, 3], [2, 6], [5, 7])
            vt = np.linalg.svd(A)[2]
            F1, F2 = vt[7].reshape(3, 3), vt[8].reshape(3, 3)
            ls = np.array([0.0, 1.0, -1.0, 2.0])
            coef = np.linalg.solve(np.vander(ls, 4), [np.linalg.det(l * F1 + (1 - l) * F2) for l in ls])
            ev = np.roots(coef)
            ev = ev[np.abs(ev.imag) < 1e-9].real
            Fs = [(l * F1 + (1 - l) * F2).ravel() for l in ev]
            Fs = [F / np.linalg.norm(F) for F in Fs]
            return len(Fs) == 3 and min(min(np.abs(a - b).max(), np.abs(a + b).max()) for i, a in enumerate(Fs) for b in Fs[:i]) <= 3e-3
        return True
    if not (np.abs(r[:, :2]).max() < 2.0):       # (a point behind or beside the camera)
        return False
    if cname != "two poses share v":
        return True
    f = np.column_stack([r[:, :2], np.ones(3)])          # two float roots v of the route's quartic with a small 2 (cg - v ca)
    f /= np.linalg.norm(f, axis=1, keepdims=True)
    Xo = r[:, 2:]
    ca, cb, cg = f[1] @ f[2], f[0] @ f[2], f[0] @ f[1]
    a2, b2, c2 = ((Xo[1] - Xo[2]) ** 2).sum(), ((Xo[0] - Xo[2]) ** 2).sum(), ((Xo[0] - Xo[1]) ** 2).sum()
    q, rr = (a2 - c2) / b2, (a2 + c2) / b2
    A = [(q - 1) ** 2 - 4 * c2 / b2 * ca ** 2, 4 * (q * (1 - q) * cb - (1 - rr) * ca * cg + 2 * c2 / b2 * ca ** 2 * cb),
         2 * (q ** 2 - 1 + 2 * q ** 2 * cb ** 2 + 2 * (b2 - c2) / b2 * ca ** 2 - 4 * rr * ca * cb * cg + 2 * (b2 - a2) / b2 * cg ** 2),
         4 * (-q * (1 + q) * cb + 2 * a2 / b2 * cg ** 2 * cb - (1 - rr) * ca * cg), (1 + q) ** 2 - 4 * a2 / b2 * cg ** 2]
    v = np.roots(A)
    v = v[(np.abs(v.imag) < 1e-3) & (v.real > 0)].real
    return int((np.abs(2 * (cg - v * ca)) < 2e-3).sum()) >= 2


# ---- what the reference says of one sample ---------------------------------------------------------------------------------------
def _floats(v):
    return [float(x) for x in v]


def empty(name):
    slots = SLOTS[name]
    out = dict(nref=0, ref=np.full((slots, COMPARED[name]), np.nan), cond=np.full(slots, np.nan), kappa=np.full(slots, np.nan),
               tol=np.full(slots, np.nan))
    out.update(dict(homography=dict(sym=np.full(18, np.nan)), fundamental=dict(detk=np.full(slots, np.nan)),
                    pnp=dict(sep=np.full(2, np.inf), den=np.full(slots, np.nan)))[name])
    return out


def _meets(out, n, kind):
    """ACCURACY: 0 < tolerance <= 1e-6, the solutions 1000 tolerances apart; COVERAGE: problem condition <= 1e4, the solutions 1e-3
    apart relative to the largest entry (the pose: see reference(), its depths)"""
    tol = out["tol"][:n]
    dist = [np.abs(out["ref"][i] - out["ref"][j]).max() for i in range(n) for j in range(i)]
    if kind == COVERAGE:
        return bool((out["cond"][:n] <= 1e4).all() and all(d >= 1e-3 * np.abs(out["ref"][:n]).max() for d in dist))
    return bool((tol > 0).all() and (tol <= 1e-6).all() and all(d >= 1000 * tol.max() for d in dist))


def reference(name, cls, r, scale):
    """The fixture of sample rows r - dict(nref, ref, cond, kappa, tol + the type's extras) - or None where the sample does not meet
    its class's conditions.  The assertions on the reference itself are made here."""
    cname, _, _, kind = CLASSES[name][cls]
    out = empty(name)
    if name == "homography":
        d = X.h4_definition(r, 1.0)
        if kind == NO_MODEL:
            return out if d["rank_deficient"] else None
        if d["rank_deficient"] or d["sym"] is None or (cname == "h33 near zero" and not abs(d["unit"][8]) <= 1e-3):
            return None
        with X.digits(80):
            dn = X.h4_definition(r, scale)                           # the same null vector in the solver's scaled coordinates
            route = X.h4_route(r, scale)
            want = [x if dn["unit"][8] > 0 else -x for x in dn["unit"]]           # unit norm, the last entry positive (the product's is 1)
            assert max(abs(route[k] - want[k]) for k in range(9)) <= 1e-40, "the H route misses the definition"
        kappa, _ = X.h4_kappa_route(r, scale)
        out.update(nref=1, sym=np.array(_floats(d["sym"])))
        out["ref"][0] = _floats(want)
        out["cond"][0], out["kappa"][0], out["tol"][0] = X.h4_condition(r, scale), kappa, X.FACTOR * EPS * kappa
        return out if _meets(out, 1, kind) else None
    if name == "fundamental":
        d = X.f7_definition(r, scale)
        if kind == NO_MODEL:
            return out if d["rank_deficient"] or d["sols"] is None else None
        if d["rank_deficient"] or d["sols"] is None:
            return None
        sols = d["sols"]
        n = len(sols)
        want = {"one real root": 1, "three real roots": 3}.get(cname)
        if n == 0 or n > 3 or (want is not None and n != want):
            return None
        gap = min([float(max(abs(a[k] - b[k]) for k in range(9))) for i, a in enumerate(sols) for b in sols[:i]], default=np.inf)
        if cname == "two roots within 2e-3" and not gap <= 2e-3:
            return None
        if cname == "pure translation":
            # the samples on which c3 = det(F1 - F2) vanishes in the route's own chart (a skew-symmetric F whose two free entries are
            # each other's transposes): one solution is the chart's root at infinity, which the solver had no branch for
            quick = X.f7_route_plan(r, scale)
            if quick[0] == "cubic" or max(w[2] for w in quick[1]) > 1e-12:
                return None
        with X.digits(80):
            hi = X.f7_definition(r, scale)["sols"]
            for basis in ("mixed", "gj"):
                other = X.f7_definition(r, scale, basis)["sols"]
                assert len(other) == n and all(min(max(abs(a[k] - b[k]) for k in range(9)) for b in other) <= 1e-40 for a in hi), "the basis matters"
            made = [(w, X.f7_route(r, scale, w)) for w in X.f7_route_plan(r, scale)[1]]
            made = [(w, F) for w, F in made if F is not None]
            # (where the route takes c3 for zero its models solve the truncated polynomial: within the figure each plan entry carries)
            assert all(min(max(abs(a[k] - b[k]) for k in range(9)) for a in hi) <= 1e-40 + (w[2] if w[0] != "cubic" else 0)
                       for w, b in made), "the F route makes a model the definition has not"
            assert len(made) == n, ("the F route makes", len(made), "of", n, "solutions")
        plan = X.f7_route_plan(r, scale)
        out["nref"] = n
        for i, w in enumerate(plan[1]):
            F = X.f7_route(r, scale, w)
            j = min(range(n), key=lambda j: max(abs(F[k] - sols[j][k]) for k in range(9)))      # slot i of the route is solution j
            kappa, _, detk = X.f7_kappa_route(r, scale, w, plan)
            out["ref"][j] = _floats(sols[j])
            out["kappa"][j], out["tol"][j], out["detk"][j] = kappa, X.FACTOR * EPS * kappa, detk
        if kind == ACCURACY and not _meets(out, n, kind):
            return None
        for j in range(n):
            out["cond"][j] = X.f7_condition(r, scale, sols[j])
        return out if _meets(out, n, kind) else None
    sols = X.p3p_definition(r)
    n = len(sols)
    if kind == NO_MODEL:
        return out if n == 0 else None
    want = {"one solution": 1, "two solutions": 2, "three solutions": 3, "four solutions": 4}.get(cname)
    if n == 0 or n > 4 or (want is not None and n != want):
        return None
    den = [float(X.p3p_den(r, s)) for s, _ in sols]
    if kind == COVERAGE and not sum(abs(x) <= 1e-3 for x in den) >= 2:
        return None
    # the route at delta = 0 against the definition, both ways (every root v > 0 of the route's quartic whose pose has positive depths)
    with X.digits(100):
        hi = X.p3p_definition(r)
        made = [p for p in (X.p3p_route(r, v) for v in X.p3p_route_roots(r)) if p is not None]
        near = lambda a, b: max(abs(a[k] - b[k]) for k in range(12)) <= 1e-40 * max(1, max(abs(x) for x in b))
        assert len(hi) == n and all(any(near(p, q) for _, q in hi) for p in made), "the P3P route makes a pose the definition has not"
        assert all(any(near(p, q) for p in made) for _, q in hi), "the P3P route misses a solution of the definition"
    out["nref"] = n
    for i, (s, p) in enumerate(sols):
        out["ref"][i], out["den"][i] = _floats(p), den[i]
        for j in range(i):
            a, b = s, sols[j][0]
            out["sep"][0] = min(out["sep"][0], float(max(abs(a[k] - b[k]) for k in range(3)) / max(max(a), max(b))))
            out["sep"][1] = min(out["sep"][1], float(abs(a[2] / a[0] - b[2] / b[0])))
    if kind == COVERAGE and not out["sep"][0] >= 1e-3:
        return None
    for i, (s, p) in enumerate(sols):
        out["cond"][i] = X.p3p_condition(r, s)
        if kind == COVERAGE and not out["cond"][i] <= 1e4:
            return None
        out["kappa"][i] = X.p3p_kappa_route(r, s)[0]
        out["tol"][i] = X.FACTOR * EPS * out["kappa"][i]
    if kind == ACCURACY and not _meets(out, n, kind):
        return None
    return out


# ---- the file --------------------------------------------------------------------------------------------------------------------
def generate(verbose=True, draws=None, parent=None, only=None, parent_f7=None):
    """every array of the file.  draws = {type: the stored draw numbers [F]}: replay exactly those (the regeneration check: every
    type; a type that is not named is searched); parent = the recorded p3p_parent_models, required with the P3P samples"""
    data = dict(seed=np.array([SEED]))
    every = draws or {}
    for name in TYPES if only is None else only:
        draws = every if name in every else None
        key, m, D = KEY[name], SAMPLE[name], DIM[name]
        setnames = [s for s, _ in SETS[name]]
        pts = {s: ([np.full(D, a)] if name != "pnp" else []) for s, a in SETS[name]}        # the anchor row fixes the set's scale
        rec = {f: [] for f in FIELDS + EXTRA[name]}
        for cls, (cname, sname, count, kind) in enumerate(CLASSES[name]):
            scale = 1.0 if name == "pnp" else max(1.0, dict(SETS[name])[sname])
            k = 0
            for _ in range(count):
                while True:
                    fnum = len(rec["cls"])
                    if draws is not None:
                        k = int(draws[name][fnum])
                    r = rows(name, cls, k)
                    ref = None
                    if draws is not None or screen(name, cls, r):      # (a replayed draw was kept: nothing to spare, and nothing in float decides)
                        if cname == "out-of-range index":
                            ref = empty(name)
                        elif cname == "repeated index":
                            use = r.copy()
                            use[1] = use[0]
                            ref = reference(name, cls, use, scale)
                        else:
                            ref = reference(name, cls, r, scale)
                    if ref is not None:
                        break
                    assert draws is None, (name, cname, k, "a stored draw fails its class's conditions")
                    k += 1
                    assert k < MAX_DRAWS, (name, cname)
                start = len(pts[sname])
                pts[sname] += list(r)
                idx = np.arange(start, start + m)
                if cname == "repeated index":
                    idx[1] = idx[0]
                if cname == "out-of-range index":
                    idx[fnum % m] = -1 if fnum % 2 else 10 ** 6
                for f, v in dict(ref, samples=idx, set_of=setnames.index(sname), cls=cls, kind=kind, draw=k).items():
                    rec[f].append(v)
                if verbose:
                    print(name, "/", cname, "draw", k, "nref", ref["nref"], "tol", ref["tol"][:max(1, ref["nref"])], flush=True)
                k += 1
        allpts = np.concatenate([np.array(pts[s]).reshape(-1, D) for s in setnames])
        assert len(allpts) <= MAX_ROWS, (name, len(allpts))
        data[key + "_pts"] = allpts
        data[key + "_ptset"] = np.concatenate([np.full(len(pts[s]), i, dtype=np.int32) for i, s in enumerate(setnames)])
        for f in FIELDS + EXTRA[name]:
            data[key + "_" + f] = np.array(rec[f], dtype=np.int32 if f in ("samples", "set_of", "cls", "kind", "draw", "nref") else np.float64)
        if name == "fundamental":                # recorded likewise: the parent's answers on the pure-translation class, [8, 3, 9]
            mine = [f for f in range(len(rec["cls"])) if CLASSES[name][rec["cls"][f]][0] == "pure translation"]
            assert parent_f7 is not None and np.shape(parent_f7) == (len(mine), 3, 9), "f7_parent_models: the recorded array is needed"
            data["f7_parent_models"] = np.asarray(parent_f7, dtype=np.float64)
        if name == "pnp":
            # recorded data, never made here: the oracle in this tree is no longer the parent's, and its answers would make the
            # keep-the-bits test vacuous.  New P3P samples need that commit's oracle run on them (one call of pgxo_solve_minimal_range).
            assert parent is not None and np.shape(parent) == (len(data["p_samples"]), 4, 12), "p3p_parent_models: the recorded array is needed"
            data["p3p_parent_models"] = np.asarray(parent, dtype=np.float64)
    return data


if __name__ == "__main__":
    assert os.path.exists(FILE), "the fixture file holds the recorded p3p_parent_models: it cannot be written from nothing"
    old = np.load(FILE)
    # (P3P and F are replayed from their recorded draws, so that the recorded parent answers stay theirs; H is searched anew)
    data = generate(draws={"pnp": old["p_draw"], "fundamental": old["f_draw"]}, parent=old["p3p_parent_models"], parent_f7=old["f7_parent_models"])
    np.savez_compressed(FILE, **data)
    print("wrote", os.path.basename(FILE), os.path.getsize(FILE), "bytes;", {KEY[t]: len(data[KEY[t] + "_cls"]) for t in TYPES}, "fixtures")
