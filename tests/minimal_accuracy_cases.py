"""The minimal-solver accuracy fixtures (tests/golden/kat_minimal_v1.npz, written by tests/golden/make_golden_minimal.py from the
50-digit statements of tests/minimal_exact.py) and the comparisons that hold pgx_solve_minimal and the host routes of
_estimators.py to them: shared by the CPU file (tests/test_minimal_accuracy_cpu.py, OracleContext) and the GPU file
(tests/test_gpu_minimal_accuracy.py).  TEST INFRASTRUCTURE; numpy and the standard library only (no mpmath).

Per type, point sets by coordinate regime (the two-view solvers scale by max(1, max |pts|) of the resident set, so a regime is a
set of its own; an anchor row fixes every set's largest coordinate, hence its scale), the minimal samples as index rows into their
set, and per sample the reference's solution set (NaN padded), each solution's problem condition, kappa_route and tolerance
32 eps kappa_route.  A fixture is one of three kinds:
  ACCURACY   every tolerance <= 1e-6, solutions of one sample at least 1000 tolerances apart: matched within the tolerance;
  COVERAGE   kappa_route blows up there (P3P: two poses that share v = s3 / s1): problem condition <= 1e4, solutions >= 1e-3 apart
             (relative), matched within the solver's own consistency figure 1e-6 - what is asked is that no solution is lost;
  NO_MODEL   the reference has no solution (a repeated or out-of-range index, rank deficiency): every slot NaN.
What is compared: slots against reference solutions as SETS - every reference solution matched by a slot of its
own, no other filled slot, the NaN pattern the reference's - in max-entry distance; the two-view models in the solver's scaled
coordinates (carried there in rational arithmetic; at unit norm - the h33 = 1 chart is ill-scaled exactly where h33 is small, and a
bound on its entries would say nothing there -, H with the last entry positive, F up to sign); plus the invariants of each returned
model (h33 == 1.0 exactly, |F| = 1 and det F within the bound the stages from the cubic on leave, a proper rotation)."""
import os
from fractions import Fraction

import numpy as np

from pyprogressivex import _estimators

FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kat_minimal_v1.npz")
SEED = 11
EPS = 2.0 ** -52
TYPES = ["homography", "fundamental", "pnp"]
KEY = dict(homography="h", fundamental="f", pnp="p")
SLOTS = dict(homography=1, fundamental=3, pnp=4)
PARAMS = dict(homography=9, fundamental=9, pnp=12)
COMPARED = dict(homography=9, fundamental=9, pnp=12)
SAMPLE = dict(homography=4, fundamental=7, pnp=3)
DIM = dict(homography=4, fundamental=4, pnp=5)
BATCHES = (1, 63, 64, 65, 129)
ACCURACY, COVERAGE, NO_MODEL = 0, 1, 2
RANGE = 3                # (tests/minimal_closed_cases.py) inputs whose squares overflow or underflow: a slot is empty or within tolerance of a solution
COVERAGE_MATCH = 1e-6
IDENTIFIED = 1e-4        # a tenth of the separation a COVERAGE fixture guarantees: a slot this near a solution is that solution and no other
MAX_ROWS = 768
_TWO_VIEW_SETS = [("unit", 4.0), ("pixel", 2048.0), ("tiny", 2.0 ** -8)]      # (set, its anchor coordinate); the scale is max(1, anchor)
SETS = dict(homography=_TWO_VIEW_SETS, fundamental=_TWO_VIEW_SETS, pnp=[("all", 0.0)])
# (class, set, samples, kind)
CLASSES = dict(
    homography=[("coordinates of order 1", "unit", 8, ACCURACY), ("coordinates of order 1e3", "pixel", 8, ACCURACY),
                ("coordinates of order 2^-10", "tiny", 8, COVERAGE), ("strong perspective row", "pixel", 8, ACCURACY),
                ("h33 near zero", "unit", 8, ACCURACY), ("three collinear points", "unit", 8, NO_MODEL),
                ("repeated index", "unit", 8, NO_MODEL), ("out-of-range index", "unit", 8, NO_MODEL)],
    fundamental=[("coordinates of order 1", "unit", 8, ACCURACY), ("coordinates of order 1e3", "pixel", 8, ACCURACY),
                 ("coordinates of order 2^-10", "tiny", 8, COVERAGE), ("one real root", "unit", 8, ACCURACY),
                 ("three real roots", "unit", 8, ACCURACY), ("pure translation", "unit", 8, ACCURACY),
                 ("near-pure translation", "unit", 8, ACCURACY), ("planar scene", "unit", 8, NO_MODEL),
                 ("two roots within 2e-3", "unit", 8, ACCURACY), ("repeated index", "unit", 8, NO_MODEL),
                 ("out-of-range index", "unit", 8, NO_MODEL)],
    pnp=[("coordinates of order 1", "all", 8, ACCURACY), ("coordinates of order 1e3", "all", 8, ACCURACY),
         ("coordinates of order 2^-10", "all", 8, ACCURACY), ("one solution", "all", 8, ACCURACY), ("two solutions", "all", 8, ACCURACY),
         ("three solutions", "all", 8, ACCURACY), ("four solutions", "all", 8, ACCURACY), ("two poses share v", "all", 16, COVERAGE),
         ("isosceles, q = 1", "all", 8, ACCURACY), ("far camera", "all", 8, ACCURACY), ("repeated index", "all", 8, NO_MODEL),
         ("out-of-range index", "all", 8, NO_MODEL)])
SHARED_V = [c[0] for c in CLASSES["pnp"]].index("two poses share v")
FIELDS = ("samples", "set_of", "cls", "kind", "draw", "nref", "ref", "cond", "kappa", "tol")
EXTRA = dict(homography=("sym",), fundamental=("detk",), pnp=("sep", "den"))
# What a sibling table (tests/minimal_closed_cases.py) adds per type besides its rows in CLASSES, SLOTS, PARAMS and COMPARED:
FLIP = dict(fundamental=[-1.0] * 9)      # the entries whose common sign is free in the comparison
AS_RETURNED = {"pnp"}                    # compared as returned, without a change of coordinates
CHECKS = {}                              # name -> check(case, f, model, reference solution, tolerance): the type's invariants and exact contracts


class Case:
    """one type's fixtures: sets [(name, pts, scale)], samples [F, m] (rows of their set), set_of [F], cls [F], kind [F], draw [F],
    nref [F], ref [F, slots, compared entries], cond / kappa / tol [F, slots]; homography: sym [F, 18] ([H | H^-1] in the given
    coordinates); fundamental: detk [F, slots] (32 eps detk bounds |det F|); pnp: sep [F, 2] (depths relative, v), den [F, slots],
    parent [F, 4, 12] (the oracle's output at the commit before the P3P change, recorded)"""


def read_case(z, name, k, set_names, fields, scale=lambda pts: 1.0):
    """one type's Case from the arrays k_* of the file z"""
    c = Case()
    c.name = name
    c.sets = []
    for s, sname in enumerate(set_names):
        pts = np.ascontiguousarray(z[k + "_pts"][z[k + "_ptset"] == s])
        c.sets.append((sname, pts, scale(pts)))
    for field in fields:
        setattr(c, field, z[k + "_" + field])
    return c


def load():
    z = np.load(FILE)
    out = {}
    for name in TYPES:
        c = read_case(z, name, KEY[name], [sname for sname, _ in SETS[name]], FIELDS + EXTRA[name],
                      (lambda pts: 1.0) if name == "pnp" else (lambda pts: max(1.0, float(np.abs(pts).max()))))
        if name == "pnp":
            c.parent = z["p3p_parent_models"]
        if name == "fundamental":       # the parent's answers on the pure-translation class (recorded), by fixture number
            mine = np.flatnonzero(c.cls == [x[0] for x in CLASSES[name]].index("pure translation"))
            c.parent = {int(f): z["f7_parent_models"][i] for i, f in enumerate(mine)}
        out[name] = c
    return out


def class_name(name, cls):
    return CLASSES[name][int(cls)][0]


# ---- a returned model in the space where it is compared -------------------------------------------------------------------------
def compared(name, model, scale):
    """homography: S H S^-1 (S = diag(1/scale, 1/scale, 1)) at unit norm with the last entry positive; fundamental matrix:
    S^-1 F S^-1 at unit norm; both in rational arithmetic up to the final normalisation; pose: as returned"""
    model = np.asarray(model, dtype=np.float64)
    if name in AS_RETURNED:
        return model
    m = [Fraction(float(x)) for x in model[:9]]
    s = Fraction(float(scale))
    if name == "homography":
        m[2], m[5], m[6], m[7] = m[2] / s, m[5] / s, m[6] * s, m[7] * s
        m = [x if m[8] > 0 else -x for x in m]
    else:
        for k, power in enumerate((2, 2, 1, 2, 2, 1, 1, 1, 0)):
            m[k] = m[k] * s ** power
    big = max(abs(x) for x in m)
    v = np.array([float(x / big) for x in m])
    return v / np.linalg.norm(v)


def check_invariants(name, model, where):
    model = np.asarray(model, dtype=np.float64)
    if name == "homography":
        assert model[8] == 1.0, where
    if name == "fundamental":
        assert abs(np.linalg.norm(model) - 1.0) <= 4 * EPS, where
    if name == "pnp":
        R = model.reshape(3, 4)[:, :3]
        assert np.abs(R.T @ R - np.eye(3)).max() <= 64 * EPS, where
        assert np.linalg.det(R) > 0, where


def _det_exact(v):
    a = [Fraction(float(x)) for x in v]
    return float(a[0] * (a[4] * a[8] - a[5] * a[7]) - a[1] * (a[3] * a[8] - a[5] * a[6]) + a[2] * (a[3] * a[7] - a[4] * a[6]))


def match(name, case, f, models, scale, where=(), strict=True, coverage_tol=None):
    """One sample's returned slots (rows of models, NaN = empty) against fixture f as sets: the worst error / tolerance over the
    reference solutions (COVERAGE: error / 1e-6), inf where a solution has no slot of its own, a filled slot has no solution,
    the counts differ or an invariant is broken.  strict: those are assertion failures that say which.  coverage_tol: the
    distance within which a COVERAGE fixture's solutions are matched, in place of 1e-6 (IDENTIFIED: is every solution there at all)."""
    models = np.asarray(models, dtype=np.float64)
    filled = [m for m in models if np.isfinite(m).all()]
    partly = [m for m in models if np.isfinite(m).any() and not np.isfinite(m).all()]
    nref = int(case.nref[f])
    ranged = case.kind[f] == RANGE

    def refuse(what):
        if strict:
            raise AssertionError((name, class_name(name, case.cls[f]), int(f)) + tuple(where) + (what,))
        return np.inf
    if partly:
        return refuse("a slot is partly NaN")
    if len(filled) != nref and not (ranged and len(filled) < nref):
        return refuse(f"{len(filled)} models, the reference has {nref}")
    if nref == 0 or not filled:
        return 0.0
    got = np.array([compared(name, m, scale) for m in filled])
    ref = case.ref[f][:nref, :COMPARED[name]]
    tol = np.full(nref, coverage_tol or COVERAGE_MATCH) if case.kind[f] == COVERAGE else case.tol[f][:nref]
    dist = np.abs(got[None, :, :] - ref[:, None, :]).max(axis=2)            # [reference solution, slot]
    if name in FLIP:
        dist = np.minimum(dist, np.abs(got[None, :, :] * np.asarray(FLIP[name]) - ref[:, None, :]).max(axis=2))
    if ranged:                                  # every filled slot is a reference solution of its own; an empty slot is accepted
        back = dist.argmin(axis=0)
        if len(set(back.tolist())) != len(filled):
            return refuse(f"two slots are nearest to one reference solution (distances {dist.tolist()})")
        ref, tol, dist, nref = ref[back], tol[back], dist[back], len(filled)
    pick = dist.argmin(axis=1)
    if len(set(pick.tolist())) != nref:
        return refuse(f"two reference solutions are nearest to one slot (distances {dist.tolist()})")
    worst = float((dist[np.arange(nref), pick] / tol).max())
    if not worst <= 1.0:
        return refuse(f"error / tolerance {worst:.3g} (distances {dist[np.arange(nref), pick].tolist()}, tolerances {tol.tolist()})")
    try:
        for i, m in enumerate(filled):
            check_invariants(name, m, where)
        if name in CHECKS:
            for r in range(nref):
                CHECKS[name](case, f, filled[pick[r]], ref[r], tol[r])
        if name == "fundamental":           # rank 2, in the compared coordinates: |det| within what the stages from the cubic on can leave
            for r in range(nref):
                assert abs(_det_exact(got[pick[r]])) <= 32 * EPS * case.detk[f][r] + 16 * EPS * np.abs(got[pick[r]]).max() ** 3, \
                    ("det F", _det_exact(got[pick[r]]), 32 * EPS * case.detk[f][r])
    except AssertionError as e:
        return refuse(f"invariant: {e}")
    return worst


def batch_of(case, s, S):
    """the S samples of a launch on set s: the set's fixtures in order, repeated to S -> (fixture numbers [S], index rows [S, m])"""
    mine = np.flatnonzero(case.set_of == s)
    take = mine[np.arange(S) % len(mine)]
    return take, np.ascontiguousarray(case.samples[take], dtype=np.int32)


def device_ratios(name, case, ctx, strict=True, batches=BATCHES, coverage_tol=None):
    """Every fixture through ctx.solve_minimal at every batch size: {(set, S, fixture): error / tolerance}"""
    est = _estimators.ESTIMATORS[name]()
    slots, P = SLOTS[name], PARAMS[name]
    out = {}
    for s, (sname, pts, scale) in enumerate(case.sets):
        ctx.set_points(est.model_type, pts)
        if hasattr(case, "prepare"):            # what the set has resident besides its points (normals, radius ranges)
            case.prepare(ctx, s)
        for S in batches:
            take, idx = batch_of(case, s, S)
            models = np.asarray(ctx.solve_minimal(idx)).reshape(S, slots, P)
            for j, f in enumerate(take):
                out[(sname, S, int(f))] = match(name, case, f, models[j], scale, (sname, S), strict, coverage_tol)
    if hasattr(case, "prepare"):
        case.prepare(ctx, None)                 # the context's ranges as at creation
    return out


def host_ratios(name, case, strict=True, symmetric=False, coverage_tol=None):
    """Every fixture with in-range indices through the host route Estimator.minimal: {(set, 'host', fixture): error / tolerance}.
    symmetric: SymmetricHomographyEstimator, whose models are [H | H^-1] - the H part is compared as the homography's, the
    inverse against the 50-digit inverse of the reference H within 32 eps cond(H) |H^-1| (the inversion's rounding) +
    9 |H^-1|^2 scale tol (the error the H part may carry, through d H^-1 = -H^-1 dH H^-1)."""
    est = _estimators.ESTIMATORS["homography_sym" if symmetric else name]()
    out = {}
    for s, (sname, pts, scale) in enumerate(case.sets):
        mine = np.flatnonzero(case.set_of == s)
        mine = mine[[bool((case.samples[f] >= 0).all() and (case.samples[f] < len(pts)).all()) for f in mine]]
        models, src = est.minimal(pts, case.samples[mine].astype(np.int64))
        models, src = np.asarray(models), np.asarray(src)
        for j, f in enumerate(mine):
            rows = models[src == j]
            key = (sname, "host", int(f))
            if len(rows) > SLOTS[name]:
                if strict:
                    raise AssertionError((name, key, "more models than slots"))
                out[key] = np.inf
                continue
            got = np.full((SLOTS[name], models.shape[1] if models.ndim == 2 and models.shape[1] else PARAMS[name]), np.nan)
            got[:len(rows)] = rows
            out[key] = match(name, case, f, got[:, :PARAMS[name]], scale, key[:2], strict, coverage_tol)
            if symmetric and len(rows) == 1 and case.nref[f] == 1:
                H, inv = rows[0][:9].reshape(3, 3), case.sym[f][9:]
                bound = 32 * EPS * np.linalg.cond(H) * np.abs(inv).max() + 9 * np.abs(inv).max() ** 2 * scale * case.tol[f][0] / case.ref[f][0][8]
                err = np.abs(rows[0][9:] - inv).max()
                out[key] = max(out[key], float(err / bound))
                if strict:
                    assert err <= bound, (name, key, "H^-1 against the 50-digit inverse", err, bound)
    return out


def report(name, where, case, ratios):
    """the lines the tests print: per class the worst error / tolerance, the reference solutions and how many samples were matched"""
    lines = []
    for cls in sorted(set(case.cls.tolist())):
        mine = {k: v for k, v in ratios.items() if case.cls[k[2]] == cls}
        if not mine:
            continue
        key = max(mine, key=mine.get)
        fx = sorted({k[2] for k in mine})
        nsol = int(sum(case.nref[f] for f in fx))
        lost = sum(1 for f in fx if any(not v <= 1.0 for k, v in mine.items() if k[2] == f))
        lines.append(f"minimal accuracy [{where}] {name} / {class_name(name, cls)}: worst error/tolerance {mine[key]:.3g} at {key}; "
                     f"{len(fx)} samples with {nsol} reference solutions, {len(fx) - lost} samples fully matched")
    return "\n".join(lines)
