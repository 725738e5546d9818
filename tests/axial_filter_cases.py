"""The cases of tests/golden/kat_axial_filters_v1.npz: what the f32 filters built on the distance to an axis DECIDE - Filter32 of the 3-D
line, the cylinder, the cone and the torus (csrc/score_filters.hip.h), alone (types 12, 14, 16, 22) and behind the class of the mixed
primitives (18, 20).  tests/golden/make_golden_axial_filters.py records them on the MI355X, tests/test_gpu_axial_filters.py replays them;
both go through run_on().  The scoring tests show that a filter is invisible (counts and masks are the dense path's), which every
conservative filter is, whatever its budget; the keep words of the cull kernel and the work counters are the filter itself.

One scene for all six types: N points - two 3-D lines, a plane, a sphere, a cylinder, a cone, two tori and uniform outliers - with
their normals (type 20 reads them).  N = 64 * 64 + 3: two tiles of the cull kernel, nine super-groups, a tail group of three points;
plan_score (csrc/score_plan.h) has no smallest size for the cull + group-major path, so the size is chosen for the tail and the tiles.
M = 130 hypotheses per type: three keep words, two bits in the last.  hypotheses() lays a type's batch out."""
import os

import numpy as np

from pyprogressivex import _lib, datasets

FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kat_axial_filters_v1.npz")
TYPES = (_lib.LINE3D, _lib.CYLINDER3D, _lib.CONE3D, _lib.TORUS3D, _lib.PRIMITIVE3D, _lib.ORIENTED_PRIMITIVE3D)
N = 64 * 64 + 3
M = 130
MPAD = 256
THR = 0.05
T2 = 2.25 * THR * THR
TPP = 1.5 * THR * (1.0 + 1.0 / 64.0)          # T'' of the filters: a surface moved by it leaves its inliers on the filter's threshold
KAPPA = float(np.cos(np.deg2rad(20.0)) ** 2)  # type 20: normals within 20 degrees
COUNTERS = ("surviving_group_steps", "exact_evaluations", "inlier_pairs")
SEED = 2210


def scene():
    """(points [N, 3], normals [N, 3], {name: ground-truth rows}), shuffled; a pure function of SEED"""
    rng = np.random.default_rng(SEED)
    pl, _, g_line = datasets.make_lines3d(n_per_line=250, n_lines=2, n_outliers=0, seed=SEED)
    pp, np_, _, _, g_prim = datasets.make_primitives(n_per=300, n_outliers=0, seed=SEED + 1)
    pt, nt, _, g_torus = datasets.make_tori(n_per_torus=400, n_tori=2, n_outliers=0, seed=SEED + 2)
    nl = rng.normal(size=pl.shape)
    rest = N - len(pl) - len(pp) - len(pt)
    po, no = rng.uniform(0, 10.0, (rest, 3)), rng.normal(size=(rest, 3))
    pts, nrm = np.vstack([pl, pp, pt, po]), np.vstack([nl / np.linalg.norm(nl, axis=1)[:, None], np_, nt, no / np.linalg.norm(no, axis=1)[:, None]])
    order = rng.permutation(N)
    return np.ascontiguousarray(pts[order]), np.ascontiguousarray(nrm[order]), dict(line=g_line, primitive=g_prim, torus=g_torus)


def _bases(mt, gt):
    """the models a type's batch is built around: its own ground truth and the other structures' axes dressed as the type"""
    line, prim, torus = gt["line"], gt["primitive"], gt["torus"]
    cyl, cone = prim[2, 1:8], prim[3, 1:9]
    cs20 = [np.cos(np.deg2rad(20.0)), np.sin(np.deg2rad(20.0))]
    if mt == _lib.LINE3D:
        return [line[0], line[1], cyl[:6], cone[:6]]
    if mt == _lib.CYLINDER3D:
        return [cyl, np.append(line[0], 0.3), np.append(cone[:6], 0.5)]
    if mt == _lib.CONE3D:
        return [cone, np.concatenate([line[1], cs20]), np.concatenate([cyl[:6], cs20])]
    if mt == _lib.TORUS3D:
        return [torus[0], torus[1], np.concatenate([cyl[:6], [1.0, 0.3]])]
    return [prim[0], prim[1], prim[2], prim[3]]


def _moved_by_tpp(mt, m, sign, rng):
    """m with its surface moved by sign * T'' along its normal (the cone's apex along the axis, the line's point across it)"""
    m = m.copy()
    cls, q = (mt, m) if mt < _lib.PRIMITIVE3D or mt == _lib.TORUS3D else (int(m[0]), m[1:])
    if cls == _lib.PLANE3D:
        q[3] += sign * TPP
    elif cls == _lib.SPHERE3D:
        q[3] += sign * TPP
    elif cls == _lib.LINE3D:
        perp = np.cross(q[3:6], rng.normal(size=3))
        q[:3] += sign * TPP * perp / np.linalg.norm(perp)
    elif cls == _lib.CYLINDER3D:
        q[6] += sign * TPP
    elif cls == _lib.CONE3D:
        q[:3] += sign * TPP / q[7] * q[3:6]
    else:
        q[7] += sign * TPP
    return m


def hypotheses(mt, gt):
    """[M, P]: around each base in turn - itself, moved by +-T'', perturbed by 1e-6 .. 1e-1 and by 0.3, a random model of the box - and
    in the last rows the special ones, SPECIAL[mt] names them by their distance from the end"""
    rng = np.random.default_rng(SEED + mt)
    bases = _bases(mt, gt)
    P = _lib.PARAM_DIM[mt]
    union = mt in (_lib.PRIMITIVE3D, _lib.ORIENTED_PRIMITIVE3D)
    first = 1 if union else 0                                  # the class is never perturbed
    out = np.zeros((M, P))
    for j in range(M):
        b = np.asarray(bases[j % len(bases)], dtype=np.float64)
        kind = (j // len(bases)) % 6
        m = b.copy()
        if kind in (1, 2):
            m = _moved_by_tpp(mt, b, 1.0 if kind == 1 else -1.0, rng)
        elif kind in (3, 4):
            used = int(np.flatnonzero(b).max()) + 1
            m[first:used] += rng.normal(0, 10.0 ** rng.uniform(-6, -1) if kind == 3 else 0.3, used - first)
        elif kind == 5:
            used = int(np.flatnonzero(b).max()) + 1
            m[first:first + 3] = rng.uniform(0, 10.0, 3)
            m[first + 3:used] = b[first + 3:used] * rng.uniform(0.5, 1.5, used - first - 3)
        out[j] = m
    d = slice(first + 3, first + 6)
    axial = [b for b in bases if not union or b[0] in (_lib.CYLINDER3D, _lib.CONE3D)]
    out[M - 1] = axial[0]
    out[M - 1, first + 4] = np.nan                             # a NaN entry: culled everywhere
    out[M - 2] = axial[-1]
    out[M - 2, d] = 0.0                                        # d = 0: never culled
    out[M - 3] = axial[0]
    out[M - 3, d] *= 2.0 ** -40
    out[M - 4] = axial[-1]
    out[M - 4, d] *= 2.0 ** 40
    if mt in (_lib.CYLINDER3D, _lib.TORUS3D) or union:
        out[M - 5] = bases[2] if union else bases[0]
        out[M - 5, first + 6] = 1e18                           # a radius beyond the filter's range: never culled
    if mt == _lib.TORUS3D:
        out[M - 6] = bases[1]
        out[M - 6, first + 7] = 1e18
    if mt == _lib.CONE3D or union:
        out[M - 6] = bases[3] if union else bases[0]
        out[M - 6, first + 6:first + 8] = 2.0 ** -12           # |c| + |s| = 2^-11, below the band: never culled
    if union:
        out[M - 7] = bases[2]
        out[M - 7, 0] = 7.0                                    # an unknown class: never culled
        out[M - 8] = bases[3]
        out[M - 8, 0] = np.nan                                 # a NaN class: culled everywhere
    return out


# rows counted from the end of the batch: culled in every group / kept in every group
SPECIAL = {_lib.LINE3D: ((1,), (2,)), _lib.CYLINDER3D: ((1,), (2, 5)), _lib.CONE3D: ((1,), (2, 6)), _lib.TORUS3D: ((1,), (2, 5, 6)),
           _lib.PRIMITIVE3D: ((1, 8), (2, 5, 6, 7)), _lib.ORIENTED_PRIMITIVE3D: ((1, 8), (2, 5, 6, 7))}


def run_on(ctx, mt, pts, nrm, models):
    """one counters launch of the batch on `ctx`: (path, filter level, the three work counters [3], the keep words [groups, MPAD / 64])"""
    ctx.score_set_global_n(0)
    ctx.set_normal_tolerance(KAPPA if mt == _lib.ORIENTED_PRIMITIVE3D else 0.0)
    ctx.set_points(mt, pts)
    if mt == _lib.ORIENTED_PRIMITIVE3D:
        ctx.set_normals(nrm)
    ctx.set_compound(None)
    ctx.score_upload(models)
    st = ctx.score_stats(T2)
    return st["path"], st["filter"], np.array([st[k] for k in COUNTERS], dtype=np.int64), ctx.score_keep_words(MPAD)


def popcount(a):
    return int(np.unpackbits(np.ascontiguousarray(a).view(np.uint8)).sum())


def column(keep, row):
    """the keep bits of hypothesis `row` over the groups"""
    return (keep[:, row >> 6] >> np.uint64(row & 63)) & np.uint64(1)
