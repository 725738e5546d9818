"""pgx_instance_extents restated in numpy from the text of include/pgx.h (TEST INFRASTRUCTURE; not a port of the kernel: no table, no
keys, no atomics - coordinates for all points at once, then numpy's min / max / bitwise_or per instance), and the cases the CPU driver
and the GPU run: extents(points, labels, frames) returns what Context.instance_extents returns."""
import math

import numpy as np

FRAME = 15
LDS_INSTANCES = 256            # PGX_EXTENTS_LDS_INSTANCES
TAN = np.array([0.09849140335716425, 0.198912367379658, 0.3033466836073424, 0.41421356237309503, 0.5345111359507916,
                0.6681786379192989, 0.8206787908286602])
UNUSED, LINEAR, ANGULAR = 0, 1, 2
MODES = {0: (LINEAR, LINEAR), 1: (LINEAR, UNUSED), 2: (LINEAR, ANGULAR), 3: (LINEAR, ANGULAR), 4: (ANGULAR, ANGULAR)}
KEYS = ("count", "lo", "hi", "sectors", "occupancy")


def dot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def sector(x, y):
    """S(x, y) of the header, elementwise; x, y finite and not both zero"""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    ax, ay = np.abs(x), np.abs(y)
    swap = ay > ax
    with np.errstate(all="ignore"):
        t = np.where(swap, ax / ay, ay / ax)
    s = (t[..., None] >= TAN).sum(axis=-1)
    q = np.where(swap, 15 - s, s)
    return np.where(y >= 0, np.where(x >= 0, q, 31 - q), np.where(x < 0, 32 + q, 63 - q)).astype(np.int64)


def coordinates(points, labels, frames):
    """(live [n] bool, in_range [n] bool, mode [n, 2], c [n, 2] float64, s [n, 2] int64)"""
    points = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    labels = np.asarray(labels).reshape(-1)
    frames = np.asarray(frames, dtype=np.float64).reshape(-1, FRAME)
    n, K = len(points), len(frames)
    in_range = (labels >= 0) & (labels < K)
    mode = np.zeros((n, 2), dtype=np.int64)
    c = np.zeros((n, 2))
    s = np.zeros((n, 2), dtype=np.int64)
    if K == 0 or n == 0:
        return np.zeros(n, dtype=bool), in_range, mode, c, s
    f = frames[np.where(in_range, labels, 0)]
    kind = f[:, 0]
    live = in_range & np.isin(kind, [0.0, 1.0, 2.0, 3.0, 4.0]) & np.isfinite(points).all(axis=1)
    with np.errstate(all="ignore"):
        e = points - f[:, 1:4]
        eg, eu, ev, ee = dot(e, f[:, 4:7]), dot(e, f[:, 7:10]), dot(e, f[:, 10:13]), dot(e, e)
        rho = np.sqrt(eu * eu + ev * ev)
        cosine = eg / np.sqrt(ee)

        def linear(rows, w, value, defined=True):
            nonlocal live
            value = value + 0.0
            mode[rows, w] = LINEAR
            c[rows, w] = value[rows]
            live = live & ~(rows & ~(np.isfinite(value) & defined))

        def angular(rows, w, x, y):
            nonlocal live
            defined = np.isfinite(x) & np.isfinite(y) & ~((x == 0) & (y == 0))
            mode[rows, w] = ANGULAR
            s[rows, w] = sector(np.where(defined, x, 1.0), np.where(defined, y, 0.0))[rows]
            live = live & ~(rows & ~defined)

        linear(kind == 0, 0, eu)
        linear(kind == 0, 1, ev)
        linear(kind == 1, 0, eg)
        linear(kind == 2, 0, eg)
        angular(kind == 2, 1, eu, ev)
        linear(kind == 3, 0, cosine, ee != 0)
        angular(kind == 3, 1, eu, ev)
        angular(kind == 4, 0, eu, ev)
        angular(kind == 4, 1, rho - f[:, 13], eg)
    return live, in_range, mode, c, s


def bins(mode, c, s, lo, hi):
    """the occupancy bin of one coordinate of some points of one instance"""
    if mode == ANGULAR:
        return s >> 3
    if mode != LINEAR or hi == lo:
        return np.zeros(len(c), dtype=np.int64)
    with np.errstate(all="ignore"):
        f = ((c - lo) / (hi - lo)) * 8.0
    out = np.zeros(len(c), dtype=np.int64)
    mid = (f >= 1.0) & (f < 7.0)
    out[mid] = f[mid].astype(np.int64)
    out[f >= 7.0] = 7
    return out


def extents(points, labels, frames):
    frames = np.asarray(frames, dtype=np.float64).reshape(-1, FRAME)
    labels = np.asarray(labels).reshape(-1)
    K = len(frames)
    live, in_range, mode, c, s = coordinates(points, labels, frames)
    count = np.zeros(K, dtype=np.int64)
    lo = np.full((K, 2), np.inf)
    hi = np.full((K, 2), -np.inf)
    sectors = np.zeros((K, 2), dtype=np.uint64)
    occupancy = np.zeros(K, dtype=np.uint64)
    for j in range(K):
        mine = np.flatnonzero(live & (labels == j))
        count[j] = len(mine)
        if not len(mine):
            continue
        modes = MODES[int(frames[j, 0])]
        b = []
        for w in range(2):
            if modes[w] == LINEAR:
                lo[j, w], hi[j, w] = c[mine, w].min(), c[mine, w].max()
            elif modes[w] == ANGULAR:
                sectors[j, w] = np.bitwise_or.reduce(np.uint64(1) << s[mine, w].astype(np.uint64))
            b.append(bins(modes[w], c[mine, w], s[mine, w], lo[j, w], hi[j, w]))
        occupancy[j] = np.bitwise_or.reduce(np.uint64(1) << (8 * b[0] + b[1]).astype(np.uint64))
    return dict(count=count, lo=lo, hi=hi, sectors=sectors, occupancy=occupancy, skipped=int((in_range & ~live).sum()))


def same(got, ref):
    """every output array bit for bit (the floats as their words: -0 is not +0 here), dtypes and shapes included, and skipped"""
    for key in KEYS:
        g, r = got[key], ref[key]
        if g.dtype != r.dtype or g.shape != r.shape:
            return False
        if not np.array_equal(np.ascontiguousarray(g).view(np.uint64), np.ascontiguousarray(r).view(np.uint64)):
            return False
    return int(got["skipped"]) == int(ref["skipped"])


# ---- scenes ---------------------------------------------------------------------------------------------------------------------------
# one model row per single type: a tilted plane, sphere, line, cylinder, cone and torus
def single_models(rng):
    d = [v / np.linalg.norm(v) for v in rng.normal(size=(5, 3))]
    plane = np.concatenate([d[0], [0.3]])
    sphere = np.array([2.0, -1.0, 0.5, 0.7])
    line = np.concatenate([[0.1, 0.2, -0.3], 3.0 * d[1]])                       # a direction that is not unit
    cylinder = np.concatenate([[-1.0, 1.0, 0.0], d[2], [0.4]])
    half = math.radians(25.0)
    cone = np.concatenate([[0.5, 0.5, 2.0], d[3], [math.cos(half), math.sin(half)]])
    torus = np.concatenate([[-2.0, -2.0, 1.0], d[4], [1.5, 0.3]])
    return {6: plane, 8: sphere, 12: line, 14: cylinder, 16: cone, 22: torus}


def basis(d):
    d = d / np.linalg.norm(d)
    a = np.cross(d, [1.0, 0.0, 0.0] if abs(d[0]) < 0.9 else [0.0, 1.0, 0.0])
    a /= np.linalg.norm(a)
    return d, a, np.cross(d, a)


def sample_surface(surface, q, m, rng, noise=1e-3):
    """m points near the surface of the model row q"""
    if surface == 6:
        g, a, b = basis(q[:3])
        pts = -q[3] * g + rng.uniform(-1, 1, (m, 1)) * a + rng.uniform(-0.5, 0.5, (m, 1)) * b
    elif surface == 8:
        v = rng.normal(size=(m, 3))
        pts = q[:3] + q[3] * v / np.linalg.norm(v, axis=1, keepdims=True)
    elif surface == 12:
        pts = q[:3] + rng.uniform(-2, 2, (m, 1)) * q[3:6]
    elif surface == 14:
        g, a, b = basis(q[3:6])
        phi = rng.uniform(0, math.pi, (m, 1))                                    # a half shell
        pts = q[:3] + rng.uniform(0, 2, (m, 1)) * g + q[6] * (np.cos(phi) * a + np.sin(phi) * b)
    elif surface == 16:
        g, a, b = basis(q[3:6])
        phi = rng.uniform(0, 2 * math.pi, (m, 1))
        h = rng.uniform(0.5, 1.5, (m, 1))
        pts = q[:3] + h * g + h * (q[7] / q[6]) * (np.cos(phi) * a + np.sin(phi) * b)
    else:
        g, a, b = basis(q[3:6])
        phi, theta = rng.uniform(0, 2 * math.pi, (m, 1)), rng.uniform(0, 2 * math.pi, (m, 1))
        out = np.cos(phi) * a + np.sin(phi) * b
        pts = q[:3] + (q[6] + q[7] * np.cos(theta)) * out + q[7] * np.sin(theta) * g
    return pts + noise * rng.normal(size=(m, 3))


SURFACES = (6, 8, 12, 14, 16, 22)


def scene(n=2000, seed=0, outliers=0.2):
    """(points [n, 3], labels [n] int32, models by type): one instance of each kind, shuffled; instance j is SURFACES[j], the outliers
    carry -1, 6 or 2 ** 31 - 1"""
    rng = np.random.default_rng(seed)
    models = single_models(rng)
    which = rng.integers(0, len(SURFACES), n)
    pts = np.empty((n, 3))
    for j, surface in enumerate(SURFACES):
        rows = np.flatnonzero(which == j)
        pts[rows] = sample_surface(surface, models[surface], len(rows), rng)
    labels = which.astype(np.int64)
    out = rng.uniform(size=n) < outliers
    pts[out] = rng.uniform(-3, 3, (int(out.sum()), 3))
    labels[out] = rng.choice([-1, len(SURFACES), 2 ** 31 - 1], int(out.sum()))
    return np.ascontiguousarray(pts), labels.astype(np.int32), models


def scene_frames(models, union=False):
    """the six frame rows of scene(): from the single types, or - the four classes that have one - from type 18 rows"""
    from pyprogressivex import _extents
    rows = []
    for surface in SURFACES:
        q = models[surface]
        if union and surface in _extents.UNION_CLASSES:
            row = np.zeros(9)
            row[0], row[1:1 + len(q)] = surface, q
            rows.append(_extents.frames(row[None], 18)[0][0])
        else:
            rows.append(_extents.frames(q[None], surface)[0][0])
    return np.array(rows)


def many_frames(K, seed=1):
    """K frame rows of cylinders and planes in turn, and 3 000 points with random labels 0 .. K-1 (a few out of range)"""
    from pyprogressivex import _extents
    rng = np.random.default_rng(seed)
    rows = []
    for j in range(K):
        d = rng.normal(size=3)
        if j % 2:
            rows.append(_extents.frames(np.concatenate([d / np.linalg.norm(d), [rng.normal()]])[None], 6)[0][0])
        else:
            rows.append(_extents.frames(np.concatenate([rng.normal(size=3), d, [0.5]])[None], 14)[0][0])
    pts = rng.uniform(-2, 2, (3000, 3))
    labels = rng.integers(-1, K + 1, 3000).astype(np.int32)
    return pts, labels, np.array(rows)


SIZES = (1, 63, 64, 65, 129, 257)
SWITCH = (1, LDS_INSTANCES, LDS_INSTANCES + 1)


def size_cases():
    pts, labels, models = scene(257, seed=3, outliers=0.1)
    frames = scene_frames(models)
    for n in SIZES:
        yield f"size-{n}", pts[:n], labels[:n], frames


def scene_cases():
    pts, labels, models = scene(2000, seed=4)
    yield "scene-single-types", pts, labels, scene_frames(models)
    yield "scene-type-18-rows", pts, labels, scene_frames(models, union=True)


def switch_cases():
    for K in SWITCH:
        pts, labels, frames = many_frames(K, seed=K)
        yield f"instances-{K}", pts, labels, frames


def layout_cases():
    pts, labels, models = scene(1500, seed=5, outliers=0.0)
    frames = scene_frames(models)
    cyl = frames[3:4]
    yield "one-instance", pts, np.zeros(len(pts), np.int32), cyl                  # every lane on one row
    yield "shuffled", pts, labels, frames                                        # no wave is uniform
    order = np.argsort(labels, kind="stable")
    yield "sorted", pts[order], labels[order], frames                            # whole waves of one label, and the seams between them
    gap = np.where(labels >= 2, labels + 1, labels).astype(np.int32)             # instance 2 has no points
    yield "instance-without-points", pts, gap, np.vstack([frames[:2], frames[5:6], frames[2:]])
    yield "all-out-of-range", pts, np.where(labels % 2, -1, 6).astype(np.int32), frames
    one = labels.copy()
    one[:] = -1
    one[777] = 4
    yield "one-live-point", pts, one, frames


def bad_cases():
    pts, labels, models = scene(600, seed=6, outliers=0.1)
    frames = scene_frames(models)
    pts = pts.copy()
    pts[5, 0], pts[17, 1], pts[40, 2], pts[41] = np.nan, np.inf, -np.inf, np.nan
    yield "nan-and-inf-rows", pts, labels, frames
    pts, labels, _ = scene(600, seed=7, outliers=0.1)
    pts = pts.copy()
    cyl, sph, tor = frames[3], frames[1], frames[5]
    pts[:4] = cyl[1:4] + np.array([[0.0], [0.5], [-1.0], [2.0]]) * cyl[4:7]       # on the cylinder's axis (as far as rounding lets them be)
    labels = labels.copy()
    labels[:4] = 3
    pts[4], labels[4] = sph[1:4], 1                                              # the sphere's centre
    pts[5], labels[5] = tor[1:4], 5                                              # the torus' centre: on the axis
    yield "axis-and-centre", pts, labels, frames
    none = frames.copy()
    none[2] = np.nan
    none[2, 0] = -1.0
    yield "frame-of-kind--1", pts, labels, none


def exact_cases():
    """axis-aligned frames, where coordinates are exact: -0.0, hi == lo, points at lo and at hi (bins 0 and 7), points on the axis"""
    from pyprogressivex import _extents
    plane = _extents.frames(np.array([[0.0, 0.0, 1.0, 0.0]]), 6)[0][0]            # g = e_z, u = e_x, v = e_y, o = 0
    cyl = _extents.frames(np.array([[0.0, 0.0, 0.0, 0.0, 0.0, 2.0, 1.0]]), 14)[0][0]
    line = _extents.frames(np.array([[1.0, 1.0, 1.0, 0.0, 1.0, 0.0]]), 12)[0][0]
    sph = _extents.frames(np.array([[0.0, 0.0, 0.0, 1.0]]), 8)[0][0]
    frames = np.array([plane, cyl, line, sph])
    pts = np.array([[-0.0, -0.0, -0.0], [0.0, 0.0, 0.0], [-0.0, 1.0, 0.0], [0.0, 8.0, -0.0],          # plane: a is +-0 only (hi == lo), b 0..8
                    [0.0, 7.0, 0.0], [0.0, 0.999, 0.0], [0.0, 1.0, 0.0], [0.0, 6.999, 0.0],
                    [1.0, 0.0, 0.0], [0.0, 1.0, 1.0], [-1.0, -0.0, 0.5], [0.0, 0.0, 0.3], [-0.0, -0.0, -0.7],  # cylinder: two on the axis
                    [1.0, 5.0, 1.0], [1.0, 5.0, 1.0],                                                    # line: one place twice
                    [0.0, 0.0, 1.0], [0.0, 0.0, -1.0], [1.0, 0.0, 0.0], [0.0, 0.0, 0.0], [-0.0, 1.0, -0.0]])   # sphere: poles (no azimuth), centre
    labels = np.array([0] * 8 + [1] * 5 + [2] * 2 + [3] * 5, dtype=np.int32)
    yield "exact", pts, labels, frames
    yield "exact-reversed", pts[::-1].copy(), labels[::-1].copy(), frames


def all_cases():
    for make in (size_cases, scene_cases, switch_cases, layout_cases, bad_cases, exact_cases):
        yield from make()
