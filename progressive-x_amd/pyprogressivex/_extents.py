"""instanceExtents' host side: from model rows to the frame rows pgx_instance_extents takes, and from the sector masks and the occupancy
it returns to arcs and areas.  Pure numpy, no GPU: the instances are a few thousand at most, whatever the number of points
(DESIGN.md 4.17 derives the cell areas).

A frame row is PGX_EXTENTS_FRAME = 15 doubles: kind, o[3], g[3], u[3], v[3], R, r.  The library knows five kinds and no model types."""
import math

import numpy as np

FRAME = 15
KIND_NONE, KIND_PLANE, KIND_LINE, KIND_AXIAL, KIND_SPHERE, KIND_TORUS = -1, 0, 1, 2, 3, 4
PLANE3D, SPHERE3D, LINE3D, CYLINDER3D, CONE3D, PRIMITIVE3D, ORIENTED_PRIMITIVE3D, TORUS3D = 6, 8, 12, 14, 16, 18, 20, 22
SINGLE_TYPES = {PLANE3D: 4, SPHERE3D: 4, LINE3D: 6, CYLINDER3D: 7, CONE3D: 8, TORUS3D: 8}    # type -> doubles per model row
UNION_TYPES = (PRIMITIVE3D, ORIENTED_PRIMITIVE3D)                                             # rows (class, q0 .. q7)
UNION_CLASSES = (PLANE3D, SPHERE3D, CYLINDER3D, CONE3D)
MODEL_TYPES = tuple(sorted(SINGLE_TYPES)) + UNION_TYPES
PARAM_DIM = {**SINGLE_TYPES, **{t: 9 for t in UNION_TYPES}}
SECTORS = 64
SECTOR = 2.0 * math.pi / SECTORS


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def triad(d):
    """(g, u, v) for a direction d, or None for a zero or non-finite one: g = d / sqrt(d.d); k the index of the smallest |g_k|, the
    lowest on ties; t = e_k - g_k g; u = t / sqrt(t.t); v = g x u"""
    d = np.asarray(d, dtype=np.float64)
    with np.errstate(over="ignore"):
        dd = _dot(d, d)
    if not (dd > 0.0 and math.isfinite(dd)):
        return None
    g = d / math.sqrt(dd)
    k = int(np.argmin(np.abs(g)))                                # the first of equal minima
    t = -g[k] * g
    t[k] = 1.0 - g[k] * g[k]
    tt = _dot(t, t)
    if not tt > 0.0:
        return None
    u = t / math.sqrt(tt)
    v = np.array([g[1] * u[2] - g[2] * u[1], g[2] * u[0] - g[0] * u[2], g[0] * u[1] - g[1] * u[0]])
    if not (np.isfinite(g).all() and np.isfinite(u).all() and np.isfinite(v).all()):
        return None
    return g, u, v


def frame_row(surface, q):
    """the frame row of the model row q of the single type `surface`; kind -1 and NaN elsewhere for a row with a non-finite parameter or
    a zero direction"""
    bad = np.full(FRAME, np.nan)
    bad[0] = KIND_NONE
    width = SINGLE_TYPES.get(surface)
    if width is None:
        return bad
    q = np.asarray(q, dtype=np.float64)[:width]
    if len(q) < width or not np.isfinite(q).all():
        return bad
    if surface == SPHERE3D:
        return np.array([KIND_SPHERE, q[0], q[1], q[2], 0.0, 0.0, 1.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0, q[3], 0.0])
    if surface == PLANE3D:
        frame = triad(q[:3])
        if frame is None:
            return bad
        # the foot of the origin: -(d / |n|) g, which is -d n for the unit normal the solver and the refit return, and lies on the plane
        # for a row (s n, s d) too
        o = -(q[3] / math.sqrt(_dot(q[:3], q[:3]))) * frame[0]
        kind, radii = KIND_PLANE, (0.0, 0.0)
    else:
        frame = triad(q[3:6])
        if frame is None:
            return bad
        o = q[:3]
        kind = KIND_LINE if surface == LINE3D else KIND_TORUS if surface == TORUS3D else KIND_AXIAL
        radii = (0.0, 0.0) if surface == LINE3D else (q[6], 0.0) if surface == CYLINDER3D else (q[6], q[7])
    row = np.concatenate([[kind], o, frame[0], frame[1], frame[2], radii]).astype(np.float64)
    return row if np.isfinite(row).all() else bad


def surface_of(model_type, row):
    """(the single type a model row describes, its parameters): a union row's class must be one of 6, 8, 14, 16 - else -1"""
    if model_type in UNION_TYPES:
        cls = row[0]
        if not any(cls == c for c in UNION_CLASSES):             # NaN included
            return -1, row[1:]
        return int(cls), row[1:]
    return model_type, row


def frames(models, model_type, parent=None):
    """(frames [K', 15], surface [K'] int32): one frame row per instance - instance j lies on models[parent[j]], on models[j] without a
    parent - and the single type it describes (-1: no frame)"""
    models = np.asarray(models, dtype=np.float64)
    rows = np.empty((len(models), FRAME))
    surface = np.empty(len(models), dtype=np.int32)
    for i, row in enumerate(models):
        surface[i], q = surface_of(model_type, row)
        rows[i] = frame_row(int(surface[i]), q)
        if rows[i, 0] == KIND_NONE:
            surface[i] = -1
    if parent is not None:
        parent = np.asarray(parent, dtype=np.int64)
        rows, surface = rows[parent], surface[parent]
    return np.ascontiguousarray(rows.reshape(-1, FRAME)), np.ascontiguousarray(surface)


def mask_to_arc(mask):
    """(start, length) in radians of the shortest run of whole sectors, taken circularly, that holds every set bit of the 64-bit mask:
    the complement of the longest run of empty sectors (the first such run on ties).  (0, 2 pi) without an empty sector, (NaN, NaN) for
    an empty mask."""
    mask = int(mask)
    if mask == 0:
        return math.nan, math.nan
    best_len, best_end = 0, 0                                    # the longest empty run and the sector behind it
    for s in range(SECTORS):
        if (mask >> s) & 1 and not (mask >> ((s + 1) % SECTORS)) & 1:
            run = 0                                              # empty sectors from s + 1 on
            while not (mask >> ((s + 1 + run) % SECTORS)) & 1:
                run += 1
            if run > best_len:
                best_len, best_end = run, (s + 1 + run) % SECTORS
    if best_len == 0:
        return 0.0, 2.0 * math.pi
    return best_end * SECTOR, (SECTORS - best_len) * SECTOR


def _octant_widths(mask):
    """the angular width of each of the 8 bins of an angular coordinate: its occupied sectors, 2 pi / 64 each"""
    mask = int(mask)
    return np.array([bin((mask >> (8 * b)) & 0xff).count("1") * SECTOR for b in range(8)])


def _edges(lo, hi):
    return lo + (hi - lo) * (np.arange(9) / 8.0)


def area(surface, radii, lo, hi, sectors, occupancy):
    """the area of the occupied cells of one instance in its surface's metric; NaN for a line or no frame"""
    occupancy = int(occupancy)
    cells = np.array([[(occupancy >> (8 * a + b)) & 1 for b in range(8)] for a in range(8)], dtype=np.float64)
    if surface in (-1, LINE3D):
        return math.nan
    if occupancy == 0:
        return 0.0
    R, r = float(radii[0]), float(radii[1])
    if surface == PLANE3D:
        return float(cells.sum() * ((hi[0] - lo[0]) / 8.0) * ((hi[1] - lo[1]) / 8.0))
    if surface == TORUS3D:
        dphi = _octant_widths(sectors[0])
        band = np.zeros(8)                                       # per theta bin: the sum over its occupied sectors of r (R dtheta + r dsin)
        for t in range(SECTORS):
            if (int(sectors[1]) >> t) & 1:
                band[t >> 3] += r * (R * SECTOR + r * (math.sin((t + 1) * SECTOR) - math.sin(t * SECTOR)))
        return float((cells * np.outer(dphi, band)).sum())
    dphi = _octant_widths(sectors[1])
    e = _edges(lo[0], hi[0])
    if surface == CYLINDER3D:
        strip = R * np.diff(e)                                   # r dh
    elif surface == SPHERE3D:
        strip = R * R * np.diff(e)                               # r^2 dcos
    elif surface == CONE3D:
        c, s = R, r                                              # the frustum between two axial heights, per radian: (s / c^2) |h1^2 - h0^2| / 2
        strip = (s / (c * c)) * np.diff(e * np.abs(e)) / 2.0 if c != 0.0 else np.full(8, math.nan)
    else:
        return math.nan
    return float((cells * np.outer(strip, dphi)).sum())


def derive(surface, frame_rows, lo, hi, sectors, occupancy):
    """(arc [K', 2, 2], area [K']) of the instances"""
    k = len(surface)
    arc = np.full((k, 2, 2), np.nan)
    out = np.full(k, np.nan)
    for j in range(k):
        for w in range(2):
            arc[j, w] = mask_to_arc(sectors[j, w])
        out[j] = area(int(surface[j]), frame_rows[j, 13:15], lo[j], hi[j], sectors[j], occupancy[j])
    return arc, out
