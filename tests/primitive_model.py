"""The mixed-primitive type (PGX_PRIMITIVE3D = 18) in numpy: a model row is (class, q0 .. q7) and its residual is the constituent's on q.
Nothing is restated twice: the cylinder's and the cone's arithmetic are tests/cylinder_model.py's and tests/cone_model.py's, the plane's
and the sphere's are the formulas of the plane and sphere tests (a left fold of the dot product; a left fold of the squared distance, a
root and a subtraction).  Any other class - NaN, a number that is no class, a class number with a fraction - gives NaN residuals."""
import numpy as np

from cone_model import sq_cone
from cylinder_model import sq_cylinder

PLANE, SPHERE, CYLINDER, CONE = 6, 8, 14, 16
CLASSES = (PLANE, SPHERE, CYLINDER, CONE)                   # in the slot order of the device solver
PARAMS = {PLANE: 4, SPHERE: 4, CYLINDER: 7, CONE: 8}        # doubles of the constituent's model row
PREFIX = {PLANE: 3, SPHERE: 4, CYLINDER: 2, CONE: 3}        # points of the four-point sample the constituent's solver reads


def sq_plane(pts, m):
    r = np.abs(((m[0] * pts[:, 0] + m[1] * pts[:, 1]) + m[2] * pts[:, 2]) + m[3])
    return r * r


def sq_sphere(pts, m):
    with np.errstate(invalid="ignore", over="ignore"):
        dx, dy, dz = pts[:, 0] - m[0], pts[:, 1] - m[1], pts[:, 2] - m[2]
        r = np.abs(np.sqrt((dx * dx + dy * dy) + dz * dz) - m[3])
        return r * r


SQ = {PLANE: sq_plane, SPHERE: sq_sphere, CYLINDER: sq_cylinder, CONE: sq_cone}


def class_of(m):
    """the class of a union row, or None"""
    for c in CLASSES:
        if m[0] == float(c):
            return c
    return None


def sq_primitive(pts, m):
    """squared residuals of the union row m [9]"""
    c = class_of(m)
    if c is None:
        return np.full(len(pts), np.nan)
    return SQ[c](pts, m[1:1 + PARAMS[c]])


def union_rows(cls, models):
    """[B, P] rows of one constituent type -> [B, 9] union rows: the class in front, zeros behind; an all-NaN row stays all NaN"""
    models = np.asarray(models, dtype=np.float64).reshape(-1, PARAMS[cls])
    out = np.zeros((len(models), 9))
    out[:, 0] = cls
    out[:, 1:1 + PARAMS[cls]] = models
    out[np.isnan(models).all(axis=1)] = np.nan
    return out


def interleave(per_class):
    """{class: [S, 9] union rows} for all four classes -> [4 S, 9] in the solver's order, row 4 s + j = slot j of sample s"""
    S = len(per_class[PLANE])
    out = np.empty((4 * S, 9))
    for j, c in enumerate(CLASSES):
        out[j::4] = per_class[c]
    return out
