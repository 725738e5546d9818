"""findPrimitives without a GPU: the ABI entries of the union type PGX_PRIMITIVE3D = 18, the numpy restatement of its residual
(tests/primitive_model.py), PrimitiveEstimator's solver and refit against its constituents', the public call's signature and input
checks and the make_primitives generator.  Every comparison is bit for bit against code that exists without the union."""
import ctypes
import inspect

import numpy as np
import pytest

import cone_model
import cylinder_model
import pyprogressivex as px
from primitive_model import CLASSES, CONE, CYLINDER, PARAMS, PLANE, PREFIX, SPHERE, SQ, class_of, sq_primitive, union_rows
from pyprogressivex import _estimators, _lib, datasets

PART = {PLANE: _estimators.PlaneEstimator, SPHERE: _estimators.SphereEstimator, CYLINDER: _estimators.CylinderEstimator,
        CONE: _estimators.ConeEstimator}
NAME = {PLANE: "plane", SPHERE: "sphere", CYLINDER: "cylinder", CONE: "cone"}


def test_model_dims_of_the_primitive_type():
    lib = _lib.load()
    d, p = ctypes.c_int(), ctypes.c_int()
    assert lib.pgx_model_dims(18, ctypes.byref(d), ctypes.byref(p)) == 0
    assert (d.value, p.value) == (3, 9) == _lib.MODEL_TABLE[18][:2]
    assert _lib.PRIMITIVE3D == 18 and _lib.MODEL_TABLE[18] == (3, 9, 4, 4)
    assert _lib.POINT_DIM[18] == 3 and _lib.PARAM_DIM[18] == 9
    for unassigned in (17, 19, -1):
        assert lib.pgx_model_dims(unassigned, None, None) != 0 and unassigned not in _lib.MODEL_TABLE
    assert lib.pgx_model_dims(16, ctypes.byref(d), ctypes.byref(p)) == 0 and (d.value, p.value) == (3, 8)
    est = _estimators.PrimitiveEstimator
    assert (est.model_type, est.sample_size, est.device_slots, est.cols, est.device_minimal) == (18, 4, 4, 9, True)
    assert (est.sample_size, est.device_slots) == _lib.MODEL_TABLE[18][2:] and est.cols == _lib.PARAM_DIM[18]
    assert _estimators.ESTIMATORS["primitive"] is est and datasets.MODEL_TYPES["primitive"] == 18
    assert hasattr(lib, "pgx_set_primitive_classes") and "pgx_set_primitive_classes" in _lib.ABI_SYMBOLS
    assert px.PRIMITIVE_CLASSES == {"plane": 6, "sphere": 8, "cylinder": 14, "cone": 16} == _estimators.PRIMITIVE_CLASSES
    assert list(px.PRIMITIVE_CLASSES.values()) == list(CLASSES)                  # the slot order
    for c in CLASSES:
        assert PARAMS[c] == _lib.PARAM_DIM[c] == PART[c].cols and PREFIX[c] == PART[c].sample_size == _lib.MODEL_TABLE[c][2]
        assert _lib.POINT_DIM[c] == 3


def test_the_estimator_follows_its_enabled_classes():
    full = _estimators.PrimitiveEstimator()
    assert list(full.parts) == list(CLASSES) and full.class_mask == 15 and full.nonminimal_sample_size == 6
    assert [type(full.parts[c]) for c in CLASSES] == [PART[c] for c in CLASSES]
    assert full.radius_range == (0.0, np.inf) and full.sine_range == (0.0, 1.0) and full.takes_radius_range
    for names, mask, nonmin in ((("plane",), 1, 3), (("sphere", "plane"), 3, 4), (("cylinder",), 4, 5), (("cone", "plane"), 9, 6),
                                (("cylinder", "sphere"), 6, 5)):
        est = _estimators.PrimitiveEstimator(names)
        assert est.class_mask == mask and est.nonminimal_sample_size == nonmin and est.sample_size == 4 and est.device_slots == 4
        assert sorted(est.parts) == sorted(px.PRIMITIVE_CLASSES[k] for k in names)
    for bad in ((), ("plane", "plane"), ("torus",), ("plane", "line3d"), None, "plane", 6):
        with pytest.raises(ValueError, match="classes"):
            _estimators.PrimitiveEstimator(bad)


def test_the_estimator_puts_normals_ranges_and_mask_on_the_context():
    calls = []

    class Ctx:
        def set_radius_range(self, lo, hi):
            calls.append(("radius", lo, hi))

        def set_normals(self, nrm):
            calls.append(("normals", nrm))

        def set_primitive_classes(self, mask, lo, hi):
            calls.append(("classes", mask, lo, hi))
    est = _estimators.PrimitiveEstimator(("sphere", "cone", "cylinder"))
    nrm = np.ones((5, 3))
    est.normals = nrm
    est.radius_range = (0.25, 2.0)
    est.sine_range = (0.1, 0.5)
    est.context_setup(Ctx())
    assert sorted(c[0] for c in calls) == ["classes", "normals", "radius"]
    got = {c[0]: c[1:] for c in calls}
    assert got["radius"] == (0.25, 2.0) and got["classes"] == (14, 0.1, 0.5) and got["normals"][0] is nrm
    assert est.parts[SPHERE].radius_range == est.parts[CYLINDER].radius_range == (0.25, 2.0)
    assert est.parts[CONE].radius_range == (0.1, 0.5)                          # the cone estimator's range is that of its sine
    assert est.parts[CYLINDER].normals is nrm and est.parts[CONE].normals is nrm


# ---- the residual's restatement -------------------------------------------------------------------------------------------------------
def _scene(seed=3, n_per=120, n_outliers=300):
    return datasets.make_primitives(n_per=n_per, n_outliers=n_outliers, seed=seed)


def test_the_restated_residual_dispatches_on_the_class():
    pts, _, _, _, gt = _scene()
    for row in gt:
        c = class_of(row)
        assert c in CLASSES and np.array_equal(sq_primitive(pts, row), SQ[c](pts, row[1:1 + PARAMS[c]]))
        assert not row[1 + PARAMS[c]:].any()
        junk = row.copy()
        junk[1 + PARAMS[c]:] = 123.0                                              # the padding is never read
        assert np.array_equal(sq_primitive(pts, junk), sq_primitive(pts, row))
    for bad in (7.0, 0.0, 6.5, -6.0, 18.0, np.nan, np.inf):
        row = gt[0].copy()
        row[0] = bad
        assert class_of(row) is None and np.isnan(sq_primitive(pts, row)).all()
    assert np.isnan(sq_primitive(pts, np.full(9, np.nan))).all()
    rows = union_rows(CYLINDER, np.vstack([gt[2, 1:8], np.full(7, np.nan)]))
    assert rows[0, 0] == 14 and np.array_equal(rows[0, 1:8], gt[2, 1:8]) and rows[0, 8] == 0 and np.isnan(rows[1]).all()


def test_every_inlier_of_make_primitives_lies_on_its_model():
    pts, nrm, cls, inst, gt = _scene(seed=5)
    assert pts.shape == nrm.shape == (4 * 120 + 300, 3) and cls.dtype == inst.dtype == np.int32 and gt.shape == (4, 9)
    assert gt[:, 0].tolist() == list(CLASSES) and np.bincount(inst).tolist() == [300, 120, 120, 120, 120]
    assert np.abs(np.linalg.norm(nrm, axis=1) - 1.0).max() < 1e-12
    for k, row in enumerate(gt):
        sel = inst == k + 1
        assert (cls[sel] == row[0]).all()
        r = np.sqrt(sq_primitive(pts[sel], row))
        assert r.max() < 6 * 0.01 and 0.005 < r.std() < 0.02                     # sigma = 0.01 along the surface normal
    assert (cls[inst == 0] == 0).all() and (pts >= -0.1).all() and (pts <= 10.1).all()
    # the normals: within normal_noise_deg = 5 degrees of the surface normal, either sign
    sel = inst == 1
    assert np.degrees(np.arccos(np.minimum(1.0, np.abs(nrm[sel] @ gt[0, 1:4])))).max() <= 5.0 + 1e-6
    sel = inst == 2
    radial = pts[sel] - gt[1, 1:4]
    radial /= np.linalg.norm(radial, axis=1)[:, None]
    ang = np.degrees(np.arccos(np.minimum(1.0, np.abs((nrm[sel] * radial).sum(axis=1)))))
    assert ang.max() <= 5.0 + 1e-6 and ang.max() > 1.0
    assert ((nrm[sel] * radial).sum(axis=1) < 0).any() and ((nrm[sel] * radial).sum(axis=1) > 0).any()


def test_make_primitives_is_seeded_and_takes_several_instances():
    a, b, c = _scene(seed=3), _scene(seed=3), _scene(seed=4)
    assert all(np.array_equal(x, y) for x, y in zip(a, b)) and not np.array_equal(a[0], c[0])
    pts, nrm, cls, inst, gt = datasets.make_primitives(n_per=50, n_outliers=0, n_each=2, seed=1)
    assert gt[:, 0].tolist() == [6, 6, 8, 8, 14, 14, 16, 16] and np.bincount(inst).tolist() == [0] + [50] * 8 and len(pts) == 400
    for k, row in enumerate(gt):
        assert np.sqrt(sq_primitive(pts[inst == k + 1], row)).max() < 0.06
    exact = datasets.make_primitives(n_per=40, n_outliers=10, sigma=0.0, normal_noise_deg=0.0, seed=2)
    for k, row in enumerate(exact[4]):
        assert np.sqrt(sq_primitive(exact[0][exact[3] == k + 1], row)).max() < 1e-12
    with pytest.raises(ValueError, match="normals"):
        datasets.make_primitives(normals="other")
    with pytest.raises(ValueError, match="n_each"):
        datasets.make_primitives(n_each=0)


# ---- the solver -------------------------------------------------------------------------------------------------------------------------
def _solver_case():
    pts, nrm, _, inst, _ = _scene(seed=7)
    pts, nrm = pts.copy(), nrm.copy()
    n = len(pts)
    rng = np.random.default_rng(1)
    samples = rng.integers(20, n, (200, 4)).astype(np.int32)
    for k in range(4):                                                           # and samples inside one instance: models in range
        samples[20 * k:20 * k + 20] = rng.choice(np.flatnonzero(inst == k + 1), (20, 4))
    pts[5], nrm[5] = pts[4], nrm[4]                                              # a duplicate point with its normal
    nrm[6] = 0.0
    nrm[7] = -3.0 * nrm[3]                                                       # parallel normals
    nrm[8, 1] = np.nan
    pts[9] = [1e200, 0.0, 0.0]
    special = np.array([[4, 5, 30, 31], [11, 11, 11, 11], [12, 12, 13, 14], [6, 15, 16, 17], [3, 7, 18, 19], [8, 15, 16, 17], [9, 21, 22, 23],
                        [30, 31, 32, 30], [40, 41, 42, 42]], np.int32)
    samples[100:100 + len(special)] = special
    return pts, nrm, samples


def _slots(est, pts, samples):
    """est.minimal's rows as {(sample, class): row}"""
    with np.errstate(all="ignore"):                                          # (a coordinate of 1e200 overflows a square)
        rows, src = est.minimal(pts, samples)
    assert rows.shape[1] == 9 and len(rows) == len(src) and (np.diff(src) >= 0).all()
    out = {}
    for r, s in zip(rows, src):
        assert class_of(r) is not None and (int(s), class_of(r)) not in out
        out[(int(s), class_of(r))] = r
    order = [(int(s), CLASSES.index(class_of(r))) for r, s in zip(rows, src)]
    assert order == sorted(order)                                                # sample by sample, slots ascending: the device's order
    return out


@pytest.mark.parametrize("names,radius,sine", [
    (("plane", "sphere", "cylinder", "cone"), (0.0, np.inf), (0.0, 1.0)),
    (("plane", "cone"), (0.0, np.inf), (0.0, 1.0)),                              # masked classes have no slot
    (("sphere", "cylinder"), (0.3, 1.2), (0.0, 1.0)),                            # radii out of range give no model
    (("plane", "sphere", "cylinder", "cone"), (0.4, 0.9), (np.sin(np.deg2rad(10.0)), np.sin(np.deg2rad(45.0)))),
])
def test_minimal_is_the_constituents_minimal_on_the_prefixes(names, radius, sine):
    pts, nrm, samples = _solver_case()
    est = _estimators.PrimitiveEstimator(names)
    est.normals, est.radius_range, est.sine_range = nrm, radius, sine
    got = _slots(est, pts, samples)
    want = {}
    for c in CLASSES:
        if NAME[c] not in names:
            continue
        part = PART[c]()
        if c in (CYLINDER, CONE):
            part.normals = nrm
        if c in (SPHERE, CYLINDER):
            part.radius_range = radius
        if c == CONE:
            part.radius_range = sine
        with np.errstate(all="ignore"):
            models, src = part.minimal(pts, np.ascontiguousarray(samples[:, :PREFIX[c]]))
        for m, s in zip(models, src):
            want[(int(s), c)] = union_rows(c, m)[0]
    assert sorted(got) == sorted(want)
    for key in want:
        assert np.array_equal(got[key], want[key], equal_nan=True), key
    per_class = {c: sum(1 for k in got if k[1] == c) for c in CLASSES}
    for c in CLASSES:
        assert (per_class[c] > 10) == (NAME[c] in names), per_class
    assert not any(k[0] in (101,) for k in got)                                  # four times the same point: no class has a model
    if radius != (0.0, np.inf):
        r = np.array([row[4] if c == SPHERE else row[7] for (s, c), row in got.items() if c in (SPHERE, CYLINDER)])
        assert len(r) and r.min() >= radius[0] and r.max() <= radius[1]
        full = _estimators.PrimitiveEstimator(names)
        full.normals = nrm
        assert len(_slots(full, pts, samples)) > len(got)                        # the range did remove models
    if sine != (0.0, 1.0):
        s_ = np.array([row[8] for (s, c), row in got.items() if c == CONE])
        assert len(s_) and s_.min() >= sine[0] and s_.max() <= sine[1]


# ---- the refit ---------------------------------------------------------------------------------------------------------------------------
# which classes may ask for a kind of row (the affine rows also serve the cylinder's refit: the foot of its points' mean)
KIND_OF = {_lib.GRAM_AFFINE: (PLANE, SPHERE, CYLINDER), _lib.GRAM_SPHERE: (SPHERE,), _lib.GRAM_CYL_GN: (CYLINDER,), _lib.GRAM_CONE_GN: (CONE,)}


def _gram_provider(sets, log):
    """a recording Gram provider over per-item point sets, in numpy: the affine rows (1, p), the sphere's (1, q, |q|^2), the cylinder's and
    the cone's Gauss-Newton rows (tests/cylinder_model.py, tests/cone_model.py)"""
    def gram(kind, prm, use_w, wpow, rows):
        rows = [int(r) for r in rows]
        log.append((kind, None if prm is None else np.array(prm, copy=True), rows))
        assert prm is None or len(prm) == len(rows)
        G, cnt, bad = [], [], []
        for i, b in enumerate(rows):
            p = sets[b]
            nb = 0
            if kind == _lib.GRAM_AFFINE:
                A = np.column_stack([np.ones(len(p)), p])
            elif kind == _lib.GRAM_SPHERE:
                q = (p - prm[i, :3]) / prm[i, 3]
                A = np.column_stack([np.ones(len(p)), q, (q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]])
            else:
                A, mask = (cylinder_model if kind == _lib.GRAM_CYL_GN else cone_model).gn_rows(p, prm[i])
                A, nb = A[~mask], int(mask.sum())
            G.append(A.T @ A)
            cnt.append(len(p))
            bad.append(nb)
        return np.array(G), np.array(cnt), np.array(bad)
    return gram


def test_fit_many_hands_each_class_its_items_and_puts_the_class_back():
    pts, _, _, inst, gt = _scene(seed=11, n_per=200)
    bump = {PLANE: 0.0, SPHERE: 0.0, CYLINDER: 0.01, CONE: 0.01}
    #          item: 0      1     2     3       4         5      6      7        8     9      10
    classes = [PLANE, CONE, None, SPHERE, 7.0, CYLINDER, PLANE, np.nan, CONE, SPHERE, CYLINDER]
    sets, inits = [], []
    rng = np.random.default_rng(2)
    for b, c in enumerate(classes):
        k = CLASSES.index(c) if c in CLASSES else 0
        sets.append(pts[rng.choice(np.flatnonzero(inst == k + 1), 60 + b, replace=False)])
        if c is None:
            inits.append(None)
            continue
        row = gt[k].copy()
        row[0] = c
        if c in CLASSES:
            row[1:4] += bump[c]
        inits.append(row)
    log = []
    est = _estimators.PrimitiveEstimator()
    got = est._fit_many(_gram_provider(sets, log), len(classes), inits)
    assert len(got) == len(classes)
    assert got[2] == [] and got[4] == [] and got[7] == []                         # no init, an unknown class, a NaN class
    for c in CLASSES:
        items = [b for b, x in enumerate(classes) if x == c]
        alone_log = []
        alone = PART[c]()._fit_many(_gram_provider([sets[b] for b in items], alone_log), len(items), [inits[b][1:1 + PARAMS[c]] for b in items])
        mine = [(kind, prm, rows) for kind, prm, rows in log if set(rows) <= set(items)]
        assert len(mine) == len(alone_log) > 0
        for (kind, prm, rows), (akind, aprm, arows) in zip(mine, alone_log):       # exactly its rows and parameter rows
            assert kind == akind and c in KIND_OF[kind] and rows == [items[r] for r in arows]
            assert (prm is None and aprm is None) or np.array_equal(prm, aprm)
        for b, models in zip(items, alone):                                      # in place, the class in front, zeros behind
            assert len(models) == len(got[b]) == 1
            assert got[b][0].shape == (9,) and got[b][0][0] == c and np.array_equal(got[b][0][1:1 + PARAMS[c]], models[0])
            assert not got[b][0][1 + PARAMS[c]:].any()
            assert np.sqrt(sq_primitive(sets[b], got[b][0])).max() < 0.06            # and it is a fit of its points
    for kind, prm, rows in log:                                                  # no request mixes kinds or classes
        owners = {classes[b] for b in rows}
        assert len(owners) == 1 and owners.pop() in KIND_OF[kind]
    # a class that is not enabled is an unknown class; an estimator of one class still refits it
    planes_only = _estimators.PrimitiveEstimator(("plane",))
    got = planes_only._fit_many(_gram_provider(sets, []), len(classes), inits)
    assert [len(g) for g in got] == [1 if c == PLANE else 0 for c in classes]
    assert est._fit_many(_gram_provider(sets, []), 3, [None, None, None]) == [[], [], []]


def test_a_refit_never_changes_the_class_of_its_init():
    """a cylinder's points under a cone init stay a cone (or no model), and the other way round"""
    pts, _, _, inst, gt = _scene(seed=11, n_per=200)
    est = _estimators.PrimitiveEstimator()
    cyl_pts, cone_pts = pts[inst == 3], pts[inst == 4]
    cone_on_cyl = np.concatenate([[16.0], gt[2, 1:4] - 20.0 * gt[2, 4:7], gt[2, 4:7], [np.cos(0.05), np.sin(0.05)]])
    cyl_on_cone = np.concatenate([[14.0], gt[3, 1:4] + 2.5 * gt[3, 4:7], gt[3, 4:7], [1.0, 0.0]])
    got = est._fit_many(_gram_provider([cyl_pts, cone_pts], []), 2, [cone_on_cyl, cyl_on_cone])
    for models, cls in zip(got, (16.0, 14.0)):
        assert all(m[0] == cls for m in models)


# ---- the public call ----------------------------------------------------------------------------------------------------------------------
def test_find_primitives_is_exported_with_its_signature():
    assert "findPrimitives" in px.__all__ and "PRIMITIVE_CLASSES" in px.__all__ and callable(px.findPrimitives)
    sig = inspect.signature(px.findPrimitives)
    cone = inspect.signature(px.findCones).parameters
    positional = [k for k, v in sig.parameters.items() if v.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD]
    assert positional == [k for k, v in cone.items() if v.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD]
    assert sig.parameters["normals"].default is inspect.Parameter.empty
    assert [sig.parameters[k].default for k in positional[2:]] == [cone[k].default for k in positional[2:]]
    kw = {k: v.default for k, v in sig.parameters.items() if v.kind is inspect.Parameter.KEYWORD_ONLY}
    want = {k: v.default for k, v in cone.items() if v.kind is inspect.Parameter.KEYWORD_ONLY}
    assert {k: v for k, v in kw.items() if k not in ("classes", "radius_range")} == want
    assert kw["classes"] == ("plane", "sphere", "cylinder", "cone") and kw["radius_range"] is None and kw["angle_range"] == (1.0, 89.0)
    assert list(kw)[:3] == ["classes", "radius_range", "angle_range"]
    doc = px.findPrimitives.__doc__
    assert "required" in doc.lower() and "estimateNormals" in doc and "radius" in doc and "class" in doc and "4.13" in doc


@pytest.mark.parametrize("points", [np.zeros((10, 2)), np.zeros((10, 4)), np.zeros(30), np.zeros((3, 3)), np.zeros((0, 3))])
def test_find_primitives_rejects_bad_points(points):
    normals = np.zeros((points.shape[0], 3))
    with pytest.raises(ValueError, match=r"points should be an array with dims \[n,3\], n>=4"):
        px.findPrimitives(points, normals)


@pytest.mark.parametrize("normals", [np.zeros((10, 2)), np.zeros((9, 3)), np.zeros(30), np.zeros((10, 3, 1)), None])
@pytest.mark.parametrize("classes", [("plane", "sphere", "cylinder", "cone"), ("plane",)])
def test_find_primitives_needs_normals_whatever_the_classes(normals, classes):
    with pytest.raises(ValueError, match=r"normals should be an array with dims \[n,3\]"):
        px.findPrimitives(np.zeros((10, 3)), normals, classes=classes)


def test_find_primitives_rejects_bad_classes_ranges_and_weights():
    p, nrm = np.zeros((10, 3)), np.zeros((10, 3))
    for bad in ((), ("plane", "plane"), ("torus",), "sphere", None, ("plane", 8)):
        with pytest.raises(ValueError, match="classes"):
            px.findPrimitives(p, nrm, classes=bad)
    for bad in ((0.0, 10.0), (-1.0, 10.0), (20.0, 10.0), (np.nan, 10.0), (10.0, 90.0), 3.0, (1.0, 2.0, 3.0)):
        with pytest.raises(ValueError, match="angle_range"):
            px.findPrimitives(p, nrm, angle_range=bad)
    for bad in ((-1.0, 1.0), (2.0, 1.0), (np.nan, 1.0), 3.0, (1.0, 2.0, 3.0)):
        with pytest.raises(ValueError, match="radius_range"):
            px.findPrimitives(p, nrm, radius_range=bad)
    with pytest.raises(ValueError, match="weights"):
        px.findPrimitives(p, nrm, np.ones(9))


def test_find_primitives_unknown_sampler_prints_and_returns_no_model(capsys):
    pts, nrm, _, _, _ = _scene()
    models, labels = px.findPrimitives(pts, nrm, sampler_id=7)
    assert models.shape == (0, 9) and models.dtype == np.float64
    assert labels.shape == (pts.shape[0],) and labels.dtype == np.int32 and not labels.any()
    assert "Unknown sampler identifier: 7" in capsys.readouterr().err
