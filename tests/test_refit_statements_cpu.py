"""The one statement of every least-squares refit (`_fit_many`, pyprogressivex/_estimators.py) against the single-item bodies it
replaced (tests/refit_reference.py), both fed by the same OracleContext: through `nonminimal`, `nonminimal_labels` and
`nonminimal_batch` the models have the count, dtype, shape and bytes of the reference body run once per selection, and the
context sees the calls it saw before - the same `gram` calls from `nonminimal`, and from the other two one `gram_labels` /
`gram_batch` call per request for all the items that made that request.  PnP is held by tests/test_host_logic.py (its two
statements agree to rounding only).  A second test feeds non-finite Gram matrices: no model, no exception, no warning.
At the end, the one Gauss-Newton loop of the four iterative refits against the four copies of it, byte for byte and request
for request."""
import warnings

import numpy as np
import pytest

import cone_model
import cylinder_model
import refit_reference
import torus_model
from oracle_ctx import OracleContext
from pyprogressivex import _estimators, _lib, datasets

NAMES = ["line", "plane", "sphere", "circle", "vanishing_point", "homography", "homography_sym", "fundamental"]
MAX_REQUESTS = dict(line=1, plane=1, vanishing_point=1, sphere=2, circle=2, homography=2, homography_sym=2, fundamental=2)
FAR = dict(sphere=np.array([1e4, -2e4, 5e3]), circle=np.array([1e6, -2e6]))
DUPLICATES = 12       # = the batch's selection size


def _scene(name):
    """(points, instance of every point: 1, 2 or 0 = outlier, the radius of instance 1 or None): two instances of 120 points and 60
    outliers, then DUPLICATES copies of one point of instance 1 (instance -1)"""
    kw = dict(n_outliers=60, seed=3)
    radius = None
    if name == "line":
        pts, gt, _ = datasets.make_lines(n_per_line=120, n_lines=2, **kw)
    elif name == "plane":
        pts, gt, _ = datasets.make_planes(n_per_plane=120, n_planes=2, **kw)
    elif name == "sphere":
        pts, gt, models = datasets.make_spheres(n_per_sphere=120, n_spheres=2, **kw)
        radius = models[0, -1]
    elif name == "circle":
        pts, gt, models = datasets.make_circles(n_per_circle=120, n_circles=2, **kw)
        radius = models[0, -1]
    elif name == "vanishing_point":
        pts, gt, _ = datasets.make_vanishing_points(n_inliers=240, n_vps=2, **kw)
    elif name == "fundamental":
        pts, gt, _ = datasets.make_two_view_motions(n_per_motion=120, n_motions=2, **kw)
    else:
        pts, gt, _ = datasets.make_homographies(n_per_plane=120, n_planes=2, **kw)
    one = pts[np.flatnonzero(gt == 1)[:1]]
    return np.vstack([pts, np.tile(one, (DUPLICATES, 1))]), np.concatenate([gt, np.full(DUPLICATES, -1)]), radius


class Counting:
    """the context, with every Gram call written down"""

    def __init__(self, ctx):
        self.ctx, self.calls = ctx, []

    def _note(self, method, kind, params, weights, wpow, what):
        self.calls.append(dict(method=method, kind=kind, params=None if params is None else np.array(params, dtype=np.float64),
                               weights=weights, wpow=wpow, what=what))

    def gram(self, kind, sel, params=None, weights=None, wpow=2):
        self._note("gram", kind, params, weights, wpow, (sel[0], np.array(sel[1])))
        return self.ctx.gram(kind, sel, params=params, weights=weights, wpow=wpow)

    def gram_labels(self, kind, K, params=None, weights=None, wpow=2):
        self._note("gram_labels", kind, params, weights, wpow, K)
        with np.errstate(divide="ignore", invalid="ignore"):      # (the oracle divides by the zero scale of the labels not asked about)
            return self.ctx.gram_labels(kind, K, params=params, weights=weights, wpow=wpow)

    def gram_batch(self, kind, index, params=None, weights=None, wpow=2):
        self._note("gram_batch", kind, params, weights, wpow, np.array(index))
        return self.ctx.gram_batch(kind, index, params=params, weights=weights, wpow=wpow)

    def eigh_smallest_batch(self, A):
        return self.ctx.eigh_smallest_batch(A)


def _same_models(got, want, where):
    assert len(got) == len(want), where
    for a, b in zip(got, want):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (where, a, b)


def _reference(est, ctx, sel, w):
    """(models, calls) of the reference body on one selection"""
    counting = Counting(ctx)
    return refit_reference.nonminimal(est, counting, sel, w), counting.calls


def _check_single_calls(calls, ref_calls, where):
    """`nonminimal` makes the reference's calls: same order, kind, params, weights switch, wpow and selection"""
    assert len(calls) == len(ref_calls), where
    for c, r in zip(calls, ref_calls):
        assert c["method"] == r["method"] == "gram" and c["kind"] == r["kind"] and c["wpow"] == r["wpow"], where
        assert c["weights"] is r["weights"], where
        assert (c["params"] is None) == (r["params"] is None), where
        if c["params"] is not None:
            assert c["params"].shape == r["params"].shape and c["params"].tobytes() == r["params"].tobytes(), where
        assert c["what"][0] == r["what"][0] and np.array_equal(c["what"][1], r["what"][1]), where


def _check_stacked_calls(name, calls, method, ref_calls, full, where):
    """The j-th call of `nonminimal_labels` / `nonminimal_batch` is the j-th request of every item whose reference body made
    one, in one launch.  ref_calls = {item: the reference's calls}; full = the number of params rows of a call when it carries
    one per label (the rows of the other labels are zero), None when it carries one per item that asked."""
    assert len(calls) == max((len(c) for c in ref_calls.values()), default=0) <= MAX_REQUESTS[name], where
    for j, c in enumerate(calls):
        asked = sorted(i for i, rc in ref_calls.items() if len(rc) > j)
        first = ref_calls[asked[0]][j]
        assert c["method"] == method and c["kind"] == first["kind"] and c["wpow"] == first["wpow"] and c["weights"] is first["weights"], where
        assert all(ref_calls[i][j]["kind"] == first["kind"] and ref_calls[i][j]["weights"] is first["weights"] for i in asked), where
        if method == "gram_batch":
            assert np.array_equal(c["what"], np.array([ref_calls[i][j]["what"][1] for i in asked])), where
        else:
            assert c["what"] == full, where
        if first["params"] is None:
            assert c["params"] is None, where
            continue
        want = np.array([ref_calls[i][j]["params"] for i in asked])
        if full is not None:
            rows = np.zeros((full, want.shape[1]))
            rows[asked] = want
            want = rows
        assert c["params"].shape == want.shape and c["params"].tobytes() == want.tobytes(), where


@pytest.mark.parametrize("solver", ["lapack", "jacobi"])
@pytest.mark.parametrize("name", NAMES)
def test_the_one_refit_statement_is_bitwise_the_single_item_bodies(name, solver):
    pts, inst, radius = _scene(name)
    n = len(pts)
    rng = np.random.default_rng(7)
    est = _estimators.ESTIMATORS[name]()
    est.refit_solver = solver
    few = est.nonminimal_sample_size - 1
    one, two, out, dup = (np.flatnonzero(inst == v) for v in (1, 2, 0, -1))
    # labels: 0 = instance 1 (well supported), 1 = instance 2 (in `skip`), 2 = fewer points than a refit needs, 3 = no point at all,
    # 4 = coincident points, 5 = the other outliers
    K, skip = 6, (1,)
    labels = np.full(n, 5, dtype=np.int32)
    labels[one], labels[two], labels[out[:few]], labels[dup] = 0, 1, 2, 4
    # selections of one size: instance 1, instance 2, the coincident points, outliers; and selections too small for a refit
    m = DUPLICATES
    batch = np.array([np.sort(rng.choice(one, m, replace=False)), np.sort(rng.choice(two, m, replace=False)), dup,
                      np.sort(rng.choice(out, m, replace=False))])
    small = np.array([one[:few], two[:few]])
    w_some = rng.uniform(0.5, 2.0, n)
    w_some[two] = 0.0                                    # instance 2 has no weight: selections of unequal fate inside one batch
    weightings = [("unweighted", None), ("weighted", rng.uniform(0.5, 2.0, n)), ("instance 2 without weight", w_some),
                  ("all-zero weights", np.zeros(n))]
    scenes = [("plain", pts, (0.0, np.inf))]
    if radius is not None:
        scenes.append(("far from the origin", pts + FAR[name], (0.0, np.inf)))
        scenes.append(("radius range that excludes the fit", pts, (0.0, 0.5 * radius)))
    seen = {entry: set() for entry in ("nonminimal", "nonminimal_labels", "nonminimal_batch")}
    mixed_batches = 0

    def note(entry, models):
        seen[entry].add(len(models) > 0)

    for scene, p, rr in scenes:
        ctx = OracleContext()
        ctx.set_points(est.model_type, p)
        ctx.set_labels(labels)
        if radius is not None:
            est.radius_range = rr
        for wname, w in weightings:
            where = (name, solver, scene, wname)
            # -- one selection: by label and by index
            for sel in [("label", k) for k in range(K)] + [("index", row) for row in batch] + [("index", small[0])]:
                want, ref_calls = _reference(est, ctx, sel, w)
                counting = Counting(ctx)
                got = est.nonminimal(counting, sel, w)
                _same_models(got, want, where + (sel,))
                _check_single_calls(counting.calls, ref_calls, where + (sel,))
                assert len(ref_calls) <= MAX_REQUESTS[name]
                note("nonminimal", got)
            # -- all labels at once
            ref = {k: _reference(est, ctx, ("label", k), w) for k in range(K) if k not in skip}
            counting = Counting(ctx)
            got = est.nonminimal_labels(counting, K, w, skip=skip)
            assert len(got) == K and got[1] == [] and got[3] == []           # the label in `skip`, the empty label
            for k in ref:
                _same_models(got[k], ref[k][0], where + ("label", k))
                note("nonminimal_labels", got[k])
            _check_stacked_calls(name, counting.calls, "gram_labels", {k: r[1] for k, r in ref.items()}, K, where)
            assert est.nonminimal_labels(Counting(ctx), K, w, skip=tuple(range(K))) == [[]] * K
            # -- a batch of selections
            for index in (batch, small):
                ref = {b: _reference(est, ctx, ("index", index[b]), w) for b in range(len(index))}
                counting = Counting(ctx)
                got = est.nonminimal_batch(counting, index, w)
                assert len(got) == len(index)
                for b in ref:
                    _same_models(got[b], ref[b][0], where + ("batch row", b))
                    note("nonminimal_batch", got[b])
                _check_stacked_calls(name, counting.calls, "gram_batch", {b: r[1] for b, r in ref.items()}, None, where)
                mixed_batches += len({len(g) for g in got}) == 2
    for entry, fates in seen.items():
        assert fates == {True, False}, (name, entry, fates)     # every entry point gave a model somewhere and none somewhere
    # a selection without weight (line, plane, round family) or of coincident points (round family) fails next to ones that fit; the
    # other estimators fit any finite Gram matrix of enough points, so their batches, whose selections share a size, share a fate
    if name in ("line", "plane", "sphere", "circle"):
        assert mixed_batches > 0


class Poisoned(Counting):
    """the context, with one entry (and its mirror image) of every Gram matrix of one kind replaced"""

    def __init__(self, ctx, kind, entry, value):
        super().__init__(ctx)
        self.kind, self.entry, self.value = kind, entry, value

    def _poison(self, kind, res):
        G = np.array(res[0], dtype=np.float64)
        if kind == self.kind:
            i, j = self.entry
            G[..., i, j] = G[..., j, i] = self.value
        return (G,) + tuple(res[1:])

    def gram(self, kind, *a, **kw):
        return self._poison(kind, super().gram(kind, *a, **kw))

    def gram_labels(self, kind, *a, **kw):
        return self._poison(kind, super().gram_labels(kind, *a, **kw))

    def gram_batch(self, kind, *a, **kw):
        return self._poison(kind, super().gram_batch(kind, *a, **kw))


@pytest.mark.parametrize("solver", ["lapack", "jacobi"])
@pytest.mark.parametrize("name", [n for n in NAMES if n != "line"])
def test_a_non_finite_gram_matrix_gives_no_model_through_every_entry_point(name, solver):
    """NaN or Inf in a Gram matrix - the first request's or the second's; the weight sum, a first moment or the last diagonal entry -
    ends the refit with no model: no exception out of LAPACK, no warning, the same answer from the three entry points.  (The line
    is not here: its refit raises what eigh raises on a non-finite scatter, from every entry point.)"""
    pts, inst, _ = _scene(name)
    est = _estimators.ESTIMATORS[name]()
    est.refit_solver = solver
    ctx = OracleContext()
    ctx.set_points(est.model_type, pts)
    labels = np.where(inst == 1, 0, np.where(inst == 2, 1, 2)).astype(np.int32)
    ctx.set_labels(labels)
    rng = np.random.default_rng(5)
    index = np.array([np.sort(rng.choice(np.flatnonzero(inst == v), 20, replace=False)) for v in (1, 2)])
    w = rng.uniform(0.5, 2.0, len(pts))
    counting = Counting(ctx)
    assert len(est.nonminimal(counting, ("label", 0), w)) == 1               # the same calls on clean matrices: a model
    kinds = [c["kind"] for c in counting.calls]
    assert len(kinds) == MAX_REQUESTS[name]
    for kind in kinds:
        q = _lib.GRAM_Q.get(kind, _lib.POINT_DIM[est.model_type] + 1)
        for entry in ((0, 0), (0, 1), (q - 1, q - 1)):
            for value in (np.nan, np.inf):
                bad = Poisoned(ctx, kind, entry, value)
                with warnings.catch_warnings():
                    warnings.simplefilter("error")
                    assert est.nonminimal(bad, ("label", 0), w) == [], (kind, entry, value)
                    assert est.nonminimal(bad, ("index", index[0]), None) == [], (kind, entry, value)
                    assert est.nonminimal_labels(bad, 3, w) == [[], [], []], (kind, entry, value)
                    assert est.nonminimal_batch(bad, index, w) == [[], []], (kind, entry, value)
                assert {c["kind"] for c in bad.calls} >= {kind}              # the poisoned request was made


def test_the_line_refit_answers_a_non_finite_gram_matrix_as_its_single_item_body_did():
    """the line is the exception: what numpy's eigh on the non-finite scatter raises or returns comes out of every entry point"""
    pts, inst, _ = _scene("line")
    est = _estimators.LineEstimator()
    ctx = OracleContext()
    ctx.set_points(est.model_type, pts)
    ctx.set_labels(np.where(inst == 1, 0, 1).astype(np.int32))
    index = np.array([np.flatnonzero(inst == v)[:20] for v in (1, 2)])

    def answer(fn):
        try:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                return fn()
        except np.linalg.LinAlgError as e:
            return type(e)
    for entry in ((0, 0), (0, 1), (2, 2)):
        for value in (np.nan, np.inf):
            bad = Poisoned(ctx, _lib.GRAM_AFFINE, entry, value)
            want = answer(lambda: refit_reference.nonminimal(est, bad, ("label", 0), None))
            for got in (answer(lambda: est.nonminimal(bad, ("label", 0), None)), answer(lambda: est.nonminimal_labels(bad, 1)[0])):
                assert type(got) is type(want)
                if isinstance(want, list):
                    _same_models(got, want, (entry, value))
            want = [answer(lambda: refit_reference.nonminimal(est, bad, ("index", row), None)) for row in index]
            got = answer(lambda: est.nonminimal_batch(bad, index))
            if isinstance(got, list):
                for g, w_ in zip(got, want):
                    _same_models(g, w_, (entry, value))
            else:
                assert got in want


# ---- the Gauss-Newton refits: the one loop (_estimators._gauss_newton) against the four copies of it (tests/refit_reference.py) --------
GN = {"cylinder": (cylinder_model, 5), "cone": (cone_model, 6), "torus": (torus_model, 7)}     # the model module, the fewest points


def _set_provider(sets, log):
    """A Gram provider over items with their own point sets, sets[r] = (model module, pts, w): every request is written down with
    its rows, and the module's numpy_gram answers each row on its own.  Returns (provider, what numpy_gram logged per item)."""
    per_item = [[] for _ in sets]

    def gram(kind, prm, use_w, wpow, rows):
        log.append((kind, None if prm is None else np.array(prm), use_w, wpow, np.array(rows)))
        out = [sets[r][0].numpy_gram(sets[r][1], sets[r][2], log=per_item[r])(kind, None if prm is None else prm[k:k + 1], use_w, wpow, [0])
               for k, r in enumerate(rows)]
        return np.concatenate([o[0] for o in out]), np.concatenate([o[1] for o in out]), np.concatenate([o[2] for o in out])
    return gram, per_item


def _same_requests(got, want, where):
    """two logs of _set_provider: the same requests in the same order - kind, parameter rows (bytes), use_weights, wpow, rows"""
    assert len(got) == len(want), where
    for g, r in zip(got, want):
        assert g[0] == r[0] and g[2] is r[2] and g[3] == r[3] and np.array_equal(g[4], r[4]), where
        assert (g[1] is None) == (r[1] is None), where
        if g[1] is not None:
            assert g[1].dtype == r[1].dtype and g[1].shape == r[1].shape and g[1].tobytes() == r[1].tobytes(), where


@pytest.mark.parametrize("name", list(GN))
def test_the_one_gauss_newton_loop_is_bitwise_the_copy_it_replaced(name):
    """Five items that leave the loop at different times, on the smallest of the type's refit fixtures: its start (several steps), no
    init (never starts), a start at the fit itself (stops early), an all-NaN start (never starts) and a selection one point short
    (fails at its first request).  Product and reference body return the same bytes and make the same requests."""
    model, n = GN[name]
    pts, w, gt, start = model.refit_fixture(n, 0.0, False, seed=n)
    est = _estimators.ESTIMATORS[name]()
    body = refit_reference.FIT_MANY[type(est)]
    (fitted,), = body(est, model.numpy_gram(pts, w), 1, [start])
    sets = [(model, pts, w)] * 4 + [(model, pts[:n - 1], None)]
    inits = [start, None, fitted, np.full(len(gt), np.nan), start]
    runs = {}
    for which, fit in (("product", est._fit_many), ("reference", lambda *a: body(est, *a))):
        log = []
        gram, per_item = _set_provider(sets, log)
        runs[which] = (fit(gram, 5, inits), log, [sum(r[0] != _lib.GRAM_AFFINE for r in item) for item in per_item])
    got, want = runs["product"], runs["reference"]
    assert len(got[0]) == len(want[0]) == 5
    for b in range(5):
        _same_models(got[0][b], want[0][b], (name, b))
    _same_requests(got[1], want[1], name)
    assert [len(m) for m in want[0]] == [1, 0, 1, 0, 0]
    steps = want[2]                                         # Gauss-Newton requests per item
    assert steps[1] == steps[3] == 0 and steps[4] == 1 and 1 <= steps[2] < steps[0] <= 10 and got[2] == steps, (name, steps)


def test_a_mixed_batch_hands_each_constituent_exactly_its_rows():
    """two cylinders and two cones interleaved through PrimitiveEstimator._fit_many: the constituents' loops and the reference
    bodies return the same bytes from the same requests, no request mixes the classes' items, and every item's model is the one
    its constituent's reference body fits alone"""
    sets, inits, alone = [], [], []
    est = _estimators.PrimitiveEstimator(("cylinder", "cone"))
    for n, weighted in ((0, False), (64, True)):
        for model, cls in ((cylinder_model, _lib.CYLINDER3D), (cone_model, _lib.CONE3D)):
            part = est.parts[cls]
            fewest = part.nonminimal_sample_size
            pts, w, gt, start = model.refit_fixture(n or fewest, 0.0, weighted, seed=n + fewest)
            sets.append((model, pts, w))
            inits.append(est._row(cls, start))
            (one,), = refit_reference.FIT_MANY[type(part)](part, model.numpy_gram(pts, w), 1, [start])
            alone.append(est._row(cls, one))
    ref = _estimators.PrimitiveEstimator(("cylinder", "cone"))
    for part in ref.parts.values():
        refit_reference.with_reference_fit_many(part)
    runs = []
    for e in (est, ref):
        log = []
        runs.append((e._fit_many(_set_provider(sets, log)[0], 4, inits), log))
    (got, log), (want, ref_log) = runs
    for b in range(4):
        _same_models(got[b], want[b], b)
        _same_models(got[b], [alone[b]], b)
    _same_requests(log, ref_log, "mixed")
    kinds = {_lib.GRAM_CYL_GN: {0, 2}, _lib.GRAM_AFFINE: {0, 2}, _lib.GRAM_CONE_GN: {1, 3}}
    assert {r[0] for r in log} == set(kinds)
    for kind, _, _, _, rows in log:
        assert set(rows.tolist()) <= kinds[kind], (kind, rows)
    assert log[0][4].tolist() == [0, 2] and any(r[4].tolist() == [1, 3] for r in log)        # both items of a class in one request


def _pnp_scene():
    """(ctx with labels 0 .. 4 set, weights, inits per label, selections [5, 8] with a start for them): label 0 = object 1 and
    label 1 = object 2 from two different finite starts (the test moves label 0's to its fit, so that it stops first), label 2 without an init, label 3 from an all-NaN start, label 4 with three
    points (a PnP refit needs four); the selections: object 1 twice, one point eight times, object 2, outliers"""
    x1, x2, K, gt, poses = datasets.make_poses(n_per_object=120, n_objects=2, n_outliers=40, seed=2)
    pts, _ = datasets.normalize_pnp(x1, x2, K)
    rng = np.random.default_rng(11)
    one, two, out = (np.flatnonzero(gt == v) for v in (1, 2, 0))
    labels = np.full(len(pts), 5, dtype=np.int32)
    labels[one[:60]], labels[two], labels[one[60:90]], labels[one[90:]], labels[out[:3]] = 0, 1, 2, 3, 4
    ctx = OracleContext()
    ctx.set_points(_lib.PNP, pts)
    ctx.set_labels(labels)
    far = poses[0].copy()
    far[[3, 7, 11]] += [1.0, -1.0, 2.0]
    inits = [poses[0] + 1e-3 * rng.normal(size=12), poses[1] + 1e-2 * rng.normal(size=12), None, np.full(12, np.nan), poses[0], None]
    index = np.array([np.sort(rng.choice(one, 8, replace=False)), np.sort(rng.choice(one, 8, replace=False)), np.full(8, one[7]),
                      np.sort(rng.choice(two, 8, replace=False)), np.sort(rng.choice(out, 8, replace=False))])
    return ctx, rng.uniform(0.5, 2.0, len(pts)), inits, index, far


def _same_calls(calls, ref_calls, where):
    """two logs of Counting: the same context calls in the same order"""
    assert len(calls) == len(ref_calls), where
    for c, r in zip(calls, ref_calls):
        assert c["method"] == r["method"] and c["kind"] == r["kind"] and c["wpow"] == r["wpow"] and c["weights"] is r["weights"], where
        assert c["params"].dtype == r["params"].dtype and c["params"].shape == r["params"].shape, where
        assert c["params"].tobytes() == r["params"].tobytes(), where
        assert np.array_equal(c["what"], r["what"]), where


def test_the_pnp_refit_through_the_one_loop_is_bitwise_the_copy_it_replaced():
    """PnP's stacked refit on the OracleContext, through nonminimal_labels (five labels that leave the loop at different times) and
    through the base nonminimal_batch (five selections from one start; then no start, then an all-NaN start): the same bytes and
    the same gram_labels / gram_batch calls as the reference body.  The all-NaN start is SENT (PnP does not look at its start: the
    sums fail it), which the equal calls hold."""
    ctx, w, inits, index, far = _pnp_scene()
    est = _estimators.PnPEstimator()
    ref = refit_reference.with_reference_fit_many(_estimators.PnPEstimator())
    with np.errstate(all="ignore"):
        # -- all labels at once
        for weights in (w, None):
            inits[0] = ref.nonminimal_labels(ctx, 6, weights, inits=inits, skip=(1, 2, 3, 4, 5))[0][0]     # label 0 starts at its fit
            runs = []
            for e in (est, ref):
                counting = Counting(ctx)
                runs.append((e.nonminimal_labels(counting, 6, weights, inits=inits, skip=(5,)), counting.calls))
            (got, calls), (want, ref_calls) = runs
            for k in range(6):
                _same_models(got[k], want[k], ("label", k))
            _same_calls(calls, ref_calls, "labels")
            assert [len(m) for m in want] == [1, 1, 0, 0, 0, 0]
            assert all(c["method"] == "gram_labels" and c["kind"] == _lib.GRAM_PNP_GN and c["wpow"] == 2 for c in calls)
            sent = [np.flatnonzero(np.any(c["params"] != 0, axis=1)).tolist() for c in calls]    # NaN != 0: label 3 shows
            assert sent[0] == [0, 1, 3, 4] and all(set(s) <= {0, 1} for s in sent[1:]) and 2 < len(sent) <= 10
            assert len({sum(k in s for s in sent) for k in (0, 1)}) == 2                        # ... the two fits stop at different times
        # -- selections of one size from one start
        base = _estimators.Estimator.nonminimal_batch
        for init in (far, None, np.full(12, np.nan)):
            runs = []
            for e in (est, ref):
                counting = Counting(ctx)
                runs.append((base(e, counting, index, w, init), counting.calls))
            (got, calls), (want, ref_calls) = runs
            assert len(got) == len(want) == 5
            for b in range(5):
                _same_models(got[b], want[b], ("batch row", b))
            _same_calls(calls, ref_calls, "batch")
            if init is far:
                assert 2 < len(calls) <= 10 and len({len(c["what"]) for c in calls}) > 1      # the selections stop at different times
                assert len(want[0]) == len(want[1]) == 1
            else:
                assert want == [[]] * 5 and len(calls) == (0 if init is None else 1)
