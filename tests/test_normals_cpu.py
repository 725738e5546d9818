"""estimateNormals without a GPU: the public function's argument checks, the ABI entry, and the numpy restatement of
pgx_estimate_normals (normals_model.py) held to the 50-digit fixture tests/golden/kat_normals_v1.npz within the tolerance
C(m) * EPS * lambda_max / (lambda_1 - lambda_0) that DESIGN.md 4.10 derives from the operation order - and four planted errors, each
refused by that same tolerance."""
import ctypes
import inspect
import os

import numpy as np
import pytest

import normals_model as NM
import pyprogressivex as px
from pyprogressivex import _lib, datasets

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kat_normals_v1.npz")


@pytest.fixture(scope="module")
def kat():
    z = np.load(GOLDEN)
    d = {k: z[k] for k in z.files}
    d["off"], d["idx"], d["centres"] = NM.star_graph(d["sizes"])
    gap = d["eig"][:, 1] - d["eig"][:, 0]
    d["tol"] = np.array([NM.tolerance_factor(int(m)) for m in d["sizes"]]) * NM.EPS * d["eig"][:, 2] / gap
    return d


def angles(kat, normals):
    return np.array([NM.angle_to(normals[c], kat["normal_hi"][f], kat["normal_lo"][f]) for f, c in enumerate(kat["centres"])])


def test_estimate_normals_is_exported_with_its_signature():
    assert "estimateNormals" in px.__all__
    sig = inspect.signature(px.estimateNormals)
    assert list(sig.parameters) == ["points", "k", "radius", "viewpoint", "return_curvature"]
    assert [p.default for p in sig.parameters.values()][1:] == [16, None, None, False]
    doc = " ".join(px.estimateNormals.__doc__.split())
    for phrase in ("more than k neighbours", "unsigned", "findCylinders accepts either", "propagation", "NaN rows"):
        assert phrase in doc, phrase
    assert "estimateNormals" in px.findCylinders.__doc__


GOOD = np.arange(30.0).reshape(10, 3)


@pytest.mark.parametrize("points", [np.zeros((2, 3)), np.zeros((5, 2)), np.zeros(9), np.zeros((2, 3, 3))])
def test_estimate_normals_rejects_bad_points(points):
    with pytest.raises(ValueError, match=r"points should be an array with dims \[n,3\], n>=3"):
        px.estimateNormals(points)


@pytest.mark.parametrize("kw, match", [(dict(k=1), "k should be"), (dict(k=0), "k should be"), (dict(k=2.5), "k should be"),
                                       (dict(k=True), "k should be"), (dict(k=None), "k or radius"),
                                       (dict(radius=0.0), "radius should be"), (dict(radius=-1.0), "radius should be"),
                                       (dict(radius=float("nan")), "radius should be"), (dict(radius="far"), "radius should be"),
                                       (dict(viewpoint=[0.0, 1.0]), "viewpoint should be"),
                                       (dict(viewpoint=[0.0, 1.0, float("inf")]), "viewpoint should be"),
                                       (dict(viewpoint=[0.0, float("nan"), 1.0]), "viewpoint should be"),
                                       (dict(viewpoint="here"), "viewpoint should be")])
def test_estimate_normals_rejects_bad_arguments_before_it_touches_the_context(kw, match, monkeypatch):
    from pyprogressivex import _api

    def no_context():
        raise AssertionError("the context was touched before the arguments were checked")
    monkeypatch.setattr(_api, "_context", no_context)
    with pytest.raises(ValueError, match=match):
        px.estimateNormals(GOOD, **kw)


def test_the_library_exports_the_entry_point():
    assert "pgx_estimate_normals" in _lib.ABI_SYMBOLS
    assert len(_lib.ABI_SYMBOLS) == len(set(_lib.ABI_SYMBOLS))
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pgx.h")).read()
    assert "int pgx_estimate_normals(pgx_ctx *ctx, const double *points, int64_t n, const double *viewpoint" in header
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "pgx_estimate_normals")
    assert hasattr(_lib.Context, "estimate_normals")


def test_make_cylinders_keeps_its_default_normals():
    a = datasets.make_cylinders(n_per_cylinder=50, n_cylinders=2, n_outliers=20, seed=3)
    b = datasets.make_cylinders(n_per_cylinder=50, n_cylinders=2, n_outliers=20, seed=3, normals="synthetic")
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    with pytest.raises(ValueError, match="normals"):
        datasets.make_cylinders(n_per_cylinder=50, n_cylinders=2, n_outliers=20, seed=3, normals="guessed")


def test_the_fixture_meets_its_conditions(kat):
    assert len(kat["sizes"]) == 240 and kat["points"].shape == (int(kat["sizes"].sum()), 3)
    assert kat["sizes"].min() == 3 and kat["sizes"].max() > 17                  # the smallest neighbourhood and hubs beyond k + 1
    assert (kat["eig"][:, 1] > kat["eig"][:, 0]).all() and (kat["tol"] <= 1e-6).all() and (kat["tol"] > 0).all()
    unit = np.linalg.norm(kat["normal_hi"] + kat["normal_lo"], axis=1)
    assert np.abs(unit - 1.0).max() <= 2 * NM.EPS
    moved = kat["groups"][kat["group"], 1] != 0
    assert moved.sum() == 60 and (np.abs(kat["points"][np.repeat(moved, kat["sizes"])]) > 9e5).all()


def test_restatement_against_the_definition_at_50_digits(kat, oracle):
    got = NM.estimate(kat["points"], kat["off"], kat["idx"])
    c = kat["centres"]
    assert got["defined"][c].all()
    assert got["undefined"] == len(kat["points"]) - len(c)                      # the leaves of the stars have one neighbour
    assert got["sweeps"][c].max() <= NM.MAX_SWEEPS                              # the premise of C(m)'s Jacobi term
    ratio = angles(kat, got["normals"]) / kat["tol"]
    print(f"worst angle / tolerance {ratio.max():.4f} (fixture {int(ratio.argmax())}, m = {int(kat['sizes'][ratio.argmax()])}); "
          f"most sweeps {int(got['sweeps'][c].max())}")
    assert ratio.max() <= 1.0
    # the eigenvalue the curvature is made of: lambda_0 / trace against the 50-digit eigenvalues, to the same perturbation bound
    exact = kat["eig"][:, 0] / kat["eig"].sum(axis=1)
    bound = np.array([NM.tolerance_factor(int(m)) for m in kat["sizes"]]) * NM.EPS
    assert (np.abs(got["curvature"][c] - exact) <= bound).all()
    assert np.abs(np.linalg.norm(got["normals"][c], axis=1) - 1.0).max() <= 64 * NM.EPS


@pytest.mark.parametrize("plant", ["no_self", "uncentred", "f32", "largest"])
def test_a_planted_error_is_refused_by_the_same_tolerance(kat, oracle, plant):
    got = NM.estimate(kat["points"], kat["off"], kat["idx"], plant=plant)
    c = kat["centres"]
    use = got["defined"][c]                                                     # (without the self term m = 2 neighbourhoods are undefined)
    if plant == "uncentred":                                                    # three points: the plane through them holds the centre, and the
        use = use & (kat["sizes"] > 3)                                          # scatter about the centre has the same normal - no error to refuse
    assert use.sum() >= 180
    ratio = (angles(kat, np.nan_to_num(got["normals"])) / kat["tol"])[use]
    print(f"{plant}: angle / tolerance from {ratio.min():.3g} to {ratio.max():.3g}, {int((ratio > 1).sum())} of {int(use.sum())} refused")
    assert (ratio > 1.0).all()


def test_sign_rule(oracle):
    x = [1.0, 2.0, 3.0]
    assert NM.orient([0.5, -0.5, 0.1], x) == [0.5, -0.5, 0.1]                   # tie of magnitudes: the lowest index decides
    assert NM.orient([-0.5, 0.5, 0.1], x) == [0.5, -0.5, -0.1]
    assert NM.orient([0.1, -0.7, 0.7], x) == [-0.1, 0.7, -0.7]
    assert NM.orient([0.0, 0.0, -1.0], x) == [0.0, 0.0, 1.0]
    assert NM.orient([0.0, 0.0, 1.0], x, viewpoint=[1.0, 2.0, 10.0]) == [0.0, 0.0, 1.0]      # the viewpoint on the normal's side
    assert NM.orient([0.0, 0.0, 1.0], x, viewpoint=[1.0, 2.0, -10.0]) == [0.0, 0.0, -1.0]    # on the other side
    assert NM.orient([0.0, 0.0, -1.0], x, viewpoint=[1.0, 2.0, -10.0]) == [0.0, 0.0, -1.0]
    assert NM.orient([0.0, 0.0, 1.0], x, viewpoint=[5.0, -4.0, 3.0]) == [0.0, 0.0, 1.0]      # t == 0: no second flip
    assert NM.orient([0.0, 0.0, -1.0], x, viewpoint=[5.0, -4.0, 3.0]) == [0.0, 0.0, 1.0]
    # through estimate(): a 3 x 3 grid in the plane z = 0, seen from above and from below
    g = np.array([[i, j, 0.0] for i in range(3) for j in range(3)], dtype=np.float64)
    off = np.arange(0, 9 * 8 + 1, 8, dtype=np.int32)
    idx = np.array([j for i in range(9) for j in range(9) if j != i], dtype=np.int32)
    up = NM.estimate(g, off, idx, viewpoint=[0.0, 0.0, 5.0])
    down = NM.estimate(g, off, idx, viewpoint=[0.0, 0.0, -5.0])
    flat = NM.estimate(g, off, idx)
    assert (up["normals"][:, 2] == 1.0).all() and (down["normals"][:, 2] == -1.0).all() and (flat["normals"][:, 2] == 1.0).all()
    assert (up["curvature"] == 0.0).all() and up["undefined"] == 0
