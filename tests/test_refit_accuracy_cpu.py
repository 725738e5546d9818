"""The non-minimal refits against a least-squares answer computed some other way: every fixture of tests/golden/kat_refits_v1.npz
(the refits restated from their definitions at 50 digits, tests/refit_exact.py) through every entry point of the estimators on the
OracleContext, with both refit_solver values; tolerances, selections and entry points are those of tests/refit_accuracy_cases.py.
The GPU context runs the same comparisons in tests/test_gpu_refit_accuracy.py.

What the oracle cannot show - it shares its row generators, its weight handling and the pose Jacobian with the kernels and the
host - shows here: the planted errors below (a weight power, a dropped point, one Gram entry off by 1e-9, the Hartley scale from
weighted moments, a negated Jacobian column) pass every oracle comparison by construction and are each refused by this one.

Worst error / tolerance on the OracleContext (LAPACK and Jacobi alike unless stated): see docs/lab-notebook.md, "Refit accuracy"."""
import glob
import importlib.util
import os

import numpy as np
import pytest

import refit_accuracy_cases as cases
import refit_exact
from oracle_ctx import OracleContext
from pyprogressivex import _lib

EIGEN_TYPES = [t for t in cases.TYPES if t != "pnp"]
FINAL_KIND = dict(line=_lib.GRAM_AFFINE, plane=_lib.GRAM_AFFINE, circle=_lib.GRAM_CIRCLE, sphere=_lib.GRAM_SPHERE,
                  vanishing_point=_lib.GRAM_VP, homography=_lib.GRAM_DLT_H, homography_sym=_lib.GRAM_DLT_H,
                  fundamental=_lib.GRAM_EPI_F, pnp=_lib.GRAM_PNP_GN)


@pytest.fixture(scope="module")
def fixtures():
    return cases.load()


def test_the_fixture_file_holds_every_selection_and_meets_its_conditions(fixtures):
    others = [os.path.getsize(f) for f in glob.glob(os.path.join(os.path.dirname(cases.FILE), "kat_*.npz")) if f != cases.FILE]
    assert os.path.getsize(cases.FILE) <= max(others)
    for name, case in fixtures.items():
        stored = "homography" if name == "homography_sym" else name
        assert case.n <= 3000 and case.weights[2][cases.ZERO_AT] == 0.0
        assert case.weights[2].max() == 1e3 and case.weights[2][case.weights[2] > 0].min() == 1e-3
        sizes = {len(cases.members(case, s)) for s in range(len(case.sels)) if case.sels[s][0] is not None}
        assert sizes >= {cases.MINIMAL[stored], cases.MINIMAL[stored] + 1, 9, 21, 63, 64, 65, 128, 129, 200}
        assert any(len(set(idx.tolist())) < len(idx) for idx, _ in case.sels if idx is not None)          # a repeated index
        big = cases.members(case, [s for s in range(len(case.sels)) if case.sels[s][1] == 0][0])
        assert len(big) >= 200 and big.min() < 64 and big.max() >= 256                                    # across blocks of 256
        seen = {(s, wt) for s, wt, _ in case.fixtures}
        assert all((s, 0) in seen and (s, 1) in seen for s in range(len(case.sels)))                      # weights off and on
        wide = [s for s, wt, _ in case.fixtures if wt == 2]
        assert len(wide) >= 3 and all(cases.ZERO_AT in cases.members(case, s) for s in wide)
        for s, wt, row in case.fixtures:
            assert 0 < row[cases.C_TOL] <= 1e-6, (name, s, wt)
            if name == "pnp":
                assert row[cases.C_KAPPA] <= 1e10, (s, wt)
                assert 1 <= row[cases.C_FIRST] <= 6, (s, wt)          # the reference's own run converges: no pose fixture without its run


@pytest.mark.parametrize("solver", ["lapack", "jacobi"])
@pytest.mark.parametrize("name", EIGEN_TYPES)
def test_eigen_refits_are_within_the_derived_tolerance_of_the_50_digit_fit(fixtures, name, solver):
    ratios = cases.eigen_ratios(name, fixtures[name], OracleContext(), solver)
    print(cases.report(name, f"cpu/{solver}", ratios))
    assert len({(s, wt) for _, s, wt in ratios}) == len(fixtures[name].fixtures)      # no case left out
    bad = {k: v for k, v in ratios.items() if not v <= 1.0}
    assert not bad, bad


def test_pose_refits_take_the_reference_step_and_end_where_its_step_vanishes(fixtures):
    ratios = cases.pose_ratios(fixtures["pnp"], OracleContext())
    print(cases.report("pnp", "cpu", ratios))
    case = fixtures["pnp"]
    every = {(s, wt) for s, wt, _ in case.fixtures}
    by_label = {(s, wt) for s, wt in every if case.sels[s][0] is None}
    want = {"step/pnp_refine_batch": every, "step/_fit_many": every, "run/nonminimal_batch": every, "run/nonminimal_batch/reversed": every,
            "run/nonminimal/index": every - by_label, "run/nonminimal/label": by_label, "run/nonminimal_labels": by_label}
    assert {e: {(s, wt) for e2, s, wt in ratios if e2 == e} for e in {e for e, _, _ in ratios}} == want      # no case, no entry point left out
    bad = {k: v for k, v in ratios.items() if not v <= 1.0}
    assert not bad, bad


# ---- planted errors: each passes the oracle comparisons by construction (both sides would share it) and must be refused here --------
class Planted(OracleContext):
    """the oracle context with one error in what its Gram calls answer"""

    def __init__(self, error, kind=None):
        super().__init__()
        self.error, self.kind, self.current_weights = error, kind, None

    def gram(self, kind, sel, params=None, weights=None, wpow=2):
        if self.error == "weight power lowered by one" and weights is not None:
            weights, wpow = (weights, 1) if wpow == 2 else (None, 1)
        if self.error == "last selected point dropped":
            index = np.asarray(sel[1]) if sel[0] == "index" else np.flatnonzero(self.labels == int(sel[1]))
            sel = ("index", index[:-1])
        hartley = self.error == "Hartley scale from the weighted moments" and kind == _lib.GRAM_AFFINE and weights is None \
            and self.current_weights is not None
        if hartley:
            weights = self.current_weights
        G, cnt, bad = super().gram(kind, sel, params=params, weights=weights, wpow=wpow)
        G = np.array(G, dtype=np.float64)
        if hartley and G[0, 0] > 0:       # the estimator divides by the count: sum w^2 x / sum w^2, the weighted moments proper
            G *= cnt / G[0, 0]
        if self.error == "one Gram entry and its mirror scaled by 1 + 1e-9" and kind == self.kind:
            # the off-diagonal entry of largest magnitude: an entry that is zero by construction (the first moments of centred
            # coordinates) has no error to scale
            off = np.abs(np.triu(G, 1))
            i, j = np.unravel_index(int(np.argmax(off)), off.shape)
            if kind == _lib.GRAM_PNP_GN:      # the pose: the translation along x against the one along the optical axis, in the badly
                i, j = 3, 5                   # determined block (kappa ~ 1e6: in the rotation block 1e-9 stays inside the bound, measured 0.01 tol)
            G[i, j] = G[j, i] = G[i, j] * (1.0 + 1e-9)
        if self.error == "one pose Jacobian column negated" and kind == _lib.GRAM_PNP_GN:
            G[1, :] *= -1.0
            G[:, 1] *= -1.0
        return G, cnt, bad

    def gram_batch(self, kind, index, params=None, weights=None, wpow=2):
        res = [self.gram(kind, ("index", row), params=None if params is None else np.asarray(params)[b], weights=weights, wpow=wpow)
               for b, row in enumerate(np.asarray(index))]
        return np.array([r[0] for r in res]), np.array([r[2] for r in res], dtype=np.int32)


PLANTED = [(error, name) for error, names in [
    ("weight power lowered by one", cases.TYPES),
    ("last selected point dropped", cases.TYPES),
    ("one Gram entry and its mirror scaled by 1 + 1e-9", cases.TYPES),
    ("Hartley scale from the weighted moments", ["homography", "homography_sym", "fundamental"]),
    ("one pose Jacobian column negated", ["pnp"]),
] for name in names]


@pytest.mark.parametrize("error,name", PLANTED)
def test_a_planted_error_is_refused(fixtures, error, name):
    ctx = Planted(error, FINAL_KIND[name])
    if name == "pnp":
        ratios = cases.pose_ratios(fixtures[name], ctx, strict=False)
    else:
        ratios = cases.eigen_ratios(name, fixtures[name], ctx, "lapack", strict=False, before=lambda w: setattr(ctx, "current_weights", w))
    refused = {k: v for k, v in ratios.items() if not v <= 1.0}
    assert refused, (error, name, max(ratios.values()))
    if error == "one Gram entry and its mirror scaled by 1 + 1e-9" or error == "last selected point dropped":
        return
    # an error in the weights leaves the unweighted fixtures alone: the comparison refuses what is wrong, not everything
    if error != "one pose Jacobian column negated":
        assert all(wt != 0 for _, _, wt in refused), (error, name)


# ---- the fixture file is what the generator writes (needs mpmath: the one check that may skip) -----------------------------------------
def test_the_generator_reproduces_the_fixture_file():
    pytest.importorskip("mpmath")
    spec = importlib.util.spec_from_file_location("make_golden_refits", os.path.join(os.path.dirname(cases.FILE), "make_golden_refits.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    z = np.load(cases.FILE)
    W = gen.weights()
    # every array of the file, bit for bit, from the draw the file records per type (the draws before it failed a condition)
    data = gen.generate(verbose=False, first_attempt={name: z["npts"][t, 1] for t, name in enumerate(cases.STORED)})
    assert set(data) == set(z.files)
    for key in z.files:
        assert data[key].dtype == z[key].dtype and np.array_equal(data[key], z[key]), key
    # the decimal statement of the pose step that the comparisons run is the mpmath one
    p = gen.plan("pnp", int(z["npts"][cases.STORED.index("pnp"), 1]))
    idx = gen.members(p, 3)
    start = z["fx"][[f for f in range(len(z["meta"])) if z["meta"][f, 0] == cases.STORED.index("pnp")][0], cases.C_START]
    want = refit_exact.pnp_state(p["pts"][idx], W[0][idx], start)["delta"]
    got = refit_exact.pnp_step_decimal(p["pts"][idx], W[0][idx], start)
    assert np.abs(got - want).max() <= 1e-30 * np.abs(want).max() or np.array_equal(got, want)
