"""The iterative minimal solvers (4-point homography, 7-point fundamental matrix, P3P) against answers computed some other way: every
fixture of tests/golden/kat_minimal_v1.npz (the problems restated from their definitions at 50 digits, tests/minimal_exact.py)
through pgx_solve_minimal's restatement on the OracleContext at every batch size, and through the host routes Estimator.minimal;
fixtures, kinds, tolerances and the set comparison are those of tests/minimal_accuracy_cases.py.  The GPU context runs the same
comparisons in tests/test_gpu_minimal_accuracy.py.

What oracle and kernel share - a wrong coefficient, a missed root, a gate that drops a valid solution - passes their bit parity by
construction and shows here.  It did: the parent of this file's commit lost poses of the class "two poses share v" (the count is
asserted below from the recorded output), which the second way to u in solve_p3p returns.

Worst error / tolerance per type and class: see docs/lab-notebook.md, "Minimal-solver accuracy"."""
import glob
import importlib.util
import os

import numpy as np
import pytest

import minimal_accuracy_cases as cases
from oracle_ctx import OracleContext
from pyprogressivex import _estimators

ACCURACY, COVERAGE, NO_MODEL = cases.ACCURACY, cases.COVERAGE, cases.NO_MODEL


@pytest.fixture(scope="module")
def fixtures():
    return cases.load()


def test_the_fixture_file_holds_every_class_and_meets_its_conditions(fixtures):
    others = [os.path.getsize(f) for f in glob.glob(os.path.join(os.path.dirname(cases.FILE), "kat_*.npz")) if f != cases.FILE]
    assert os.path.getsize(cases.FILE) <= max(others)
    for name, case in fixtures.items():
        assert sum(len(pts) for _, pts, _ in case.sets) <= cases.MAX_ROWS
        for s, (sname, pts, scale) in enumerate(case.sets):
            assert len(cases.batch_of(case, s, 1)[0]) == 1 and set(case.set_of.tolist()) == set(range(len(case.sets)))
            if name != "pnp":
                assert scale == max(1.0, dict(cases.SETS[name])[sname])
        for cls, (cname, sname, count, kind) in enumerate(cases.CLASSES[name]):
            mine = np.flatnonzero(case.cls == cls)
            assert len(mine) == count >= 8 and (case.kind[mine] == kind).all(), (name, cname)
            if cname == "repeated index":
                assert all(len(set(case.samples[f].tolist())) < case.samples.shape[1] for f in mine)
            if cname == "out-of-range index":
                n = len(case.sets[[s for s, _ in cases.SETS[name]].index(sname)][1])
                assert all((case.samples[f] < 0).any() or (case.samples[f] >= n).any() for f in mine)
        for f in range(len(case.cls)):
            n, where = int(case.nref[f]), (name, cases.class_name(name, case.cls[f]), f)
            ref = case.ref[f][:n]
            assert np.isfinite(ref).all() and np.isnan(case.ref[f][n:]).all(), where
            dist = [np.abs(ref[i] - ref[j]).max() for i in range(n) for j in range(i)]
            if case.kind[f] == NO_MODEL:
                assert n == 0, where
            elif case.kind[f] == ACCURACY:
                assert n >= 1 and (case.tol[f][:n] > 0).all() and (case.tol[f][:n] <= 1e-6).all(), where
                assert all(d >= 1000 * case.tol[f][:n].max() for d in dist), where
            else:
                assert n >= 1 and (case.cond[f][:n] <= 1e4).all(), where
                assert all(d >= 1e-3 * np.abs(ref).max() for d in dist), where
    p = fixtures["pnp"]
    counts = {int(p.nref[f]) for f in range(len(p.cls)) if p.kind[f] != NO_MODEL}
    assert counts >= {1, 2, 3, 4}
    shared = np.flatnonzero(p.cls == cases.SHARED_V)
    assert len(shared) >= 16
    for f in shared:
        assert (np.abs(p.den[f][:p.nref[f]]) <= 1e-3).sum() >= 2 and p.sep[f][0] >= 1e-3, f
    fm = fixtures["fundamental"]
    assert {int(fm.nref[f]) for f in range(len(fm.cls)) if fm.kind[f] == ACCURACY} >= {1, 3}


def _complete(name, case, ratios):
    """no fixture left out, at every batch size of its set"""
    for s, (sname, _, _) in enumerate(case.sets):
        mine = set(np.flatnonzero(case.set_of == s).tolist())
        for S in cases.BATCHES:
            assert {f for (sn, S2, f) in ratios if sn == sname and S2 == S} == set(cases.batch_of(case, s, S)[0].tolist())
        assert {f for (sn, _, f) in ratios if sn == sname} == mine            # (the largest launch holds every fixture of the set)


def _shared_v(name, case, key):
    return name == "pnp" and case.cls[key[2]] == cases.SHARED_V


@pytest.mark.parametrize("name", cases.TYPES)
def test_solve_minimal_returns_the_reference_solution_set(fixtures, name):
    """every class but "two poses share v", which has the two tests below"""
    case = fixtures[name]
    ratios = cases.device_ratios(name, case, OracleContext(), strict=False)
    print(cases.report(name, "cpu", case, ratios))
    _complete(name, case, ratios)
    bad = {k: v for k, v in ratios.items() if not v <= 1.0 and not _shared_v(name, case, k)}
    assert not bad, bad


@pytest.mark.parametrize("name", cases.TYPES + ["homography_sym"])
def test_the_host_route_returns_the_reference_solution_set(fixtures, name):
    sym = name == "homography_sym"
    name = "homography" if sym else name
    case = fixtures[name]
    ratios = cases.host_ratios(name, case, strict=False, symmetric=sym)
    print(cases.report(name, "host" + ("/symmetric" if sym else ""), case, ratios))
    inside = {f for f in range(len(case.cls)) if cases.class_name(name, case.cls[f]) != "out-of-range index"}
    assert {f for _, _, f in ratios} == inside
    bad = {k: v for k, v in ratios.items() if not v <= 1.0 and not _shared_v(name, case, k)}
    assert not bad, bad


# ---- P3P where two poses share v: no pose lost (holds since the second way to u), each within 1e-6 (open) ----------------------------
def _shared_v_ratios(case, coverage_tol):
    dev = cases.device_ratios("pnp", case, OracleContext(), strict=False, coverage_tol=coverage_tol)
    host = cases.host_ratios("pnp", case, strict=False, coverage_tol=coverage_tol)
    return {k: v for k, v in {**dev, **host}.items() if _shared_v("pnp", case, k)}


def test_where_two_poses_share_v_every_pose_is_returned(fixtures):
    """as many models as the reference has poses, each pose with a slot of its own within a tenth of the class's separation, at every
    batch size and on the host route.  The parent lost poses here (below)."""
    ratios = _shared_v_ratios(fixtures["pnp"], cases.IDENTIFIED)
    assert {k[2] for k in ratios} == set(np.flatnonzero(fixtures["pnp"].cls == cases.SHARED_V).tolist())
    bad = {k: v for k, v in ratios.items() if not v <= 1.0}
    assert not bad, bad


@pytest.mark.xfail(strict=True, reason="open defect (DESIGN.md 4.5b): where two poses share v the returned poses are within 1e-6 of the 50-digit "
                   "ones on 10 of the 16 samples only (oracle and device; the host route on 11; the parent commit on 4) - no pose is lost any "
                   "more, but the worst is 3.4e-6 off (host 1.5e-5): v itself is ill-determined next to a double root.  Of the 6 "
                   "samples, 3 have the inaccurate poses from the second way to u (a Newton step on that path alone would repair them) "
                   "and 3 from the linear formula with the parent's bits, where no residual threshold separates them from complete samples")
def test_where_two_poses_share_v_every_pose_is_within_the_consistency_figure(fixtures):
    ratios = _shared_v_ratios(fixtures["pnp"], None)
    bad = {k: v for k, v in ratios.items() if not v <= 1.0}
    assert not bad, bad


# ---- the P3P change: what the parent lost, and what it must keep ---------------------------------------------------------------------
def _parent_ratio(case, f):
    return cases.match("pnp", case, f, case.parent[f], 1.0, strict=False)


def test_the_parent_lost_poses_that_share_v_and_the_change_keeps_every_complete_sample_bit_for_bit(fixtures):
    case = fixtures["pnp"]
    shared = np.flatnonzero(case.cls == cases.SHARED_V)
    short = [int(f) for f in shared if not cases.match("pnp", case, f, case.parent[f], 1.0, strict=False, coverage_tol=cases.IDENTIFIED) <= 1.0]
    lost = [int(f) for f in shared if not _parent_ratio(case, f) <= 1.0]
    print(f"P3P, two poses share v, {len(shared)} samples: the parent commit's oracle is short of a pose on {len(short)}, "
          f"and has every pose but one further than 1e-6 off on {len(lost) - len(short)} more")
    assert (len(shared), len(short), len(lost)) == (16, 10, 12) and set(short) <= set(lost)
    ctx = OracleContext()
    ctx.set_points(_estimators.PnPEstimator.model_type, case.sets[0][1])
    now = np.asarray(ctx.solve_minimal(np.ascontiguousarray(case.samples, dtype=np.int32))).reshape(-1, 4, 12)
    kept = [f for f in range(len(case.cls)) if _parent_ratio(case, f) <= 1.0]
    assert len(kept) >= len(case.cls) - len(shared)
    for f in kept:
        assert np.array_equal(now[f], case.parent[f], equal_nan=True), (f, cases.class_name("pnp", case.cls[f]))


def test_the_parent_lost_the_root_at_infinity_under_pure_translation(fixtures):
    """Every sample of the class is one on which c3 = det(F1 - F2) vanishes in the route's chart.  The parent commit's oracle
    (recorded) is short of one solution on each - F1 - F2 itself, for which it had no branch - and what it did return is returned
    still, bit for bit."""
    case = fixtures["fundamental"]
    assert len(case.parent) == 8
    ctx = OracleContext()
    for f, old in case.parent.items():
        s = int(case.set_of[f])
        assert np.isfinite(old[:, 0]).sum() == case.nref[f] - 1, f
        assert not cases.match("fundamental", case, f, old, case.sets[s][2], strict=False) <= 1.0
        ctx.set_points(_estimators.FundamentalEstimator.model_type, case.sets[s][1])
        now = np.asarray(ctx.solve_minimal(case.samples[f][None].astype(np.int32))).reshape(3, 9)
        assert all(any(np.array_equal(m, n) for n in now) for m in old if np.isfinite(m).all()), f
        assert cases.match("fundamental", case, f, now, case.sets[s][2], strict=False) <= 1.0


# ---- planted errors: each passes the oracle-to-device parity by construction and must be refused here ----------------------------------
class Planted(OracleContext):
    """the oracle context with one error in what pgx_solve_minimal answers"""

    def __init__(self, error, name):
        super().__init__()
        self.error, self.name = error, name

    def solve_minimal(self, samples, fetch=True):
        slots, P = cases.SLOTS[self.name], cases.PARAMS[self.name]
        out = np.array(super().solve_minimal(samples)).reshape(len(samples), slots, P)
        for j, m in enumerate(out):
            filled = [k for k in range(slots) if np.isfinite(m[k]).all()]
            if not filled:
                continue
            if self.error == "one entry scaled by 1 + 1e-9":
                for k in filled:
                    m[k, self.entry(m[k])] *= 1.0 + 1e-9
            if self.error == "the last filled slot dropped":
                m[filled[-1]] = np.nan
            if self.error == "two slots merged" and len(filled) >= 2:
                m[filled[1]] = m[filled[0]]
            if self.error == "rank 2 broken by 1e-9":
                for k in filled:
                    U, sv, Vt = np.linalg.svd(m[k].reshape(3, 3))
                    G = (U * [sv[0], sv[1], 1e-9 * sv[0]]) @ Vt
                    m[k] = (G / np.linalg.norm(G)).reshape(-1)
            if self.error == "translation from the wrong sample point":
                X0, X1 = self.pts[samples[j][0], 2:], self.pts[samples[j][1], 2:]
                for k in filled:
                    Q = m[k].reshape(3, 4)
                    Q[:, 3] += Q[:, :3] @ (X0 - X1)                # t = Y0 - R X1
        return out.reshape(-1, P)

    def entry(self, model):
        return 0 if self.name == "homography" else int(np.argmax(np.abs(model)))        # h11: the same entry at every coordinate scale


PLANTED = [(error, name) for error, names in [
    ("one entry scaled by 1 + 1e-9", cases.TYPES),
    ("the last filled slot dropped", cases.TYPES),
    ("two slots merged", ["fundamental", "pnp"]),
    ("rank 2 broken by 1e-9", ["fundamental"]),
    ("translation from the wrong sample point", ["pnp"]),
] for name in names]


@pytest.mark.parametrize("error,name", PLANTED)
def test_a_planted_error_is_refused(fixtures, error, name):
    case = fixtures[name]
    ctx = Planted(error, name)
    ratios = cases.device_ratios(name, case, ctx, strict=False, batches=(129,))
    refused = {f for (_, _, f), v in ratios.items() if not v <= 1.0}
    every = set(range(len(case.cls)))
    none = {f for f in every if case.nref[f] == 0}
    assert not refused & none, (error, name)                       # the classes without a model have nothing to get wrong: they stay accepted
    if error == "one entry scaled by 1 + 1e-9":
        # refused wherever the planted change exceeds the tolerance - in particular on every fixture whose tolerance is below 1e-10
        # and whose scaled entry is at least 0.1 in the compared space; a type without such a fixture has nothing to show here
        must = set()
        for f in every - none:
            if case.kind[f] != ACCURACY:
                continue
            scale = case.sets[case.set_of[f]][2]
            for r in range(case.nref[f]):
                ref = case.ref[f][r]
                moved = 1e-9 * abs(ref[ctx.entry(ref)])
                if name == "fundamental":
                    must.add(f)                                    # (the norm leaves 1 by 1e-9 |entry|^2: the invariant refuses it)
                elif case.tol[f][r] < 1e-10 and moved > 2 * case.tol[f][r]:
                    must.add(f)
        assert must and must <= refused, (error, name, sorted(must - refused))
    elif error == "rank 2 broken by 1e-9":
        # refused wherever the det bound is below the break (1e-9 s1^2 s2 >= 1e-10 at unit norm).  Where the route takes c3 for zero
        # the returned F1 - F2 has det = c3 as the elimination left it, the bound says so (1e-11 .. 3e-9) and the break hides in it
        must = {f for f in every - none if 32 * cases.EPS * np.nanmax(case.detk[f]) < 1e-11}
        assert len(must) >= len(every - none) - 8 and must <= refused, (error, name, sorted(must - refused))
    elif error == "two slots merged":
        assert refused == {f for f in every if case.nref[f] >= 2}, (error, name)
    else:
        assert refused == every - none, (error, name, sorted((every - none) - refused))


# ---- the fixture file is what the generator writes (needs mpmath: the one check that may skip) -----------------------------------------
def test_the_generator_reproduces_the_fixture_file():
    pytest.importorskip("mpmath")
    spec = importlib.util.spec_from_file_location("make_golden_minimal", os.path.join(os.path.dirname(cases.FILE), "make_golden_minimal.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    z = np.load(cases.FILE)
    # every array of the file, bit for bit, from the draws the file records (the draws before them failed a condition of their class)
    data = gen.generate(verbose=False, draws={name: z[cases.KEY[name] + "_draw"] for name in cases.TYPES}, parent=z["p3p_parent_models"],
                        parent_f7=z["f7_parent_models"])
    assert set(data) == set(z.files)
    for key in z.files:
        assert data[key].dtype == z[key].dtype and np.array_equal(data[key], z[key], equal_nan=True), key
