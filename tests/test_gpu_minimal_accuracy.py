"""The iterative minimal solvers on the device against the 50-digit solution sets of tests/golden/kat_minimal_v1.npz: the comparisons
of tests/test_minimal_accuracy_cpu.py (tests/minimal_accuracy_cases.py: fixtures, kinds, tolerances, the set comparison) on the
libpgx context, one test per type - solve_h4_kernel, solve_f7_kernel and solve_p3p_kernel at S = 1, 63, 64, 65 and 129 samples (one
lane per sample in blocks of 64; perm filled by a grid-stride loop over the padded slots: both edges crossed), on every point set
of the type.  No case is left out and none skips.  Each test prints its type's worst error / tolerance per class
(docs/lab-notebook.md, "Minimal-solver accuracy")."""
import numpy as np
import pytest

import minimal_accuracy_cases as cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fixtures():
    return cases.load()


@pytest.mark.parametrize("name", cases.TYPES)
def test_device_solve_minimal_returns_the_reference_solution_set(gpu_ctx, fixtures, name):
    case = fixtures[name]
    ratios = cases.device_ratios(name, case, gpu_ctx, strict=False)
    print(cases.report(name, "gpu", case, ratios))
    for s, (sname, _, _) in enumerate(case.sets):
        for S in cases.BATCHES:
            assert {f for (sn, S2, f) in ratios if sn == sname and S2 == S} == set(cases.batch_of(case, s, S)[0].tolist())
        assert {f for (sn, _, f) in ratios if sn == sname} == set(np.flatnonzero(case.set_of == s).tolist())      # no fixture left out
    # ("two poses share v" has the two tests below)
    bad = {k: v for k, v in ratios.items() if not v <= 1.0 and not (name == "pnp" and case.cls[k[2]] == cases.SHARED_V)}
    assert not bad, bad


def _shared_v_ratios(gpu_ctx, case, coverage_tol):
    ratios = cases.device_ratios("pnp", case, gpu_ctx, strict=False, coverage_tol=coverage_tol)
    return {k: v for k, v in ratios.items() if case.cls[k[2]] == cases.SHARED_V}


def test_device_p3p_returns_every_pose_where_two_poses_share_v(gpu_ctx, fixtures):
    ratios = _shared_v_ratios(gpu_ctx, fixtures["pnp"], cases.IDENTIFIED)
    assert {k[2] for k in ratios} == set(np.flatnonzero(fixtures["pnp"].cls == cases.SHARED_V).tolist())
    bad = {k: v for k, v in ratios.items() if not v <= 1.0}
    assert not bad, bad


@pytest.mark.xfail(strict=True, reason="open defect (DESIGN.md 4.5b; tests/test_minimal_accuracy_cpu.py says the same of the oracle): where two "
                   "poses share v the device's poses are within 1e-6 of the 50-digit ones on 10 of the 16 samples only, the worst 3.4e-6 off")
def test_device_p3p_is_within_the_consistency_figure_where_two_poses_share_v(gpu_ctx, fixtures):
    ratios = _shared_v_ratios(gpu_ctx, fixtures["pnp"], None)
    bad = {k: v for k, v in ratios.items() if not v <= 1.0}
    assert not bad, bad


def test_device_p3p_keeps_the_bits_of_every_sample_the_parent_had_complete(gpu_ctx, fixtures):
    from pyprogressivex import _estimators
    case = fixtures["pnp"]
    gpu_ctx.set_points(_estimators.PnPEstimator.model_type, case.sets[0][1])
    now = np.asarray(gpu_ctx.solve_minimal(np.ascontiguousarray(case.samples, dtype=np.int32))).reshape(-1, 4, 12)
    kept = [f for f in range(len(case.cls)) if cases.match("pnp", case, f, case.parent[f], 1.0, strict=False) <= 1.0]
    assert len(kept) >= len(case.cls) - int((case.cls == cases.SHARED_V).sum())
    for f in kept:
        assert np.array_equal(now[f], case.parent[f], equal_nan=True), (f, cases.class_name("pnp", case.cls[f]))
