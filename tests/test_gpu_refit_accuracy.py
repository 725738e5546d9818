"""The non-minimal refits on the device against the 50-digit fits of tests/golden/kat_refits_v1.npz: the comparisons of
tests/test_refit_accuracy_cpu.py (tests/refit_accuracy_cases.py: fixtures, tolerances, entry points) on the libpgx context, one test
per type.  The paths: pgx_gram with index and label selections (nonminimal), pgx_gram_labels (nonminimal_labels), pgx_gram_batch
(nonminimal_batch; for the pose the single step of _fit_many), pgx_eigh_smallest_batch (refit_solver = "jacobi", next to LAPACK on
the device's Gram matrices) and pgx_pnp_refine_batch at iterations 1 and 10, with and without weights_sel.  No case is left out and
none skips.  Each test prints its type's worst error / tolerance (docs/lab-notebook.md, "Refit accuracy")."""
import pytest

import refit_accuracy_cases as cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fixtures():
    return cases.load()


@pytest.mark.parametrize("name", [t for t in cases.TYPES if t != "pnp"])
def test_device_eigen_refits_are_within_the_derived_tolerance_of_the_50_digit_fit(gpu_ctx, fixtures, name):
    for solver in ("lapack", "jacobi"):
        ratios = cases.eigen_ratios(name, fixtures[name], gpu_ctx, solver)
        print(cases.report(name, f"gpu/{solver}", ratios))
        assert len({(s, wt) for _, s, wt in ratios}) == len(fixtures[name].fixtures)      # no case left out
        entries = {e for e, _, _ in ratios}
        assert entries == {"nonminimal/label", "nonminimal/index", "nonminimal_labels", "nonminimal_batch", "nonminimal_batch/reversed"}
        bad = {k: v for k, v in ratios.items() if not v <= 1.0}
        assert not bad, bad


def test_device_pose_refits_take_the_reference_step_and_end_where_its_step_vanishes(gpu_ctx, fixtures):
    case = fixtures["pnp"]
    ratios = cases.pose_ratios(case, gpu_ctx)
    print(cases.report("pnp", "gpu", ratios))
    every = {(s, wt) for s, wt, _ in case.fixtures}
    by_label = {(s, wt) for s, wt in every if case.sels[s][0] is None}
    assert {wt for _, wt in every} == {0, 1, 2}                       # weights_sel off and on
    # iterations = 1 (step/) and 10 (run/) at every size, no case and no entry point left out
    want = {"step/pnp_refine_batch": every, "step/_fit_many": every, "run/nonminimal_batch": every, "run/nonminimal_batch/reversed": every,
            "run/nonminimal/index": every - by_label, "run/nonminimal/label": by_label, "run/nonminimal_labels": by_label}
    assert {e: {(s, wt) for e2, s, wt in ratios if e2 == e} for e in {e for e, _, _ in ratios}} == want
    bad = {k: v for k, v in ratios.items() if not v <= 1.0}
    assert not bad, bad
