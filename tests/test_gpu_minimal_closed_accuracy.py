"""The nine closed-form minimal solvers on the device against the 50-digit solution sets of tests/golden/kat_minimal_closed_v1.npz:
the comparisons of tests/test_minimal_closed_accuracy_cpu.py (tests/minimal_closed_cases.py: fixtures, kinds, tolerances, checks; the
set comparison is minimal_accuracy_cases.match) on the libpgx context, one test per type - solve_kernel<MT>, one lane per model row
in blocks of 256, at S = 1, 255, 256 and 257 samples and for the torus (two rows per sample) also 127, 128 and 129: both sides of
the block's edge in rows = slots x S - on every point set of the type, with the set's normals and radius ranges resident and the
ranges put back afterwards.  No fixture is left out and none skips.  Each test prints its type's worst error / tolerance per
class (docs/lab-notebook.md, "Minimal-solver accuracy")."""
import numpy as np
import pytest

import minimal_accuracy_cases as cases
import minimal_closed_cases as closed

pytestmark = pytest.mark.gpu
CUBES = "tiny differences, cubes underflow"
OPEN = {("circle", CUBES), ("torus", CUBES)}          # the strict xfail below (tests/test_minimal_closed_accuracy_cpu.py says the same of the estimators)


@pytest.fixture(scope="module")
def fixtures():
    return closed.load()


@pytest.mark.parametrize("name", closed.TYPES)
def test_device_solve_minimal_returns_the_reference_solution_set(gpu_ctx, fixtures, name):
    case = fixtures[name]
    ratios = closed.device_ratios(name, case, gpu_ctx, strict=False)
    print(cases.report(name, "gpu", case, ratios))
    for s, (sname, _, _) in enumerate(case.sets):
        for S in closed.BATCHES[name]:
            assert {f for (sn, S2, f) in ratios if sn == sname and S2 == S} == set(cases.batch_of(case, s, S)[0].tolist())
        assert {f for (sn, _, f) in ratios if sn == sname} == set(np.flatnonzero(case.set_of == s).tolist())      # no fixture left out
    bad = {k: v for k, v in ratios.items() if not v <= 1.0 and (name, cases.class_name(name, case.cls[k[2]])) not in OPEN}
    assert not bad, bad


@pytest.mark.parametrize("name", sorted(n for n, _ in OPEN))
@pytest.mark.xfail(strict=True, reason="open defect (DESIGN.md 4.5b): with coordinate differences of 2^-404 the products of three differences "
                   "underflow and the circle and the torus return finite rows that are no solution")
def test_device_rows_are_empty_or_solutions_where_cubes_underflow(gpu_ctx, fixtures, name):
    case = fixtures[name]
    ratios = closed.device_ratios(name, case, gpu_ctx, strict=False, batches=(257,))
    mine = {k: v for k, v in ratios.items() if cases.class_name(name, case.cls[k[2]]) == CUBES}
    assert mine and not {k: v for k, v in mine.items() if not v <= 1.0}
