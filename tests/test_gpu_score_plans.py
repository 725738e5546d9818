"""The same launch decides the same and produces the same bits: tests/golden/score_plans_v1.json, recorded on an MI355X before the
launch decisions of pgx_score went into csrc/score_plan.h, replayed on the library as built (cases and recorded fields:
tests/score_plan_cases.py) - and the one rule the batch's owner added: results are handed out only for the batch they were computed
from (include/pgx.h, "Results belong to a batch")."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import score_plan_cases
from helpers import make_case

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "score_plans_v1.json")) as f:
    GOLDEN = json.load(f)


def test_the_recording_covers_every_case_and_dropped_nothing_it_must_keep():
    assert sorted(GOLDEN["cases"]) == sorted(score_plan_cases.cases())
    for entry in GOLDEN["header"]["dropped"]:
        assert not score_plan_cases.must_keep(entry.rsplit(":", 1)[1]), entry
    for case in GOLDEN["cases"].values():
        assert {"path", "filter", "counts", "values", "shared"} <= set(case)
    for name, _ in score_plan_cases.WINDOWS:      # the window flips the path between 2 and 1
        assert GOLDEN["cases"][f"window-{name}-inside"]["path"] == "cull + group-major"
        assert GOLDEN["cases"][f"window-{name}-outside"]["path"] == "every pair"
    for case_id, twin in score_plan_cases.GEOMETRY_TWINS.items():      # the launch geometry does not show in the results
        a, b = GOLDEN["cases"][case_id], GOLDEN["cases"][twin]
        assert a["path"] == b["path"] == "cull + group-major"
        for k in score_plan_cases.DIGESTS:
            assert a[k] == b[k], (case_id, k)


@pytest.mark.gpu
@pytest.mark.parametrize("case_id", list(score_plan_cases.cases()))
def test_score_plan_replays(gpu_ctx, case_id):
    want = GOLDEN["cases"][case_id]
    got = score_plan_cases.run_on(gpu_ctx, case_id)
    assert set(want) <= set(got)
    differ = {k: (want[k], got[k]) for k in want if want[k] != got[k]}
    assert not differ, f"{case_id}: (recorded, now) {differ}"


def _same(got, ref, masks=False):
    assert np.array_equal(got["counts"], ref["counts"])
    assert np.allclose(got["values"], ref["values"], rtol=1e-9, atol=0) and np.allclose(got["shared"], ref["shared"], rtol=1e-9, atol=0)
    if masks:
        assert np.array_equal(got["masks"], ref["masks"])


@pytest.mark.gpu
def test_results_are_handed_out_only_for_the_batch_they_were_computed_from(gpu_ctx, oracle):
    from pyprogressivex import _lib
    from pyprogressivex._proposal import mask_to_indices
    mt, pts, models, thr = make_case("homography", 513, 257, seed=21)
    T2 = 2.25 * thr * thr
    gpu_ctx.set_points(mt, pts)
    gpu_ctx.set_compound(None)
    # launch (M = 65) -> upload (M = 257): the table on the device is the 65-row one, the order and M are the new batch's
    gpu_ctx.score_upload(models[:65])
    gpu_ctx.score_launch(T2)
    gpu_ctx.score_upload(models)
    with pytest.raises(_lib.PgxError, match="changed since the last launch"):
        gpu_ctx.score_fetch()
    gpu_ctx.score_launch(T2)
    _same(gpu_ctx.score_fetch(), oracle.score(mt, pts, models, T2))
    # masks launch -> one-sample solve_minimal: the mask rows are the old batch's, the row count the new one's
    got = gpu_ctx.score(models[:65], T2, want_masks=True)
    ref65 = oracle.score(mt, pts, models[:65], T2, want_masks=True)
    _same(got, ref65, masks=True)
    assert np.array_equal(gpu_ctx.score_inliers(64), mask_to_indices(ref65["masks"][64], 513))
    gpu_ctx.solve_minimal(np.array([[0, 1, 2, 3]], np.int32))
    with pytest.raises(_lib.PgxError, match="changed since the last launch"):
        gpu_ctx.score_inliers(0)
    with pytest.raises(_lib.PgxError, match="changed since the last launch"):
        gpu_ctx.score_fetch()
    # a refused upload (M = 0) changes nothing: the previous launch stays fetchable
    gpu_ctx.score_upload(models)
    gpu_ctx.score_launch(T2, want_masks=True)
    with pytest.raises(_lib.PgxError, match="empty hypothesis batch"):
        gpu_ctx._ck(gpu_ctx._lib.pgx_score_upload(gpu_ctx._h, models.ctypes.data_as(C.POINTER(C.c_double)), C.c_int(0)), "pgx_score_upload")
    _same(gpu_ctx.score_fetch(want_masks=True), oracle.score(mt, pts, models, T2, want_masks=True), masks=True)
    assert len(gpu_ctx.score_inliers(256)) == int(oracle.score(mt, pts, models, T2)["counts"][256])
