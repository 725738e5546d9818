"""The f32 filters of the axial types decide what they decided: tests/golden/kat_axial_filters_v1.npz, recorded on an MI355X with the
library of the commit before Filter32 of the 3-D line, the cylinder, the cone and the torus were written as one (AxialFilter32,
csrc/score_filters.hip.h), replayed on the library as built - the keep words of the cull kernel (group_reject) bit for bit, and the
surviving steps, the exact evaluations (reject) and the inlier pairs as numbers.  The scene, the batches and what a launch records:
tests/axial_filter_cases.py.  The points and the hypotheses are the file's, not regenerated."""
import numpy as np
import pytest

import axial_filter_cases as A
from pyprogressivex import _lib

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    with np.load(A.FILE) as f:
        return {k: f[k] for k in f.files}


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)                                       # its own: the normal tolerance is context state
    yield c
    c.close()


@pytest.mark.parametrize("mt", A.TYPES)
def test_axial_filter_decides_as_recorded(ctx, golden, mt):
    pts, nrm, models = golden["pts"], golden["nrm"], golden[f"models_{mt}"]
    assert golden["T2"][0] == A.T2 and golden["kappa"][0] == A.KAPPA and list(golden["types"]) == list(A.TYPES)
    assert pts.shape == (A.N, 3) and A.N % 64 != 0 and models.shape == (A.M, _lib.PARAM_DIM[mt])
    path, filt, counters, keep = A.run_on(ctx, mt, pts, nrm, models)
    assert path == "cull + group-major" and filt == "f32"
    want = golden[f"keep_{mt}"]
    assert keep.shape == want.shape == ((A.N + 63) // 64, A.MPAD // 64)
    print("counters (recorded, now):", dict(zip(A.COUNTERS, zip(golden[f"counters_{mt}"].tolist(), counters.tolist()))))
    assert np.array_equal(keep, want), ("keep words (group, word)", np.argwhere(keep != want)[:8])
    assert np.array_equal(counters, golden[f"counters_{mt}"])
    assert A.popcount(keep) == counters[0] and not keep[:, 3:].any() and not (keep[:, 2] >> np.uint64(A.M - 128)).any()
    culled, kept = A.SPECIAL[mt]
    for back in culled:                                       # a NaN entry, a NaN class
        assert not A.column(keep, A.M - back).any(), back
    for back in kept:                                         # d = 0, a radius of 1e18, |c| + |s| = 2^-11, an unknown class
        assert A.column(keep, A.M - back).all(), back
