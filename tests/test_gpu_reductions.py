"""The Gram and residual-sum reduction passes against the bits an MI355X produced before they were stated once
(tests/golden/kat_reductions_v1.npz, recorded by tests/golden/make_golden_reductions.py; the cases and why these sizes are in
tests/reduction_cases.py).

pgx_gram / pgx_gram_labels and pgx_residual_sum / pgx_residual_sums are one kernel each, so the tests that compare the single-label
call with the all-labels call (tests/test_gpu_switches.py) compare a kernel with itself.  This pin is the independent side: the
single-label, the all-labels, the index-list, the one-wave-per-selection and the Gauss-Newton forms as the separate kernels of the
recorded commit computed them.  Every tree is fixed (lanes by shuffle, waves in order, blocks in a fixed stride), so every output is
reproducible bit for bit: floats are compared as uint64 (a NaN must be the same NaN), counters as integers."""
import os

import numpy as np
import pytest

import reduction_cases

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kat_reductions_v1.npz")


def _first_difference(calls, got_f, ref_f, got_i, ref_i):
    f = i = 0
    for call, nf, ni in calls:
        if got_f[f:f + nf].tobytes() != ref_f[f:f + nf].tobytes() or not np.array_equal(got_i[i:i + ni], ref_i[i:i + ni]):
            return call
        f, i = f + nf, i + ni
    return None


def test_reduction_passes_are_bitwise_the_recorded_ones(gpu_ctx):
    kat = np.load(GOLDEN)
    floats, ints, calls, digest = reduction_cases.run(gpu_ctx)
    assert digest == str(kat["inputs_sha256"]), "the generated inputs moved (numpy's generator stream?): the pin compares nothing"
    assert {f"f_{g}" for g in floats} | {f"i_{g}" for g in ints} == set(kat.files) - {"inputs_sha256", "recorded_at_commit"}
    for g in floats:
        ref_f, ref_i = kat[f"f_{g}"], kat[f"i_{g}"]
        assert floats[g].shape == ref_f.shape and ints[g].shape == ref_i.shape, g
        same = np.array_equal(floats[g].view(np.uint64), ref_f.view(np.uint64)) and np.array_equal(ints[g], ref_i)
        assert same, f"{g}: first differing call {_first_difference(calls[g], floats[g], ref_f, ints[g], ref_i)}"
