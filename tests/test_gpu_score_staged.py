"""The group-major scoring kernel on pose batches small enough to reach every branch of its staging and of its two exact paths
(csrc/score.hip: HypRow, drain(), direct(); csrc/score_runs.h): hypothesis rows staged as the prefix reject() reads, the queued
path's packed segmented reduction, the in-place path with and without anything shared with the compound instance.

Sizes: n = 197 is four 64-point groups with a 5-point tail group inside a partial super-group, n = 577 two super-groups and a
1-point tail group; two objects, so a ground-truth pose has most of a group as candidates (the in-place path at the default
dense_min = 32).  M = 1, 65, 130: one word, a word boundary, padding inside Mpad = 256.  The batch holds the ground truth,
perturbed copies, a hypothesis with a NaN entry, one scaled by 1e-24, one by 1e80 (outside the band of scales: never rejected)
and one whose camera plane cuts through the object (pz ~ 0: the trust test of the f32 filter fails for those pairs).

Held: counts, masks, values and shared against the oracle (the comparisons of tests/test_gpu_parity.py); the integer accumulators
bitwise equal over split x dense_min x group_xcd (all in place, mixed, all queued); PGX_VERIFY=1 finds no inlier that the bound or
the filter removed."""
import functools
import itertools
import os

import numpy as np
import pytest

from pyprogressivex import _lib, datasets

pytestmark = pytest.mark.gpu

REL = 1e-9
SIZES = {197: (80, 37), 577: (240, 97)}          # n: (points per object, outliers)
GEOMETRIES = [dict(split=s, dense_min=d, group_xcd=x) for s, d, x in itertools.product((1, 2, 5), (1, 32, 65), (0, 1))]
DEFAULT_GEOMETRY = dict(split=0, dense_min=32, group_xcd=-1)


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.max(np.abs(a - b) / np.maximum(1e-300, np.maximum(np.abs(a), np.abs(b)))) if a.size else 0.0


@functools.lru_cache(maxsize=None)
def problem(n, M):
    per, outl = SIZES[n]
    x1, x2, K, _, gt = datasets.make_poses(n_per_object=per, n_objects=2, n_outliers=outl, seed=n)
    pts, f = datasets.normalize_pnp(x1, x2, K)
    assert pts.shape[0] == n
    thr = 4.0 / f
    hyps = datasets.make_pose_hypotheses(gt, M=max(M, 8), max_angle_deg=2.0, max_shift_mm=5.0, seed=n + M)[:M].copy()
    if M > 8:
        hyps[3] = gt[0]
        hyps[3, 5] = np.nan                      # a NaN entry: every residual is NaN, never an inlier
        hyps[4] = gt[1] * 1e-24                  # the same pose at a scale where f32 squares underflow
        hyps[5] = gt[0] * 1e80                   # outside the band of scales: c0 = inf, only the exact path decides
        hyps[6] = gt[0]
        hyps[6, 11] = 0.0                        # the camera plane through the object's centre: pz = r3 . X, around 0
        hyps[M - 1] = gt[1] * 1e-24              # inliers in the last, partly filled word
    for a in (pts, hyps):
        a.setflags(write=False)
    return pts, hyps, 2.25 * thr * thr, gt


@functools.lru_cache(maxsize=None)
def reference(n, M, compound):
    import pgx_oracle as O
    pts, hyps, T2, gt = problem(n, M)
    comp = O.preference(O.PNP, pts, gt[0], T2) if compound else None     # the compound instance: object 0's preference vector
    with np.errstate(all="ignore"):
        ref = O.score(O.PNP, pts, hyps, T2, compound=comp, has_compound=compound, exponent=2, want_masks=True)
    for a in ref.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return comp, ref


@pytest.fixture(scope="module")
def verify_ctx():
    """a context created with PGX_VERIFY=1: its pgx_score_stats also re-decides every pair with the exact residual"""
    saved = os.environ.get("PGX_VERIFY")
    os.environ["PGX_VERIFY"] = "1"
    try:
        ctx = _lib.Context(0)
    finally:
        if saved is None:
            os.environ.pop("PGX_VERIFY", None)
        else:
            os.environ["PGX_VERIFY"] = saved
    yield ctx
    ctx.close()


@pytest.mark.parametrize("compound", [False, True], ids=["plain", "compound"])
@pytest.mark.parametrize("M", [1, 65, 130])
@pytest.mark.parametrize("n", list(SIZES))
def test_staged_rows_and_both_exact_paths(gpu_ctx, verify_ctx, oracle, n, M, compound):
    pts, hyps, T2, _ = problem(n, M)
    comp, ref = reference(n, M, compound)
    try:
        gpu_ctx.score_debug_geometry(**DEFAULT_GEOMETRY)
        gpu_ctx.set_points(_lib.PNP, pts)
        gpu_ctx.set_compound(comp)
        # ---- against the oracle: the mask-producing variant (every step in place) ...
        got = gpu_ctx.score(hyps, T2, has_compound=compound, exponent=2, want_masks=True)
        assert np.array_equal(got["counts"], ref["counts"]), "inlier counts differ"
        assert np.array_equal(got["masks"], ref["masks"]), "inlier masks differ"
        assert _rel(got["values"], ref["values"]) <= REL and _rel(got["shared"], ref["shared"]) <= REL
        if M > 8:
            assert got["counts"][3] == 0 and got["counts"][4] == got["counts"][M - 1] > 32 and got["counts"][5] > 32
        # ... and the queued variant at the default geometry: the same per-pair integers, bitwise the same sums
        again = gpu_ctx.score(hyps, T2, has_compound=compound, exponent=2)
        for k in ("counts", "values", "shared"):
            assert np.array_equal(again[k], got[k]), k
        base = gpu_ctx.score_accumulators()
        assert np.array_equal(base["counts"].astype(np.int64), ref["counts"])
        if not compound:
            assert not base["shared_q"].any()
        # ---- the integer accumulators do not depend on the launch geometry: all in place, mixed, all queued
        for geo in GEOMETRIES:
            gpu_ctx.score_debug_geometry(**geo)
            gpu_ctx.score(hyps, T2, has_compound=compound, exponent=2)
            acc = gpu_ctx.score_accumulators()
            for k in base:
                assert np.array_equal(acc[k], base[k]), (geo, k)
    finally:
        gpu_ctx.score_debug_geometry(**DEFAULT_GEOMETRY)
    # ---- every decision of the bound and of the staged filter against the exact residual
    verify_ctx.set_points(_lib.PNP, pts)
    verify_ctx.set_compound(comp)
    verify_ctx.score_upload(hyps)
    st = verify_ctx.score_stats(T2, has_compound=compound)
    assert st["path"] == "cull + group-major" and st["filter"] == "f32"
    assert st["contradictions"] == 0, st
    assert st["inlier_pairs"] == int(ref["counts"].sum())
