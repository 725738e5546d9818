"""The group-major kernel's way into its step loop and its filter step (csrc/score.hip, PGX_SCORE_TRIM bits 8 - 64): the counts of a
listed workgroup in one round trip and the (class, position) by selects, the item's keep words as one load, the filter run in every
lane with the tail group's lanes beyond n masked out of the ballot.  None of it may show: every case runs with the lists off, the
plan's own choice and forced on (the modes of tests/test_gpu_score_worklist.py) and must give the same bits in all three, and those
are the oracle's - counts, the integer accumulators (helpers.fixed_point_accumulators), values and shared as those integers over 2^q.

n: 1 one lane | 63, 64, 65 either side of one group | 104 a tail group of 40 lanes | 513 one super-group + 1.
M: 64 one word | 65 the reorder begins | 257, 321 two items per group, the second with empty words behind M.

The tail lanes hold a copy of the LAST point of the device's order, which a test cannot choose (the points are Morton-sorted on the
device).  So the tail-lane scenes are made of inliers only: every point is an inlier of hypothesis 0 (asserted on the CPU with the
oracle before the GPU is touched), hence so is the last one in any order, and an unmasked copy of it raises hypothesis 0's count.  At
n = 104 the tail group's 40 points are all candidates of hypothesis 0: a dense step (>= 32), evaluated in place - unmasked it would
count 64; at n = 65 the tail group's single point is queued - unmasked the step would be dense and count 64."""
import functools
import os

import numpy as np
import pytest

from helpers import fixed_point_accumulators, make_case
from pyprogressivex import _lib, parallel

pytestmark = pytest.mark.gpu

REL = 1e-9
NS = (1, 63, 64, 65, 104, 513)
MS = (64, 65, 257, 321)
MODES = {"off": dict(worklist=0, group_xcd=-1), "auto": dict(worklist=-1, group_xcd=-1), "forced": dict(worklist=1, group_xcd=1)}
RESET = dict(worklist=-1, group_xcd=-1)
COUNTERS = ("surviving_group_steps", "exact_evaluations", "inlier_pairs")
ACCS = ("counts", "values_q", "shared_q")


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.max(np.abs(a - b) / np.maximum(1e-300, np.maximum(np.abs(a), np.abs(b)))) if a.size else 0.0


def _missing(models):
    """as tests/test_gpu_score_worklist.py: the poses shifted sideways by four times their depth - no point is near any of them"""
    out = models.copy().reshape(-1, 3, 4)
    out[:, 0, 3] += 4.0 * np.abs(out[:, 2, 3])
    return np.ascontiguousarray(out.reshape(-1, 12))


def _references(O, mt, pts, models, T2, comp):
    refs = {}
    with np.errstate(all="ignore"):
        for compound in (False, True):
            r = O.score(O.PNP, pts, models, T2, compound=comp if compound else None, has_compound=compound, exponent=2)
            r["acc"] = fixed_point_accumulators(O, mt, pts, models, T2, comp=comp if compound else None)
            assert np.array_equal(r["acc"]["counts"], r["counts"])
            refs[compound] = r
    return refs


@functools.lru_cache(maxsize=None)
def problem(n, M, kind="grid"):
    """(model type, points, models, T2, compound values, oracle references); read-only, shared by the tests that need it"""
    import pgx_oracle as O
    mt, pts, models, thr = make_case("pnp", max(n, 400) if kind != "grid" else n, max(M, 8), seed=n + M)
    T2 = 2.25 * thr * thr
    gt = models[:3].copy()
    models = models[:M].copy()
    if kind in ("tail", "odd"):
        # inliers of the first ground-truth pose only, n of them
        with np.errstate(all="ignore"):
            inl = np.flatnonzero(O.squared_residuals(O.PNP, pts, gt[0]) < 0.25 * T2)
        assert inl.size >= 40
        pts = np.ascontiguousarray(pts[np.resize(inl, n)])
    if kind == "odd":
        # a word of their own behind 64 ordinary hypotheses: a NaN entry (never an inlier), and pose 0 scaled by 1e-80 - the same
        # projective map with the same inliers, outside the filter's band, so no pair of it is ever rejected
        assert M in (65, 66)
        tail = [np.where(np.arange(12) == 5, np.nan, gt[1]), gt[0] * 1e-80]
        models[64:] = tail[:M - 64] if M == 66 else tail[-1:]
    if kind == "miss":
        models = _missing(np.resize(gt, (M, 12)))
    comp = O.preference(O.PNP, pts, gt[0], T2)
    refs = _references(O, mt, pts, models, T2, comp)
    # ---- the constructions, on the CPU
    c = refs[False]["counts"]
    if kind in ("tail", "odd"):
        assert c[0] == n                      # every point - so the last of any order - is an inlier of hypothesis 0
        assert refs[True]["shared"][0] > 0
    if kind == "odd":
        assert c[M - 1] == n and (M == 65 or c[64] == 0)
    if kind == "miss":
        assert not c.any() and not refs[True]["values"].any()
    for a in (pts, models, comp):
        a.setflags(write=False)
    return mt, pts, models, T2, comp, refs


def _launch(ctx, models, T2, comp, compound, listed):
    ctx.set_compound(comp if compound else None)
    ctx.score_upload(models)
    st = ctx.score_stats(T2, has_compound=compound)
    assert st["path"] == "cull + group-major" and st["filter"] == "f32"
    rec = {k: st[k] for k in COUNTERS}
    table = ctx.score(models, T2, has_compound=compound, exponent=2)
    for k in ("counts", "values", "shared"):
        rec[k] = table[k].copy()
    rec.update({"acc_" + k: v for k, v in ctx.score_accumulators().items()})
    if listed:
        rec["lists"] = ctx.score_worklist_counts()
    else:
        with pytest.raises(_lib.PgxError, match="work lists"):
            ctx.score_worklist_counts()
    return rec


def _same_bits(a, b, where):
    for k in a:
        if k == "lists":
            continue
        if k in COUNTERS:
            assert a[k] == b[k], (where, k, a[k], b[k])
        elif a[k].dtype.kind == "f":
            assert np.array_equal(a[k].view(np.uint64), b[k].view(np.uint64)), (where, k)
        else:
            assert np.array_equal(a[k], b[k]), (where, k)


def _is_the_oracle(rec, ref, n, compound, where):
    M = len(ref["counts"])
    assert np.array_equal(rec["counts"], ref["counts"]), (where, "inlier counts", rec["counts"][:4], ref["counts"][:4])
    for k in ACCS:
        assert np.array_equal(rec["acc_" + k][:M].astype(np.int64), ref["acc"][k]), (where, k)
    q = parallel.fixed_point_scale(n)
    for k, kq in (("values", "values_q"), ("shared", "shared_q")):       # what the finish kernel makes of the integers, bit for bit
        assert np.array_equal(rec[k].view(np.uint64), (ref["acc"][kq].astype(np.float64) / q).view(np.uint64)), (where, k)
        assert _rel(rec[k], ref[k]) <= REL, (where, k)
    assert rec["inlier_pairs"] == int(ref["counts"].sum()), where


def _three_modes(ctx, n, M, kind, compounds):
    mt, pts, models, T2, comp, refs = problem(n, M, kind)       # (CPU: the construction is asserted in here)
    try:
        ctx.set_points(mt, pts)
        out = {}
        for compound in compounds:
            recs = {}
            for mode, geo in MODES.items():
                ctx.score_debug_geometry(**geo)
                recs[mode] = _launch(ctx, models, T2, comp, compound, listed=mode == "forced" or (mode == "auto" and M > 64))
            for mode in ("auto", "forced"):
                _same_bits(recs["off"], recs[mode], (n, M, kind, compound, mode))
            _is_the_oracle(recs["off"], refs[compound], n, compound, (n, M, kind, compound))
            out[compound] = recs
        return out
    finally:
        ctx.score_debug_geometry(**RESET)


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("n", NS)
def test_every_mode_gives_the_oracles_bits(gpu_ctx, oracle, n, M):
    _three_modes(gpu_ctx, n, M, "grid", (True,))


@pytest.mark.parametrize("M", (65, 257))
@pytest.mark.parametrize("n", (65, 104))
def test_tail_lanes_hold_the_last_point_and_count_nothing(gpu_ctx, oracle, n, M):
    out = _three_modes(gpu_ctx, n, M, "tail", (False, True))
    for compound, recs in out.items():
        for mode, rec in recs.items():
            assert rec["counts"][0] == n, (compound, mode)           # (64 + 64 with an unmasked tail)


@pytest.fixture(scope="module")
def unsorted_ctx():
    """a context created with PGX_NO_SORT=1: batches keep the caller's order, so a test decides which word a hypothesis lands in"""
    saved = os.environ.get("PGX_NO_SORT")
    os.environ["PGX_NO_SORT"] = "1"
    try:
        ctx = _lib.Context(0)
    finally:
        if saved is None:
            os.environ.pop("PGX_NO_SORT", None)
        else:
            os.environ["PGX_NO_SORT"] = saved
    yield ctx
    ctx.close()


@pytest.mark.parametrize("M", (65, 66))
def test_nan_and_out_of_band_hypotheses_in_a_word_of_their_own(unsorted_ctx, oracle, M):
    """M = 65: the 1e-80 pose alone in word 1; M = 66: a NaN hypothesis and the 1e-80 pose.  The filter rejects no pair of the scaled
    pose, so in the tail group (n = 104: 40 points) all 64 lanes pass it: only the mask keeps the 24 copies of the last point out"""
    mt, pts, models, T2, comp, refs = problem(104, M, "odd")
    ctx = unsorted_ctx
    try:
        ctx.set_points(mt, pts)
        for compound in (False, True):
            recs = {}
            for mode in ("off", "forced"):          # (an unsorted batch does not take the lists by itself)
                ctx.score_debug_geometry(**MODES[mode])
                recs[mode] = _launch(ctx, models, T2, comp, compound, listed=mode == "forced")
            _same_bits(recs["off"], recs["forced"], (M, compound))
            _is_the_oracle(recs["off"], refs[compound], 104, compound, (M, compound))
            assert recs["off"]["counts"][M - 1] == 104 and (M == 65 or recs["off"]["counts"][64] == 0)
    finally:
        ctx.score_debug_geometry(**RESET)


def test_a_batch_that_misses_every_point_leaves_from_every_workgroup(gpu_ctx, oracle):
    mt, pts, models, T2, comp, refs = problem(513, 257, "miss")
    try:
        gpu_ctx.set_points(mt, pts)
        for compound in (False, True):
            for mode in ("auto", "forced"):
                gpu_ctx.score_debug_geometry(**MODES[mode])
                rec = _launch(gpu_ctx, models, T2, comp, compound, listed=True)
                assert not rec["lists"].any()                   # zero list totals: every workgroup of the grid leaves after its counts
                for k in ("counts", "values", "shared", "acc_counts", "acc_values_q", "acc_shared_q"):
                    assert not rec[k].any(), (mode, k)
                assert [rec[k] for k in COUNTERS] == [0, 0, 0]
                _is_the_oracle(rec, refs[compound], 513, compound, ("miss", mode, compound))
    finally:
        gpu_ctx.score_debug_geometry(**RESET)
