"""score_cull_kernel (csrc/score.hip, PGX_SCORE_TRIM bits 128 - 512): the keep words held in registers and stored once per tile, the
first tile's bound rows requested with the model, the segments behind the last group left early.  None of it may show.  Every case
is launched as the plan has it, with the lists forced on, with the lists off, with 1, 5 and 31 segments (multi-tile segments through
the instance without lists) and on the spread mapping; the keep words (pgx_score_debug_fetch(7)) of all of them are the same bytes, and

  - the set bits of the keep words are the surviving (hypothesis, group) steps pgx_score_stats counts;
  - the lists' counts are the (group, 4-word) items the keep words imply, per [g & 7][class];
  - counts, values, shared and the integer accumulators are the same bits in every launch, and the counts are the oracle's.

groups: 1 | 7, 8, 9 either side of a super-group | 63, 64, 65 either side of a tile | 72 a tile and one super-group | 129 a third
tile of one group; n = 64 g +- 1 for a tail group of 63 lanes and of one.  M: 1 | 65 a second word | 300 two items, the second short
| 513 a third item of one word.  With 256 segments every one of these sizes leaves most segments behind the last group.
One size past 64 x 256 groups gives the instance WITH lists a segment of two tiles."""
import functools
import os

import numpy as np
import pytest

from helpers import make_case
from pyprogressivex import _lib

pytestmark = pytest.mark.gpu

T_DEFAULT = (24, 64, 160)
GROUPS = (1, 7, 8, 9, 63, 64, 65, 72, 129)
MS = (1, 65, 300, 513)
GRID = [(64 * g, MS[(i + k) % 4]) for i, g in enumerate(GROUPS) for k in (0, 1)]
TAILS = [(64 * g + d, M) for g, M in ((8, 65), (64, 300), (129, 65)) for d in (-1, 1)]
MODES = {"plan": {}, "lists forced": dict(worklist=1, group_xcd=1), "lists off": dict(worklist=0), "1 segment": dict(cull_segs=1),
         "5 segments": dict(cull_segs=5), "31 segments": dict(cull_segs=31), "spread": dict(group_xcd=0)}
RESET = dict(worklist=-1, group_xcd=-1, cull_segs=256)
COUNTERS = ("surviving_group_steps", "exact_evaluations", "inlier_pairs")


def _missing(models):
    """as tests/test_gpu_score_worklist.py: the poses shifted sideways by four times their depth - they look away from every point"""
    out = models.copy().reshape(-1, 3, 4)
    out[:, 0, 3] += 4.0 * np.abs(out[:, 2, 3])
    return np.ascontiguousarray(out.reshape(-1, 12))


@functools.lru_cache(maxsize=None)
def problem(n, M, kind="grid"):
    """(model type, points, models, T2, the oracle's counts or None); read-only, shared by the tests that need it"""
    import pgx_oracle as O
    mt, pts, models, thr = make_case("pnp", n, max(M, 8), seed=n + M)
    gt = models[:3].copy()
    models = models[:M].copy()
    T2 = 2.25 * thr * thr
    if kind == "miss":
        models = _missing(np.resize(gt, (M, 12)))
    elif kind == "odd":      # a word of their own behind 64 ordinary hypotheses: a NaN entry, and pose 0 scaled out of the filter's band
        assert M == 66
        models[64] = np.where(np.arange(12) == 5, np.nan, gt[1])
        models[65] = gt[0] * 1e-80
    elif kind == "tiny":     # T / 8: still inside the f32 filter's range (score_plan.h), nearly every group culled
        T2 /= 64.0
    elif kind == "wide":     # 1000 T, several image widths: the bound of a pose that looks at the scene reaches every group
        T2 *= 1e6
    counts = None
    if kind != "large":
        with np.errstate(all="ignore"):
            counts = O.score(O.PNP, pts, models, T2, compound=None, has_compound=False, exponent=2)["counts"]
        if kind == "miss":
            assert not counts.any()
        if kind == "odd":
            assert counts[64] == 0 and counts[65] == counts[0] > 0
        counts.setflags(write=False)
    for a in (pts, models):
        a.setflags(write=False)
    return mt, pts, models, T2, counts


def _popcount(a):
    return np.unpackbits(np.ascontiguousarray(a).view(np.uint8)).reshape(a.shape + (64,)).sum(axis=-1, dtype=np.int64)


def _expected_lists(keep, t=T_DEFAULT):
    """[g & 7][class] from the keep words: an item is a group x 4 adjacent words, its weight the set bits in them"""
    groups, W = keep.shape
    weight = _popcount(keep).reshape(groups, W // 4, 4).sum(axis=2)      # (W = Mpad / 64 is a multiple of 4)
    cls = (weight >= t[0]).astype(int) + (weight >= t[1]) + (weight >= t[2])
    want = np.zeros((8, 4), np.int64)
    for g, x in zip(*np.nonzero(weight)):
        want[g & 7, cls[g, x]] += 1
    return want


def _lists_or_none(ctx):
    try:
        return ctx.score_worklist_counts()
    except _lib.PgxError as e:
        assert "work lists" in str(e)
        return None


def _launch(ctx, models, T2, Mpad):
    ctx.set_compound(None)
    ctx.score_upload(models)
    st = ctx.score_stats(T2)
    assert st["path"] == "cull + group-major" and st["filter"] == "f32"
    rec = {k: st[k] for k in COUNTERS}
    rec["keep"] = ctx.score_keep_words(Mpad)
    rec["lists"] = _lists_or_none(ctx)
    table = ctx.score(models, T2, exponent=2)
    for k in ("counts", "values", "shared"):
        rec[k] = table[k].copy()
    rec.update({"acc_" + k: v for k, v in ctx.score_accumulators().items()})
    assert np.array_equal(ctx.score_keep_words(Mpad), rec["keep"]), "the timed launch's keep words are the counters launch's"
    lists = _lists_or_none(ctx)
    assert (lists is None) == (rec["lists"] is None) and (lists is None or np.array_equal(lists, rec["lists"]))
    return rec


def _every_launch_the_same(ctx, n, M, kind, modes=MODES, sorted_batch=True):
    mt, pts, models, T2, counts = problem(n, M, kind)
    Mpad = (M + 255) // 256 * 256
    try:
        ctx.set_points(mt, pts)
        recs = {}
        for mode, geo in modes.items():
            ctx.score_debug_geometry(**RESET)
            ctx.score_debug_geometry(**geo)
            recs[mode] = _launch(ctx, models, T2, Mpad)
    finally:
        ctx.score_debug_geometry(**RESET)
    base = recs["plan"]
    keep = base["keep"]
    assert keep.shape == ((n + 63) // 64, Mpad // 64)
    assert int(_popcount(keep).sum()) == base["surviving_group_steps"], (n, M, kind)
    assert not keep[:, (M + 63) // 64:].any(), "words behind M"
    if M % 64:
        assert not (keep[:, M // 64] >> np.uint64(M % 64)).any(), "bits behind M"
    for mode, rec in recs.items():
        where = (n, M, kind, mode)
        assert np.array_equal(rec["keep"], keep), (where, "keep words", np.argwhere(rec["keep"] != keep)[:4])
        for k in COUNTERS:
            assert rec[k] == base[k], (where, k, rec[k], base[k])
        for k in ("counts", "acc_counts", "acc_values_q", "acc_shared_q"):
            assert np.array_equal(rec[k], base[k]), (where, k)
        for k in ("values", "shared"):
            assert np.array_equal(rec[k].view(np.uint64), base[k].view(np.uint64)), (where, k)
        if rec["lists"] is not None:
            assert np.array_equal(rec["lists"], _expected_lists(keep)), (where, rec["lists"])
    assert recs["lists forced"]["lists"] is not None
    assert (base["lists"] is not None) == (sorted_batch and M > 64)       # what plan_score decides (a batch in locality order)
    for mode in modes:
        if mode not in ("plan", "lists forced"):
            assert recs[mode]["lists"] is None, mode
    if counts is not None:
        assert np.array_equal(base["counts"], counts), (n, M, kind, "the oracle's counts")
    return recs


@pytest.mark.parametrize("n,M", GRID + TAILS)
def test_keep_words_do_not_depend_on_the_launch(gpu_ctx, oracle, n, M):
    _every_launch_the_same(gpu_ctx, n, M, "grid")


def test_a_batch_every_group_culls(gpu_ctx, oracle):
    recs = _every_launch_the_same(gpu_ctx, 64 * 72 + 1, 300, "miss")
    assert not recs["plan"]["keep"].any() and not recs["lists forced"]["lists"].any()


def test_a_tiny_threshold(gpu_ctx, oracle):
    _every_launch_the_same(gpu_ctx, 64 * 65, 300, "tiny")


def test_nearly_every_group_survives(gpu_ctx, oracle):
    n, M = 64 * 65 - 1, 300
    recs = _every_launch_the_same(gpu_ctx, n, M, "wide")
    # three in four of make_case's hypotheses are the scene's poses, exact or perturbed (the fourth is a random matrix): each of those
    # projects every point within a few image widths of its observation, so none of its 65 groups can be culled
    assert recs["plan"]["surviving_group_steps"] >= 65 * 225


def _ctx_with(name):
    saved = os.environ.get(name)
    os.environ[name] = "1"
    try:
        return _lib.Context(0)
    finally:
        if saved is None:
            os.environ.pop(name, None)
        else:
            os.environ[name] = saved


def test_nan_and_out_of_band_hypotheses_in_a_word_of_their_own(oracle):
    """PGX_NO_SORT=1 keeps the caller's order, so hypotheses 64 and 65 are word 1: the NaN one is culled everywhere, the scaled one
    (no pair of it is ever rejected) keeps every group"""
    ctx = _ctx_with("PGX_NO_SORT")
    try:
        n = 64 * 9 + 1
        recs = _every_launch_the_same(ctx, n, 66, "odd", sorted_batch=False)
        assert (recs["plan"]["keep"][:, 1] == np.uint64(2)).all()
    finally:
        ctx.close()


def test_the_exact_recount_finds_nothing_the_bound_removed(oracle):
    ctx = _ctx_with("PGX_VERIFY")
    try:
        mt, pts, models, T2, counts = problem(64 * 72, 300)
        ctx.set_points(mt, pts)
        ctx.score_upload(models)
        st = ctx.score_stats(T2)
        assert st["path"] == "cull + group-major" and st["contradictions"] == 0, st
        assert st["inlier_pairs"] == int(counts.sum())
    finally:
        ctx.close()


def test_a_listed_segment_of_two_tiles(gpu_ctx):
    """16 386 groups in 256 segments: 72 groups per segment, a tile of 64 and one of 8, in the instance that also weighs the items"""
    n, M = 64 * 16385 + 1, 65
    modes = {k: MODES[k] for k in ("plan", "lists forced", "lists off", "31 segments")}
    recs = _every_launch_the_same(gpu_ctx, n, M, "large", modes=modes)
    assert recs["plan"]["lists"] is not None and recs["plan"]["surviving_group_steps"] > 0
