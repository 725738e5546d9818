"""The group-major kernel taking (group, 4-word) items from the cull kernel's work lists (csrc/score.hip, csrc/score_worklist.h)
against the same launch with the lists switched off: counts, masks and the integer accumulators array_equal, values and shared
bitwise, the three work counters of pgx_score_stats equal - and all of it against the oracle as tests/test_gpu_parity.py compares.

Each case runs three ways: lists off (worklist = 0), the plan's own choice (on for a locality-ordered pose batch, i.e. M > 64), and
forced on (worklist = 1 with the co-located mapping), which also covers the one-word batch.  After every listed launch the counts
the cull kernel left are read back and must be exactly what the survivor words say: per [g & 7][class] the number of (group, 4-word)
items with that weight, so their total is the number of items with a non-zero keep word.

n: 65 two groups | 513 one super-group + 1 | 4097 more groups than one tile of the cull kernel | 64 * 8 * 3 + 1 a group count that is
no multiple of 8.  M: 64, 65, 257, 321 (one word; the reorder begins; two items per group, the second with empty words behind M).
The constructions are checked against the oracle on the CPU (module scope) before a case touches the GPU."""
import functools
import os

import numpy as np
import pytest

from helpers import make_case
from pyprogressivex import _lib

pytestmark = pytest.mark.gpu

REL = 1e-9
NS = (65, 513, 4097, 64 * 8 * 3 + 1)
MS = (64, 65, 257, 321)
T_DEFAULT = (24, 64, 160)
MODES = {"off": dict(worklist=0, group_xcd=-1), "auto": dict(worklist=-1, group_xcd=-1), "forced": dict(worklist=1, group_xcd=1)}
RESET = dict(worklist=-1, group_xcd=-1, wl_t1=T_DEFAULT[0], wl_t2=T_DEFAULT[1], wl_t3=T_DEFAULT[2])
COUNTERS = ("surviving_group_steps", "exact_evaluations", "inlier_pairs")


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.max(np.abs(a - b) / np.maximum(1e-300, np.maximum(np.abs(a), np.abs(b)))) if a.size else 0.0


def _missing(models):
    """the same poses shifted sideways by four times their depth: every projection lands about four focal lengths outside the image,
    at a scale the f32 bound still decides (a shift by a thousand depths leaves its trusted range and every group survives)"""
    out = models.copy().reshape(-1, 3, 4)
    out[:, 0, 3] += 4.0 * np.abs(out[:, 2, 3])
    return np.ascontiguousarray(out.reshape(-1, 12))


@functools.lru_cache(maxsize=None)
def problem(n, M, kind="grid"):
    import pgx_oracle as O
    mt, pts, models, thr = make_case("pnp", n, max(M, 8), seed=n + M)
    gt = models[:3].copy()
    models = models[:M].copy()
    if kind == "miss":
        models = _missing(np.resize(gt, (M, 12)))
    elif kind == "heavy":
        # four item columns of 256 hypotheses: 200 copies of object 0 | 100 of object 1 | 40 of object 2 | 3 of object 0, the rest misses
        assert M == 4 * 256
        models = _missing(np.resize(gt, (M, 12)))
        models[0:200] = gt[0]
        models[256:356] = gt[1]
        models[512:552] = gt[2]
        models[768:771] = gt[0]
    T2 = 2.25 * thr * thr
    comp = O.preference(O.PNP, pts, gt[0], T2)
    refs = {}
    with np.errstate(all="ignore"):
        for compound in (False, True):
            refs[compound] = O.score(O.PNP, pts, models, T2, compound=comp if compound else None, has_compound=compound, exponent=2,
                                     want_masks=True)
    # ---- the construction, on the CPU
    c = refs[False]["counts"]
    if kind == "miss":
        assert not c.any() and not refs[True]["values"].any()
    elif kind == "heavy":
        assert c[0:200].min() > 0 and c[256:356].min() > 0 and c[512:552].min() > 0 and c[768:771].min() > 0
        assert np.count_nonzero(c) == 200 + 100 + 40 + 3
    else:
        assert c[:3].min() > 8 and np.count_nonzero(c) >= min(M, 3)          # the ground truth has its inliers
    for a in (pts, models, comp):
        a.setflags(write=False)
    return mt, pts, models, T2, comp, refs


def _expected_counts(keep, t):
    """[g & 7][class] from the survivor words: an item is a group x 4 adjacent words, its weight the set bits in them"""
    groups, W = keep.shape
    pop = np.unpackbits(keep.view(np.uint8), axis=1).reshape(groups, W, 64).sum(axis=2)
    cols = (W + 3) // 4
    weight = np.zeros((groups, cols), np.int64)
    for x in range(cols):
        weight[:, x] = pop[:, 4 * x:4 * x + 4].sum(axis=1)
    cls = (weight >= t[0]).astype(int) + (weight >= t[1]) + (weight >= t[2])
    want = np.zeros((8, 4), np.int64)
    for g, x in zip(*np.nonzero(weight)):
        want[g & 7, cls[g, x]] += 1
    return want, weight


def _launch(ctx, models, T2, comp, compound, Mpad, listed, t=T_DEFAULT):
    """stats + one score on the resident points; the record every mode must agree on, and the lists' counts when `listed`"""
    ctx.set_compound(comp if compound else None)
    ctx.score_upload(models)
    st = ctx.score_stats(T2, has_compound=compound)
    assert st["path"] == "cull + group-major" and st["filter"] == "f32"
    rec = {k: st[k] for k in COUNTERS}
    if listed:
        want, _ = _expected_counts(ctx.score_keep_words(Mpad), t)
        assert np.array_equal(ctx.score_worklist_counts(), want), "the counters launch's lists"
    table = ctx.score(models, T2, has_compound=compound, exponent=2)
    for k in ("counts", "values", "shared"):
        rec[k] = table[k].copy()
    rec.update({"acc_" + k: v for k, v in ctx.score_accumulators().items()})
    if listed:
        want, weight = _expected_counts(ctx.score_keep_words(Mpad), t)
        got = ctx.score_worklist_counts()
        assert np.array_equal(got, want), (got, want)
        assert int(got.sum()) == np.count_nonzero(weight)
        rec["lists"], rec["weight"] = got, weight
    else:
        with pytest.raises(_lib.PgxError, match="work lists"):
            ctx.score_worklist_counts()
    return rec


def _same_bits(a, b, where):
    for k in a:
        if k in ("lists", "weight"):
            continue
        if k in COUNTERS:
            assert a[k] == b[k], (where, k, a[k], b[k])
        elif a[k].dtype.kind == "f":
            assert np.array_equal(a[k].view(np.uint64), b[k].view(np.uint64)), (where, k)
        else:
            assert np.array_equal(a[k], b[k]), (where, k)


def _against_oracle(rec, ref):
    assert np.array_equal(rec["counts"], ref["counts"]), "inlier counts differ"
    assert _rel(rec["values"], ref["values"]) <= REL and _rel(rec["shared"], ref["shared"]) <= REL
    assert np.array_equal(rec["acc_counts"].astype(np.int64)[:len(ref["counts"])], ref["counts"])
    assert rec["inlier_pairs"] == int(ref["counts"].sum())


@pytest.mark.parametrize("compound", [False, True], ids=["plain", "compound"])
@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("n", NS)
def test_lists_on_equals_lists_off_and_the_oracle(gpu_ctx, oracle, n, M, compound):
    mt, pts, models, T2, comp, refs = problem(n, M)
    Mpad = (M + 255) // 256 * 256
    try:
        gpu_ctx.set_points(mt, pts)
        recs = {}
        for mode, geo in MODES.items():
            gpu_ctx.score_debug_geometry(**geo)
            recs[mode] = _launch(gpu_ctx, models, T2, comp, compound, Mpad, listed=mode == "forced" or (mode == "auto" and M > 64))
        for mode in ("auto", "forced"):
            _same_bits(recs["off"], recs[mode], mode)
        _against_oracle(recs["off"], refs[compound])
        # masks come from the in-place variant, which keeps the strided parts: equal under every setting of the switch
        for geo in MODES.values():
            gpu_ctx.score_debug_geometry(**geo)
            got = gpu_ctx.score(models, T2, has_compound=compound, exponent=2, want_masks=True)
            assert np.array_equal(got["masks"], refs[compound]["masks"]) and np.array_equal(got["counts"], refs[compound]["counts"])
    finally:
        gpu_ctx.score_debug_geometry(**RESET)


def test_hypotheses_that_miss_every_point_leave_every_list_empty(gpu_ctx, oracle):
    mt, pts, models, T2, comp, refs = problem(4097, 257, "miss")
    try:
        gpu_ctx.set_points(mt, pts)
        for compound in (False, True):
            rec = _launch(gpu_ctx, models, T2, comp, compound, 512, listed=True)
            assert not rec["lists"].any() and not rec["weight"].any()
            for k in ("counts", "values", "shared", "acc_counts", "acc_values_q", "acc_shared_q"):
                assert not rec[k].any(), k
            assert [rec[k] for k in COUNTERS] == [0, 0, 0]
            _against_oracle(rec, refs[compound])
    finally:
        gpu_ctx.score_debug_geometry(**RESET)


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


def test_graded_items_populate_every_class(unsorted_ctx, oracle):
    """200 / 100 / 40 / 3 copies of a ground-truth pose in four different item columns, everything else misses: a group holding an
    inlier of the pose keeps all its copies (the bound removes no inlier), so its items weigh 200 -> class 3, 100 -> 2, 40 -> 1, 3 -> 0 at the thresholds 24 / 64 / 160"""
    ctx = unsorted_ctx
    mt, pts, models, T2, comp, refs = problem(4097, 1024, "heavy")
    try:
        ctx.set_points(mt, pts)
        ctx.score_debug_geometry(**MODES["off"])
        off = _launch(ctx, models, T2, comp, True, 1024, listed=False)
        ctx.score_debug_geometry(**MODES["forced"])
        on = _launch(ctx, models, T2, comp, True, 1024, listed=True)
        _same_bits(off, on, "heavy")
        _against_oracle(on, refs[True])
        weight, lists = on["weight"], on["lists"]
        assert weight[:, 0].max() == 200 and weight[:, 1].max() == 100 and weight[:, 2].max() == 40 and weight[:, 3].max() == 3
        assert np.all(lists.sum(axis=0) > 0), lists              # every class holds items
        assert int(lists.sum()) == np.count_nonzero(weight)
        # other thresholds, two classes: the same bits, the counts follow the thresholds
        for t in ((4, 41, 201), (51, 1 << 30, 1 << 30)):
            ctx.score_debug_geometry(wl_t1=t[0], wl_t2=t[1], wl_t3=t[2])
            again = _launch(ctx, models, T2, comp, True, 1024, listed=True, t=t)
            _same_bits(off, again, t)
        assert not again["lists"][:, 2:].any() and again["lists"][:, 1].any() and again["lists"][:, 0].any()
    finally:
        ctx.score_debug_geometry(**RESET)


def test_counts_are_zero_again_for_the_next_launch_and_the_next_batch(gpu_ctx, oracle):
    mt, pts, models, T2, comp, refs = problem(4097, 321)
    other = np.ascontiguousarray(models[::-1][:257])
    with np.errstate(all="ignore"):
        other_refs = {c: oracle.score(oracle.PNP, pts, other, T2, compound=comp if c else None, has_compound=c, exponent=2) for c in (False, True)}
    try:
        gpu_ctx.set_points(mt, pts)
        gpu_ctx.score_debug_geometry(**MODES["auto"])
        first = _launch(gpu_ctx, models, T2, comp, True, 512, listed=True)
        # launches in a row without anything in between: stale counts would double the lists and the sums
        for _ in range(3):
            gpu_ctx.score_launch(T2, has_compound=True)
        table = gpu_ctx.score_fetch(exponent=2)
        assert np.array_equal(table["counts"], first["counts"]) and np.array_equal(table["values"].view(np.uint64), first["values"].view(np.uint64))
        assert np.array_equal(gpu_ctx.score_worklist_counts(), first["lists"])
        # a changed batch, a launch with the lists off in between, the first batch again
        _against_oracle(_launch(gpu_ctx, other, T2, comp, False, 512, listed=True), other_refs[False])
        gpu_ctx.score_debug_geometry(**MODES["off"])
        _against_oracle(_launch(gpu_ctx, other, T2, comp, True, 512, listed=False), other_refs[True])
        gpu_ctx.score_debug_geometry(**MODES["auto"])
        _same_bits(first, _launch(gpu_ctx, models, T2, comp, True, 512, listed=True), "again")
        # new points reallocate nothing the lists depend on wrongly: a smaller problem, then the first one
        mt2, pts2, models2, T2b, comp2, refs2 = problem(513, 257)
        gpu_ctx.set_points(mt2, pts2)
        _against_oracle(_launch(gpu_ctx, models2, T2b, comp2, True, 512, listed=True), refs2[True])
        gpu_ctx.set_points(mt, pts)
        _same_bits(first, _launch(gpu_ctx, models, T2, comp, True, 512, listed=True), "after other points")
    finally:
        gpu_ctx.score_debug_geometry(**RESET)
