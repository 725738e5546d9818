"""The scoring cases of tests/golden/score_plans_v1.json: which path a scoring launch takes, at which filter level, with how much
work, and the bits it produces - pinned before the launch decisions moved into csrc/score_plan.h.
tests/golden/make_golden_score_plans.py records them, tests/test_gpu_score_plans.py replays them; both go through run_case().

A case: set_points, set_compound, upload, pgx_score_stats (path, filter level, surviving steps, exact evaluations, inlier pairs),
then one pgx_score.  Recorded: those five counters, SHA-256 of counts / values / shared (and of the masks where taken) and, on the
group-major path, of the integer accumulators.
  grid-*      all eight model types x n in {65, 513, 4097} (two groups; one super-group + 1; nine super-groups) x M in {64, 65, 257}
              (one word; the locality reorder begins; two padded blocks), without and with compound + masks
  window-*    per bound kind one T2 inside and one outside the window of its f32 filter: the path flips between 2 and 1
  geometry-*  one pose and one line case under split = 3, group_xcd = 0 / 1, nrep = 16, cull_segs = 1: the result digests must be
              the default geometry's (GEOMETRY_TWINS)"""
import functools
import hashlib

import numpy as np

from helpers import make_case

# the eight types the golden file was recorded with, in its order (helpers.ALL_MODEL_CASES has grown since: circles are not recorded)
PLAN_TYPES = ("line", "homography", "fundamental", "pnp", "vanishing_point", "homography_sym", "plane", "sphere")
NS = (65, 513, 4097)
MS = (64, 65, 257)
# (type, T2 outside the window): kBoundBall | kBoundBoxAll | kBoundVanishing | the homography family | kBoundBox (umax > T * 2^14)
WINDOWS = (("line", 1e25), ("fundamental", 1e13), ("vanishing_point", 1e31), ("homography", 1e25), ("pnp", 1e-12))
GEOMETRIES = ({}, {"split": 3}, {"group_xcd": 0}, {"group_xcd": 1}, {"nrep": 16}, {"cull_segs": 1})
GEOMETRY_TYPES = ("pnp", "line")
WORK_COUNTERS = ("surviving_group_steps", "exact_evaluations", "inlier_pairs")   # may be dropped where the parent's two runs differ
DIGESTS = ("counts", "values", "shared", "masks", "acc_counts", "acc_values_q", "acc_shared_q")


def _geo_id(geo):
    return ",".join(f"{k}={v}" for k, v in geo.items()) or "default"


def cases():
    """{case id: (type, n, M, T2 or None for the case's own threshold, compound + masks, geometry)} in a fixed order"""
    out = {}
    for name in PLAN_TYPES:
        for n in NS:
            for M in MS:
                for full in (False, True):
                    out[f"grid-{name}-{n}-{M}-{'compound+masks' if full else 'plain'}"] = (name, n, M, None, full, {})
    for name, outside in WINDOWS:
        out[f"window-{name}-inside"] = (name, 513, 65, None, False, {})
        out[f"window-{name}-outside"] = (name, 513, 65, outside, False, {})
    for name in GEOMETRY_TYPES:
        for geo in GEOMETRIES:
            out[f"geometry-{name}-{_geo_id(geo)}"] = (name, 4097, 257, None, True, geo)
    return out


GEOMETRY_TWINS = {f"geometry-{name}-{_geo_id(geo)}": f"geometry-{name}-default" for name in GEOMETRY_TYPES for geo in GEOMETRIES[1:]}


def must_keep(field):
    return field not in WORK_COUNTERS


@functools.lru_cache(maxsize=None)
def problem(name, n, M):
    mt, pts, models, thr = make_case(name, n, M, seed=n + M)
    comp = np.random.default_rng(n * 1000 + M).random(n)
    return mt, pts, models, 2.25 * thr * thr, comp


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def run_on(ctx, case_id):
    """the record of one case on `ctx` (default switches; the geometry settings are the case's and are put back)"""
    name, n, M, T2, full, geo = cases()[case_id]
    mt, pts, models, T2_own, comp = problem(name, n, M)
    T2 = T2_own if T2 is None else T2
    ctx.score_debug_geometry(**geo)
    try:
        ctx.set_points(mt, pts)
        ctx.set_compound(comp if full else None)
        ctx.score_upload(models)
        st = ctx.score_stats(T2, has_compound=full)
        out = {"path": st["path"], "filter": st["filter"]}
        for k in WORK_COUNTERS:
            out[k] = st[k]
        table = ctx.score(models, T2, has_compound=full, want_masks=full)
        for k in ("counts", "values", "shared") + (("masks",) if full else ()):
            out[k] = _sha(table[k])
        if st["path"] == "cull + group-major":
            for k, v in ctx.score_accumulators().items():
                out["acc_" + k] = _sha(v)
        return out
    finally:
        ctx.score_debug_geometry(split=0, group_xcd=-1, nrep=0, cull_segs=256)
