#!/usr/bin/env python3
"""findPrimitives' evidence: what a scoring launch of the union type PGX_PRIMITIVE3D = 18 costs against the four constituent launches it
replaces, and what the mixed fit recovers against the four single-class calls.

Scoring: 10^6 points x 2048 union hypotheses, 512 of each class, interleaved as the solver emits them (row 4 s + j = class j); next to
it the four constituent launches of 512 hypotheses each, the same model rows under their own types on the same points.  The cull and
the group-major kernel are timed separately by HIP events (pgx_score_profile / pgx_score_kernel_times), medians over --steps launches;
the yardstick is the sum of the four constituent launches, reported as a ratio per kernel.  The counts must be identical.

Recovery: findPrimitives on make_primitives scenes (two instances of each class, half of the points uniform outliers, 1 cm noise, tilted
synthetic normals, points in random order) at 10^4 / 10^5 / 10^6 points: returned and found per class and the class-confusion table (true
class of an instance against the class of the model matched to it); next to it what findPlanes, findSpheres, findCylinders and
findCones find of their own class on the same scene.  A model is matched to an instance when more than half of the instance's points
lie within the threshold of it.  Writes one JSON record (default profiles/primitives_bench.json) and prints it; the numbers go to
DESIGN.md 4.13.  There is no target for them, and recovery is reported as found, not tuned.

usage: bench_primitives.py [--steps 20] [--sizes 10000,100000,1000000] [--mpn-divisor 40] [--out FILE] [--no-recovery]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "progressive-x_amd"), os.path.join(ROOT, "scripts")]
import pyprogressivex as px  # noqa: E402
from bench_planes import context, score_step  # noqa: E402
from pyprogressivex import _lib, datasets  # noqa: E402

THR, SIGMA = 0.05, 0.01
RADIUS_RANGE, ANGLE_RANGE = (0.2, 3.0), (5.0, 60.0)
CLASSES = (6, 8, 14, 16)
NAMES = {6: "plane", 8: "sphere", 14: "cylinder", 16: "cone"}
PARAMS = {6: 4, 8: 4, 14: 7, 16: 8}


def scene(n, seed=0):
    """make_primitives with two instances of each class and half of the points uniform outliers, metre scale"""
    return datasets.make_primitives(n_per=n // 16, n_outliers=n - 8 * (n // 16), n_each=2, sigma=SIGMA, seed=seed)


def residual(pts, m):
    """the distance of pts to the union row m (not bit for bit: the scripts do not decide inliers)"""
    c, q = int(m[0]), m[1:]
    if c == 6:
        return np.abs(pts @ q[:3] + q[3])
    if c == 8:
        return np.abs(np.linalg.norm(pts - q[:3], axis=1) - q[3])
    e = pts - q[:3]
    rho = np.linalg.norm(np.cross(e, q[3:6]), axis=1)
    if c == 14:
        return np.abs(rho - q[6])
    return np.abs(q[6] * rho - q[7] * (e @ q[3:6]))


def union(c, rows):
    out = np.zeros((len(rows), 9))
    out[:, 0] = c
    out[:, 1:1 + PARAMS[c]] = rows
    return out


def matches(pts, inst, gt, models):
    """per ground-truth instance: the index of the returned model that holds more than half of its points within the threshold, or -1"""
    out = []
    for k in range(len(gt)):
        sel = pts[inst == k + 1]
        hits = [int((residual(sel, m) < THR).sum()) for m in models]
        j = int(np.argmax(hits)) if hits else -1
        out.append(j if j >= 0 and hits[j] > len(sel) // 2 else -1)
    return out


def cell_samples(pts, rng, S, cell=0.5):
    """S quadruples of points that share a grid cell of side `cell` (what NAPSAC-like samplers propose; bench_cones.py's for m = 4)"""
    key = np.floor(pts / cell).astype(np.int64)
    key = (key[:, 0] * 1000003 + key[:, 1]) * 1000003 + key[:, 2]
    order = np.argsort(key, kind="stable")
    sk = key[order]
    starts = np.flatnonzero(np.r_[True, sk[1:] != sk[:-1]])
    ends = np.r_[starts[1:], len(sk)]
    big = np.flatnonzero(ends - starts >= 4)
    c = big[rng.integers(0, len(big), S)]
    pick = (starts[c][:, None] + (rng.random((S, 4)) * (ends[c] - starts[c])[:, None]).astype(np.int64))
    return order[pick].astype(np.int32)


def kernel_times(ctx, models, T2, steps):
    """medians of the cull and the group-major kernel's HIP-event times over `steps` profiled launches of the batch, ms"""
    ctx.score_profile(2)
    ts = []
    for s in range(steps + 2):
        ctx.score_upload(models)
        ctx.score_launch(T2)
        ctx.score_fetch()
        if s >= 2:
            ts.append(ctx.score_kernel_times())
    ctx.score_profile(0)
    ts = np.array(ts)
    return float(np.median(ts[:, 0])), float(np.median(ts[:, 1])), float(np.median(ts[:, 2]))


def scoring(args, out):
    T2 = 2.25 * THR * THR
    pts, nrm, _, _, _ = scene(1_000_000)
    n = pts.shape[0]
    rng = np.random.default_rng(1)
    smp = cell_samples(pts, rng, 64 * 512)                                                       # four points of one grid cell
    smp[::2] = rng.integers(0, n, (len(smp[::2]), 4))                                            # and uniformly random quadruples
    ctx = context({})
    out["device"] = ctx.device_info()["name"]
    ctx.set_points(_lib.PRIMITIVE3D, pts)
    ctx.set_normals(nrm)
    ctx.set_radius_range(*RADIUS_RANGE)
    ctx.set_primitive_classes(15, *(float(np.sin(np.deg2rad(a))) for a in ANGLE_RANGE))
    solved = ctx.solve_minimal(smp)
    rows, yields = {}, {}
    for j, c in enumerate(CLASSES):
        slot = solved[j::4]
        ok = np.isfinite(slot).all(axis=1)
        yields[NAMES[c]] = float(ok.mean())
        rows[c] = slot[ok][:512]
        assert len(rows[c]) == 512, (c, int(ok.sum()))
    batch = np.empty((2048, 9))
    for j, c in enumerate(CLASSES):
        batch[j::4] = rows[c]
    ms, counts = score_step(ctx, batch, T2, args.steps)
    ctx.score_upload(batch)
    st = ctx.score_stats(T2)
    cull, group, finish = kernel_times(ctx, batch, T2, args.steps)
    rec = dict(hypotheses=2048, solver_yield=yields, score_ms=ms, cull_ms=cull, group_ms=group, finish_ms=finish, path=st["path"], filter=st["filter"],
               group_survival=st["surviving_group_steps"] / max(st["group_pairs"], 1), exact_fraction=st["exact_evaluations"] / max(st["pairs"], 1),
               median_inliers=float(np.median(counts)))
    parts, same = {}, True
    for j, c in enumerate(CLASSES):
        q = np.ascontiguousarray(rows[c][:, 1:1 + PARAMS[c]])
        ctx.set_points(c, pts)
        ms_c, counts_c = score_step(ctx, q, T2, args.steps)
        ctx.score_upload(q)
        st_c = ctx.score_stats(T2)
        cull_c, group_c, finish_c = kernel_times(ctx, q, T2, args.steps)
        same = same and bool(np.array_equal(counts_c, counts[j::4]))
        parts[NAMES[c]] = dict(hypotheses=512, score_ms=ms_c, cull_ms=cull_c, group_ms=group_c, finish_ms=finish_c,
                               group_survival=st_c["surviving_group_steps"] / max(st_c["group_pairs"], 1),
                               exact_fraction=st_c["exact_evaluations"] / max(st_c["pairs"], 1), median_inliers=float(np.median(counts_c)))
    ctx.close()
    tot = {k: sum(p[k] for p in parts.values()) for k in ("score_ms", "cull_ms", "group_ms", "finish_ms")}
    out["scoring"] = dict(n=n, union=rec, constituents=parts, constituents_sum=tot, counts_identical=same,
                          ratio_cull=cull / tot["cull_ms"], ratio_group=group / tot["group_ms"], ratio_step=ms / tot["score_ms"])


def recovery(args, out):
    calls = {}
    single = dict(plane=lambda p, nr, kw: px.findPlanes(p, **kw),
                  sphere=lambda p, nr, kw: px.findSpheres(p, radius_range=RADIUS_RANGE, **kw),
                  cylinder=lambda p, nr, kw: px.findCylinders(p, nr, radius_range=RADIUS_RANGE, **kw),
                  cone=lambda p, nr, kw: px.findCones(p, nr, angle_range=ANGLE_RANGE, **kw))
    for size in [int(s) for s in args.sizes.split(",") if s]:
        p, nr, cls, inst, gt = scene(size, seed=2)
        order = np.random.default_rng(0).permutation(len(p))
        p, nr, cls, inst = np.ascontiguousarray(p[order]), np.ascontiguousarray(nr[order]), cls[order], inst[order]
        # minimum_point_number = n / divisor.  An instance has n / 16 points; a slab of width 3 thr across the box, the largest shell
        # here, holds 1.5 % of the outliers: n / 133
        kw = dict(threshold=THR, minimum_point_number=size // args.mpn_divisor, seed=1)
        w = min(size, 20000)
        px.findPrimitives(p[:w], nr[:w], radius_range=RADIUS_RANGE, angle_range=ANGLE_RANGE, **kw)                  # warm-up (kernels, context)
        t0 = time.perf_counter()
        models, labels = px.findPrimitives(p, nr, radius_range=RADIUS_RANGE, angle_range=ANGLE_RANGE, **kw)
        dt = time.perf_counter() - t0
        got = matches(p, inst, gt, models)
        confusion = {NAMES[c]: {} for c in CLASSES}
        for g, j in zip(gt, got):
            key = "none" if j < 0 else NAMES[int(models[j][0])]
            confusion[NAMES[int(g[0])]][key] = confusion[NAMES[int(g[0])]].get(key, 0) + 1
        rec = dict(seconds=dt, returned={NAMES[c]: int((models[:, 0] == c).sum()) for c in CLASSES},
                   found={NAMES[c]: sum(1 for g, j in zip(gt, got) if g[0] == c and j >= 0 and models[j][0] == c) for c in CLASSES},
                   unmatched=int(len(models) - len({j for j in got if j >= 0})), confusion=confusion, labelled=int((labels < len(models)).sum()))
        alone = {}
        for c in CLASSES:
            name = NAMES[c]
            single[name](p[:w], nr[:w], kw)
            t0 = time.perf_counter()
            m, _ = single[name](p, nr, kw)
            dt_c = time.perf_counter() - t0
            um = union(c, m)
            got_c = matches(p, inst, gt, um)
            alone[name] = dict(seconds=dt_c, returned=int(len(m)), found=sum(1 for g, j in zip(gt, got_c) if g[0] == c and j >= 0),
                               holds_other_classes=sum(1 for g, j in zip(gt, got_c) if g[0] != c and j >= 0))
        calls[str(size)] = dict(findPrimitives=rec, single_class=alone, minimum_point_number=size // args.mpn_divisor)
        print(size, calls[str(size)], file=sys.stderr, flush=True)
        with open(args.out + ".partial", "w") as f:              # (a long run that is cut short keeps what it measured)
            f.write(json.dumps(dict(out, recovery=calls)) + "\n")
    out["recovery"] = calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--sizes", default="10000,100000,1000000")
    ap.add_argument("--mpn-divisor", type=int, default=40)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "primitives_bench.json"))
    ap.add_argument("--no-recovery", action="store_true")
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    out = dict(workload="primitives", threshold=THR, radius_range=list(RADIUS_RANGE), angle_range=list(ANGLE_RANGE))
    scoring(args, out)
    with open(args.out + ".partial", "w") as f:
        f.write(json.dumps(out) + "\n")
    if not args.no_recovery:
        recovery(args, out)
    text = json.dumps(out)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    if os.path.exists(args.out + ".partial"):
        os.remove(args.out + ".partial")
    print(text, flush=True)


if __name__ == "__main__":
    main()
