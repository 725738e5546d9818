#!/usr/bin/env python3
"""findOrientedPrimitives' evidence: what the test of the normals costs a scoring launch, and what it changes in what the fit returns.

Scoring: bench_primitives.py's batch - 10^6 points x 2048 union hypotheses, 512 of each class, interleaved as the solver emits them -
scored under PGX_ORIENTED_PRIMITIVE3D = 20 at --tolerance degrees and under PGX_PRIMITIVE3D = 18, the same rows on the same points in
the same session: the time of a step (upload + launch + fetch), the cull and the group-major kernel by HIP events, the work counters
and the inlier counts.  Type 20's count may not exceed type 18's for any hypothesis (asserted).

Recovery: bench_primitives.py's scenes (two instances of each class, half of the points uniform outliers, 1 cm noise, points in random
order) at 10^4 / 10^5 / 10^6 points, with the generator's normals (the true ones tilted by up to 5 degrees) and with estimateNormals'
over a ball (radius per size below: some tens of neighbours on a surface, at least 15 sigma): findPrimitives against
findOrientedPrimitives at 10, 20 and 40 degrees - returned and found per class, class errors (an instance matched by a model of
another class), returned models that match no instance, seconds.  Writes one JSON record (default
profiles/oriented_primitives_bench.json) and prints it; the numbers go to DESIGN.md 4.14 as found.  There is no target for them.

usage: bench_oriented_primitives.py [--steps 20] [--sizes 10000,100000,1000000] [--tolerance 20] [--mpn-divisor 40] [--out FILE]
                                    [--no-recovery] [--no-scoring]"""
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
from bench_primitives import ANGLE_RANGE, CLASSES, NAMES, RADIUS_RANGE, THR, cell_samples, kernel_times, matches, scene  # noqa: E402
from pyprogressivex import _lib  # noqa: E402

BALL = {10_000: 0.57, 100_000: 0.3, 1_000_000: 0.15}     # estimateNormals' ball radius per scene size
TOLERANCES = (10.0, 20.0, 40.0)


def scoring(args, out):
    T2 = 2.25 * THR * THR
    pts, nrm, _, _, _ = scene(1_000_000)
    n = pts.shape[0]
    rng = np.random.default_rng(1)
    smp = cell_samples(pts, rng, 64 * 512)
    smp[::2] = rng.integers(0, n, (len(smp[::2]), 4))
    ctx = context({})
    out["device"] = ctx.device_info()["name"]
    ctx.set_points(_lib.PRIMITIVE3D, pts)
    ctx.set_normals(nrm)
    ctx.set_radius_range(*RADIUS_RANGE)
    ctx.set_primitive_classes(15, *(float(np.sin(np.deg2rad(a))) for a in ANGLE_RANGE))
    solved = ctx.solve_minimal(smp)
    batch = np.empty((2048, 9))
    for j in range(4):
        slot = solved[j::4]
        batch[j::4] = slot[np.isfinite(slot).all(axis=1)][:512]
    kappa = float(np.cos(np.deg2rad(args.tolerance)) ** 2)
    rec, counts = {}, {}
    for name, mt in (("type18", _lib.PRIMITIVE3D), ("type20", _lib.ORIENTED_PRIMITIVE3D)):
        ctx.set_points(mt, pts)
        ctx.set_normals(nrm)
        ctx.set_normal_tolerance(kappa)
        ms, counts[name] = score_step(ctx, batch, T2, args.steps)
        ctx.score_upload(batch)
        st = ctx.score_stats(T2)
        cull, group, finish = kernel_times(ctx, batch, T2, args.steps)
        rec[name] = dict(score_ms=ms, cull_ms=cull, group_ms=group, finish_ms=finish, path=st["path"], filter=st["filter"],
                         surviving_group_steps=st["surviving_group_steps"], exact_evaluations=st["exact_evaluations"], inlier_pairs=st["inlier_pairs"],
                         median_inliers=float(np.median(counts[name])), total_inliers=int(counts[name].sum()))
    solved20 = ctx.solve_minimal(smp)                    # the oriented solver on the same samples: the slots Schnabel's candidate test keeps
    ctx.close()
    assert (counts["type20"] <= counts["type18"]).all()
    per_class = {NAMES[c]: dict(type18=int(counts["type18"][j::4].sum()), type20=int(counts["type20"][j::4].sum())) for j, c in enumerate(CLASSES)}
    kept = {NAMES[c]: [float(np.isfinite(solved[j::4]).all(axis=1).mean()), float(np.isfinite(solved20[j::4]).all(axis=1).mean())] for j, c in enumerate(CLASSES)}
    out["scoring"] = dict(n=n, hypotheses=2048, tolerance_deg=args.tolerance, counts_never_above_type18=True, inliers_per_class=per_class,
                          solver_yield_type18_type20=kept, ratio_step=rec["type20"]["score_ms"] / rec["type18"]["score_ms"],
                          ratio_cull=rec["type20"]["cull_ms"] / rec["type18"]["cull_ms"], ratio_group=rec["type20"]["group_ms"] / rec["type18"]["group_ms"], **rec)


def summary(p, inst, gt, models, dt):
    got = matches(p, inst, gt, models)
    return dict(seconds=dt, returned={NAMES[c]: int((models[:, 0] == c).sum()) for c in CLASSES},
                found={NAMES[c]: sum(1 for g, j in zip(gt, got) if g[0] == c and j >= 0 and models[j][0] == c) for c in CLASSES},
                found_total=sum(1 for g, j in zip(gt, got) if j >= 0 and models[j][0] == g[0]), returned_total=int(len(models)),
                class_errors=sum(1 for g, j in zip(gt, got) if j >= 0 and models[j][0] != g[0]),
                unmatched=int(len(models) - len({j for j in got if j >= 0})))


def recovery(args, out):
    calls = {}
    for size in [int(s) for s in args.sizes.split(",") if s]:
        p, nr, cls, inst, gt = scene(size, seed=2)
        order = np.random.default_rng(0).permutation(len(p))
        p, nr, cls, inst = np.ascontiguousarray(p[order]), np.ascontiguousarray(nr[order]), cls[order], inst[order]
        radius = BALL.get(size, 0.3)
        t0 = time.perf_counter()
        ball = px.estimateNormals(p, k=None, radius=radius)
        t_normals = time.perf_counter() - t0
        defined = np.isfinite(ball).all(axis=1)
        kw = dict(threshold=THR, minimum_point_number=size // args.mpn_divisor, seed=1, radius_range=RADIUS_RANGE, angle_range=ANGLE_RANGE)
        w = min(size, 20000)
        rec = dict(minimum_point_number=size // args.mpn_divisor, ball_radius=radius, estimateNormals_seconds=t_normals, undefined_normals=int((~defined).sum()))
        for kind, normals in (("true_normals", nr), ("ball_normals", ball)):
            px.findPrimitives(p[:w], normals[:w], **kw)                                                     # warm-up (kernels, context)
            t0 = time.perf_counter()
            models, _ = px.findPrimitives(p, normals, **kw)
            row = dict(findPrimitives=summary(p, inst, gt, models, time.perf_counter() - t0))
            for tol in TOLERANCES:
                px.findOrientedPrimitives(p[:w], normals[:w], normal_tolerance=tol, **kw)
                t0 = time.perf_counter()
                models, _ = px.findOrientedPrimitives(p, normals, normal_tolerance=tol, **kw)
                row[f"oriented_{int(tol)}"] = summary(p, inst, gt, models, time.perf_counter() - t0)
            rec[kind] = row
            print(size, kind, row, file=sys.stderr, flush=True)
            calls[str(size)] = rec
            with open(args.out + ".partial", "w") as f:              # (a long run that is cut short keeps what it measured)
                f.write(json.dumps(dict(out, recovery=calls)) + "\n")
    out["recovery"] = calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--sizes", default="10000,100000,1000000")
    ap.add_argument("--tolerance", type=float, default=20.0)
    ap.add_argument("--mpn-divisor", type=int, default=40)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "oriented_primitives_bench.json"))
    ap.add_argument("--no-recovery", action="store_true")
    ap.add_argument("--no-scoring", action="store_true")
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    out = dict(workload="oriented_primitives", threshold=THR, radius_range=list(RADIUS_RANGE), angle_range=list(ANGLE_RANGE), instances_per_scene=8)
    if not args.no_scoring:
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
