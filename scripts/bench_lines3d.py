#!/usr/bin/env python3
"""findLines3D's evidence of speed: the scoring step at 10^6 points x 2048 line hypotheses on the cull + group-major path with the
f32 tube filter - lines through two uniformly random points and lines through two points of one grid cell - against the same library
with both switched off (PGX_NO_FILTER=1 PGX_SCORE_NO_CULL=1, identical counts as a condition), the survival fractions of
pgx_score_stats, and findLines3D per sampler at 10^4, 10^5 and 10^6 points (six lines, half of the points uniform outliers, 1 cm
noise, points in random order): lines found / returned and wall time.  Writes one JSON record (default profiles/lines3d_bench.json)
and prints it; the numbers go to DESIGN.md.  There is no target for them.

usage: bench_lines3d.py [--steps 20] [--sizes 10000,100000,1000000] [--samplers 3,2,1,0] [--mpn-divisors 40,150] [--out FILE]"""
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


def scene(n, seed=0):
    """make_lines3d with six lines and half of the points uniform outliers, metre scale (10 m box, 1 cm noise)"""
    return datasets.make_lines3d(n_per_line=n // 12, n_lines=6, n_outliers=n - 6 * (n // 12), sigma=SIGMA, seed=seed)


def cell_samples(pts, rng, S, cells=16):
    """S pairs of points of one cell of a cells^3 grid over the bounding box (the baselines a local sampler draws)"""
    lo, hi = pts.min(axis=0), pts.max(axis=0)
    q = np.minimum(((pts - lo) / (hi - lo) * cells).astype(np.int64), cells - 1)
    key = (q[:, 0] * cells + q[:, 1]) * cells + q[:, 2]
    order = np.argsort(key, kind="stable")
    start = np.searchsorted(key[order], np.arange(cells ** 3 + 1))
    out = np.empty((S, 2), np.int32)
    k = 0
    while k < S:
        c = key[rng.integers(0, len(pts))]                  # a cell drawn by one of its points
        members = order[start[c]:start[c + 1]]
        if len(members) >= 2:
            out[k] = rng.choice(members, 2, replace=False)
            k += 1
    return out


def found(lines, gt):
    """ground-truth lines a returned line passes within 3 sigma of, 2 m either side of the midpoint (every segment is at least 4 m)"""
    n = 0
    for g in gt:
        ends = g[:3] + np.array([[-2.0], [2.0]]) * g[3:]
        for m in lines:
            c = np.cross(ends - m[:3], m[3:])
            if (np.linalg.norm(c, axis=1) < 3 * SIGMA).all():
                n += 1
                break
    return n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--sizes", default="10000,100000,1000000")
    ap.add_argument("--samplers", default="3,2,1,0")
    ap.add_argument("--mpn-divisors", default="40,150")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lines3d_bench.json"))
    args = ap.parse_args()
    T2 = 2.25 * THR * THR
    pts, _, _ = scene(1_000_000)
    n = pts.shape[0]
    out = dict(workload="lines3d", n_score=n, threshold=THR)
    rng = np.random.default_rng(1)
    batches = dict(random_points=rng.integers(0, n, (2048, 2)).astype(np.int32), grid_cell=cell_samples(pts, rng, 2048))

    ctx = context({})
    out["device"] = ctx.device_info()["name"]
    ctx.set_points(_lib.LINE3D, pts)
    models, fast = {}, {}
    for name, smp in batches.items():
        m = ctx.solve_minimal(smp)
        models[name] = m[np.isfinite(m).all(axis=1)]
        ms, counts = score_step(ctx, models[name], T2, args.steps)
        ctx.score_upload(models[name])
        st = ctx.score_stats(T2)
        fast[name] = counts
        out[name] = dict(hypotheses=int(len(models[name])), score_ms=ms, score_models_per_s=len(models[name]) / (ms * 1e-3),
                         path=st["path"], filter=st["filter"], group_survival=st["surviving_group_steps"] / max(st["group_pairs"], 1),
                         exact_fraction=st["exact_evaluations"] / max(st["pairs"], 1), median_inliers=float(np.median(counts)))
    ctx.close()

    dense = context({"PGX_NO_FILTER": "1", "PGX_SCORE_NO_CULL": "1"})
    dense.set_points(_lib.LINE3D, pts)
    for name in batches:
        ms_d, counts_d = score_step(dense, models[name], T2, args.steps)
        out[name].update(dense_score_ms=ms_d, cull_speedup=ms_d / out[name]["score_ms"],
                         dense_counts_identical=bool(np.array_equal(fast[name], counts_d)))
    dense.close()

    calls = {}
    for size in [int(s) for s in args.sizes.split(",") if s]:
        p, gen, gt = scene(size, seed=2)
        order = np.random.default_rng(0).permutation(len(p))
        p = np.ascontiguousarray(p[order])
        # minimum_point_number = n / divisor.  A line has n / 12 inliers; a tube of radius 1.5 thr along the box's diagonal holds
        # 1.5e-4 n outliers, and a line crossing two true lines at 30 degrees about 2 * (0.3 m / 7 m) * n / 12 = n / 140 of their points.
        # The run's stop rule sets the other side: its prediction of still-unseen inliers falls with the sample size, and
        # with n / 40 no sampler returns all six lines
        for div in [int(s) for s in args.mpn_divisors.split(",") if s]:
            kw = dict(threshold=THR, minimum_point_number=size // div, seed=1)
            for sid in [int(s) for s in args.samplers.split(",") if s]:
                px.findLines3D(p[: min(size, 20000)], sampler_id=sid, **kw)          # warm-up (kernels, context)
                t0 = time.perf_counter()
                lines, labels = px.findLines3D(p, sampler_id=sid, **kw)
                dt = time.perf_counter() - t0
                key = f"{size}@sampler={sid}@mpn=n/{div}"
                calls[key] = dict(seconds=dt, returned=int(len(lines)), found=found(lines, gt))
                print(key, calls[key], file=sys.stderr, flush=True)
    out["findLines3D"] = calls
    text = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text, flush=True)


if __name__ == "__main__":
    main()
