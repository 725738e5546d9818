#!/usr/bin/env python3
"""findCircles' evidence of speed: the scoring step at 10^6 points x 2048 circle hypotheses on two batches - (a) circles through
three uniformly random points, (b) circles through three points of one cell of the 16^2 grid (what Progressive NAPSAC proposes) -
on the group cull + f32 filter path and with both switched off as the dense reference (identical counts), the share of
(hypothesis, group) pairs that survives the cull (pgx_score_stats), and findCircles wall time and circles recovered on six circles
with 50 % outliers at 10^4, 10^5 and 10^6 points for samplers 0, 2 and 3, with minimum_point_number = n / 40 and n / 25.  Prints
one JSON line; the numbers go to profiles/circles_bench.json, DESIGN.md and README.md.

usage: bench_circles.py [--steps 20] [--sizes 10000,100000,1000000]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "progressive-x_amd")]
import pyprogressivex as px  # noqa: E402
from pyprogressivex import _lib, datasets  # noqa: E402


def scene(n, seed=0, sigma=0.5):
    """make_circles with six circles and half of the points uniform outliers, pixel scale (1000 x 1000 box, half a pixel of noise),
    in a random order (Progressive NAPSAC and PROSAC take the points as ordered by quality: in make_circles' order every proposal
    would start inside the first circle)"""
    p, lab, gt = datasets.make_circles(n_per_circle=n // 12, n_circles=6, n_outliers=n - 6 * (n // 12), sigma=sigma, seed=seed)
    order = np.random.default_rng(seed + 100).permutation(len(p))
    return np.ascontiguousarray(p[order]), lab[order], gt


def score_step(ctx, models, T2, steps):
    """upload + launch + fetch of one batch, as the proposal engine runs it; median over `steps` after two warm-ups"""
    buf = None
    ts = []
    for s in range(steps + 2):
        t0 = time.perf_counter()
        ctx.score_upload(models)
        ctx.score_launch(T2)
        if buf is None:
            buf = ctx.score_buffers()
        out = ctx.score_fetch(out=buf)
        if s >= 2:
            ts.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(ts)), out["counts"].copy()


def context(env):
    """a context created under the switches `env` (read at creation); the caller's environment is restored afterwards"""
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return _lib.Context(0)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def cell_samples(pts, S, rng, cells=16):
    """S samples of three distinct points from one random non-empty cell of the cells^2 grid over the bounding box each"""
    lo = pts.min(axis=0)
    ext = np.maximum(pts.max(axis=0) - lo, 1e-300)
    c = np.minimum((pts - lo) / ext * cells, cells - 1).astype(np.int64)
    key = c[:, 0] * cells + c[:, 1]
    order = np.argsort(key, kind="stable")
    ks, start, cnt = np.unique(key[order], return_index=True, return_counts=True)
    full = np.flatnonzero(cnt >= 3)
    out = np.empty((S, 3), np.int32)
    for s in range(S):
        j = full[rng.integers(len(full))]
        out[s] = order[start[j] + rng.choice(cnt[j], 3, replace=False)]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--sizes", default="10000,100000,1000000")
    args = ap.parse_args()
    thr = 2.0
    T2 = 2.25 * thr * thr
    pts, _, _ = scene(1_000_000)
    n = pts.shape[0]
    out = dict(workload="circles", n_score=n, threshold=thr)

    ctx = context({})
    dense = context({"PGX_NO_FILTER": "1", "PGX_SCORE_NO_CULL": "1"})
    out["device"] = ctx.device_info()["name"]
    ctx.set_points(_lib.CIRCLE2D, pts)
    dense.set_points(_lib.CIRCLE2D, pts)
    rng = np.random.default_rng(1)
    batches = {"uniform": rng.integers(0, n, (2200, 3)).astype(np.int32), "grid_cell": cell_samples(pts, 2200, rng)}
    for name, smp in batches.items():
        models = ctx.solve_minimal(smp)
        models = models[np.isfinite(models).all(axis=1)][:2048]
        ms, counts = score_step(ctx, models, T2, args.steps)
        ctx.score_upload(models)
        st = ctx.score_stats(T2)
        ms_d, counts_d = score_step(dense, models, T2, args.steps)
        out[name] = dict(hypotheses=int(models.shape[0]), median_radius=float(np.median(models[:, 2])), score_ms=ms,
                         score_models_per_s=models.shape[0] / (ms * 1e-3), path=st["path"], filter=st["filter"],
                         group_survival=st["surviving_group_steps"] / max(st["group_pairs"], 1),
                         exact_fraction=st["exact_evaluations"] / max(st["pairs"], 1),
                         dense_score_ms=ms_d, dense_models_per_s=models.shape[0] / (ms_d * 1e-3), cull_speedup=ms_d / ms,
                         dense_counts_identical=bool(np.array_equal(counts, counts_d)))
    ctx.close()
    dense.close()

    calls = {}
    for size in [int(s) for s in args.sizes.split(",") if s]:
        p, gen, gt = scene(size, seed=2)
        px.findCircles(p[: min(size, 20000)], threshold=thr, minimum_point_number=size // 40, seed=1)     # warm-up (kernels, context)
        # minimum_point_number: above the uniform outliers the annulus of a large spurious circle holds (about n / 100; a circle has
        # n / 12 inliers), and small enough for the stop on the predicted unseen inliers (_engine.predicted_unseen_inliers): with a
        # 3-point sample and conf = 0.5 that prediction falls below 6 % of the uncovered points after 4 000 iterations, so n / 25 ends
        # the run with two circles left; both are measured
        for sampler_id, div in [(s, d) for d in (40, 25) for s in (0, 2, 3)]:
            kw = dict(threshold=thr, minimum_point_number=size // div, sampler_id=sampler_id, seed=1)
            t0 = time.perf_counter()
            circles, labels = px.findCircles(p, **kw)
            dt = time.perf_counter() - t0
            found = 0
            for g in gt:
                if len(circles):
                    k = int(np.argmin(np.linalg.norm(circles[:, :2] - g[:2], axis=1)))
                    found += bool(np.linalg.norm(circles[k, :2] - g[:2]) < 1.0 and abs(circles[k, 2] - g[2]) < 1.0)
            key = f"{size}@sampler={sampler_id}@mpn=n/{div}"
            calls[key] = dict(seconds=dt, circles=int(len(circles)), gt_recovered=found)
            print(json.dumps({key: calls[key]}), file=sys.stderr, flush=True)
    out["findCircles"] = calls
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
