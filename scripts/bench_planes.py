#!/usr/bin/env python3
"""findPlanes' evidence of speed: the scoring step at 10^6 points x 2048 plane hypotheses (the group cull + f32 slab filter
path, and the same step with both switched off as the dense reference), the survival fractions of pgx_score_stats, and
findPlanes wall time at 10^4, 10^5 and 10^6 points (2 mm and 1 cm noise, scoring exponent 1 and 2, with the ground-truth
planes recovered).  Prints one JSON line; the numbers go to DESIGN.md / README.md.

usage: bench_planes.py [--steps 20] [--sizes 10000,100000,1000000]"""
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


def scene(n, seed=0, sigma=0.01):
    """make_planes with six planes and half of the points uniform outliers, metre scale (10 m box, 1 cm noise by default)"""
    return datasets.make_planes(n_per_plane=n // 12, n_planes=6, n_outliers=n - 6 * (n // 12), sigma=sigma, seed=seed)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--sizes", default="10000,100000,1000000")
    args = ap.parse_args()
    thr = 0.05
    T2 = 2.25 * thr * thr
    pts, _, _ = scene(1_000_000)
    n = pts.shape[0]
    out = dict(workload="planes", n_score=n, hypotheses=2048, threshold=thr)

    ctx = context({})
    out["device"] = ctx.device_info()["name"]
    ctx.set_points(_lib.PLANE3D, pts)
    rng = np.random.default_rng(1)
    models = ctx.solve_minimal(rng.integers(0, n, (2048, 3)).astype(np.int32))     # RANSAC-like batch: planes through 3 random points
    models = models[np.isfinite(models).all(axis=1)]
    out["hypotheses"] = int(models.shape[0])
    ms, counts = score_step(ctx, models, T2, args.steps)
    ctx.score_upload(models)
    st = ctx.score_stats(T2)
    out.update(score_ms=ms, score_models_per_s=models.shape[0] / (ms * 1e-3),
               score_pairs_per_s=models.shape[0] * n / (ms * 1e-3), path=st["path"], filter=st["filter"],
               group_survival=st["surviving_group_steps"] / max(st["group_pairs"], 1),
               exact_fraction=st["exact_evaluations"] / max(st["pairs"], 1))
    ctx.close()

    dense = context({"PGX_NO_FILTER": "1", "PGX_SCORE_NO_CULL": "1"})
    dense.set_points(_lib.PLANE3D, pts)
    ms_d, counts_d = score_step(dense, models, T2, args.steps)
    dense.close()
    out.update(dense_score_ms=ms_d, dense_models_per_s=models.shape[0] / (ms_d * 1e-3), cull_speedup=ms_d / ms,
               dense_counts_identical=bool(np.array_equal(counts, counts_d)))

    calls = {}
    # scoring_exponent 1 and 2 (the signature's default): with 2 the squared shared support of a candidate grows with n^2 and the
    # runs end with 3-5 of the 6 planes at 10^5 and 10^6
    for size, sigma, e in [(int(s), sg, e) for s in args.sizes.split(",") if s for sg in (0.002, 0.01) for e in (1, 2)]:
        p, gen, gt = scene(size, seed=2, sigma=sigma)
        mpn = size // 40                  # above the uniform outliers a slab of width 3 thr holds (a plane has n / 12 inliers)
        kw = dict(threshold=thr, scoring_exponent=e, minimum_point_number=mpn, seed=1)
        px.findPlanes(p[: min(size, 20000)], **kw)                                   # warm-up (kernels, context)
        t0 = time.perf_counter()
        planes, labels = px.findPlanes(p, **kw)
        dt = time.perf_counter() - t0
        found = 0
        for g in gt:
            if len(planes) and np.degrees(np.arccos(min(1.0, float(np.max(np.abs(planes[:, :3] @ g[:3])))))) < 2.0:
                found += 1
        calls[f"{size}@sigma={sigma}@exponent={e}"] = dict(seconds=dt, planes=int(len(planes)), gt_recovered=found)
    out["findPlanes"] = calls
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
