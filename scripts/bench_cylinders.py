#!/usr/bin/env python3
"""findCylinders' evidence of speed: the scoring step at 10^6 points x 2048 cylinder hypotheses on the cull + group-major path with the
f32 shell filter - cylinders from two uniformly random oriented points and from two oriented points of one grid cell - against the
same library with both switched off (PGX_NO_FILTER=1 PGX_SCORE_NO_CULL=1, identical counts as a condition), the survival fractions of
pgx_score_stats, and findCylinders per sampler at 10^4, 10^5 and 10^6 points (six cylinders, half of the points uniform outliers, 1 cm
noise along the radius, normals within 5 degrees of radial with random sign, points in random order): cylinders found / returned and
wall time.  Writes one JSON record (default profiles/cylinders_bench.json) and prints it; the numbers go to DESIGN.md.  There is no
target for them.

--normals estimated runs the findCylinders table alone, with estimateNormals(points, k=--normals-k) - or, with --normals-radius R, the
ball graph estimateNormals(points, k=None, radius=R) - in place of the scene's synthetic normals (the time of that call is recorded per size), and writes profiles/cylinders_estimated_normals_bench.json: DESIGN.md 4.10.

usage: bench_cylinders.py [--steps 20] [--sizes 10000,100000,1000000] [--samplers 3,2,1,0] [--mpn-divisors 40,150] [--out FILE]
                          [--normals synthetic|estimated] [--normals-k 16] [--normals-radius R]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "progressive-x_amd"), os.path.join(ROOT, "scripts")]
import pyprogressivex as px  # noqa: E402
from bench_lines3d import cell_samples  # noqa: E402
from bench_planes import context, score_step  # noqa: E402
from pyprogressivex import _lib, datasets  # noqa: E402

THR, SIGMA, RADII = 0.05, 0.01, (0.3, 1.0)


def scene(n, seed=0):
    """make_cylinders with six cylinders and half of the points uniform outliers, metre scale (10 m box, 1 cm noise)"""
    return datasets.make_cylinders(n_per_cylinder=n // 12, n_cylinders=6, n_outliers=n - 6 * (n // 12), sigma=SIGMA, radius=RADII,
                                   seed=seed)


def found(cyls, gt):
    """ground-truth cylinders a returned one matches: radius within 3 sigma, axis within 3 sigma of the true axis 1.5 m either side
    of the midpoint (every cylinder is at least 3 m long)"""
    n = 0
    for g in gt:
        ends = g[:3] + np.array([[-1.5], [1.5]]) * g[3:6]
        for m in cyls:
            c = np.cross(ends - m[:3], m[3:6])
            if abs(m[6] - g[6]) < 3 * SIGMA and (np.linalg.norm(c, axis=1) < 3 * SIGMA).all():
                n += 1
                break
    return n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--sizes", default="10000,100000,1000000")
    ap.add_argument("--samplers", default="3,2,1,0")
    ap.add_argument("--mpn-divisors", default="40,150")
    ap.add_argument("--out", default=None)
    ap.add_argument("--normals", default="synthetic", choices=("synthetic", "estimated"))
    ap.add_argument("--normals-k", type=int, default=16)
    ap.add_argument("--normals-radius", type=float, default=None)
    args = ap.parse_args()
    estimated = args.normals == "estimated"
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "cylinders_estimated_normals_bench.json" if estimated else "cylinders_bench.json")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    T2 = 2.25 * THR * THR
    if estimated:
        return recovery(args, dict(workload="cylinders", normals="estimated", normals_k=args.normals_k, normals_radius=args.normals_radius, threshold=THR, radius_range=[0.1, 2.0]))
    pts, nrm, _, _ = scene(1_000_000)
    n = pts.shape[0]
    out = dict(workload="cylinders", n_score=n, threshold=THR, radius_range=[0.1, 2.0])
    rng = np.random.default_rng(1)
    # most pairs of oriented points give no cylinder with a radius in the range: sixteen times the samples, the first 2048 models kept
    batches = dict(random_points=rng.integers(0, n, (16 * 2048, 2)).astype(np.int32), grid_cell=cell_samples(pts, rng, 16 * 2048))

    ctx = context({})
    out["device"] = ctx.device_info()["name"]
    ctx.set_radius_range(0.1, 2.0)
    ctx.set_points(_lib.CYLINDER3D, pts)
    ctx.set_normals(nrm)
    models, fast = {}, {}
    for name, smp in batches.items():
        m = ctx.solve_minimal(smp)
        valid = np.isfinite(m).all(axis=1)
        models[name] = m[valid][:2048]
        ms, counts = score_step(ctx, models[name], T2, args.steps)
        ctx.score_upload(models[name])
        st = ctx.score_stats(T2)
        fast[name] = counts
        out[name] = dict(hypotheses=int(len(models[name])), solver_yield=float(valid.mean()), score_ms=ms, score_models_per_s=len(models[name]) / (ms * 1e-3),
                         path=st["path"], filter=st["filter"], group_survival=st["surviving_group_steps"] / max(st["group_pairs"], 1),
                         exact_fraction=st["exact_evaluations"] / max(st["pairs"], 1), median_inliers=float(np.median(counts)))
    ctx.close()

    dense = context({"PGX_NO_FILTER": "1", "PGX_SCORE_NO_CULL": "1"})
    dense.set_points(_lib.CYLINDER3D, pts)
    for name in batches:
        ms_d, counts_d = score_step(dense, models[name], T2, args.steps)
        out[name].update(dense_score_ms=ms_d, cull_speedup=ms_d / out[name]["score_ms"],
                         dense_counts_identical=bool(np.array_equal(fast[name], counts_d)))
    dense.close()
    recovery(args, out)


def recovery(args, out):
    """findCylinders per size, minimum_point_number and sampler: cylinders found / returned and wall time"""
    estimated = args.normals == "estimated"
    graph = dict(k=args.normals_k) if args.normals_radius is None else dict(k=None, radius=args.normals_radius)
    calls = {}
    for size in [int(s) for s in args.sizes.split(",") if s]:
        p, nr, gen, gt = scene(size, seed=2)
        order = np.random.default_rng(0).permutation(len(p))
        p, nr, gen = np.ascontiguousarray(p[order]), np.ascontiguousarray(nr[order]), gen[order]
        if estimated:
            px.estimateNormals(p[: min(size, 20000)], **graph)                                     # warm-up
            t0 = time.perf_counter()
            nr = px.estimateNormals(p, **graph)
            dt = time.perf_counter() - t0
            inl = (gen > 0) & ~np.isnan(nr).any(axis=1)
            g = gt[gen[inl] - 1]
            radial = p[inl] - g[:, :3]
            radial -= (radial * g[:, 3:6]).sum(1)[:, None] * g[:, 3:6]
            radial /= np.linalg.norm(radial, axis=1)[:, None]
            err = np.degrees(np.arccos(np.clip(np.abs((radial * nr[inl]).sum(1)), 0.0, 1.0)))
            out.setdefault("estimateNormals", {})[str(size)] = dict(seconds=dt, median_error_deg=float(np.median(err)),
                                                                    p95_error_deg=float(np.percentile(err, 95)), undefined=int(np.isnan(nr).any(axis=1).sum()))
        # minimum_point_number = n / divisor.  A cylinder has n / 12 inliers; a shell of width 3 thr about a cylinder of radius 1 and
        # length 6 holds 2 pi x 6 x 0.15 / 1000 = 0.6 % of the outliers, n / 350
        for div in [int(s) for s in args.mpn_divisors.split(",") if s]:
            kw = dict(threshold=THR, minimum_point_number=size // div, seed=1, radius_range=(0.1, 2.0))
            for sid in [int(s) for s in args.samplers.split(",") if s]:
                px.findCylinders(p[: min(size, 20000)], nr[: min(size, 20000)], sampler_id=sid, **kw)      # warm-up (kernels, context)
                t0 = time.perf_counter()
                cyls, labels = px.findCylinders(p, nr, sampler_id=sid, **kw)
                dt = time.perf_counter() - t0
                key = f"{size}@sampler={sid}@mpn=n/{div}"
                calls[key] = dict(seconds=dt, returned=int(len(cyls)), found=found(cyls, gt))
                print(key, calls[key], file=sys.stderr, flush=True)
                with open(args.out + ".partial", "w") as f:          # (a long run that is cut short keeps what it measured)
                    f.write(json.dumps(dict(out, findCylinders=calls)) + "\n")
    out["findCylinders"] = calls
    text = json.dumps(out)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    if os.path.exists(args.out + ".partial"):
        os.remove(args.out + ".partial")
    print(text, flush=True)


if __name__ == "__main__":
    main()
