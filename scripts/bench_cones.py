#!/usr/bin/env python3
"""findCones' evidence of speed: the scoring step at 10^6 points x 2048 cone hypotheses on the cull + group-major path with the f32
filter - cones from three uniformly random oriented points and from three oriented points of one grid cell - against the same library
with both switched off (PGX_NO_FILTER=1 PGX_SCORE_NO_CULL=1, identical counts as a condition), the survival fractions of
pgx_score_stats, and findCones per sampler at 10^4, 10^5 and 10^6 points (six cones, half of the points uniform outliers, 1 cm noise
along the surface normal, normals within 5 degrees of the surface's with random sign, points in random order): cones found / returned
and wall time.  Writes one JSON record (default profiles/cones_bench.json) and prints it; the numbers go to DESIGN.md.  There is no
target for them, and recovery is reported as found, not tuned.

--normals estimated runs the findCones table alone, with estimateNormals(points, k=--normals-k) - or, with --normals-radius R, the ball
graph estimateNormals(points, k=None, radius=R) - in place of the scene's synthetic normals (the time of that call is recorded per
size), and writes profiles/cones_estimated_normals_bench.json.

usage: bench_cones.py [--steps 20] [--sizes 10000,100000,1000000] [--samplers 3,2,1,0] [--mpn-divisors 40,150] [--out FILE]
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
from bench_planes import context, score_step  # noqa: E402
from pyprogressivex import _lib, datasets  # noqa: E402

THR, SIGMA, ANGLES, EXTENT = 0.05, 0.01, (15.0, 40.0), (1.0, 4.0)
ANGLE_RANGE = (5.0, 60.0)


def scene(n, seed=0):
    """make_cones with six cones and half of the points uniform outliers, metre scale (10 m box, 1 cm noise)"""
    return datasets.make_cones(n_per_cone=n // 12, n_cones=6, n_outliers=n - 6 * (n // 12), sigma=SIGMA, half_angle_deg=ANGLES,
                               extent=EXTENT, seed=seed)


def rings(g):
    """sixteen exact points of the cone g on the rings that bound its piece"""
    a, d, c, s = g[:3], g[3:6], g[6], g[7]
    e1 = np.cross(d, [1.0, 0.0, 0.0] if abs(d[0]) < 0.9 else [0.0, 1.0, 0.0])
    e1 /= np.linalg.norm(e1)
    e2 = np.cross(d, e1)
    phi = np.arange(8) * (np.pi / 4)
    rad = np.cos(phi)[:, None] * e1 + np.sin(phi)[:, None] * e2
    return np.vstack([a + h * d + h * (s / c) * rad for h in EXTENT])


def found(cones, gt):
    """ground-truth cones a returned one matches: it points the same way and passes within 3 sigma of the sixteen ring points"""
    n = 0
    for g in gt:
        r = rings(g)
        for m in cones:
            e = r - m[:3]
            h = e @ m[3:6]
            rho = np.linalg.norm(np.cross(e, m[3:6]), axis=1)
            if m[3:6] @ g[3:6] > 0 and (np.abs(m[6] * rho - m[7] * h) < 3 * SIGMA).all():
                n += 1
                break
    return n


def cell_triples(pts, rng, S, cell=0.5):
    """S triples of points that share a grid cell of side `cell` (what NAPSAC-like samplers propose)"""
    key = np.floor(pts / cell).astype(np.int64)
    key = (key[:, 0] * 1000003 + key[:, 1]) * 1000003 + key[:, 2]
    order = np.argsort(key, kind="stable")
    sk = key[order]
    starts = np.flatnonzero(np.r_[True, sk[1:] != sk[:-1]])
    ends = np.r_[starts[1:], len(sk)]
    big = np.flatnonzero(ends - starts >= 3)
    c = big[rng.integers(0, len(big), S)]
    pick = (starts[c][:, None] + (rng.random((S, 3)) * (ends[c] - starts[c])[:, None]).astype(np.int64))
    return order[pick].astype(np.int32)


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
        args.out = os.path.join(ROOT, "profiles", "cones_estimated_normals_bench.json" if estimated else "cones_bench.json")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    T2 = 2.25 * THR * THR
    if estimated:
        return recovery(args, dict(workload="cones", normals="estimated", normals_k=args.normals_k, normals_radius=args.normals_radius,
                                   threshold=THR, angle_range=list(ANGLE_RANGE)))
    pts, nrm, _, _ = scene(1_000_000)
    n = pts.shape[0]
    out = dict(workload="cones", n_score=n, threshold=THR, angle_range=list(ANGLE_RANGE))
    rng = np.random.default_rng(1)
    # most triples of oriented points give no cone with a half-angle in the range: sixteen times the samples, the first 2048 models kept
    batches = dict(random_points=rng.integers(0, n, (16 * 2048, 3)).astype(np.int32), grid_cell=cell_triples(pts, rng, 16 * 2048))
    lo, hi = (float(np.sin(np.deg2rad(a))) for a in ANGLE_RANGE)

    ctx = context({})
    out["device"] = ctx.device_info()["name"]
    ctx.set_radius_range(lo, hi)
    ctx.set_points(_lib.CONE3D, pts)
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
    dense.set_points(_lib.CONE3D, pts)
    for name in batches:
        ms_d, counts_d = score_step(dense, models[name], T2, args.steps)
        out[name].update(dense_score_ms=ms_d, cull_speedup=ms_d / out[name]["score_ms"],
                         dense_counts_identical=bool(np.array_equal(fast[name], counts_d)))
    dense.close()
    with open(args.out + ".partial", "w") as f:
        f.write(json.dumps(out) + "\n")
    recovery(args, out)


def recovery(args, out):
    """findCones per size, minimum_point_number and sampler: cones found / returned and wall time"""
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
            e = p[inl] - g[:, :3]
            radial = e - (e * g[:, 3:6]).sum(1)[:, None] * g[:, 3:6]
            radial /= np.linalg.norm(radial, axis=1)[:, None]
            true = g[:, 6:7] * radial - g[:, 7:8] * g[:, 3:6]
            err = np.degrees(np.arccos(np.clip(np.abs((true * nr[inl]).sum(1)), 0.0, 1.0)))
            out.setdefault("estimateNormals", {})[str(size)] = dict(seconds=dt, median_error_deg=float(np.median(err)),
                                                                    p95_error_deg=float(np.percentile(err, 95)), undefined=int(np.isnan(nr).any(axis=1).sum()))
        # minimum_point_number = n / divisor.  A cone has n / 12 inliers; a shell of width 3 thr about the largest cone (slant length
        # 3.9, mean circumference 13.2) holds 51 x 0.15 / 1000 = 0.8 % of the outliers, n / 260
        for div in [int(s) for s in args.mpn_divisors.split(",") if s]:
            kw = dict(threshold=THR, minimum_point_number=size // div, seed=1, angle_range=ANGLE_RANGE)
            for sid in [int(s) for s in args.samplers.split(",") if s]:
                px.findCones(p[: min(size, 20000)], nr[: min(size, 20000)], sampler_id=sid, **kw)      # warm-up (kernels, context)
                t0 = time.perf_counter()
                cones, labels = px.findCones(p, nr, sampler_id=sid, **kw)
                dt = time.perf_counter() - t0
                key = f"{size}@sampler={sid}@mpn=n/{div}"
                calls[key] = dict(seconds=dt, returned=int(len(cones)), found=found(cones, gt))
                print(key, calls[key], file=sys.stderr, flush=True)
                with open(args.out + ".partial", "w") as f:          # (a long run that is cut short keeps what it measured)
                    f.write(json.dumps(dict(out, findCones=calls)) + "\n")
    out["findCones"] = calls
    text = json.dumps(out)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    if os.path.exists(args.out + ".partial"):
        os.remove(args.out + ".partial")
    print(text, flush=True)


if __name__ == "__main__":
    main()
