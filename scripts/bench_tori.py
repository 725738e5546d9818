#!/usr/bin/env python3
"""findTori's evidence of speed: the scoring step at 10^6 points x 2048 torus hypotheses on the cull + group-major path with the f32
filter - tori from four uniformly random oriented points and from four oriented points of one grid cell - against the same library
with both switched off (PGX_NO_FILTER=1 PGX_SCORE_NO_CULL=1, identical counts as a condition), the survival fractions of
pgx_score_stats, and findTori per sampler at 10^4, 10^5 and 10^6 points (six tori, half of the points uniform outliers, 1 cm noise
along the surface normal, normals within 2 degrees of the surface's with random sign, points in random order): tori found / returned
and wall time.  Writes one JSON record (default profiles/tori_bench.json) and prints it; the numbers go to DESIGN.md.  There is no
target for them, and recovery is reported as found, not tuned.

usage: bench_tori.py [--steps 20] [--sizes 10000,100000,1000000] [--samplers 3,2,1,0] [--mpn-divisors 40,150] [--tilt 2.0] [--out FILE]"""
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

THR, SIGMA, MAJOR, MINOR = 0.05, 0.01, (0.8, 2.0), (0.2, 0.5)
MAJOR_RANGE, MINOR_RANGE = (0.5, 3.0), (0.1, 0.8)


def scene(n, tilt, seed=0):
    """make_tori with six tori and half of the points uniform outliers, metre scale (10 m box, 1 cm noise)"""
    return datasets.make_tori(n_per_torus=n // 12, n_tori=6, n_outliers=n - 6 * (n // 12), sigma=SIGMA, major_radius=MAJOR,
                              minor_radius=MINOR, normal_noise_deg=tilt, seed=seed)


def spine(g):
    """sixteen exact points of the torus g on its spine, the tube's centre circle"""
    d = g[3:6]
    e1 = np.cross(d, [1.0, 0.0, 0.0] if abs(d[0]) < 0.9 else [0.0, 1.0, 0.0])
    e1 /= np.linalg.norm(e1)
    e2 = np.cross(d, e1)
    phi = np.arange(16) * (np.pi / 8)
    return g[:3] + g[6] * (np.cos(phi)[:, None] * e1 + np.sin(phi)[:, None] * e2)


def found(tori, gt):
    """ground-truth tori a returned one matches: the true spine within 3 sigma of the found one and both radii within 3 sigma"""
    n = 0
    for g in gt:
        s = spine(g)
        for m in tori:
            e = s - m[:3]
            h = e @ m[3:6]
            rho = np.linalg.norm(np.cross(e, m[3:6]), axis=1)
            if (np.hypot(rho - m[6], h) < 3 * SIGMA).all() and abs(m[6] - g[6]) < 3 * SIGMA and abs(m[7] - g[7]) < 3 * SIGMA:
                n += 1
                break
    return n


def cell_samples(pts, rng, S, m=4, cell=0.5):
    """S samples of m points that share a grid cell of side `cell` (what NAPSAC-like samplers propose)"""
    key = np.floor(pts / cell).astype(np.int64)
    key = (key[:, 0] * 1000003 + key[:, 1]) * 1000003 + key[:, 2]
    order = np.argsort(key, kind="stable")
    sk = key[order]
    starts = np.flatnonzero(np.r_[True, sk[1:] != sk[:-1]])
    ends = np.r_[starts[1:], len(sk)]
    big = np.flatnonzero(ends - starts >= m)
    c = big[rng.integers(0, len(big), S)]
    pick = (starts[c][:, None] + (rng.random((S, m)) * (ends[c] - starts[c])[:, None]).astype(np.int64))
    return order[pick].astype(np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--sizes", default="10000,100000,1000000")
    ap.add_argument("--samplers", default="3,2,1,0")
    ap.add_argument("--mpn-divisors", default="40,150")
    ap.add_argument("--tilt", type=float, default=2.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tori_bench.json"))
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    T2 = 2.25 * THR * THR
    pts, nrm, _, _ = scene(1_000_000, args.tilt)
    n = pts.shape[0]
    out = dict(workload="tori", n_score=n, threshold=THR, radius_range=list(MINOR_RANGE), major_radius_range=list(MAJOR_RANGE),
               normal_noise_deg=args.tilt)
    rng = np.random.default_rng(1)
    # most samples of four oriented points give no ring torus with radii in the ranges (random points: 0.2 % of the slots, one cell:
    # 8 %): many times the samples, the first 2048 models kept
    batches = dict(random_points=rng.integers(0, n, (512 * 2048, 4)).astype(np.int32), grid_cell=cell_samples(pts, rng, 64 * 2048))

    ctx = context({})
    out["device"] = ctx.device_info()["name"]
    ctx.set_radius_range(*MINOR_RANGE)
    ctx.set_major_radius_range(*MAJOR_RANGE)
    ctx.set_points(_lib.TORUS3D, pts)
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
        out[name] = dict(hypotheses=int(len(models[name])), solver_yield_per_slot=float(valid.mean()), score_ms=ms,
                         score_models_per_s=len(models[name]) / (ms * 1e-3), path=st["path"], filter=st["filter"],
                         group_survival=st["surviving_group_steps"] / max(st["group_pairs"], 1),
                         exact_fraction=st["exact_evaluations"] / max(st["pairs"], 1), median_inliers=float(np.median(counts)))
    ctx.close()

    dense = context({"PGX_NO_FILTER": "1", "PGX_SCORE_NO_CULL": "1"})
    dense.set_points(_lib.TORUS3D, pts)
    for name in batches:
        ms_d, counts_d = score_step(dense, models[name], T2, args.steps)
        out[name].update(dense_score_ms=ms_d, cull_speedup=ms_d / out[name]["score_ms"],
                         dense_counts_identical=bool(np.array_equal(fast[name], counts_d)))
    dense.close()
    with open(args.out + ".partial", "w") as f:
        f.write(json.dumps(out) + "\n")
    recovery(args, out)


def recovery(args, out):
    """findTori per size, minimum_point_number and sampler: tori found / returned and wall time"""
    calls = {}
    for size in [int(s) for s in args.sizes.split(",") if s]:
        p, nr, gen, gt = scene(size, args.tilt, seed=2)
        order = np.random.default_rng(0).permutation(len(p))
        p, nr, gen = np.ascontiguousarray(p[order]), np.ascontiguousarray(nr[order]), gen[order]
        # minimum_point_number = n / divisor.  A torus has n / 12 inliers; a shell of width 3 thr about the largest torus (area
        # 4 pi^2 R r = 39.5) holds 39.5 x 0.15 / 1000 = 0.6 % of the outliers, n / 340
        for div in [int(s) for s in args.mpn_divisors.split(",") if s]:
            kw = dict(threshold=THR, minimum_point_number=size // div, seed=1, radius_range=MINOR_RANGE, major_radius_range=MAJOR_RANGE)
            for sid in [int(s) for s in args.samplers.split(",") if s]:
                px.findTori(p[: min(size, 20000)], nr[: min(size, 20000)], sampler_id=sid, **kw)      # warm-up (kernels, context)
                t0 = time.perf_counter()
                tori, labels = px.findTori(p, nr, sampler_id=sid, **kw)
                dt = time.perf_counter() - t0
                key = f"{size}@sampler={sid}@mpn=n/{div}"
                calls[key] = dict(seconds=dt, returned=int(len(tori)), found=found(tori, gt))
                print(key, calls[key], file=sys.stderr, flush=True)
                with open(args.out + ".partial", "w") as f:          # (a long run that is cut short keeps what it measured)
                    f.write(json.dumps(dict(out, findTori=calls)) + "\n")
    out["findTori"] = calls
    text = json.dumps(out)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    if os.path.exists(args.out + ".partial"):
        os.remove(args.out + ".partial")
    print(text, flush=True)


if __name__ == "__main__":
    main()
