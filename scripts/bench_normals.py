#!/usr/bin/env python3
"""estimateNormals' measurements: the graph build and pgx_estimate_normals, separately, on make_cylinders scenes (six cylinders, half
of the points uniform outliers, 1 cm noise, points in random order) of 10^4, 10^5 and 10^6 points, for the k-NN graph at k = 8 and 16
and for a ball graph whose radius is bisected to a mean row length of about 32 (pgx_graph_build takes k <= 16, so k = 32 itself is
refused and recorded as such); and the angular error of the estimated normals against the true radial directions on the inliers,
median and 95th percentile in degrees, per graph.

Times are host-clock times of calls that end in a stream synchronisation (both entry points do), after `--warmup` calls, `--reps`
repetitions: median, minimum and maximum.  The normals call is upload of the points (24 n bytes) + kernel + read-back (24 n bytes); the
kernel alone comes from a second run of this script under `rocprofv3 --kernel-trace --output-format csv -d DIR -- python
scripts/bench_normals.py --kernel-run`, merged with `--merge DIR` (per-dispatch durations of estimate_normals_kernel: the --kernel-run
launches warmup + reps of them per configuration, in the order of the first run).  The working set of the kernel - points, offsets,
neighbour indices, the order, the outputs - is recorded next to the L2 (4 MB per XCD) and the 256 MB memory-side cache, with the regime
it falls in.  Writes profiles/normals_bench.json and prints it.

usage: bench_normals.py [--sizes 10000,100000,1000000] [--ks 8,16] [--warmup 2] [--reps 9] [--out FILE] [--kernel-run | --merge DIR]"""
import argparse
import csv
import glob
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "progressive-x_amd"), os.path.join(ROOT, "scripts")]
from pyprogressivex import _lib, datasets  # noqa: E402

SIGMA, RADII = 0.01, (0.3, 1.0)
L2_BYTES, MALL_BYTES = 4 << 20, 256 << 20
KERNEL = "estimate_normals_kernel"


def scene(n, seed=2):
    p, _, gen, gt = datasets.make_cylinders(n_per_cylinder=n // 12, n_cylinders=6, n_outliers=n - 6 * (n // 12), sigma=SIGMA, radius=RADII,
                                            seed=seed)
    order = np.random.default_rng(0).permutation(len(p))
    return np.ascontiguousarray(p[order]), gen[order], gt


def angular_error(pts, gen, gt, nrm):
    """degrees between the estimated normal and the true radial direction, over the inliers with a defined normal"""
    inl = (gen > 0) & ~np.isnan(nrm).any(axis=1)
    g = gt[gen[inl] - 1]
    radial = pts[inl] - g[:, :3]
    radial -= (radial * g[:, 3:6]).sum(1)[:, None] * g[:, 3:6]
    radial /= np.linalg.norm(radial, axis=1)[:, None]
    return np.degrees(np.arccos(np.clip(np.abs((radial * nrm[inl]).sum(1)), 0.0, 1.0)))


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return dict(median_ms=float(np.median(t)), min_ms=float(min(t)), max_ms=float(max(t)), reps=reps)


def ball_radius(ctx, pts, want=32.0):
    """a radius whose ball graph has a mean row length within 10 % of `want`: from the mean spacing of points on 120 square units of
    surface, scaled by sqrt(want / mean row) - most arcs join points of one surface - by at most 1.5 a step, so that no step builds a
    graph much larger than the one wanted"""
    n = len(pts)
    r = 3.0 * np.sqrt(120.0 / n)
    for _ in range(24):
        deg = ctx.graph_build(pts, _lib.GRAPH_BALL, radius=r, fetch=False) / n
        if abs(deg - want) <= 0.1 * want:
            break
        r *= float(np.clip(np.sqrt(want / max(deg, 1e-3)), 1.0 / 1.5, 1.5))
    return r


def configurations(ctx, pts, ks):
    out = [(f"knn k={k}", _lib.GRAPH_KNN, 0.0, k) for k in ks]
    r = ball_radius(ctx, pts)
    return out + [(f"ball r={r:.4g}", _lib.GRAPH_BALL, r, 1)]


def regime(bytes_):
    return "L2-resident" if bytes_ <= L2_BYTES else "memory-side-cache-resident, not L2" if bytes_ <= MALL_BYTES else "HBM"


def merge(path, trace_dir, warmup, reps):
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        raise SystemExit(f"no kernel trace under {trace_dir}")
    rows = [r for f in sorted(files) for r in csv.DictReader(open(f))]
    col = {key.lower(): key for key in rows[0]}
    name, t0, t1 = col["kernel_name"], col["start_timestamp"], col["end_timestamp"]
    durs = [(int(r[t0]), (int(r[t1]) - int(r[t0])) / 1e3) for r in rows if KERNEL in r[name]]
    durs = [d for _, d in sorted(durs)]
    rec = json.load(open(path))
    keys = [(s, c) for s in rec["sizes"] for c in rec["sizes"][s]["graphs"]]
    per = warmup + reps
    if len(durs) != per * len(keys):
        raise SystemExit(f"{len(durs)} dispatches of {KERNEL} in the trace, {per * len(keys)} expected")
    for j, (s, c) in enumerate(keys):
        d = durs[j * per + warmup:(j + 1) * per]
        g = rec["sizes"][s]["graphs"][c]
        g["kernel_us"] = dict(median=float(np.median(d)), min=float(min(d)), max=float(max(d)), dispatches=len(d), source="rocprofv3 --kernel-trace")
        g["kernel_gather_GBps"] = g["gather_bytes"] / (np.median(d) * 1e-6) / 1e9
    text = json.dumps(rec)
    open(path, "w").write(text + "\n")
    print(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="10000,100000,1000000")
    ap.add_argument("--ks", default="8,16")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "normals_bench.json"))
    ap.add_argument("--kernel-run", action="store_true", help="only the pgx_estimate_normals calls, for a kernel trace; writes nothing")
    ap.add_argument("--merge", default=None, help="directory of the kernel trace to merge into --out")
    args = ap.parse_args()
    if args.merge:
        return merge(args.out, args.merge, args.warmup, args.reps)
    ks = [int(s) for s in args.ks.split(",") if s]
    ctx = _lib.Context(int(os.environ.get("PGX_DEVICE", "0")))
    out = dict(workload="normals", device=ctx.device_info()["name"], warmup=args.warmup,
               timing="host clock around calls that end in a stream synchronisation; normals call = upload 24 n B + kernel + read-back 24 n B",
               k32="refused: pgx_graph_build takes k <= 16; the ball graph of mean row length ~32 stands in for the long rows",
               l2_bytes=L2_BYTES, memory_side_cache_bytes=MALL_BYTES, sizes={})
    for size in [int(s) for s in args.sizes.split(",") if s]:
        pts, gen, gt = scene(size)
        n = len(pts)
        graphs = {}
        for tag, kind, radius, k in configurations(ctx, pts, ks):
            arcs = ctx.graph_build(pts, kind, radius=radius, k=k, fetch=False)
            if args.kernel_run:
                for _ in range(args.warmup + args.reps):
                    ctx.estimate_normals(pts)
                graphs[tag] = {}
                continue
            g = dict(arcs=int(arcs), mean_row=arcs / n)
            g["graph_build"] = timed(lambda: ctx.graph_build(pts, kind, radius=radius, k=k, fetch=False), args.warmup, args.reps)
            g["normals_call"] = timed(lambda: ctx.estimate_normals(pts), args.warmup, args.reps)
            nrm, curv, undefined = ctx.estimate_normals(pts, want_curvature=True)
            err = angular_error(pts, gen, gt, nrm)
            g["undefined"] = undefined
            g["angular_error_deg"] = dict(median=float(np.median(err)), p95=float(np.percentile(err, 95)), inliers=int(len(err)))
            # what the kernel touches: points (read once per site and once per arc in each pass), CSR, order, outputs
            g["working_set_bytes"] = 24 * n + 4 * (n + 1) + 4 * int(arcs) + 4 * n + 24 * n
            g["gather_bytes"] = 2 * 24 * int(arcs) + 2 * 4 * int(arcs) + 24 * n + 8 * n + 24 * n
            g["regime"] = regime(g["working_set_bytes"])
            graphs[tag] = g
            print(size, tag, g, file=sys.stderr, flush=True)
        out["sizes"][str(size)] = dict(n=n, graphs=graphs)
    ctx.close()
    if args.kernel_run:
        return
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    text = json.dumps(out)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text, flush=True)


if __name__ == "__main__":
    main()
